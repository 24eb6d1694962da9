#!/usr/bin/env python3
"""Goldens of the region strategies, produced by running the REFERENCE's own Python in the build container:

    python tests/golden/make_golden_r9.py   ->  tests/golden/r9_regions.npz

Executed from the reference, unmodified (absent third-party names are inert placeholders, see make_golden.py):

  * patch_utils.get_vars_2d (patch_utils.py:794-826; scipy's convolve2d is the real one)
  * patch_utils.partition_2d_indices (:735-791); its three outputs are np.array(list(set)) in an undefined order, stored sorted
  * PW_NNAL.get_HV_inds (PW_NNAL.py:632-669) for two patch shapes (even and odd window)
  * PW_NNAL.superpix_scoring (:944-1021) and PW_AL.get_SuPix_inds (PW_AL.py:1168-1231).  skimage is absent, so a NumPy stand-in
    for skimage.measure.regionprops is bound to the name both modules imported: one entry per label > 0 of the slice in
    ascending label order, with 'label', 'min_intensity' (minimum of the intensity image over the region) and 'coords' (the
    region's pixels in row-major order) - the three documented properties the two functions read.

The file holds data only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402


class _Region(dict):
    pass


def regionprops(label_image, intensity_image=None):
    out = []
    for l in np.unique(label_image):
        if l <= 0:
            continue
        ii, jj = np.nonzero(label_image == l)
        r = _Region(label=int(l), coords=np.stack([ii, jj], axis=1))
        if intensity_image is not None:
            r['min_intensity'] = intensity_image[ii, jj].min()
        out.append(r)
    return out


def textured_volume(rs, shape):
    """Flat blocks (variance 0), gentle ramps and noisy blocks, so that a threshold of 2 splits the voxels; values k / 8."""
    H, W, S = shape
    v = np.zeros(shape)
    for z in range(S):
        base = rs.randint(0, 60)
        v[:, :, z] = base
        for _ in range(4):
            i, j = rs.randint(0, H - 8), rs.randint(0, W - 8)
            h, w = rs.randint(4, 16), rs.randint(4, 16)
            kind = rs.randint(0, 3)
            blk = v[i:i + h, j:j + w, z]
            if kind == 0:
                blk[...] = rs.randint(0, 4096)
            elif kind == 1:
                blk[...] = rs.randint(0, 40, size=blk.shape) + rs.randint(0, 8, size=blk.shape) / 8.
            else:
                blk[...] += np.arange(blk.shape[1])[None, :] * 0.5
    return v


def main():
    NNAL_tools, patch_utils, PW_NN, PW_NNAL = make_golden.import_reference()
    import PW_AL
    PW_NNAL.regionprops = regionprops
    PW_AL.regionprops = regionprops
    rs = np.random.RandomState(9001)
    out = {}
    shape = (40, 38, 12)
    vol = textured_volume(rs, shape)
    out['vol'] = vol.astype(np.float32)
    assert np.array_equal(out['vol'].astype(np.float64), vol)

    # get_vars_2d on three slices
    ds = [2, 5, 12]
    out['gv_d'] = np.array(ds)
    out['gv_slices'] = np.array([0, 5, 11])
    for d in ds:
        out['gv_var_%d' % d] = np.stack([patch_utils.get_vars_2d(vol[:, :, z], d) for z in out['gv_slices']], axis=2)

    # partition_2d_indices
    mask = (rs.rand(shape[0], shape[1]) > .8).astype(np.int64)
    a, b, c = patch_utils.partition_2d_indices(vol[:, :, 3], mask)
    out.update(part_slice=np.array(3), part_mask=mask.astype(np.uint8), part_masked=np.sort(np.asarray(a, dtype=np.int64)),
               part_hvar=np.sort(np.asarray(b, dtype=np.int64)), part_lvar=np.sort(np.asarray(c, dtype=np.int64)))

    # get_HV_inds: radius 4 (even window) and radius 3 (odd window), out-of-order pool
    pool = rs.permutation(int(np.prod(shape)))[:4000]
    out['hv_pool'] = pool.astype(np.int64)
    for tag, pshape in (('a', (9, 9, 3)), ('b', (7, 5, 1))):
        rads = [int((p - 1) / 2) for p in pshape]
        padded = np.pad(vol, [(r, r) for r in rads], 'constant')
        got = PW_NNAL.get_HV_inds(padded, pshape, 2., pool)
        out['hv_pshape_' + tag] = np.array(pshape)
        out['hv_valid_' + tag] = np.asarray(got, dtype=np.int64)
        print('get_HV_inds', pshape, len(got), 'of', len(pool))

    # superpix_scoring / get_SuPix_inds: labels 0..30 in 5 x 5 cells that move from slice to slice, some background
    seg = np.zeros(shape, dtype=np.int64)
    for z in range(shape[2]):
        cells = (np.arange(shape[0])[:, None] // 8) * 6 + (np.arange(shape[1])[None, :] + 2 * z) // 8
        seg[:, :, z] = np.where(rs.rand(shape[0], shape[1]) < .1, 0, 1 + (cells + z) % 30)
    seg[:, :, 7][seg[:, :, 7] > 20] = 3                      # labels absent from a slice
    inds = np.sort(rs.permutation(int(np.prod(shape)))[:2500])
    inds = inds[(inds % shape[2]) != 4]                      # a slice without any scored voxel
    scores = np.round(rs.rand(len(inds)) * .5, 2)            # exact ties
    scores[:7] = 0.
    table = PW_NNAL.superpix_scoring(seg, inds, scores)
    out.update(sp_seg=seg.astype(np.uint8), sp_inds=inds.astype(np.int64), sp_scores=scores, sp_table=table)
    flat = np.argsort(np.where(np.isfinite(table), table, np.inf).ravel(), kind='stable')[:9]
    codes = np.array(np.unravel_index(flat, table.shape))
    lists = PW_AL.get_SuPix_inds(seg, codes)
    out.update(sp_codes=codes.astype(np.int64), sp_lens=np.array([len(l) for l in lists]),
               sp_vox=np.concatenate([np.asarray(l, dtype=np.int64) for l in lists]))
    print('superpix_scoring: finite entries', int(np.isfinite(table).sum()), 'of', table.size)
    path = os.path.join(HERE, 'r9_regions.npz')
    np.savez_compressed(path, **out)
    print('r9_regions.npz: %d bytes' % os.path.getsize(path))


if __name__ == '__main__':
    main()
