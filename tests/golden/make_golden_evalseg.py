#!/usr/bin/env python3
"""Segmentation-evaluation golden, produced by running the REFERENCE's own Python in the build container:

    python tests/golden/make_golden_evalseg.py   ->  tests/golden/evalseg.npz

Executed from /root/reference, unmodified: `eval_utils.eval_full_segs_explicit_partitions` (two subjects; a nested list of cut
points, and an array of per-subject partitions with two cut points), `eval_utils.eval_full_segs_label_percentage` (one clean
three-fold subject and one subject with two gaps, the skip branch; a subject without a gap, whose IndexError is recorded),
`eval_utils.binary_F1_score` and `multi_F1_score` (C = 3, one absent class; scikit-learn's f1_score is installed here),
`datasets.lesion_utils.find_lesion_components` and `drop_lesions_with_threshold` (thr in {2, 8, 30}).

tensorflow / nibabel / imageio / nrrd / h5py are the inert placeholder modules of make_golden.import_reference(); nothing of
them is called.  skimage is absent as well, and `lesion_utils` calls `skimage.measure.label`: the script installs a stand-in
under that module's name `label` which calls scipy.ndimage.label with the full 3 x 3 x 3 structure - the same components
(skimage's default is full connectivity), numbered in the same raster order of their first voxels, 0 for the zero voxels.

Dilated random seeds give many components of equal volume, among which the reference's np.argsort(-vols) has no defined
order: the lesion volume must hold at least 5 components whose volume is unique (asserted below), and the tests compare exact
ranks only on those, the partition and the volume at every voxel everywhere.

The file holds data only: the volumes (uint8, compressed), the arguments and the recorded outputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

SHAPE = (40, 36, 24)
LESION_SHAPE = (34, 30, 24)
THRESHOLDS = (2, 8, 30)


def blob_pair(rs, shape, values=1):
    """A (seg, mask) pair: a mask of `values` nested ellipsoid shells around the volume's middle, and a segmentation that is the
    mask with 6 % of its voxels redrawn."""
    H, W, Z = shape
    i, j, z = np.meshgrid(np.arange(H), np.arange(W), np.arange(Z), indexing='ij')
    r = np.sqrt(((i - H / 2.) / (H / 2.)) ** 2 + ((j - W / 2.) / (W / 2.)) ** 2 + ((z - Z / 2.) / (Z / 2.)) ** 2)
    mask = np.zeros(shape, dtype=np.uint8)
    mask[r < 0.75] = 1
    if values > 1:
        mask[r < 0.4] = 2
    seg = mask.copy()
    flip = rs.rand(*shape) < 0.06
    seg[flip] = rs.randint(0, values + 1, size=int(flip.sum()))
    return seg, mask


def banded_mask(shape, full_slices):
    """A mask whose label 1 covers half of every slice in `full_slices` and an eighth of every other slice."""
    mask = np.zeros(shape, dtype=np.uint8)
    mask[:shape[0] // 8] = 1
    for z in full_slices:
        mask[:shape[0] // 2, :, z] = 1
    return mask


def lesion_volume(rs, shape, density=0.004):
    """Random seeds, some of them grown: single voxels, 3 x 3 x 3 cubes, plates and rods of different lengths."""
    vol = np.zeros(shape, dtype=np.uint8)
    seeds = np.argwhere(rs.rand(*shape) < density)
    for n, (i, j, z) in enumerate(seeds):
        kind = n % 5
        if kind == 0:
            vol[i, j, z] = 1
        elif kind == 1:
            vol[max(i - 1, 0):i + 2, max(j - 1, 0):j + 2, max(z - 1, 0):z + 2] = 1
        elif kind == 2:
            vol[i, j, z:z + 2 + n % 7] = 1
        elif kind == 3:
            vol[i:i + 1 + n % 4, j:j + 2, z] = 1
        else:
            vol[i:i + 2 + n % 3, j, z] = 1
    vol[0, 0, 0] = 0
    return vol


def install_label_standin(lesion_utils):
    from scipy import ndimage

    def label(mask):
        return ndimage.label(np.asarray(mask) != 0, structure=np.ones((3, 3, 3), dtype=bool))[0]
    lesion_utils.label = label


def main():
    make_golden.import_reference()
    import eval_utils
    from datasets import lesion_utils
    install_label_standin(lesion_utils)
    rs = np.random.RandomState(7300)
    out = {}

    # ---- explicit partitions: one binary subject, one with values {0, 1, 2}
    pairs = [blob_pair(rs, SHAPE, 1), blob_pair(rs, SHAPE, 2)]
    segs, masks = [p[0] for p in pairs], [p[1] for p in pairs]
    for k in range(2):
        out['ep_seg_%d' % k], out['ep_mask_%d' % k] = segs[k], masks[k]
    nested = [[8, 16]]
    out['ep_list'] = np.array(nested)
    out['ep_list_overall'], out['ep_list_parts'] = eval_utils.eval_full_segs_explicit_partitions(segs, masks, nested)
    parts = np.array([[6, 15], [10, 20]])
    out['ep_array'] = parts
    out['ep_array_overall'], out['ep_array_parts'] = eval_utils.eval_full_segs_explicit_partitions(segs, masks, parts)

    # ---- label percentage: a clean three-fold subject, a subject with two gaps (skipped: its row stays zero)
    lp_masks = [banded_mask(SHAPE, range(7, 17)), banded_mask(SHAPE, list(range(4, 9)) + list(range(14, 19)))]
    lp_segs = []
    for m in lp_masks:
        seg = m.copy()
        flip = rs.rand(*SHAPE) < 0.08
        seg[flip] = 1 - seg[flip]
        lp_segs.append(seg)
    for k in range(2):
        out['lp_seg_%d' % k], out['lp_mask_%d' % k] = lp_segs[k], lp_masks[k]
    out['lp_label'], out['lp_percentage'] = np.array(1), np.array(0.25)
    out['lp_overall'], out['lp_parts'] = eval_utils.eval_full_segs_label_percentage(lp_segs, lp_masks, 1, 0.25)
    assert np.all(out['lp_parts'][0] > 0) and np.all(out['lp_parts'][1] == 0)
    # no gap at all: every slice lies below the threshold
    nogap_mask = banded_mask(SHAPE, [])
    out['lp_nogap_seg'], out['lp_nogap_mask'] = lp_segs[0], nogap_mask
    try:
        eval_utils.eval_full_segs_label_percentage([lp_segs[0]], [nogap_mask], 1, 0.25)
        raise SystemExit('the reference did not raise on a subject without a gap')
    except IndexError as e:
        out['lp_nogap_error'] = np.array(str(e))

    # ---- F1 scores
    bp, bl = (rs.rand(30, 28) < 0.3).astype(np.uint8), (rs.rand(30, 28) < 0.35).astype(np.uint8)
    out['f1_bin_pred'], out['f1_bin_lab'] = bp, bl
    out['f1_bin'] = np.array(eval_utils.binary_F1_score(bp, bl))
    out['f1_bin_zero'] = np.array(eval_utils.binary_F1_score(np.zeros_like(bp), np.zeros_like(bl)))
    mp, ml = rs.randint(0, 3, size=(30, 28)).astype(np.uint8), rs.randint(0, 2, size=(30, 28)).astype(np.uint8)      # class 2 has no support
    out['f1_multi_pred'], out['f1_multi_lab'] = mp, ml
    scores, av = eval_utils.multi_F1_score(mp, ml, 3)
    out['f1_multi_scores'], out['f1_multi_av'] = np.asarray(scores), np.array(av)

    # ---- lesions
    vol = lesion_volume(rs, LESION_SHAPE)
    out['lesion_mask'] = vol
    ranks = lesion_utils.find_lesion_components(vol)
    out['lesion_ranks'] = ranks.astype(np.uint16)
    assert np.array_equal(out['lesion_ranks'], ranks)
    sizes = np.bincount(ranks.astype(np.int64).reshape(-1))[1:]
    unique = int(np.sum(np.bincount(sizes)[sizes] == 1))
    assert unique >= 5, unique
    out['lesion_unique_volumes'] = np.array(unique)
    out['lesion_thresholds'] = np.array(THRESHOLDS)
    for thr in THRESHOLDS:
        out['lesion_drop_%d' % thr] = lesion_utils.drop_lesions_with_threshold(vol, thr)
        assert 0 < out['lesion_drop_%d' % thr].sum() < vol.sum() or thr == 2

    path = os.path.join(HERE, 'evalseg.npz')
    np.savez_compressed(path, **out)
    print('wrote %s: %d arrays, %d bytes; %d lesions, %d of unique volume' % (path, len(out), os.path.getsize(path), len(sizes), unique))


if __name__ == '__main__':
    main()
