#!/usr/bin/env python3
"""Datasets golden, produced by running the REFERENCE's own Python in the build container:

    python tests/golden/make_golden_datasets.py   ->  tests/golden/datasets.npz

Executed from /root/reference, unmodified: `datasets.utils.gen_minibatch_labeled_unlabeled_inds`, `global2local_inds`,
`prepare_batch_BrVol`; `datasets.data_holders.regular` (the LUV split by sizes) and `D3` (`load_images`,
`create_train_valid_gens(4, [8, 8, 2], n_labeled_train=2)`, `train_gen_fn`).  tensorflow / nibabel / imageio / nrrd / h5py are
the inert placeholder modules of make_golden.import_reference(); nothing of them is called.  The data reader handed to the
data holders is an in-memory table of synthetic subjects: four subjects of two modalities with differing shapes and dtypes,
integer values, masks in {0, 1, 2} plus one out-of-class value; two labelled, two unlabelled, one of those with the mask path
'NA'.  After every recorded sequence one more `np.random.rand()` is recorded: the position of the random stream.

The file holds data only: the subjects, the seeds, the recorded indices and batches."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402

SHAPES = [(12, 10, 6), (9, 11, 8), (12, 10, 7), (10, 10, 6)]
DTYPES = [np.int16, np.float64, np.float32, np.uint8]
MODS = ['T1', 'T2']
C = 3
OUT_OF_CLASS = 7


def subjects(seed=5200):
    """(table path -> array, img_addrs, mask_addrs)"""
    rs = np.random.RandomState(seed)
    table, img_addrs, mask_addrs = {}, {mod: [] for mod in MODS}, []
    for s_, (shp, dt) in enumerate(zip(SHAPES, DTYPES)):
        for mod in MODS:
            p = '/synthetic/sub%d_%s' % (s_, mod)
            lo = 0 if dt is np.uint8 else -40
            table[p] = rs.randint(lo, 200, size=shp).astype(dt)
            img_addrs[mod].append(p)
        mask = rs.randint(0, C, size=shp).astype(np.float64)
        mask[rs.rand(*shp) < 0.05] = OUT_OF_CLASS
        p = '/synthetic/sub%d_mask' % s_
        table[p] = mask
        mask_addrs.append('NA' if s_ == 3 else p)
    return table, img_addrs, mask_addrs


def main():
    make_golden.import_reference()
    from datasets import data_holders, utils
    table, img_addrs, mask_addrs = subjects()
    out = dict(shapes=np.array(SHAPES), subject_seed=np.array(5200), C=np.array(C), out_of_class=np.array(OUT_OF_CLASS))
    for p, a in table.items():
        out['table' + p.replace('/', '__')] = a
    reader = lambda p: table[p]

    # ---- index batches
    L_indic = np.array([1, 0, 1, 1, 0, 0, 0, 1, 0, 0, 1])
    out['mix_L_indic'] = L_indic
    for tag, n_labeled, seed in (('all', None, 11), ('fixed', 1, 12)):
        np.random.seed(seed)
        gen = utils.gen_minibatch_labeled_unlabeled_inds(L_indic, 3, n_labeled)
        for k in range(9):
            parts = next(gen)
            out['mix_%s_%d' % (tag, k)] = np.concatenate(parts)
            out['mix_%s_%d_parts' % (tag, k)] = np.array([len(p) for p in parts])
        out['mix_%s_seed' % tag], out['mix_%s_after' % tag] = np.array(seed), np.array(np.random.rand())
    assert any(len(out['mix_all_%d' % k]) == 2 for k in range(9))          # the remainder batch of 11 = 3 * 3 + 2

    # ---- the LUV split by sizes
    dat = data_holders.regular({m_: list(v) for m_, v in img_addrs.items()}, list(mask_addrs), reader, 3, [1, 2, 1], np.arange(C))
    for name in ('labeled_inds', 'unlabeled_inds', 'train_inds', 'valid_inds', 'test_inds', 'L_indic'):
        out['luv_' + name] = np.asarray(getattr(dat, name))
    out['luv_seed'], out['luv_sizes'] = np.array(3), np.array([1, 2, 1])

    # ---- global2local_inds
    g2l_inds, g2l_sizes = np.array([7, 0, 3, 12, 4, 9, 5, 11]), [4, 0, 5, 4]
    out['g2l_inds'], out['g2l_sizes'] = g2l_inds, np.array(g2l_sizes)
    for i, l in enumerate(utils.global2local_inds(g2l_inds, g2l_sizes)):
        out['g2l_out_%d' % i] = np.asarray(l)

    # ---- D3 training batches: subjects 0, 1 labelled, 2, 3 unlabelled (3 without a mask file), no validation subject
    luv = [np.array([0, 1]), np.array([2, 3]), np.array([], dtype=int)]
    d3 = data_holders.D3({m_: list(v) for m_, v in img_addrs.items()}, list(mask_addrs), reader, None, luv, np.arange(C))
    d3.load_images()
    np.random.seed(21)
    d3.create_train_valid_gens(4, [8, 8, 2], n_labeled_train=2)
    out['d3_train_n_slices'], out['d3_slices_L_indic'] = np.array(d3.train_n_slices), d3.slices_L_indic
    n_batches = 6
    for k in range(n_batches):
        X, Y = d3.train_gen_fn()
        # (9 unlabelled block centres in pairs: the permutation's remainder gives a batch of 2 + 1)
        assert X.shape[1:] == (2, 8, 8, 2) and Y.shape == X.shape[:4] + (C,) and X.dtype == np.float64 and len(X) in (3, 4)
        assert Y[:2].sum() > 0 and Y[2:].sum() == 0          # two labelled samples first, the unlabelled behind them
        out['d3_X_%d' % k], out['d3_Y_%d' % k] = X, Y
    out['d3_seed'], out['d3_batches'], out['d3_after'] = np.array(21), np.array(n_batches), np.array(np.random.rand())
    zero_rows = sum(int((out['d3_Y_%d' % k][:2].sum(-1) == 0).sum()) for k in range(n_batches))
    assert zero_rows > 0          # out-of-class voxels of labelled samples: all-zero one-hot rows

    # ---- prepare_batch_BrVol: listed slices, crop == the full slice (no crop draw), one unlabelled sample
    imgs = [[table[img_addrs[mod][s_]] for mod in MODS] for s_ in (0, 2)]
    masks = [table['/synthetic/sub0_mask'], table['/synthetic/sub2_mask']]
    np.random.seed(31)
    X, Y = utils.prepare_batch_BrVol(imgs, masks, [12, 10, 2], C, [3, 5], np.array([1, 0]))
    out['pb_X'], out['pb_Y'], out['pb_after'] = X, Y, np.array(np.random.rand())
    np.random.seed(31)
    assert out['pb_after'] == np.random.rand()          # nothing was drawn
    Xn, Yn = utils.prepare_batch_BrVol(imgs, masks, [12, 10, 2], None, [3, 5], np.array([1, 0]))
    out['pb_Y_nohot'] = Yn
    assert np.array_equal(Xn, X) and np.isnan(Yn[1]).all()
    np.savez_compressed(os.path.join(HERE, 'datasets.npz'), **out)
    print('datasets: %d arrays, %d bytes' % (len(out), os.path.getsize(os.path.join(HERE, 'datasets.npz'))))


if __name__ == '__main__':
    main()
