"""Shared by tests/test_datasets_host.py and tests/test_gpu_datasets.py: the subjects of tests/golden/datasets.npz (written by
tests/golden/make_golden_datasets.py from the reference's own modules) and the data holders built on them."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'datasets.npz')
MODS = ['T1', 'T2']
_cache = {}


def golden():
    if 'g' not in _cache:
        with np.load(GOLDEN) as f:
            _cache['g'] = {k: f[k] for k in f.files}
    return _cache['g']


def subjects():
    """(table path -> array, img_addrs {modality: paths}, mask_addrs) - fresh lists, shared read-only arrays."""
    g = golden()
    table = {k[len('table'):].replace('__', '/'): v for k, v in g.items() if k.startswith('table__')}
    n = len(g['shapes'])
    img_addrs = {mod: ['/synthetic/sub%d_%s' % (s, mod) for s in range(n)] for mod in MODS}
    mask_addrs = ['/synthetic/sub%d_mask' % s if s != 3 else 'NA' for s in range(n)]
    return table, img_addrs, mask_addrs


def holder(cls, luv, seed=None, sess=None, class_labels=None, load=True):
    g = golden()
    table, img_addrs, mask_addrs = subjects()
    dat = cls(img_addrs, mask_addrs, lambda p: table[p], seed, luv, np.arange(int(g['C'])) if class_labels is None else class_labels)
    if load:
        dat.load_images(sess) if sess is not None else dat.load_images()
    return dat


def d3_luv():
    return [np.array([0, 1]), np.array([2, 3]), np.array([], dtype=int)]


def labels_of(onehot):
    """One-hot rows -> class ids, -1 for an all-zero row."""
    onehot = np.asarray(onehot)
    return np.where(onehot.sum(-1) > 0, onehot.argmax(-1), -1).astype(np.int32)


def counts_of(labels, C):
    labels = np.asarray(labels)
    return np.array([(labels == j).sum() for j in range(C)] + [(labels < 0).sum()], dtype=np.int64)
