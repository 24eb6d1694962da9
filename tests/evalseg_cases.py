"""Helpers shared by tests/test_evalseg_host.py, tests/test_gpu_confusion.py and tests/test_gpu_evalseg.py: the golden of
tests/golden/make_golden_evalseg.py, literal loops for the confusion counts, a restatement of the lesion ranking with a stable
argsort directly on scipy.ndimage.label, and the comparison of a lesion ranking with the reference's under its open tie order.
TEST INFRASTRUCTURE, no test in here."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'evalseg.npz')


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        out = {k: z[k] for k in z.files}
    for v in out.values():
        v.setflags(write=False)
    return out


def confusion_loops(pred, lab, C, inner, groups, first, fill):
    """(counts [groups, C, C], skipped) by the issue's four sentences, element by element."""
    counts = np.zeros((groups, C, C), dtype=np.int64)
    skipped = 0
    for i in range(len(pred)):
        j = first + i
        g = (j // inner) % groups
        t = int(lab[i])
        if not 0 <= t < C:
            if 0 <= fill < C:
                t = fill
            else:
                skipped += 1
                continue
        p = int(pred[i])
        if not 0 <= p < C:
            skipped += 1
            continue
        counts[g][t][p] += 1
    return counts, skipped


def confusion_numpy(pred, lab, C, inner, groups, first, fill):
    """The same with np.bincount (for sizes where the loops would be slow)."""
    p, t = np.asarray(pred).astype(np.int64), np.asarray(lab).astype(np.int64)
    g = ((first + np.arange(len(p), dtype=np.int64)) // inner) % groups
    if 0 <= fill < C:
        t = np.where((t < 0) | (t >= C), fill, t)
    ok = (t >= 0) & (t < C) & (p >= 0) & (p < C)
    counts = np.bincount(((g * C + t) * C + p)[ok], minlength=groups * C * C).reshape(groups, C, C)
    return counts.astype(np.int64), int((~ok).sum())


def stable_ranks(mask):
    """Ranks 1 .. K of the 26-connected (8-connected in 2-D) components of a binary mask whose first voxel is 0, by descending
    volume, equal volumes -> the component whose first voxel comes first in C order (scipy's label order): int64."""
    from scipy import ndimage
    m = np.asarray(mask) != 0
    assert not m.reshape(-1)[0]
    lab, K = ndimage.label(m, structure=np.ones((3,) * m.ndim, dtype=bool))
    vols = np.bincount(lab.reshape(-1), minlength=K + 1)[1:]
    order = np.argsort(-vols, kind='stable')
    rank_of = np.zeros(K + 1, dtype=np.int64)
    rank_of[order + 1] = np.arange(1, K + 1)
    return rank_of[lab]


def stable_drop(mask, thr):
    r = stable_ranks(mask)
    vols = np.bincount(r.reshape(-1))
    vols[0] = 0
    return (vols[r] >= thr).astype(np.uint8)


def assert_ranks_match_reference(got, ref):
    """The condition on lesion inputs: `got` and the reference's ranks `ref` (whose order among equal volumes is not defined)
    describe the same partition into components, give every voxel the same component volume - so the sequence of sizes by rank
    is the same - and agree exactly on every component whose volume is unique.  -> the number of such components."""
    got, ref = np.asarray(got).astype(np.int64), np.asarray(ref).astype(np.int64)
    assert got.shape == ref.shape
    np.testing.assert_array_equal(got > 0, ref > 0)
    K = int(ref.max())
    assert int(got.max()) == K
    pairs = np.unique(np.stack([got.reshape(-1), ref.reshape(-1)], axis=1), axis=0)
    assert len(pairs) == K + 1 and len(np.unique(pairs[:, 0])) == K + 1 and len(np.unique(pairs[:, 1])) == K + 1      # a bijection
    vg, vr = np.bincount(got.reshape(-1), minlength=K + 1), np.bincount(ref.reshape(-1), minlength=K + 1)
    np.testing.assert_array_equal(vg[got][ref > 0], vr[ref][ref > 0])
    np.testing.assert_array_equal(vg[1:], vr[1:])
    assert np.all(np.diff(vg[1:]) <= 0)
    unique = np.array([k for k in range(1, K + 1) if np.sum(vr[1:] == vr[k]) == 1], dtype=np.int64)
    sel = np.isin(ref, unique)
    np.testing.assert_array_equal(got[sel], ref[sel])
    return len(unique)
