"""alq_confusion_counts through the C ABI (csrc/confusion.hip; GPU box) against np.bincount (tests/evalseg_cases.py): every
size around the 16-byte vectors and the 256-thread block, every class count and id-type pair the Python layer uses, every
(inner, groups) pattern, offsets, fills, skipped elements, contention on one cell, unaligned buffers, chunked calls, the capped
grid, group windows, guard margins, repeatability and the refused calls.  Integers throughout: every comparison is an
equality."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import evalseg_cases as ec  # noqa: E402

U8, I32, I64 = 0, 1, 2
NP_TYPES = {U8: np.uint8, I32: np.int32, I64: np.int64}
TYPE_PAIRS = [(I64, I32), (I64, U8), (U8, I32), (U8, U8)]          # (pred, labels): what eval_utils feeds
SIZES = (1, 15, 16, 17, 255, 256, 257, 4099)
CLASSES = (1, 2, 3, 8, 16)
GUARD = 64
PATTERN = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope='module')
def sess():
    import nnal_amd  # noqa: F401
    from nnal_amd import device
    return device.default_session()


def _patterns(n):
    return [(n, 1), (1, 1), (1, 7), (1, 64), (1, 70), (1, 300), (35, 5), (256, 3)]


def draw(rs, n, Cn, pred_type, lab_type, bad_lab=0.10, bad_pred=0.02):
    """ids with 10 % of the labels out of range (-1, or 255 as uint8) and 2 % of the predictions (C, -1 or 2^40; 255 as uint8)."""
    lab = rs.randint(0, Cn, size=n).astype(np.int64)
    pred = rs.randint(0, Cn, size=n).astype(np.int64)
    lab[rs.rand(n) < bad_lab] = 255 if lab_type == U8 else -1
    out = rs.rand(n) < bad_pred
    if pred_type == U8:
        pred[out] = 255
    else:
        pred[out] = rs.choice([Cn, -1, 1 << 40] if pred_type == I64 else [Cn, -1, 1 << 20], size=int(out.sum()))
    return pred.astype(NP_TYPES[pred_type]), lab.astype(NP_TYPES[lab_type])


def _ptr(t, offset_bytes=0):
    return C.c_void_p(t.data_ptr() + offset_bytes) if t is not None else None


class Guarded(object):
    """int64 counts [groups C C] and skipped [1] between 64-element margins of a fill pattern."""

    def __init__(self, sess, cells, start=None):
        torch = sess.torch
        self.cells = cells
        host = np.full(GUARD + cells + GUARD + 1 + GUARD, PATTERN, dtype=np.int64)
        host[GUARD:GUARD + cells] = 0 if start is None else start.reshape(-1)
        host[2 * GUARD + cells] = 0
        self.buf = sess.to_device(host, torch.int64)
        self.before = host

    def counts_ptr(self):
        return _ptr(self.buf, GUARD * 8)

    def skipped_ptr(self):
        return _ptr(self.buf, (2 * GUARD + self.cells) * 8)

    def read(self, shape):
        """-> (counts, skipped); asserts the margins"""
        a = self.buf.cpu().numpy()
        c = self.cells
        assert np.all(a[:GUARD] == PATTERN) and np.all(a[GUARD + c:2 * GUARD + c] == PATTERN) and np.all(a[2 * GUARD + c + 1:] == PATTERN)
        return a[GUARD:GUARD + c].reshape(shape), int(a[2 * GUARD + c])

    def untouched(self):
        return np.array_equal(self.buf.cpu().numpy(), self.before)


def call(sess, d_pred, pt, d_lab, lt, n, first, inner, groups, Cn, fill, g, want_skipped=True, off_p=0, off_l=0):
    sess.bind_stream()
    rc = sess.lib.alq_confusion_counts(sess.ctx, _ptr(d_pred, off_p), pt, _ptr(d_lab, off_l), lt, n, first, inner, groups, Cn, fill,
                                       g.counts_ptr(), g.skipped_ptr() if want_skipped else None)
    assert rc == 0, sess.lib.alq_last_error().decode()


def run(sess, pred, lab, pt, lt, first, inner, groups, Cn, fill, want_skipped=True, start=None, d=None):
    d_pred, d_lab = d if d is not None else (sess.to_device(pred, getattr(sess.torch, pred.dtype.name)),
                                             sess.to_device(lab, getattr(sess.torch, lab.dtype.name)))
    g = Guarded(sess, groups * Cn * Cn, start)
    call(sess, d_pred, pt, d_lab, lt, len(pred), first, inner, groups, Cn, fill, g, want_skipped)
    return g.read((groups, Cn, Cn))


# ------------------------------------------------------------------------------------------------ the grid of the issue
@pytest.mark.parametrize('types', TYPE_PAIRS, ids=lambda t: 'p%d_l%d' % t)
@pytest.mark.parametrize('Cn', CLASSES)
def test_counts_equal_numpy(sess, Cn, types):
    """n x (inner, groups) x first x fill, with out-of-range labels and predictions; d_skipped = NULL gives the same matrix."""
    pt, lt = types
    rs = np.random.RandomState(100 * Cn + 10 * pt + lt)
    torch = sess.torch
    for n in SIZES:
        pred, lab = draw(rs, n, Cn, pt, lt)
        d = (sess.to_device(pred, getattr(torch, pred.dtype.name)), sess.to_device(lab, getattr(torch, lab.dtype.name)))
        for inner, groups in _patterns(n):
            for first in (0, 3, inner * groups - 1):
                for fill in (-1, 0, Cn - 1):
                    want, skipped = ec.confusion_numpy(pred, lab, Cn, inner, groups, first, fill)
                    got, got_skipped = run(sess, pred, lab, pt, lt, first, inner, groups, Cn, fill, d=d)
                    tag = 'n=%d inner=%d groups=%d first=%d fill=%d' % (n, inner, groups, first, fill)
                    np.testing.assert_array_equal(got, want, err_msg=tag)
                    assert got_skipped == skipped and want.sum() + skipped == n, tag
        # without the skipped word: the same matrix (and the word is left alone)
        got, word = run(sess, pred, lab, pt, lt, 3, 35, 5, Cn, -1, want_skipped=False, d=d)
        np.testing.assert_array_equal(got, ec.confusion_numpy(pred, lab, Cn, 35, 5, 3, -1)[0])
        assert word == 0


def test_numpy_statement_equals_the_loops():
    """The bincount statement the grid is compared with, against the issue's sentences element by element."""
    rs = np.random.RandomState(9)
    pred, lab = draw(rs, 257, 3, I64, I32)
    for inner, groups, first, fill in ((257, 1, 0, -1), (1, 7, 3, 0), (35, 5, 174, 2), (256, 3, 767, -1)):
        want, skipped = ec.confusion_loops(pred, lab, 3, inner, groups, first, fill)
        got, got_skipped = ec.confusion_numpy(pred, lab, 3, inner, groups, first, fill)
        np.testing.assert_array_equal(got, want)
        assert got_skipped == skipped


@pytest.mark.parametrize('types', TYPE_PAIRS, ids=lambda t: 'p%d_l%d' % t)
def test_all_one_cell(sess, types):
    """The background-only volume: every element adds to one cell (the worst case for same-address contention)."""
    pt, lt = types
    for n in (4099, 300000):
        for Cn, t, p in ((2, 0, 0), (8, 0, 0), (16, 15, 15), (3, 2, 1)):
            pred, lab = np.full(n, p, dtype=NP_TYPES[pt]), np.full(n, t, dtype=NP_TYPES[lt])
            for inner, groups in ((n, 1), (1, 70), (256, 3)):
                got, skipped = run(sess, pred, lab, pt, lt, 0, inner, groups, Cn, -1)
                want = ec.confusion_numpy(pred, lab, Cn, inner, groups, 0, -1)[0]
                np.testing.assert_array_equal(got, want)
                assert skipped == 0 and got[:, t, p].sum() == n == got.sum()
    # everything skipped: no cell moves
    pred, lab = np.zeros(4099, dtype=NP_TYPES[pt]), np.full(4099, 200, dtype=NP_TYPES[lt])
    got, skipped = run(sess, pred, lab, pt, lt, 0, 1, 7, 3, -1)
    assert not got.any() and skipped == 4099


@pytest.mark.parametrize('types', TYPE_PAIRS, ids=lambda t: 'p%d_l%d' % t)
def test_unaligned_buffers_give_the_aligned_counts(sess, types):
    """Both buffers one element off 16-byte alignment."""
    pt, lt = types
    torch = sess.torch
    rs = np.random.RandomState(31)
    n, Cn = 4099, 3
    pred, lab = draw(rs, n, Cn, pt, lt)
    d_pred = sess.to_device(np.concatenate([pred[:1], pred]), getattr(torch, pred.dtype.name))
    d_lab = sess.to_device(np.concatenate([lab[:1], lab]), getattr(torch, lab.dtype.name))
    assert d_pred.data_ptr() % 16 == 0 and d_lab.data_ptr() % 16 == 0
    for inner, groups, first in ((n, 1, 0), (1, 70, 3), (35, 5, 0)):
        aligned = run(sess, pred, lab, pt, lt, first, inner, groups, Cn, 0)
        g = Guarded(sess, groups * Cn * Cn)
        call(sess, d_pred, pt, d_lab, lt, n, first, inner, groups, Cn, 0, g, off_p=pred.itemsize, off_l=lab.itemsize)
        got = g.read((groups, Cn, Cn))
        np.testing.assert_array_equal(got[0], aligned[0])
        assert got[1] == aligned[1]
        np.testing.assert_array_equal(got[0], ec.confusion_numpy(pred, lab, Cn, inner, groups, first, 0)[0])


def test_three_chunks_equal_one_call_and_the_call_adds(sess):
    torch = sess.torch
    rs = np.random.RandomState(32)
    n, Cn = 4099, 8
    pred, lab = draw(rs, n, Cn, I64, I32)
    d_pred, d_lab = sess.to_device(pred, torch.int64), sess.to_device(lab, torch.int32)
    for inner, groups, first in ((1, 70, 5), (35, 5, 0), (256, 3, 100)):
        whole, skipped = run(sess, pred, lab, I64, I32, first, inner, groups, Cn, -1, d=(d_pred, d_lab))
        g = Guarded(sess, groups * Cn * Cn)
        for a, b in ((0, 1000), (1000, 1017), (1017, n)):          # the second and third chunk start off 16-byte alignment
            call(sess, d_pred, I64, d_lab, I32, b - a, first + a, inner, groups, Cn, -1, g, off_p=a * 8, off_l=a * 4)
        got, got_skipped = g.read((groups, Cn, Cn))
        np.testing.assert_array_equal(got, whole)
        assert got_skipped == skipped
        # non-zero starting counts: the call adds
        start = rs.randint(0, 1 << 40, size=(groups, Cn, Cn)).astype(np.int64)
        got, _ = run(sess, pred, lab, I64, I32, first, inner, groups, Cn, -1, start=start, d=(d_pred, d_lab))
        np.testing.assert_array_equal(got, start + whole)


def test_past_the_capped_grid(sess):
    """n = 3 2^20 + 5 with 70 groups, inputs drawn on the device: more vectors than the grid has lanes."""
    torch = sess.torch
    n, Cn, groups = 3 * 2 ** 20 + 5, 3, 70
    gen = torch.Generator(device=sess.device)
    gen.manual_seed(77)
    lab = torch.randint(-1, Cn, (n,), generator=gen, device=sess.device, dtype=torch.int32)
    pred = torch.randint(0, Cn + 1, (n,), generator=gen, device=sess.device, dtype=torch.int64)
    h_pred, h_lab = pred.cpu().numpy(), lab.cpu().numpy()
    assert n // 4 > 256 * 8 * 256          # vectors of the int64 / int32 call against the lanes of the largest grid
    for pt, lt, dp, dl in ((I64, I32, pred, lab), (U8, U8, pred.to(torch.uint8), lab.to(torch.uint8))):
        hp, hl = dp.cpu().numpy(), dl.cpu().numpy()
        for inner, first, fill in ((1, 3, 0), (4099, 0, -1)):
            g = Guarded(sess, groups * Cn * Cn)
            call(sess, dp, pt, dl, lt, n, first, inner, groups, Cn, fill, g)
            got, skipped = g.read((groups, Cn, Cn))
            want, want_skipped = ec.confusion_numpy(hp, hl, Cn, inner, groups, first, fill)
            np.testing.assert_array_equal(got, want)
            assert skipped == want_skipped > 0
    assert np.array_equal(h_pred, pred.cpu().numpy()) and np.array_equal(h_lab, lab.cpu().numpy())          # inputs are read only


def test_group_windows(sess):
    """groups C^2 cells beyond the kernel's histogram: the launcher walks windows of alq_confusion_window(C) groups."""
    rs = np.random.RandomState(33)
    for Cn, groups, windows in ((3, 1000, 2), (16, 70, 3), (8, 200, 2), (2, 4100, 3)):
        win = sess.lib.alq_confusion_window(Cn)
        assert win >= 1 and (groups + win - 1) // win == windows, (Cn, win)
        n = 4099
        pred, lab = draw(rs, n, Cn, U8, U8)
        assert groups * Cn * Cn > 8192          # more cells than 32 KiB of 32-bit counts
        for inner, first in ((1, 0), (3, groups * 3 - 1)):
            got, skipped = run(sess, pred, lab, U8, U8, first, inner, groups, Cn, -1)
            want, want_skipped = ec.confusion_numpy(pred, lab, Cn, inner, groups, first, -1)
            np.testing.assert_array_equal(got, want)
            assert skipped == want_skipped          # counted once, not once per window
        if windows == 2:
            assert np.any(got[:win]) and np.any(got[win:])          # both windows hold counts


def test_two_identical_calls_give_identical_bits(sess):
    rs = np.random.RandomState(34)
    n, Cn = 300000, 8
    pred, lab = draw(rs, n, Cn, I64, I32)
    a = run(sess, pred, lab, I64, I32, 7, 1, 70, Cn, 0)
    b = run(sess, pred, lab, I64, I32, 7, 1, 70, Cn, 0)
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    np.testing.assert_array_equal(a[0], ec.confusion_numpy(pred, lab, Cn, 1, 70, 7, 0)[0])


def test_n_zero_does_nothing(sess):
    torch = sess.torch
    d_pred, d_lab = sess.to_device(np.zeros(16, np.int64), torch.int64), sess.to_device(np.zeros(16, np.int32), torch.int32)
    g = Guarded(sess, 7 * 9)
    call(sess, d_pred, I64, d_lab, I32, 0, 0, 1, 7, 3, 0, g)
    assert g.untouched()


def test_refused_calls_leave_the_outputs_untouched(sess):
    torch = sess.torch
    L = sess.lib
    d_pred, d_lab = sess.to_device(np.zeros(64, np.int64), torch.int64), sess.to_device(np.zeros(64, np.int32), torch.int32)
    g = Guarded(sess, 7 * 9)
    ok = dict(pred=_ptr(d_pred), pt=I64, lab=_ptr(d_lab), lt=I32, n=64, first=0, inner=1, groups=7, C=3, fill=0,
              counts=g.counts_ptr(), skipped=g.skipped_ptr())
    bad = [dict(pred=None), dict(lab=None), dict(counts=None), dict(pt=3), dict(pt=-1), dict(lt=3), dict(C=0), dict(C=17), dict(inner=0),
           dict(groups=0), dict(n=-1), dict(first=-1), dict(pred=_ptr(d_pred, 4)), dict(lab=_ptr(d_lab, 2)), dict(counts=_ptr(g.buf, GUARD * 8 + 4))]
    sess.bind_stream()
    for change in bad:
        a = dict(ok, **change)
        rc = L.alq_confusion_counts(sess.ctx, a['pred'], a['pt'], a['lab'], a['lt'], a['n'], a['first'], a['inner'], a['groups'], a['C'],
                                    a['fill'], a['counts'], a['skipped'])
        assert rc == -1, change
        assert L.alq_last_error().decode().startswith('alq_confusion_counts'), change
    assert L.alq_confusion_counts(None, ok['pred'], I64, ok['lab'], I32, 64, 0, 1, 7, 3, 0, ok['counts'], ok['skipped']) == -1
    sess.torch.cuda.synchronize()
    assert g.untouched()
    # the same arguments unchanged are accepted
    assert L.alq_confusion_counts(sess.ctx, ok['pred'], I64, ok['lab'], I32, 64, 0, 1, 7, 3, 0, ok['counts'], ok['skipped']) == 0
    got, skipped = g.read((7, 3, 3))
    assert got[:, 0, 0].tolist() == [10, 9, 9, 9, 9, 9, 9] and got.sum() == 64 and skipped == 0


def test_session_method(sess):
    """DeviceSession.confusion_counts: device tensors in, device tensors out, `counts` accumulates."""
    torch = sess.torch
    rs = np.random.RandomState(35)
    pred, lab = draw(rs, 3 * 16 * 16, 3, I64, I32)
    d_pred, d_lab = sess.to_device(pred.reshape(3, 16, 16), torch.int64), sess.to_device(lab.reshape(3, 16, 16), torch.int32)
    whole = sess.confusion_counts(d_pred, d_lab, 3, fill=0)
    assert whole.is_cuda and whole.dtype == torch.int64 and tuple(whole.shape) == (1, 3, 3)
    np.testing.assert_array_equal(whole.cpu().numpy(), ec.confusion_numpy(pred, lab, 3, len(pred), 1, 0, 0)[0])
    per, skipped = sess.confusion_counts(d_pred, d_lab, 3, inner=256, groups=3, want_skipped=True)
    want, want_skipped = ec.confusion_numpy(pred, lab, 3, 256, 3, 0, -1)
    np.testing.assert_array_equal(per.cpu().numpy(), want)
    assert int(skipped.cpu()[0]) == want_skipped
    again = sess.confusion_counts(d_pred, d_lab, 3, inner=256, groups=3, counts=per)
    assert again is per
    np.testing.assert_array_equal(per.cpu().numpy(), 2 * want)
