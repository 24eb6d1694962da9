"""csrc/weight_layout.h - the norms, layout maps and the two-class head's difference vector that weight setting
(csrc/weights.hip) computes on the host - against a NumPy restatement, without a GPU: tests/host/weight_layout_main.cpp (its
own main) is compiled as plain C++ under the address and undefined-behaviour sanitizers and run as a child process.  The fp64
sums are restated as sequential additions in the header's order (np.cumsum, not np.sum: pairwise sums give other bits).
Every comparison is by exact bits."""
import os
import subprocess

import numpy as np
import pytest

from tests.test_f16_pair_host import CSRC, ROOT, _ref_split, _rocm_clangxx

F32 = np.float32
SCALE = 1.0 + 1e-6


def _hex(a):
    return ' '.join('%08x' % b for b in np.ascontiguousarray(a, dtype=F32).reshape(-1).view(np.uint32)) + '\n'


def _bits32(a):
    return np.ascontiguousarray(a, dtype=F32).reshape(-1).view(np.uint32)


def _line32(ln):
    return np.array([int(t, 16) for t in ln.split()], dtype=np.uint32)


def _seq_sum(a):
    """fp64 sum of a 1-d array, added one term after the other."""
    return np.cumsum(np.asarray(a, dtype=np.float64))[-1]


def _draw(seed, shape, big=None):
    """Seeded normal draws; `big`: the index of one element set to 100 (every maximum is then attained where it sits)."""
    w = np.random.RandomState(seed).normal(0.0, 0.1, shape).astype(F32)
    if big is not None:
        w[big] = F32(-100.0)
    return w


def _ref_norms(W_tcico, b):
    """W in logical (tap, ci, co) order.  Sum of a ci: taps outer, co inner; sum of a co: taps outer, ci inner."""
    a = np.abs(W_tcico.astype(np.float64))
    s_in = [_seq_sum(a[:, ci, :].reshape(-1)) for ci in range(a.shape[1])]
    s_out = [_seq_sum(a[:, :, co].reshape(-1)) for co in range(a.shape[2])]
    bm = np.abs(b.astype(np.float64)).max()
    return np.float64(max(s_in)), F32(np.float64(max(s_out)) * SCALE), F32(bm * SCALE), s_in, s_out


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('weight_layout') / 'weight_layout_main')
    subprocess.check_call([_rocm_clangxx(), '-x', 'c++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I', CSRC, os.path.join(ROOT, 'tests', 'host', 'weight_layout_main.cpp'), '-o', path])
    return path


def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split('\n')
    assert lines[-1] == ''
    return lines[:-1]


def test_conv_norms_and_backward_matrix(exe):
    """conv W[tap][ci][co], 3x3x3 taps, Ci = 3, Co = 5; the second array's maxima sit at ci = 1 and co = 3, bias 2."""
    nt, Ci, Co = 27, 3, 5
    cases = [(_draw(1, (nt, Ci, Co)), _draw(2, (Co,)), None, None),
             (_draw(3, (nt, Ci, Co), big=(14, 1, 3)), _draw(4, (Co,), big=(2,)), 1, 3)]
    text = ''
    for W, b, _, _ in cases:
        text += 'conv 0 %d %d %d\n' % (nt, Ci, Co) + _hex(W) + _hex(b) + 'taps %d %d %d\n' % (Ci, Co, nt) + _hex(W)
    lines = _run(exe, text)
    assert len(lines) == 2 * len(cases)
    for i, (W, b, ci_max, co_max) in enumerate(cases):
        bwd, out, bmax, s_in, s_out = _ref_norms(W, b)
        got = lines[2 * i].split()
        assert int(got[0], 16) == int(bwd.view(np.uint64)), (i, got[0], bwd)
        assert int(got[1], 16) == int(out.view(np.uint32)) and int(got[2], 16) == int(bmax.view(np.uint32)), (i, got, out, bmax)
        if ci_max is not None:
            assert int(np.argmax(s_in)) == ci_max and int(np.argmax(s_out)) == co_max
            assert bmax == F32(100.0 * SCALE) and int(np.argmax(np.abs(b))) == 2
        # B_bwd[(tap, co)][ci] = W[(tap, ci)][co]
        assert np.array_equal(_line32(lines[2 * i + 1]), _bits32(W.transpose(0, 2, 1))), i


def test_output_channel_slices(exe):
    """columns [j w, (j + 1) w) of the forward B [(tap, ci)][co]: 3x3x3 taps, Ci = 2, Co = 6, slices of width 2."""
    nt, Ci, Co, w = 27, 2, 6, 2
    B = _draw(5, (nt * Ci, Co))
    lines = _run(exe, ''.join('slice %d %d %d %d\n' % (nt * Ci, Co, j, w) + _hex(B) for j in range(Co // w)))
    assert len(lines) == Co // w
    for j in range(Co // w):
        assert np.array_equal(_line32(lines[j]), _bits32(B[:, j * w:(j + 1) * w])), j


def test_conv_transpose_norms_full_and_class_matrices(exe):
    """conv_transpose W[tap][co][ci], 2x2x2 taps, Ci = 3, Co = 2: norms over all taps, Bfull[(tap, ci)][co] and the per-class
    gathers of the tap lists [0, 3, 5] and [7]; the second array's maxima sit at ci = 2 and co = 1."""
    nt, Ci, Co = 8, 3, 2
    cases = [(_draw(6, (nt, Co, Ci)), _draw(7, (Co,)), None, None),
             (_draw(8, (nt, Co, Ci), big=(5, 1, 2)), _draw(9, (Co,), big=(0,)), 2, 1)]
    tap_lists = [[0, 3, 5], [7]]
    text = ''
    for W, b, _, _ in cases:
        text += 'conv 1 %d %d %d\n' % (nt, Ci, Co) + _hex(W) + _hex(b) + 'taps %d %d %d\n' % (Co, Ci, nt) + _hex(W)
        for tl in tap_lists:
            text += 'taps %d %d %d %s\n' % (Co, Ci, len(tl), ' '.join(map(str, tl))) + _hex(W)
    lines = _run(exe, text)
    per = 2 + len(tap_lists)
    assert len(lines) == per * len(cases)
    for i, (W, b, ci_max, co_max) in enumerate(cases):
        bwd, out, bmax, s_in, s_out = _ref_norms(W.transpose(0, 2, 1), b)
        got = lines[per * i].split()
        assert int(got[0], 16) == int(bwd.view(np.uint64)), (i, got[0], bwd)
        assert int(got[1], 16) == int(out.view(np.uint32)) and int(got[2], 16) == int(bmax.view(np.uint32)), (i, got, out, bmax)
        if ci_max is not None:
            assert int(np.argmax(s_in)) == ci_max and int(np.argmax(s_out)) == co_max and int(np.argmax(np.abs(b))) == 0
        assert np.array_equal(_line32(lines[per * i + 1]), _bits32(W.transpose(0, 2, 1))), i
        for k, tl in enumerate(tap_lists):
            assert np.array_equal(_line32(lines[per * i + 2 + k]), _bits32(W[tl].transpose(0, 2, 1))), (i, tl)


def _head_weights(seed, Co, F, big=None):
    """fc weights W[o][f_tf].  Co = 2: W0 - W1 holds an exact zero, the maximum 1.5 (so e = 13 and ws = wv 2^13) and values
    whose ws lies on an fp16 rounding tie (ulp 8 in [2^13, 2^14), 2^-10 in [1, 2)), to either side."""
    W = _draw(seed, (Co, F), big=big)
    if Co == 2 and big is None:
        s = F32(2.0) ** -13
        W[0, 5], W[1, 5] = F32(0.0625), F32(0.0625)                         # wv = 0
        W[0, 9], W[1, 9] = F32(0.75), F32(-0.75)                            # wv = 1.5, the maximum
        W[0, 14], W[1, 14] = F32(8196.0) * s, F32(0.0)                      # tie, down to even
        W[0, 22], W[1, 22] = F32(0.0), F32(8204.0) * s                      # tie, up to even (negative)
        W[0, 31], W[1, 31] = F32(1.0 + 2.0 ** -11) * s, F32(-0.0)           # tie in [1, 2)
    return W


@pytest.mark.parametrize('Co', [2, 5])
def test_fc_reorder_transpose_norm_and_head_vector(exe, Co):
    """fc W[o][f_tf] with (D, H, W, C) = (2, 3, 2, 3): Wp[o][f_mem], its transpose B[f_mem][o], the column norm; Co = 2: the
    head's W0 - W1, its maximum and the fp16-pair pre-split [h0 h1 | h2 h3 | l0 l1 | l2 l3] (F = 36, a multiple of 4)."""
    D, H, Wd, C = 2, 3, 2, 3
    F = D * H * Wd * C
    cases = [_head_weights(10 + Co, Co, F), _head_weights(20 + Co, Co, F, big=(Co - 1, 17))]
    lines = _run(exe, ''.join('fc %d %d %d %d %d\n' % (Co, D, H, Wd, C) + _hex(W) for W in cases))
    per = 3 + (4 if Co == 2 else 0)
    assert len(lines) == per * len(cases)
    for i, W in enumerate(cases):
        ln = lines[per * i:per * (i + 1)]
        # f_tf = ((c*W+w)*H+h)*D+d -> f_mem = ((d*H+h)*W+w)*C+c
        Wp = np.ascontiguousarray(W.reshape(Co, C, Wd, H, D).transpose(0, 4, 3, 2, 1)).reshape(Co, F)
        assert np.array_equal(_line32(ln[0]), _bits32(Wp)), i
        assert np.array_equal(_line32(ln[1]), _bits32(Wp.T)), i
        col = np.cumsum(np.abs(W.astype(np.float64)), axis=0)[-1]          # per column, o = 0 first
        assert int(ln[2], 16) == int(np.float64(col.max()).view(np.uint64)), i
        if i == 1:
            assert int(np.argmax(col)) == 17
        if Co != 2:
            continue
        wv = ((F32(0.0) + Wp[0]) - Wp[1]).astype(F32)
        amax = F32(np.abs(wv).max())
        assert np.array_equal(_line32(ln[3]), _bits32(wv)), i
        assert int(ln[4], 16) == int(amax.view(np.uint32)), i
        e = 14 - int(np.frexp(amax)[1])
        assert ln[5] == 'e %d' % e
        h, lo = _ref_split(wv, e, 11)
        h, lo = h.astype(np.uint32).reshape(-1, 4), lo.astype(np.uint32).reshape(-1, 4)
        words = np.stack([h[:, 0] | (h[:, 1] << 16), h[:, 2] | (h[:, 3] << 16), lo[:, 0] | (lo[:, 1] << 16), lo[:, 2] | (lo[:, 3] << 16)], axis=1)
        assert np.array_equal(_line32(ln[6]), words.reshape(-1)), i
        if i == 0:      # the special values are what _head_weights says
            tf = lambda f: np.ravel_multi_index(np.unravel_index(f, (C, Wd, H, D))[::-1], (D, H, Wd, C))  # noqa: E731
            assert e == 13 and amax == F32(1.5) and wv[tf(5)] == 0 and wv[tf(9)] == 1.5
            f16 = lambda v: int(np.float16(v).view(np.uint16))  # noqa: E731
            hh = h.reshape(-1)
            assert hh[tf(14)] == f16(8192.0) and hh[tf(22)] == f16(-8208.0) and hh[tf(31)] == f16(1.0)
            assert hh[tf(9)] == f16(12288.0) and hh[tf(5)] == 0 and lo.reshape(-1)[tf(5)] == 0
