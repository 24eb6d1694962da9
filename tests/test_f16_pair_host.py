"""csrc/f16_pair.h - the fp16-pair split and the scale exponent every host weight packer of the layer kernels calls - against a
NumPy restatement of the statement sequence the packers had, without a GPU: tests/host/f16_pair_main.cpp (its own main) is
compiled as plain C++ under the address and undefined-behaviour sanitizers and run as a child process.  The header needs
_Float16, so the compiler is the clang++ that ships with ROCm (the one hipcc drives).  Comparison is by exact bits."""
import os
import shutil
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'nn-active-learning_amd', 'csrc')


def _rocm_clangxx():
    cands = []
    hipcc = shutil.which('hipcc')
    if hipcc:
        rocm = os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))
        cands += [os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++')]
    for rocm in (os.environ.get('ROCM_PATH'), '/opt/rocm'):
        if rocm:
            cands += [os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++'), os.path.join(rocm, 'llvm', 'bin', 'clang++')]
    for c in cands:
        if os.path.isfile(c) and os.access(c, os.X_OK):
            return c
    raise AssertionError('no ROCm clang++ among %r' % cands)


def _f32(x):
    return np.asarray(x, dtype=np.float32)


def _ref_split(w, e, shift):
    """ws = fp32(w 2^e); h = fp16(ws); l = fp16(fp32(fp32(ws - fp32(h)) 2^shift)): round to nearest even, subnormals kept."""
    ws = np.ldexp(_f32(w), e).astype(np.float32)
    h = ws.astype(np.float16)
    rem = (ws - h.astype(np.float32)).astype(np.float32)
    lo = np.ldexp(rem, shift).astype(np.float32).astype(np.float16)
    return h.view(np.uint16), lo.view(np.uint16)


def _ref_exp(w):
    amax = np.float32(np.max(np.abs(_f32(w)))) if len(w) else np.float32(0)
    ex = int(np.frexp(amax)[1]) if amax > 0 else 0
    return 14 - ex


def _arrays():
    """(name, array, expected exponent).  The first array's maximum is 1.0, so e = 13 and the scaled values ws below
    are what the comments say; every w = ws 2^-13 is exact in fp32."""
    s = np.float32(2.0) ** -13
    ws = [
        0.0, -0.0,
        8192.0,                                   # the maximum itself: [2^13, 2^14)
        # ws on an fp16 rounding tie (ulp 8 in [2^13, 2^14), 2^-10 in [1, 2)): down to even, up to even
        8192.0 + 4.0, 8192.0 + 12.0, 16384.0 - 4.0 - 8.0, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 2.0 ** -13 + 2.0 ** -24,
        # l an fp16 subnormal at shift 0 (|ws - h| < 2^-14), normal at shift 11: exact, rounded down, on a subnormal tie, rounded to zero
        1.0 + 2.0 ** -15, 1.0 + 2.0 ** -15 + 2.0 ** -23, 2.0 ** -3 + 2.0 ** -17 + 2.0 ** -26, 2.0 ** -3 + 2.0 ** -17 + 2.0 ** -25,
        2.0 ** -3 + 3 * 2.0 ** -25, 2.0 ** -6 + 2.0 ** -26, 3.0 + 2.0 ** -14 - 2.0 ** -22,
        # h an fp16 subnormal (ws < 2^-14): exact, remainder below the quantum 2^-24, ties at half a quantum, the largest subnormal
        3 * 2.0 ** -24, 3 * 2.0 ** -24 + 2.0 ** -26, 2.0 ** -25, 3 * 2.0 ** -25, 2.0 ** -26, 1023 * 2.0 ** -24 + 2.0 ** -25, 2.0 ** -14 - 2.0 ** -26,
    ]
    special = _f32(ws) * s
    special = np.concatenate([special, -special])
    draws = np.random.RandomState(20240611).normal(0.0, 0.1, 4096).astype(np.float32)
    assert np.abs(draws).max() < 1.0
    out = [('specials and draws', np.concatenate([special, draws]), 13)]
    out.append(('all zero', _f32([0.0, -0.0, 0.0]), 14))
    for k in (-126, -20, -1, 0, 1, 13, 14, 15, 100, 127):      # max |w| = 2^k -> frexp exponent k + 1
        out.append(('2^%d' % k, _f32([np.ldexp(np.float32(1), k), -np.ldexp(np.float32(0.75), k), 0.0]), 13 - k))
    out.append(('just below 2^0', _f32([np.nextafter(np.float32(1), np.float32(0)), 0.25]), 14))
    out.append(('fp32 subnormal maximum', _f32([np.ldexp(np.float32(1), -149), -np.ldexp(np.float32(1), -149)]), 14 + 148))
    out.append(('larger fp32 subnormal maximum', _f32([np.ldexp(np.float32(3), -140), np.ldexp(np.float32(1), -149)]), 14 + 138))
    return out


def test_split_and_exponent_match_the_packers_statement_sequence(tmp_path):
    exe = str(tmp_path / 'f16_pair_main')
    subprocess.check_call([_rocm_clangxx(), '-x', 'c++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I', CSRC, os.path.join(ROOT, 'tests', 'host', 'f16_pair_main.cpp'), '-o', exe])
    arrays = _arrays()
    text = ''.join(' '.join('%08x' % b for b in a.view(np.uint32)) + '\n' for _, a, _ in arrays)
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split('\n')
    pos = 0
    for name, a, want_e in arrays:
        assert lines[pos].startswith('e '), (name, lines[pos])
        e = int(lines[pos][2:])
        assert e == _ref_exp(a) and e == want_e, (name, e, _ref_exp(a), want_e)
        got = np.array([[int(t, 16) for t in ln.split()] for ln in lines[pos + 1:pos + 1 + len(a)]], dtype=np.uint16).reshape(len(a), 4)
        pos += 1 + len(a)
        for col, shift in ((0, 0), (2, 11)):
            h, lo = _ref_split(a, e, shift)
            bad = np.flatnonzero((got[:, col] != h) | (got[:, col + 1] != lo))
            assert bad.size == 0, (name, shift, [(float(a[i]), hex(got[i, col]), hex(h[i]), hex(got[i, col + 1]), hex(lo[i])) for i in bad[:5]])
    assert lines[pos:] == [''], lines[pos:pos + 3]
    # the special inputs are what their comments say (a restatement that agreed with the header on the easy cases only would pass otherwise)
    a = arrays[0][1]
    h0, l0 = _ref_split(a, 13, 0)
    _, l11 = _ref_split(a, 13, 11)

    def sub(b):      # an fp16 subnormal
        return (b & 0x7c00) == 0 and (b & 0x03ff) != 0
    assert sum(sub(int(b)) for b in h0[:46]) >= 6                                                 # hi pieces that are subnormal
    assert sum(sub(int(x)) and not sub(int(y)) and (int(y) & 0x7fff) != 0 for x, y in zip(l0[:46], l11[:46])) >= 10      # lo: subnormal at shift 0, normal at 11
    assert h0[2] == np.float16(8192).view(np.uint16) and h0[3] == h0[2] and h0[4] == np.float16(8208).view(np.uint16)      # ties go to even
