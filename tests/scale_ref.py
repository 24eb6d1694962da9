"""Plain NumPy references for the fp16-pair scale logic (tests/test_scale_ref_host.py, tests/test_gpu_scale_ranges.py).

rescale       the same network under other magnitudes: layer j's W and b times 2^k, the input-channel slice of every consumer of
              its output times 2^-k (ReLU and max-pool are positively homogeneous, a power of two changes only exponents)
l1_chain      the bound chain of weight_layout.h::conv_norms + passes.hip::fwd_bounds_args + kernels.hip::fwd_bounds_kernel in fp64
tight_input   the patch that attains the first layer's L1 bound at one interior voxel
"""
from collections import OrderedDict

import numpy as np

from oracle import netspec

TINY = float(np.finfo(np.float32).tiny)


def layer_types(ld):
    ext = netspec.is_extended(ld)
    return [(spec[0] if ext else spec[1]) for spec in ld.values()]


def skip_src_of(ld, skips):
    """Per layer: the index of the layer whose output is concatenated IN FRONT of its input, or -1."""
    src2 = [-1] * len(ld)
    for (src, dsts, kind) in skips:
        assert kind == 'con', 'only concatenating skips rescale by slices'
        for d in dsts:
            assert src2[d] < 0
            src2[d] = src
    return src2


def out_channels(pars, ld, idx):
    """The channels of layer idx's output, from the weights (a pool keeps its producer's)."""
    names, types = list(ld), layer_types(ld)
    while types[idx] == 'pool':
        idx -= 1
        assert idx >= 0
    W = pars[names[idx]][0]
    return W.shape[-1] if types[idx] == 'conv' else (W.shape[-2] if types[idx] == 'conv_transpose' else W.shape[0])


def _scaled(a, k):
    """a * 2^k, asserted to change nothing but exponents: no entry leaves the normal range, every mantissa stays."""
    a = np.asarray(a)
    with np.errstate(over="ignore", under="ignore"):
        b = np.ldexp(a, k).astype(a.dtype)
    nz = a != 0
    tiny = float(np.finfo(a.dtype).tiny)
    assert np.isfinite(b).all() and (np.abs(b[nz]) >= tiny).all() and (np.abs(a[nz]) >= tiny).all(), 'an entry left the normal range'
    ma, ea = np.frexp(a)
    mb, eb = np.frexp(b)
    assert np.array_equal(ma, mb) and np.array_equal(eb[nz], ea[nz] + k), 'more than the exponent changed'
    return b


def consumers(ld, skips, layer):
    """[(index of a parameterised layer, 'main' | 'skip')]: every input slice that reads the output of `layer` (a name, or 'input'),
    through any number of max-pools."""
    names, types, src2 = list(ld), layer_types(ld), skip_src_of(ld, skips)
    j = -1 if layer == 'input' else names.index(layer)
    assert j < 0 or types[j] != 'pool'
    carry = {j}                       # layers (or -1: the input) whose output carries the factor
    found = []
    for i in range(j + 1, len(names)):
        main = (i - 1) in carry
        if types[i] == 'pool':
            assert src2[i] < 0
            if main:
                carry.add(i)
            continue
        if main:
            found.append((i, 'main'))
        if src2[i] in carry and src2[i] >= 0:
            found.append((i, 'skip'))
    assert found or j == len(names) - 1
    return found


def rescale(pars, ld, skips, layer, k):
    """(pars', kx): the same function as (pars, x) when evaluated on x * 2^kx.  layer = a parameterised layer's name: its W and b
    times 2^k, the slices of its consumers times 2^-k, kx = 0; layer = 'input': kx = k and the first layer's W times 2^-k, its bias
    untouched.  TF layouts: conv [k.., ci, co], conv_transpose [k.., co, ci], fc [co, features]; a concat puts the skip source's
    channels first."""
    names, types, src2 = list(ld), layer_types(ld), skip_src_of(ld, skips)
    out = OrderedDict((n, [np.array(W), np.array(b)]) for n, (W, b) in pars.items())
    if layer != 'input':
        out[layer][0] = _scaled(out[layer][0], k)
        out[layer][1] = _scaled(out[layer][1], k)
    for i, part in consumers(ld, skips, layer):
        W = out[names[i]][0]
        if src2[i] < 0:
            assert part == 'main'
            sl = slice(None)
        else:
            assert types[i] != 'fc'
            nskip = out_channels(pars, ld, src2[i])
            sl = slice(0, nskip) if part == 'skip' else slice(nskip, None)
        if types[i] == 'conv':
            W[..., sl, :] = _scaled(W[..., sl, :], -k)
        elif types[i] == 'conv_transpose':
            W[..., sl] = _scaled(W[..., sl], -k)
        else:
            assert types[i] == 'fc'
            W[...] = _scaled(W, -k)
    return out, (k if layer == 'input' else 0)


def conv_norms(W, b, transposed):
    """(bwd_l1, out_l1, out_bmax) of weight_layout.h::conv_norms: fp64 sums, the two forward norms times 1 + 1e-6 and rounded to float."""
    a = np.abs(np.asarray(W, np.float64))
    ci_ax, co_ax = (a.ndim - 1, a.ndim - 2) if transposed else (a.ndim - 2, a.ndim - 1)
    per_ci = a.sum(axis=tuple(d for d in range(a.ndim) if d != ci_ax))
    per_co = a.sum(axis=tuple(d for d in range(a.ndim) if d != co_ax))
    bm = np.abs(np.asarray(b, np.float64)).max()
    return float(per_ci.max()), float(np.float32(per_co.max() * (1.0 + 1e-6))), float(np.float32(bm * (1.0 + 1e-6)))


def bounds_args(pars, ld, skips):
    """(L, B, src2) per layer as passes.hip::fwd_bounds_args fills them: a pool and an fc layer pass the bound on."""
    types, src2 = layer_types(ld), skip_src_of(ld, skips)
    L, B = [], []
    for name, t in zip(ld, types):
        if t in ('conv', 'conv_transpose'):
            _, l1, bm = conv_norms(pars[name][0], pars[name][1], t == 'conv_transpose')
            L.append(l1)
            B.append(bm)
        else:
            L.append(1.0)
            B.append(0.0)
    return np.array(L), np.array(B), src2


def chain(amax, L, B, src2, from_input):
    """bound [nl, N] in fp64: kernels.hip::fwd_bounds_kernel."""
    amax = np.asarray(amax, np.float64)
    b = [amax * L[0] + B[0] if from_input else amax.copy()]
    for k in range(1, len(L)):
        x = b[k - 1]
        if src2[k] >= 0:
            x = np.maximum(x, b[src2[k]])
        b.append(x * L[k] + B[k])
    return np.stack(b)


def l1_chain(pars, ld, skips, amax, from_input):
    """Per layer and patch, the bound on max |output| that the device derives from `amax` [N]: the measured maxima of layer 0's
    output, or (from_input) of the network input."""
    L, B, src2 = bounds_args(pars, ld, skips)
    return chain(amax, L, B, src2, from_input)


def tight_input(W, b, amax, shape):
    """(x [*shape], voxel, co): zero but for one window around the interior voxel `voxel` = shape // 2, where it is
    amax * sign(W[.., co]) * sign(b[co]) with co the output channel of the largest L1 norm: the pre-activation of a SAME conv
    (cross-correlation, odd kernel) at that voxel is sign(b[co]) * (amax * sum |W[.., co]| + |b[co]|)."""
    W = np.asarray(W)
    nd = W.ndim - 2
    assert len(shape) == nd + 1 and shape[-1] == W.shape[-2] and all(kk % 2 == 1 for kk in W.shape[:nd])
    co = int(np.abs(W.astype(np.float64)).sum(axis=tuple(range(nd + 1))).argmax())
    sb = -1.0 if np.asarray(b).ravel()[co] < 0 else 1.0
    x = np.zeros(shape, np.float32)
    voxel = tuple(s // 2 for s in shape[:nd])
    win = tuple(slice(v - kk // 2, v + kk // 2 + 1) for v, kk in zip(voxel, W.shape[:nd]))
    assert all(s.start >= 0 and s.stop <= n for s, n in zip(win, shape))
    sg = np.where(W[..., co] < 0, -1.0, 1.0)
    x[win] = (np.float32(amax) * sg * sb).astype(np.float32)
    return x, voxel, co
