"""csrc/model_plan.h - the shape pass of model creation (SAME pads, skip topology, head rules, batch caps, every rejection) and the
geometry descriptors of every contraction - against restatements in Python, without a GPU: tests/host/model_plan_main.cpp (its
own main and its own set_error) is compiled as plain C++ under the address and undefined-behaviour sanitizers and run as a child
process.  Expected values come from device.tf_param_shapes / device.out_map_shape, from TensorFlow's SAME rule and from the layers'
definitions enumerated by brute force here - never from the header."""
import itertools
import os
import re
import subprocess
from collections import OrderedDict

import numpy as np
import pytest

import nnal_amd  # noqa: F401
from nnal_amd import device, netspec
from tests.test_f16_pair_host import CSRC, ROOT, _rocm_clangxx

CONV, CONVT, POOL, FC = 0, 1, 2, 3
OK, EINVAL, EUNSUPPORTED = 0, -1, -4
INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp('model_plan') / 'model_plan_main')
    subprocess.check_call([_rocm_clangxx(), '-x', 'c++', '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined',
                           '-fno-sanitize-recover=all', '-I', CSRC, '-I', os.path.join(ROOT, 'include'),
                           os.path.join(ROOT, 'tests', 'host', 'model_plan_main.cpp'), '-o', path])
    return path


def _run(exe, text):
    r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split('\n')
    assert lines[-1] == ''
    return lines[:-1]


def _ly(type_, cout=0, k=1, s=1, relu=0, skip=-1):
    k3 = lambda v: [v] * 3 if isinstance(v, int) else list(v)  # noqa: E731
    return dict(type=type_, cout=cout, k=k3(k), s=k3(s), relu=relu, skip_src=skip)


def _dims4(in_shape):
    return [1] * (4 - len(in_shape)) + [int(v) for v in in_shape]


def _plan_text(layers, in_dims, max_batch, descs=0):
    text = 'plan %d %d %d %d %d %d %d\n' % ((max_batch,) + tuple(in_dims) + (len(layers), descs))
    for d in layers:
        text += '%d %d %d %d %d %d %d %d %d %d\n' % ((d['type'], d['cout']) + tuple(d['k']) + tuple(d['s']) + (d['relu'], d['skip_src']))
    return text


def _parse_plans(lines):
    """[(rc, message, model tuple or None, layer rows, desc rows, geom rows)] of consecutive plan outputs."""
    plans = []
    for ln in lines:
        tok = ln.split(' ')
        if tok[0] == 'rc':
            plans.append(dict(rc=int(tok[1]), msg=ln.split(' ', 2)[2], model=None, layers=[], desc=[], geom=[]))
        elif tok[0] == 'model':
            plans[-1]['model'] = tuple(int(t) for t in tok[1:])
        elif tok[0] == 'layer':
            v = [int(t) for t in tok[1:]]
            plans[-1]['layers'].append(dict(i=v[0], inp=tuple(v[1:5]), out=tuple(v[5:9]), lo=tuple(v[9:12]), pidx=v[12], w=v[13], b=v[14], F=v[15],
                                            src=v[16], dest=v[17]))
        elif tok[0] == 'desc':
            v = [int(t) for t in tok[3:]]
            nt = v[16]
            taps = [tuple(v[17 + 3 * j:20 + 3 * j]) for j in range(nt)]
            idx = v[17 + 3 * nt:]
            assert len(idx) in (0, nt)
            plans[-1]['desc'].append(dict(name=tok[1], i=int(tok[2]), I=tuple(v[0:4]), O=tuple(v[4:8]), M=tuple(v[8:11]), sm=v[11], so=v[12],
                                          ooff=tuple(v[13:16]), taps=taps, idx=idx or list(range(nt))))
        elif tok[0] == 'geom':
            v = [int(t) for t in tok[3:]]
            plans[-1]['geom'].append(dict(name=tok[1], i=int(tok[2]), kind=v[0], cls=tuple(v[1:4]), I=tuple(v[4:8]), O=tuple(v[8:12]),
                                          k=tuple(v[12:15]), s=tuple(v[15:18]), lo=tuple(v[18:21]), flipped=v[21]))
        else:
            raise AssertionError(ln)
    return plans


# ---- restatements ------------------------------------------------------------------------------------------------------------
def _tf_same(n, k, s):
    """TensorFlow's SAME rule: output size and pad-before (the smaller half of the total) of size n, window k, stride s."""
    out = -(-n // s)
    total = max((out - 1) * s + k - n, 0)
    return out, total // 2


def _ref_shapes(layers, in_dims):
    """Per layer (input shape incl. concatenated channels, output shape), (D, H, W, C)."""
    cur, outs, res = tuple(in_dims), [], []
    for d in layers:
        inp = cur if d['skip_src'] < 0 else cur[:3] + (cur[3] + outs[d['skip_src']][3],)
        if d['type'] == CONV:
            out = inp[:3] + (d['cout'],)
        elif d['type'] == CONVT:
            out = tuple(a * b for a, b in zip(inp[:3], d['s'])) + (d['cout'],)
        elif d['type'] == POOL:
            out = tuple(-(-a // b) for a, b in zip(inp[:3], d['s'])) + (inp[3],)
        else:
            out = (1, 1, 1, d['cout'])
        res.append((inp, out))
        outs.append(out)
        cur = out
    return res


def _ref_lo(d, inp):
    if d['type'] == CONVT:      # the pads of the strided conv it transposes, whose input is this layer's output
        return tuple(_tf_same(n * s, k, s)[1] for n, k, s in zip(inp[:3], d['k'], d['s']))
    if d['type'] == FC:
        return (0, 0, 0)
    return tuple(_tf_same(n, k, s)[1] for n, k, s in zip(inp[:3], d['k'], d['s']))


def _ref_cap(layers, in_dims):
    """(2^30 - 64) // the floats per patch of the largest allocation: the input, a layer's output, or a concat's two producers together."""
    shp = _ref_shapes(layers, in_dims)
    worst = int(np.prod(in_dims))
    for i, d in enumerate(layers):
        worst = max(worst, int(np.prod(shp[i][1])))
        if d['skip_src'] >= 0:
            src = shp[d['skip_src']][1]
            worst = max(worst, int(np.prod(src[:3])) * (src[3] + shp[i - 1][1][3]))
    return (2 ** 30 - 64) // worst


def _nets():
    """(name, layers in alq_layer_t terms, in_shape)."""
    out = []
    for name, net, in_shape in [('net_a', netspec.net_a(), (32, 32, 1)), ('net_b', netspec.net_b(), (25, 25, 2)),
                                ('net_c_32', netspec.net_c(), (32, 32, 32, 1)), ('net_c_8', netspec.net_c(), (8, 8, 8, 1)),
                                ('net_c_2d', netspec.net_c_2d(), (16, 16, 1)), ('net_c_dense', netspec.net_c_dense(), (16, 16, 16, 1)),
                                ('net_c_2d_dense', netspec.net_c_2d_dense(), (16, 16, 1))]:
        ld, sk = net if isinstance(net, tuple) else (net, ())
        out.append((name, device.translate_layers(ld, in_shape, sk), in_shape))
    odd = OrderedDict([('c', ['conv', [4, [3, 3, 3]], 'MA']), ('p', ['pool', [2, 2, 2]]), ('fc', ['fc', [2]])])
    out.append(('odd_pool', device.translate_layers(odd, (5, 7, 9, 1)), (5, 7, 9, 1)))      # SAME pooling rounds up: 3 x 4 x 5
    return out


NETS = _nets()


@pytest.fixture(scope='module')
def net_plans(exe):
    """Every net planned three times: asked for the largest int (the cap shows), for 7, and for 4096; descriptors with the first."""
    text = ''.join(_plan_text(ly, _dims4(sh), INT_MAX, 1) + _plan_text(ly, _dims4(sh), 7) + _plan_text(ly, _dims4(sh), 4096) for _, ly, sh in NETS)
    plans = _parse_plans(_run(exe, text))
    assert len(plans) == 3 * len(NETS)
    return {name: plans[3 * j:3 * j + 3] for j, (name, _, _) in enumerate(NETS)}


# ---- shapes and parameter counts -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,layers,in_shape', NETS, ids=[n[0] for n in NETS])
def test_shapes_and_parameter_counts(net_plans, name, layers, in_shape):
    for p in net_plans[name]:
        assert p['rc'] == OK and p['msg'] == ''
    p = net_plans[name][0]
    in_dims = _dims4(in_shape)
    nd = len(in_shape) - 1
    par = [r for r in p['layers'] if r['pidx'] >= 0]
    shapes = device.tf_param_shapes(layers, in_shape)
    assert [r['pidx'] for r in par] == list(range(len(shapes)))
    for r, (_, w_shape, b_shape) in zip(par, shapes):
        assert r['w'] == int(np.prod(w_shape)) and r['b'] == int(np.prod(b_shape)), (r, w_shape, b_shape)
    assert all(r['w'] == 0 and r['b'] == 0 for r in p['layers'] if r['pidx'] < 0)
    dense = layers[-1]['type'] == CONV
    L, got_dense, V, nclass, _ = p['model']
    omap = device.out_map_shape(layers, in_shape)
    last_map = [r for d, r in zip(layers, p['layers']) if d['type'] != FC][-1]['out']
    assert last_map[3 - nd:3] == tuple(omap) and all(v == 1 for v in last_map[:3 - nd])
    assert L == len(shapes) and nclass == layers[-1]['cout'] and got_dense == int(dense)
    assert V == (int(np.prod(omap)) if dense else 1)
    # every layer's shapes, pads and skip bookkeeping against the walk written above
    ref = _ref_shapes(layers, in_dims)
    for i, (d, r) in enumerate(zip(layers, p['layers'])):
        assert (r['inp'], r['out']) == ref[i], (i, r, ref[i])
        assert r['lo'] == _ref_lo(d, ref[i][0]), (i, r)
        assert r['F'] == (int(np.prod(ref[i][0])) if d['type'] == FC else 0)
        assert r['src'] == d['skip_src']
        assert r['dest'] == next((j for j, e in enumerate(layers) if e['skip_src'] == i), -1)
    if name == 'odd_pool':
        assert p['layers'][1]['out'] == (3, 4, 5, 4) and p['layers'][2]['F'] == 240
    if name == 'net_b':
        assert p['layers'][2]['out'][1:3] == (13, 13) and p['layers'][5]['out'][1:3] == (7, 7)


@pytest.mark.parametrize('name,layers,in_shape', NETS, ids=[n[0] for n in NETS])
def test_descriptor_fields_of_every_layer(net_plans, name, layers, in_shape):
    """Tensors of the forward descriptors are (layer input, layer output), of the backward-data ones the swap; the GEMM row grid is the
    layer's output (conv), its input (conv_transpose forward classes) or the backward GEMM's output; k, s, lo, kind, flipped, cls."""
    p = net_plans[name][0]
    ref = _ref_shapes(layers, _dims4(in_shape))
    seen = set()
    for g in p['geom']:
        d, (inp, out) = layers[g['i']], ref[g['i']]
        fwd = g['name'] in ('conv_fwd', 'convt_class', 'convt_all')
        assert (g['I'], g['O']) == ((inp, out) if fwd else (out, inp)), g
        assert g['k'] == tuple(d['k']) and g['s'] == tuple(d['s']) and g['lo'] == _ref_lo(d, inp), g
        assert g['flipped'] == int(g['name'] == 'conv_bwd')
        assert g['kind'] in {'conv_fwd': (0,), 'conv_bwd': (0,), 'convt_class': (3,), 'convt_all': (2, 4), 'convt_bwd': (1,)}[g['name']]
        assert g['name'] == 'convt_class' or g['cls'] == (0, 0, 0)
        seen.add((g['name'], g['i'], g['kind'], g['cls']))
    for c in p['desc']:
        d, (inp, out) = layers[c['i']], ref[c['i']]
        if c['name'] in ('fc_fwd', 'fc_bwd'):
            F = int(np.prod(inp))
            ci, co = (F, d['cout']) if c['name'] == 'fc_fwd' else (d['cout'], F)
            assert (c['I'], c['O'], c['M']) == ((1, 1, 1, ci), (1, 1, 1, co), (1, 1, 1)) and c['taps'] == [(0, 0, 0)]
            assert (c['sm'], c['so'], c['ooff']) == (1, 1, (0, 0, 0))
            continue
        fwd = c['name'] in ('conv_fwd', 'convt_class')
        assert (c['I'], c['O']) == ((inp, out) if fwd else (out, inp)), c
        assert c['M'] == (out[:3] if c['name'] == 'conv_fwd' else inp[:3]), c
        assert c['sm'] == (d['s'][2] if c['name'] == 'convt_bwd' else 1) and c['so'] == (d['s'][2] if c['name'] == 'convt_class' else 1)
        assert c['name'] == 'convt_class' or c['ooff'] == (0, 0, 0)
    for i, d in enumerate(layers):      # every builder ran for every layer it applies to
        if d['type'] == CONV:
            assert ('conv_fwd', i, 0, (0, 0, 0)) in seen and ('conv_bwd', i, 0, (0, 0, 0)) in seen
        if d['type'] == CONVT:
            ncz = 1 if ref[i][0][0] == 1 and d['s'][0] == 1 else d['s'][0]
            for cls in itertools.product(range(ncz), range(d['s'][1]), range(d['s'][2])):
                assert ('convt_class', i, 3, cls) in seen
            assert {('convt_all', i, 2, (0, 0, 0)), ('convt_all', i, 4, (0, 0, 0)), ('convt_bwd', i, 1, (0, 0, 0))} <= seen
            assert sum(c['i'] == i for c in p['desc']) == ncz * d['s'][1] * d['s'][2] + 1
        else:
            assert sum(c['i'] == i for c in p['desc']) == (0 if d['type'] == POOL else 2)


# ---- pads --------------------------------------------------------------------------------------------------------------------
def test_same_pads_against_tensorflows_rule(exe):
    grid = list(itertools.product(range(1, 10), (1, 2, 3, 5), (1, 2)))
    lines = _run(exe, ''.join('pads %d %d %d\n' % g for g in grid))
    assert len(lines) == len(grid)
    for (n, k, s), ln in zip(grid, lines):
        assert tuple(int(t) for t in ln.split()) == _tf_same(n, k, s), (n, k, s, ln)


# ---- taps, by brute force from the definition ------------------------------------------------------------------------------------
def _inside(p, dims):
    return all(0 <= a < n for a, n in zip(p, dims))


def _enum_taps(k):
    return list(itertools.product(range(k[0]), range(k[1]), range(k[2])))      # z outermost: the index of W[t]


def _definition_triples(d, inp, out):
    """{(output point, input point, tap index)} the layer's definition connects.
    conv: y[p] = sum_t x[p + t - lo] W[t];  conv_transpose: y[p] = sum_{s q + t - lo = p} x[q] W[t]."""
    lo = _ref_lo(d, inp)
    res = set()
    if d['type'] == CONV:
        for p in itertools.product(*map(range, out[:3])):
            for ti, t in enumerate(_enum_taps(d['k'])):
                q = tuple(a + b - c for a, b, c in zip(p, t, lo))
                if _inside(q, inp[:3]):
                    res.add((p, q, ti))
    else:
        for q in itertools.product(*map(range, inp[:3])):
            for ti, t in enumerate(_enum_taps(d['k'])):
                p = tuple(s * a + b - c for s, a, b, c in zip(d['s'], q, t, lo))
                if _inside(p, out[:3]):
                    res.add((p, q, ti))
    return res


def _descriptor_triples(c):
    """{(GEMM output point, GEMM input point, tap index)} of one ConvDesc: row m reads m sm + tap, writes m so + ooff."""
    res = set()
    for m in itertools.product(*map(range, c['M'])):
        o = tuple(a * c['so'] + b for a, b in zip(m, c['ooff']))
        assert _inside(o, c['O'][:3]), (c['name'], m, o)
        for t, ti in zip(c['taps'], c['idx']):
            q = tuple(a * c['sm'] + b for a, b in zip(m, t))
            if _inside(q, c['I'][:3]):
                assert (o, q, ti) not in res
                res.add((o, q, ti))
    return res


TAP_CASES = [('conv_333', _ly(CONV, 3, (3, 3, 3)), (4, 5, 6, 2)), ('conv_155', _ly(CONV, 3, (1, 5, 5)), (4, 5, 6, 2)),
             ('convt_k2s2', _ly(CONVT, 3, 2, 2), (3, 3, 3, 2)), ('convt_k3s2', _ly(CONVT, 3, 3, 2), (3, 3, 3, 2)),
             # the geometries tests/test_gpu_convt.py runs on the device: lo = 1 with two taps per class, three classes per
             # dimension, another lo and tap count per dimension, stride 1 (one class), the 2-D schema (s[0] = 1, one z class)
             ('convt_k4s2', _ly(CONVT, 3, 4, 2), (4, 3, 5, 2)), ('convt_k3s3', _ly(CONVT, 3, 3, 3), (2, 3, 4, 2)),
             ('convt_k234s2', _ly(CONVT, 3, (2, 3, 4), 2), (3, 4, 5, 2)), ('convt_k3s1', _ly(CONVT, 3, 3, 1), (3, 4, 5, 2)),
             ('convt_2d_k4s2', _ly(CONVT, 3, (1, 4, 4), (1, 2, 2)), (1, 5, 7, 2))]


@pytest.mark.parametrize('name,layer,in_dims', TAP_CASES, ids=[c[0] for c in TAP_CASES])
def test_taps_connect_what_the_definition_connects(exe, name, layer, in_dims):
    layers = [layer, _ly(FC, 2)]
    (p,) = _parse_plans(_run(exe, _plan_text(layers, in_dims, 8, 1)))
    assert p['rc'] == OK and p['msg'] == ''
    inp, out = _ref_shapes(layers, in_dims)[0]
    want = _definition_triples(layer, inp, out)
    assert {t[0] for t in want} == set(itertools.product(*map(range, out[:3])))      # every output point is connected
    ntap = int(np.prod(layer['k']))
    assert {t[2] for t in want} == set(range(ntap))
    mine = [c for c in p['desc'] if c['i'] == 0]
    if layer['type'] == CONV:
        fwd = [c for c in mine if c['name'] == 'conv_fwd']
        bwd = [c for c in mine if c['name'] == 'conv_bwd']
        assert len(fwd) == 1 and len(fwd[0]['taps']) == ntap
    else:
        fwd = [c for c in mine if c['name'] == 'convt_class']
        bwd = [c for c in mine if c['name'] == 'convt_bwd']
        assert len(fwd) == int(np.prod(layer['s'])) and sorted(sum((c['idx'] for c in fwd), [])) == list(range(ntap))
        assert sorted(c['ooff'] for c in fwd) == list(itertools.product(*map(range, layer['s'])))
        geoms = [g for g in p['geom'] if g['i'] == 0 and g['name'] == 'convt_class']
        assert [g['cls'] for g in geoms] == [c['ooff'] for c in fwd]
    got = set()
    for c in fwd:
        part = _descriptor_triples(c)
        assert not (got & part)
        got |= part
    assert got == want
    assert len(bwd) == 1 and len(bwd[0]['taps']) == ntap
    got_b = _descriptor_triples(bwd[0])      # (input point of the layer, output point of the layer, tap)
    assert {(o, q, t) for q, o, t in got_b} == want and {(o, q, t) for q, o, t in got_b} == got


# ---- batch caps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name,layers,in_shape', NETS, ids=[n[0] for n in NETS])
def test_batch_caps(net_plans, name, layers, in_shape):
    huge, small, mid = (p['model'][4] for p in net_plans[name])
    cap = _ref_cap(layers, _dims4(in_shape))
    if layers[-1]['type'] == CONV:      # dense: the voxels of one pass are indexed in 32 bits
        cap = min(cap, (2 ** 31 - 1) // int(np.prod(device.out_map_shape(layers, in_shape))))
    assert huge == cap
    assert small == 7 and cap > 7
    assert mid == min(4096, cap)
    if name == 'net_c_32':
        assert cap == 2047 and mid == 2047


# ---- rejections --------------------------------------------------------------------------------------------------------------
_C4 = _ly(CONV, 4, 3, 1, 1)
_HEAD = _ly(FC, 2)
# (id, layers, in_dims, code, message): each list is valid but for the one condition; the message is the whole text the library reports
REJECTIONS = [
    ('skip_adjacent', [_C4, _ly(FC, 2, skip=0)], (4, 4, 4, 4), EUNSUPPORTED, 'layer 1: skip source 0 must be an earlier, non-adjacent layer'),
    ('skip_twice', [_C4, _C4, _ly(CONV, 4, 3, 1, 1, skip=0), _ly(CONV, 4, 3, 1, 1, skip=0), _HEAD], (4, 4, 4, 4), EUNSUPPORTED,
     'layer 0 feeds more than one concat'),
    ('concat_sizes', [_C4, _ly(POOL, 0, 2, 2), _ly(CONV, 4, 3, 1, 1, skip=0), _HEAD], (4, 4, 4, 4), EUNSUPPORTED,
     'layer 2: concat of maps of different size (resize_image_with_crop_or_pad) is outside the scored path'),
    ('conv_after_fc', [_ly(FC, 4), _ly(CONV, 2)], (4, 4, 4, 4), EINVAL, 'layer 1: conv after fc'),
    ('strided_conv', [_ly(CONV, 4, 3, 2, 1), _HEAD], (4, 4, 4, 4), EUNSUPPORTED, 'layer 0: strided conv'),
    ('convt_after_fc', [_ly(FC, 4), _ly(CONVT, 2, 2, 2), _HEAD], (4, 4, 4, 4), EINVAL, 'layer 1: conv_transpose after fc'),
    ('convt_kernel', [_ly(CONVT, 4, 1, 2), _HEAD], (4, 4, 4, 4), EUNSUPPORTED, 'layer 0: conv_transpose kernel < stride'),
    ('convt_stride_zy', [_ly(CONVT, 4, 2, (1, 2, 2)), _HEAD], (4, 4, 4, 4), EUNSUPPORTED, 'layer 0: anisotropic stride'),
    ('convt_stride_yx', [_ly(CONVT, 4, 2, (2, 2, 1)), _HEAD], (4, 4, 4, 4), EUNSUPPORTED, 'layer 0: anisotropic stride'),
    ('pool_after_fc', [_ly(FC, 4), _ly(POOL, 0, 2, 2), _HEAD], (4, 4, 4, 4), EINVAL, 'layer 1: pool after fc'),
    ('pool_window_stride', [_ly(POOL, 0, 2, 1), _HEAD], (4, 4, 4, 4), EUNSUPPORTED, 'layer 0: pool window != stride'),
    ('pool_window_size', [_ly(POOL, 0, 7, 7), _HEAD], (8, 8, 8, 4), EUNSUPPORTED, 'layer 0: pool window too large'),
    ('unknown_type', [_ly(9, 2)], (4, 4, 4, 4), EINVAL, 'layer 0: unknown type 9'),
    ('head_window', [_ly(CONV, 2, 3)], (4, 4, 4, 4), EUNSUPPORTED,
     'a conv head must be 1x1 (found 3x3x3): the scored path needs an fc head or a 1x1 conv head'),
    ('head_relu', [_ly(CONV, 2, 1, 1, 1)], (4, 4, 4, 4), EUNSUPPORTED, 'a conv head takes no ReLU: its outputs are the logits'),
    ('head_on_concat', [_C4, _C4, _ly(CONV, 2, skip=0)], (4, 4, 4, 4), EUNSUPPORTED, 'a conv head on a concat (skip source 0) is unsupported'),
    ('head_classes', [_ly(CONV, 9)], (4, 4, 4, 4), EUNSUPPORTED, 'a conv head of 9 classes is unsupported (2 .. 8)'),
    ('head_channels', [_ly(CONV, 2)], (4, 4, 4, 6), EUNSUPPORTED, 'a conv head on 6 channels is unsupported (a multiple of 4, at most 64)'),
    ('no_head', [_C4, _ly(POOL, 0, 2, 2)], (4, 4, 4, 4), EUNSUPPORTED,
     'the scored path needs an fc head (get_gradients, NN_extended.py:1025) or a 1x1 conv head'),
    ('classes', [_ly(FC, 65)], (4, 4, 4, 4), EUNSUPPORTED, '65 classes unsupported'),
    ('param_layers', [_ly(FC, 4, relu=1)] * 16 + [_HEAD], (4, 4, 4, 4), EUNSUPPORTED, '17 parameterised layers > 16'),
    ('skip_topology', [_C4, _C4, _C4, _ly(CONV, 4, 3, 1, 1, skip=0), _ly(CONV, 4, 3, 1, 1, skip=2), _HEAD], (4, 4, 4, 4), EUNSUPPORTED,
     'layer 3: unsupported skip topology'),
]
# further inputs of conditions with two sides
REJECTIONS_MORE = [
    ('head_one_class', [_ly(CONV, 1)], (4, 4, 4, 4), EUNSUPPORTED, 'a conv head of 1 classes is unsupported (2 .. 8)'),
    ('head_wide', [_ly(CONV, 2)], (4, 4, 4, 68), EUNSUPPORTED, 'a conv head on 68 channels is unsupported (a multiple of 4, at most 64)'),
    ('one_class', [_ly(FC, 1)], (4, 4, 4, 4), EUNSUPPORTED, '1 classes unsupported'),
    ('no_layers', [], (4, 4, 4, 4), EUNSUPPORTED, 'the scored path needs an fc head (get_gradients, NN_extended.py:1025) or a 1x1 conv head'),
    ('concat_after_fc', [_C4, _ly(FC, 4), _ly(FC, 2, skip=0)], (1, 1, 1, 4), EUNSUPPORTED,
     'layer 2: concat of maps of different size (resize_image_with_crop_or_pad) is outside the scored path'),
]
# Two conditions of plan_shapes no layer list can trip, because a skip source lies at least two layers before its consumer
# ("must be an earlier, non-adjacent layer" comes first): the last layer (a conv head) and the layer before it feed no concat.
UNREACHABLE = ['a conv head cannot be a skip source', 'a conv head whose input is also a skip source is unsupported']


def test_every_condition_of_the_shape_pass_has_a_case():
    hdr = open(os.path.join(CSRC, 'model_plan.h')).read()
    body = hdr[hdr.index('inline int plan_shapes('):hdr.index('// ---- descriptor builders')]
    assert len(re.findall(r'ALQ_REQUIRE\(', body)) == len(REJECTIONS) + len(UNREACHABLE)
    assert len({r[0] for r in REJECTIONS}) == len(REJECTIONS) and all(u in body for u in UNREACHABLE)
    assert 'hip' not in hdr.lower()      # the header stays free of the device runtime


@pytest.mark.parametrize('name,layers,in_dims,code,message', REJECTIONS + REJECTIONS_MORE, ids=[r[0] for r in REJECTIONS + REJECTIONS_MORE])
def test_rejections(exe, name, layers, in_dims, code, message):
    (p,) = _parse_plans(_run(exe, _plan_text(layers, in_dims, 8)))
    assert (p['rc'], p['msg']) == (code, message)
    assert p['model'] is None and not p['layers']


def test_each_rejection_list_is_valid_but_for_its_flaw(exe):
    """The accepted neighbours of some cases: the same list with the flaw taken out plans."""
    good = [([_C4, _C4, _ly(FC, 2, skip=0)], (4, 4, 4, 4)),                                                   # skip_adjacent
            ([_C4, _C4, _ly(CONV, 4, 3, 1, 1, skip=0), _HEAD], (4, 4, 4, 4)),                                  # skip_twice, concat_sizes
            ([_ly(CONVT, 4, 2, 2), _HEAD], (4, 4, 4, 4)), ([_ly(CONVT, 4, 2, (1, 2, 2)), _HEAD], (1, 4, 4, 4)),  # the conv_transpose cases
            ([_ly(POOL, 0, 6, 6), _HEAD], (8, 8, 8, 4)),                                                       # pool_window_size: 216 <= 255
            ([_ly(CONV, 2)], (4, 4, 4, 4)), ([_C4, _C4, _ly(CONV, 2)], (4, 4, 4, 4)), ([_ly(CONV, 8)], (4, 4, 4, 64)),  # the head cases
            ([_ly(FC, 64)], (4, 4, 4, 4)), ([_ly(FC, 4, relu=1)] * 15 + [_HEAD], (4, 4, 4, 4)),                # classes, param_layers
            ([_C4, _C4, _C4, _ly(CONV, 4, 3, 1, 1, skip=0), _C4, _C4, _ly(CONV, 4, 3, 1, 1, skip=4), _HEAD], (4, 4, 4, 4))]   # skip_topology
    plans = _parse_plans(_run(exe, ''.join(_plan_text(ly, dims, 8) for ly, dims in good)))
    assert len(plans) == len(good)
    for p in plans:
        assert (p['rc'], p['msg']) == (OK, '') and p['model'][4] == 8
