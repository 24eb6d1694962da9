"""The conditions under which the fp64 bar of tests/hvp_cases.py means something, proven on the CPU from the fp64 oracle alone, for
every array of every case that a GPU test holds to that bar - and the claims the cases make about their nets and launches that
need no device.  Prints u64, G, e32 and b64 per array.

  noise margin     b64 >= 64 u64       discrimination   b64 <= e32 / 1024       decision margin  no fragile unit at EPS_TIGHT
"""
import numpy as np
import pytest

from tests import hvp_cases as H


def _prove(tag, y, om64, x, arrays):
    H.figures(tag, y, arrays)
    assert H.conditions(y, om64, x, arrays) == [], tag


@pytest.mark.parametrize('name', list(H.TABLE))
def test_conditions_of_the_whole_product(name):
    d = H.case(name)
    assert d['n'] <= H.MAX_BATCH
    _prove(name, H.yard(name), d['om64'], d['x'], d['arrays'])


def test_present_seeds_have_the_stated_margin():
    """What the issue records about the four nets' seeds: input seed 21 of net3d_skip_c2 has one unit inside 2e-5, hence 36."""
    import torch
    from oracle import netspec
    from oracle.model import OracleModel
    t = H.TABLE['net3d_skip_c2']
    assert t['xseed'] == 36
    pars = netspec.he_init(t['ld'], t['in_shape'], seed=t['wseed'], skips=t['sk'], bias_std=0.05)
    om64 = OracleModel(t['ld'], t['in_shape'], pars, skips=t['sk'], dtype=torch.float64)
    x21 = np.random.RandomState(21).randn(H.N, *t['in_shape']).astype(np.float32)
    assert H.fragile_units(om64, x21) == 0 and H.tight(om64, x21) == 1
    assert H.fragile_units(H.case('net3d_skip_c2')['om64'], H.case('net3d_skip_c2')['x'], eps=1e-4) == 0


@pytest.mark.parametrize('k', range(10))
def test_conditions_of_the_layer_subsets(k):
    """Every layer of net3d_skip_c4 alone and all but layer t (test_gpu_hvp.test_switched_off_terms; 'last_fc' and 'middle_conv'
    of test_layer_subsets are among them)."""
    d = H.case('net3d_skip_c4')
    chosen = H.subsets('net3d_skip_c4')[k]
    y = H.yard('net3d_skip_c4', chosen)
    _prove('net3d_skip_c4 %r' % (chosen,), y, d['om64'], d['x'], y['arrays'])


def test_conditions_of_two_apart_and_of_the_second_vector():
    """'two_apart' of test_gpu_hvp.test_layer_subsets and the vector u of test_symmetry."""
    d = H.case('net3d_skip_c4')
    names = d['names']
    y = H.yard('net3d_skip_c4', [names[0], names[3]])
    _prove('two_apart', y, d['om64'], d['x'], y['arrays'])
    _prove('u', H.yard('net3d_skip_c4', v=H.symmetry_u(d), key='u'), d['om64'], d['x'], d['arrays'])


@pytest.mark.parametrize('name', ['labels_c2', 'labels_c21'])
def test_conditions_of_the_labelled_samples_alone(name):
    d = H.case(name)
    keep, y = H.labelled_only(name)
    assert len(keep) == 4 and d['n'] == 7
    _prove(name + ' labelled only', y, d['om64'], d['x'][keep], d['arrays'])
    # an unlabelled sample adds nothing to the truth either: same G, and the products agree to the truth's own noise
    full = H.yard(name)
    for g1, g2, a, b, u in zip(full['G'], y['G'], full['hv64'], y['hv64'], y['b64']):
        assert g1 == g2 and np.abs(a - b).max() <= u / 64


def _whole_records():
    import tests.test_gpu_conv as tv
    import tests.test_gpu_convt as tc
    import tests.test_gpu_fc_small as tf
    import tests.test_gpu_fcgemm as tg
    out = [('convt ' + n, lambda n=n: tc.whole(n)) for n in tc.WHOLE] + [('conv ' + n, lambda n=n: tv.whole(n)) for n in tv.WHOLE]
    out += [('fc_small ' + n, lambda n=n: tf.whole(n)) for n in tf.WHOLE if tf.WHOLE[n][2] == 2]
    return out + [('fcgemm c2', lambda: tg.whole(2))]


@pytest.mark.parametrize('tag,rec', _whole_records(), ids=[r[0] for r in _whole_records()])
def test_conditions_of_the_whole_models_of_other_files(tag, rec):
    """Every whole model on which check_other_entry_points (tests/test_gpu_convt.py; reused by test_gpu_conv.py and
    test_gpu_fc_small.py) and tests/test_gpu_fcgemm.py compare a product: all of them pass (a model alq_model_create refuses runs
    no product), on their own patches or on the first of the same stream with the decision margin."""
    d = rec()
    if d.get('refused'):
        return
    t = H.whole_tight(d)
    print('%s: patches %r' % (tag, t['chosen'] or 'of the other checks'))
    assert t['y'] is not None, t['bad']
    H.figures(tag, t['y'], d['arrays'])
    assert t['bad'] == [], (tag, t['bad'])


# ------------------------------------------------------------------------------------------ what the cases claim, without a device
def test_pool_input_that_is_a_skip_source():
    """k_hvp_pool_bwd with accumulate = written[i - 1] = 1: in net_3d_skip the pool (layer 1) reads enc1 (layer 0), which is also
    the skip source of dec1 (layer 4).  run_hess_vecp walks the layers backward, so dec1 has written enc1's cotangent before the
    pool adds to it."""
    from nnal_amd._lib import ALQ_POOL
    from nnal_amd.device_host import translate_layers
    for name in ('net3d_skip_c4', 'net3d_skip_c2'):
        d = H.case(name)
        layers = translate_layers(d['ld'], d['in_shape'], d['sk'])
        assert layers[1]['type'] == ALQ_POOL and layers[1]['skip_src'] < 0
        assert [i for i, ly in enumerate(layers) if ly['skip_src'] == 0] == [4]


def test_slab_boundary_inside_a_sample_and_ragged_last_slab():
    """hvp_wgrad_kernel on the present nets: neta_c3's conv1 walks 2,000 rows in 7 slabs of 286 against 400 rows per sample - slab
    boundaries inside samples - and a last slab of 284."""
    prod = {p[0]: p[1:] for p in H.conv_products('neta_c3')}
    rows, vox, M, nslab, rps, limit = prod['conv1']
    assert (rows, vox, M, nslab, rps, limit) == (2000, 400, 400, 7, 286, 'rows')
    assert all((s * rps) % vox for s in range(1, nslab)) and 0 < rows - (nslab - 1) * rps < rps
    # the three limits of the rule, one case each
    assert H.wgrad_slabs(10580, 102400) == (40, 265) and H.wgrad_slabs(210, 216) == (1, 210)
    assert [p[-1] for p in H.conv_products('slab_cap')] == ['rows', 'cap']
    assert H.wgrad_slabs(256 * 70000, 8)[0] <= 65535


def test_partial_buffer_constant_is_the_librarys():
    """PARTIAL_DOUBLES restates hvp_wgrad_partial_doubles (csrc/hvp.hip)."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'nn-active-learning_amd', 'csrc', 'hvp.hip')).read()
    m = re.search(r'hvp_wgrad_partial_doubles\(long long M\) \{ return std::max<long long>\(1LL << (\d+), M\); \}', src)
    assert m and 1 << int(m.group(1)) == H.PARTIAL_DOUBLES
    assert 'std::min<long long>(std::max<long long>(rows / 256, 1), std::max<long long>(hvp_wgrad_partial_doubles(M) / M, 1))' in src
