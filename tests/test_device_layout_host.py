"""The device binding after its split by concern: the import point `nnal_amd.device` keeps the surface it had as one file
(tests/golden/device_api.json, recorded from the single-file version), and the shared helpers - pointer, tensor check,
max_batch cuts, non-zero-weight count, side-stream guard - do what their call sites relied on.  Host only."""
import inspect
import json
import os
import types

import numpy as np
import pytest
import torch

import nnal_amd  # noqa: F401
from nnal_amd import device

# private names that the tests and bench.py touch
KEPT_PRIVATE = ('_m', '_as_device_batch', '_objective_pass', '_drop_args', '_param_offsets', '_mt', '_obj', '_opt', '_xlanes', '_lane2',
                '_weights_version', '_dev_pack', '_host_repack', '_masked_args', 'pass_cut', 'lanes', 'class_slots')


def _describe(cls, name):
    """How `name` resolves on `cls` through its bases: the kind of attribute and, for a callable, its signature."""
    for base in cls.__mro__:
        if name in vars(base):
            raw = vars(base)[name]
            break
    else:
        return None
    if isinstance(raw, property):
        return 'property'
    if isinstance(raw, (staticmethod, classmethod)):
        return '%s%s' % (type(raw).__name__, inspect.signature(raw.__func__))
    if callable(raw):
        return 'method%s' % (inspect.signature(raw),)
    return 'value %r' % (raw,)


def device_api():
    """The listing recorded in tests/golden/device_api.json: the public module-level names of `device` that the package
    defines (modules and names of the standard library aside), and per class every public attribute plus KEPT_PRIVATE as
    resolved through the bases.  A kept private name that is set per instance reads 'instance attribute'."""
    out = {'module': sorted(n for n, v in vars(device).items() if not n.startswith('_') and not isinstance(v, types.ModuleType)
                            and getattr(v, '__module__', 'nnal_amd').startswith('nnal_amd')), 'classes': {}}
    for cls in (device.DeviceSession, device.DeviceModel):
        src = ''.join(inspect.getsource(b) for b in cls.__mro__ if b is not object)
        attrs = {}
        for name in sorted(set(n for n in dir(cls) if not n.startswith('_')) | set(KEPT_PRIVATE)):
            d = _describe(cls, name)
            if d is None and ('self.%s = ' % name) in src:
                d = 'instance attribute'
            if d is not None:
                attrs[name] = d
        out['classes'][cls.__name__] = attrs
    return out


def _golden(golden_dir):
    return os.path.join(golden_dir, 'device_api.json')


def test_public_surface_is_the_single_file_one(golden_dir):
    want = json.load(open(_golden(golden_dir)))
    got = device_api()
    assert got['module'] == want['module']
    for cls in want['classes']:
        assert sorted(got['classes'][cls]) == sorted(want['classes'][cls]), cls
        for name, d in want['classes'][cls].items():
            assert got['classes'][cls][name] == d, (cls, name)
    for name in KEPT_PRIVATE:
        assert name in want['classes']['DeviceModel'] or name in want['classes']['DeviceSession'], name


def test_ptr_and_check_tensor_on_cpu_tensors():
    from nnal_amd._lib import check_tensor, ptr
    assert ptr(None) is None and ptr(None, 8) is None
    t = torch.arange(12, dtype=torch.float32)
    assert ptr(t).value == t.data_ptr() and ptr(t, 24).value == t.data_ptr() + 24
    empty = torch.empty((0,), dtype=torch.float32)
    ptr(empty)
    check_tensor(empty, torch.float32, 0, empty.device)
    check_tensor(t, torch.float32)
    check_tensor(t, torch.float32, 12, torch.device('cpu'))
    check_tensor(None, torch.float32, 12, optional=True)
    for dt in (torch.uint8, torch.int32, torch.int64):
        check_tensor(torch.zeros((3,), dtype=dt), (torch.uint8, torch.int32, torch.int64), 3)
    bad = [lambda: check_tensor(t, torch.float64),                                   # dtype
           lambda: check_tensor(t, (torch.float64, torch.int32)),
           lambda: check_tensor(t.reshape(3, 4).t(), torch.float32),               # a non-contiguous view
           lambda: check_tensor(t, torch.float32, 11),                              # element count
           lambda: check_tensor(t, torch.float32, 12, torch.device('meta')),        # device
           lambda: check_tensor(None, torch.float32)]                                # a required tensor
    for fn in bad:
        with pytest.raises(AssertionError):
            fn()


@pytest.mark.parametrize('n', [0, 1, 3, 4, 5, 11])
def test_cuts_tile_the_batch_in_order(n):
    m = device.DeviceModel.__new__(device.DeviceModel)
    m.max_batch, m.elems_per_patch = 4, 6
    cuts = list(m._cuts(n))
    assert [a for a, _ in cuts] == list(range(0, n, 4)) and (cuts[-1][1] if cuts else 0) == n
    assert all(b == a2 for (_, b), (a2, _) in zip(cuts, cuts[1:]))          # each cut starts where the last one ended
    assert all(0 < b - a <= 4 for a, b in cuts)
    t = torch.zeros((max(n, 1), 6), dtype=torch.float32)
    assert m._patch_ptr(t, 2).value == t.data_ptr() + 2 * 6 * 4


def test_nonzero_weight_count_is_tf_sum_by_nonzero_weights():
    from nnal_amd.device_host import nonzero_weight_count
    rs = np.random.RandomState(7)
    lab = rs.randint(-1, 2, size=500).astype(np.int32)
    sw = (rs.rand(500) * (rs.rand(500) > 0.3)).astype(np.float32)
    for bcw in (None, [0., 2.5], [1.5, 0.], [0.25, 4.], [0., 0.]):
        for s in (None, sw):
            # TF: weights = labelled * class weight of the label * sample weight; the divisor counts the non-zero ones
            w = (lab >= 0) * (1. if bcw is None else np.asarray(bcw, np.float32)[np.maximum(lab, 0)])
            w = w * (1. if s is None else s)
            want = int(np.sum(w != 0))
            got = nonzero_weight_count(2, bcw, lab, s)
            assert isinstance(got, int) and got == want
            if s is None:
                counts = np.bincount(lab[lab >= 0], minlength=2).astype(np.int64)
                assert nonzero_weight_count(2, bcw, counts=counts) == want
    lab3 = rs.randint(-1, 3, size=200).astype(np.int32)                          # more classes: no class weights
    assert nonzero_weight_count(3, None, lab3) == nonzero_weight_count(3, counts=np.bincount(lab3[lab3 >= 0], minlength=3)) \
        == int(np.sum(lab3 >= 0))


class _StubLib(object):
    def __init__(self):
        self.calls = []

    def alq_ctx_use_side_stream(self, ctx, on):
        self.calls.append((ctx, on))
        return 0


def test_side_stream_is_back_on_after_a_body_that_raises():
    from nnal_amd.device_session import side_stream
    lib = _StubLib()
    with pytest.raises(KeyError):
        with side_stream(lib, 'ctx', 0):
            assert lib.calls == [('ctx', 0)]
            raise KeyError('a pass failed')
    assert lib.calls == [('ctx', 0), ('ctx', 1)]
    lib = _StubLib()
    with side_stream(lib, 'ctx', 0):
        pass
    assert lib.calls == [('ctx', 0), ('ctx', 1)]
    lib = _StubLib()
    with pytest.raises(KeyError):
        with side_stream(lib, 'ctx', 1):          # a single pipeline: the stream stays on, nothing to restore
            raise KeyError('a pass failed')
    assert lib.calls == [('ctx', 1)]


def test_fc_only_guards_stand_at_the_19_definitions():
    """Each method that is defined for fc-head models only carries the guard (functools.wraps keeps its signature, so the surface
    listing cannot tell) and raises on a dense model before it reads anything else."""
    names = ('get_gradients', 'grad_log_post', 'param_grads_device', 'grad_sqnorms_device', 'hess_vecp_device', 'hess_vecp',
             'fisher_device', 'fisher', 'shrunk_class_gradients', 'class_layer_sums_device', 'fisher_classes',
             'diagonal_fisher_device', 'diagonal_fisher', 'diagonal_fisher_rows_device', 'llfc_reference_order', 'llfc_grads_device',
             'llfc_hess_device', 'llfc_stoch_if_features_device', 'llfc_stoch_if_device')
    m = device.DeviceModel.__new__(device.DeviceModel)
    m.dense = True
    for name in names:
        fn = getattr(device.DeviceModel, name)
        assert hasattr(fn, '__wrapped__'), name
        with pytest.raises(NotImplementedError, match=name):
            fn(m)
