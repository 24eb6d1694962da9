"""alq_model_set_weights_device without a GPU: the symbol, its ctypes declaration, and the stale / refresh logic of
`DeviceModel.var_dict` (device.LazyVarDict) against a stand-in for the device vector."""
import ctypes as C
import os
import re
import subprocess
from collections import OrderedDict

import numpy as np
import pytest


def test_symbol_is_declared_and_exported():
    from nnal_amd import _lib
    hdr = open(os.path.join(os.path.dirname(_lib._HERE), 'include', 'alq.h')).read()
    assert re.search(r'\bint alq_model_set_weights_device\(alq_model \*m, int t, const float \*d_W, const float \*d_b\);', hdr)
    assert re.search(r'\bint alq_model_layer_packs_on_device\(const alq_model \*m, int t\);', hdr)
    # the contract the header has to state: the read-back per device-packed layer
    doc = hdr[hdr.index('Same contract as alq_model_set_weights'):hdr.index('int alq_model_set_weights_device')]
    assert 'at most 64' in doc and 'DEVICE pointers' in doc
    assert re.search(r'\b14: the number of weight elements that went through the HOST packers', hdr)
    for name in ('alq_model_set_weights_device', 'alq_model_layer_packs_on_device'):
        assert name in _lib.exported_names()
    _lib.build()
    nm = subprocess.check_output(['nm', '-D', '--defined-only', _lib.LIB_PATH]).decode()
    assert re.search(r'\bT alq_model_set_weights_device\b', nm)
    assert re.search(r'\bT alq_model_layer_packs_on_device\b', nm)
    src = open(os.path.join(_lib._HERE, 'csrc', 'build.sh')).read()
    assert len(re.findall(r'\bwpack\b', src)) == 2                  # the compile list and the link list


def test_ctypes_declaration():
    from nnal_amd import _lib
    res, args = _lib._SIGNATURES['alq_model_set_weights_device']
    assert res is C.c_int and args == [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert _lib._SIGNATURES['alq_model_set_weights_device'] == _lib._SIGNATURES['alq_model_set_weights']
    assert _lib._SIGNATURES['alq_model_layer_packs_on_device'] == (C.c_int, [C.c_void_p, C.c_int])
    L = _lib.lib()
    fn = L.alq_model_set_weights_device
    assert fn.restype is C.c_int and list(fn.argtypes) == args
    # argument checks come before any device call: a null model is ALQ_EINVAL with or without a GPU
    assert fn(None, 0, None, None) == -1
    assert b'null argument' in L.alq_last_error()
    assert L.alq_model_layer_packs_on_device(None, 0) == -1


class _DeviceVector(object):
    """Stand-in for the optimiser's flat device vector: counts how often it is copied to the host."""

    def __init__(self, values):
        self.values = np.array(values, dtype=np.float32)
        self.copies = 0

    def to_host(self):
        self.copies += 1
        return self.values.copy()


class _Model(object):
    """The part of DeviceModel that owns var_dict: host sets store arrays, device sets arm the refresh."""

    shapes = [('a', (2, 3), (3,)), ('b', (4,), (1,))]

    def __init__(self):
        from nnal_amd.device import LazyVarDict
        self.var_dict = LazyVarDict((n, None) for n, _, _ in self.shapes)

    def set_weights(self, pars):
        staged = [(n, [np.array(pars[n][0], dtype=np.float32), np.array(pars[n][1], dtype=np.float32)]) for n, _, _ in self.shapes]
        self.var_dict.mark_fresh()
        for n, wb in staged:
            self.var_dict[n] = wb

    def set_weights_device(self, vec):
        def refresh():
            flat, off = vec.to_host(), 0
            for n, ws, bs in self.shapes:
                nw, nb = int(np.prod(ws)), int(np.prod(bs))
                self.var_dict.put(n, [flat[off:off + nw].reshape(ws), flat[off + nw:off + nw + nb].reshape(bs)])
                off += nw + nb
        self.var_dict.mark_stale(refresh)


def test_var_dict_refreshes_once_on_the_first_read():
    m = _Model()
    assert not m.var_dict.stale
    assert list(m.var_dict.keys()) == ['a', 'b'] and len(m.var_dict) == 2 and 'a' in m.var_dict
    m.set_weights({'a': [np.ones((2, 3)), np.zeros(3)], 'b': [np.full(4, 2.), np.zeros(1)]})
    assert not m.var_dict.stale and m.var_dict['b'][0][0] == 2.
    vec = _DeviceVector(np.arange(14))
    m.set_weights_device(vec)
    # names, length, membership and iteration over names never fetch
    assert m.var_dict.stale and list(m.var_dict) == ['a', 'b'] and len(m.var_dict) == 2 and 'b' in m.var_dict
    assert vec.copies == 0
    # another step before anybody looked: still nothing fetched (the refresh is per access, not per step)
    vec.values += 100
    m.set_weights_device(vec)
    assert vec.copies == 0
    W, b = m.var_dict['a']
    assert vec.copies == 1 and not m.var_dict.stale
    assert W.shape == (2, 3) and np.array_equal(W.ravel(), np.arange(6) + 100) and np.array_equal(b, np.arange(6, 9) + 100)
    assert np.array_equal(m.var_dict['b'][0], np.arange(9, 13) + 100)
    assert [k for k, _ in m.var_dict.items()] == ['a', 'b'] and len(list(m.var_dict.values())) == 2
    assert vec.copies == 1


@pytest.mark.parametrize('reader', ['getitem', 'get', 'values', 'items', 'copy'])
def test_every_reader_of_values_refreshes(reader):
    m = _Model()
    vec = _DeviceVector(np.arange(14))
    m.set_weights_device(vec)
    got = {'getitem': lambda: m.var_dict['b'], 'get': lambda: m.var_dict.get('b'),
           'values': lambda: list(m.var_dict.values())[1], 'items': lambda: dict(m.var_dict.items())['b'],
           'copy': lambda: m.var_dict.copy()['b']}[reader]()
    assert vec.copies == 1 and np.array_equal(got[0], np.arange(9, 13)) and np.array_equal(got[1], [13.])
    assert m.var_dict.get('nope', 5) == 5


def test_a_host_set_clears_the_stale_mark_and_a_failing_refresh_keeps_it():
    m = _Model()
    vec = _DeviceVector(np.arange(14))
    m.set_weights_device(vec)
    m.set_weights({'a': [np.ones((2, 3)), np.zeros(3)], 'b': [np.full(4, 2.), np.zeros(1)]})
    assert not m.var_dict.stale and m.var_dict['a'][0][0, 0] == 1. and vec.copies == 0
    # passing the stale dict itself to set_weights reads it first (the refresh), then stores host copies
    m.set_weights_device(vec)
    m.set_weights(m.var_dict)
    assert vec.copies == 1 and not m.var_dict.stale and np.array_equal(m.var_dict['a'][0].ravel(), np.arange(6))

    def boom():
        raise RuntimeError('device lost')
    m.var_dict.mark_stale(boom)
    with pytest.raises(RuntimeError):
        m.var_dict['a']
    assert m.var_dict.stale          # nothing was fetched: the next read tries again
    m.var_dict.mark_fresh()
    assert m.var_dict['a'][0].shape == (2, 3)


def test_weight_files_are_written_from_a_stale_dict(tmp_path):
    """save_weights hands var_dict to weights_io.write_weights: the file holds the device's values."""
    from nnal_amd import weights_io
    m = _Model()
    m.set_weights({'a': [np.ones((2, 3)), np.zeros(3)], 'b': [np.full(4, 2.), np.zeros(1)]})
    vec = _DeviceVector(np.arange(14) * 0.5)
    m.set_weights_device(vec)
    path = str(tmp_path / 'w.npz')
    weights_io.write_weights(path, m.var_dict)
    back = weights_io.read_weights(path, ['a', 'b'])
    assert np.array_equal(np.asarray(back['a'][0]).ravel(), np.arange(6) * 0.5)
    assert np.array_equal(np.asarray(back['b'][1]).ravel(), [6.5])
    assert isinstance(m.var_dict, OrderedDict)
