"""The device context behind the reference's `sess`: stream binding, device memory, the RCCL communicator and the measurement
hooks of a libalq context; the kernel families it fronts are the mixins of device_select, device_volume and device_aopt."""
import contextlib
import ctypes as C
import os
from collections import OrderedDict

import numpy as np

from . import _lib, device_run
from ._lib import check, check_tensor, ptr
from .device_aopt import AoptOps
from .device_select import SelectOps
from .device_volume import VolumeOps

_default_session = None
_live = None   # weak set of sessions / models, closed at interpreter exit BEFORE the HIP runtime unloads


def _track(obj):
    global _live
    if _live is None:
        import atexit
        import weakref
        _live = weakref.WeakSet()

        def _close_all():
            objs = list(_live)
            for o in objs:                      # models first: they hold device memory of a context
                if not isinstance(o, DeviceSession):
                    o.close()
            for o in objs:
                if isinstance(o, DeviceSession):
                    o.close()
        atexit.register(_close_all)
    _live.add(obj)


def default_session():
    """The process-wide session used by functions whose reference signature carries no `sess`
    (patch_utils.get_patches).  One process drives one GPU (LOCAL_RANK picks it)."""
    global _default_session
    if _default_session is None:
        _default_session = DeviceSession(int(os.environ.get('LOCAL_RANK', '0')))
    return _default_session


@contextlib.contextmanager
def side_stream(lib, ctx, on):
    """Runs the body with the context's side stream switched to `on` (alq_ctx_use_side_stream) and leaves it switched on -
    what every single-pipeline call relies on - however the body ends."""
    check(lib.alq_ctx_use_side_stream(ctx, 1 if on else 0))
    try:
        yield
    except BaseException:
        if not on:
            lib.alq_ctx_use_side_stream(ctx, 1)          # (unchecked: the body's error is the one to report)
        raise
    if not on:
        check(lib.alq_ctx_use_side_stream(ctx, 1))


class DeviceSession(SelectOps, VolumeOps, AoptOps):
    """One GPU, one stream.  `run(fetch, feed_dict)` keeps unported strategies working."""

    def __init__(self, device=0):
        import torch
        if not torch.cuda.is_available():
            raise _lib.AlqError('no GPU visible: the query-scoring path has no CPU fallback')
        self.torch = torch
        self.device = torch.device('cuda', device)
        torch.cuda.set_device(self.device)
        self.lib = _lib.lib()
        self._ctx = C.c_void_p()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        check(self.lib.alq_ctx_create(device, C.c_void_p(stream), C.byref(self._ctx)))
        self._stream = stream
        self.comm_world = 0          # > 0 once pool_shard.attach_comm gave this context an RCCL communicator
        _track(self)

    @property
    def ctx(self):
        return self._ctx

    def bind_stream(self):
        """Points the library at torch's CURRENT stream on this device.  Every device call interleaves libalq
        launches with torch ops and caching-allocator frees, which are ordered on torch's current stream; a
        caller inside `torch.cuda.stream(s)` would otherwise have the library race with torch's reuse of the
        buffers it was handed.  One pointer compare per call when nothing changed."""
        s = self.torch.cuda.current_stream(self.device).cuda_stream
        if s != self._stream:
            check(self.lib.alq_ctx_set_stream(self._ctx, C.c_void_p(s)))
            self._stream = s

    def synchronize(self):
        check(self.lib.alq_ctx_synchronize(self._ctx))

    def close(self):
        if self._ctx:
            self.lib.alq_ctx_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- torch helpers --------------------------------------------------------------------
    def to_device(self, arr, dtype):
        return self.torch.as_tensor(np.ascontiguousarray(arr)).to(device=self.device, dtype=dtype)

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device=self.device)

    def run(self, fetch, feed_dict=None):
        """`sess.run(fetch, feed_dict)` of the reference: device_run.run states the fetches."""
        return device_run.run(fetch, feed_dict)

    # -- RCCL communicator of the sharded pool (pool_shard.attach_comm) --------------------
    def comm_unique_id(self):
        buf = C.create_string_buffer(128)
        check(self.lib.alq_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, uid, rank, world):
        self.bind_stream()
        check(self.lib.alq_comm_init(self._ctx, C.c_char_p(uid), int(rank), int(world)))
        self.comm_world = int(world)

    def comm_destroy(self):
        check(self.lib.alq_comm_destroy(self._ctx))
        self.comm_world = 0

    def allreduce_sum_(self, t):
        """In-place all-reduce(sum) of a float64 device tensor over the context's RCCL communicator."""
        check_tensor(t, self.torch.float64)
        self.bind_stream()
        check(self.lib.alq_allreduce_sum(self._ctx, ptr(t), t.numel()))
        return t

    # -- measurement hooks ----------------------------------------------------------------
    def prof_enable(self, on=True):
        """True / 1: time every launch; k > 1: the launches of every k-th Fisher pass; False / 0: off."""
        check(self.lib.alq_prof_enable(self._ctx, int(on)))

    def prof_reset(self):
        check(self.lib.alq_prof_reset(self._ctx))

    def prof_read(self):
        out = OrderedDict()
        for c in range(self.lib.alq_prof_num_classes()):
            ms, n, fl = C.c_double(), C.c_int64(), C.c_double()
            check(self.lib.alq_prof_read(self._ctx, c, C.byref(ms), C.byref(n), C.byref(fl)))
            out[self.lib.alq_prof_class_name(c).decode()] = dict(ms=ms.value, launches=n.value, flops=fl.value)
        return out
