"""Device context ("session") and device model behind the reference's `sess` / `model` pair.

The reference hands every query function a `tf.Session` and a `CNN` object and reaches the
device through `sess.run(getattr(model, var), feed_dict)` (PW_NN.py:466,522).  Here `sess` is a
`DeviceSession` (one HIP stream on one MI355X, a libalq context) and `model` a `DeviceModel`
(a libalq model: weights + activation workspace resident in HBM).  PyTorch-ROCm is used only
for device memory, the stream and (in pool_shard.py) torch.distributed.
"""
import ctypes as C
import functools
import os
from collections import OrderedDict

import numpy as np

from . import _lib
from ._lib import ALQ_CONV, ALQ_CONVT, ALQ_FC, ALQ_POOL, LayerT, LossT, check


def _torch():
    import torch
    return torch


class Handle(object):
    """Stand-in for a TF tensor attribute of the reference model (`model.x`, `.posteriors`, ...)."""

    class _Dim(object):
        def __init__(self, v):
            self.value = v

    def __init__(self, name, shape=()):
        self.name = name
        self.shape = [Handle._Dim(s) for s in shape]

    def __repr__(self):
        return '<device handle %s>' % self.name


class MethodHandle(Handle):
    """A fetch that shares its name with a method of the model (`model.hess_vecp`: Influence.get_hess_vec_product stores the
    fetch under the name DeviceModel's own product method has): calling it is calling that method."""

    def __call__(self, *args, **kwargs):
        return getattr(type(self.model), self.name)(self.model, *args, **kwargs)


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
                if isinstance(o, DeviceModel):
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
        import os
        _default_session = DeviceSession(int(os.environ.get('LOCAL_RANK', '0')))
    return _default_session


class DeviceSession(object):
    """One GPU, one stream.  `run(fetch, feed_dict)` keeps unported strategies working."""

    def __init__(self, device=0):
        torch = _torch()
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

    def uncertainty_filter(self, posts, B, with_keys=False):
        """The B positions of `posts` (device fp32 [n]) closest to 0.5, ascending |p - .5|, ties -> lower position
        (alq_score_entropy + alq_topk_uncertain); int64 device tensor [min(B, n)] (+ their fp64 keys on request)."""
        from .PW_NNAL import device_uncertainty_filter
        return device_uncertainty_filter(self, posts, B, with_keys)

    def topk_smallest(self, keys, B):
        """Positions of the B smallest entries of a float64 device vector, ascending, ties -> lower position (numeric order
        for either sign, -0.0 immediately before +0.0; +inf and then a NaN with the sign bit clear come last, a NaN with the sign bit
        set comes FIRST, before -inf - the order of sign and magnitude bits; include/alq.h, alq_topk_uncertain)."""
        torch = self.torch
        self.bind_stream()
        n = int(keys.numel())
        work = self.empty((self.lib.alq_topk_work_bytes(n),), torch.uint8)
        out = self.empty((int(B),), torch.int64)
        check(self.lib.alq_topk_uncertain(self._ctx, C.c_void_p(keys.data_ptr()), n, int(B), C.c_void_p(out.data_ptr()),
                                          C.c_void_p(work.data_ptr())))
        return out

    def committee_update(self, p1, member, mode, mean_p, mean_h=None, keys=None):
        """alq_committee_update: member `member` (0-based, in order) of the ensemble (mode 0) or QBC-JS (mode 1) committee,
        p1 = its class-1 posteriors (float32 device [n]); updates the float64 device running means mean_p (and mean_h,
        QBC-JS) in place and, when `keys` is given, writes the float64 top-k keys for topk_smallest into it."""
        torch = self.torch
        self.bind_stream()
        n = int(p1.numel())
        for t, dt in ((p1, torch.float32), (mean_p, torch.float64), (mean_h, torch.float64), (keys, torch.float64)):
            assert t is None or (t.dtype == dt and t.is_contiguous() and int(t.numel()) == n and t.device == self.device)

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        check(self.lib.alq_committee_update(self._ctx, ptr(p1), n, int(member), int(mode), ptr(mean_p), ptr(mean_h), ptr(keys)))

    def eval_counts(self, pred, inds, mask, counts, seg=None):
        """alq_eval_counts: adds the confusion counts (P, N, TP, FP, TN, FN; get_preds_stats) of the predictions `pred` (int64
        device [n]) against the labels mask[inds] - `mask` the subject's un-padded mask volume on the device (float32 or
        float64, NaN = ignored), `inds` int64 device [n] raveled indices into it, or None when `mask` is the label vector
        itself - to the int64 device totals `counts` [6]; with `seg` (uint8 device, the mask's size) also seg[inds] = pred."""
        torch = self.torch
        self.bind_stream()
        n = int(pred.numel())
        assert mask.dtype in (torch.float32, torch.float64) and mask.is_contiguous() and mask.device == self.device
        assert counts.dtype == torch.int64 and counts.is_contiguous() and int(counts.numel()) == 6 and counts.device == self.device
        for t, dt in ((pred, torch.int64), (inds, torch.int64)):
            assert t is None or (t.dtype == dt and t.is_contiguous() and int(t.numel()) == n and t.device == self.device)
        elems = int(mask.numel())
        assert inds is not None or elems >= n
        assert seg is None or (seg.dtype == torch.uint8 and seg.is_contiguous() and seg.device == self.device and
                               int(seg.numel()) >= (elems if inds is not None else n))

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        check(self.lib.alq_eval_counts(self._ctx, ptr(pred), ptr(inds), n, ptr(mask), 1 if mask.dtype == torch.float64 else 0,
                                       elems, ptr(counts), ptr(seg)))

    def confusion_counts(self, pred, labels, C, inner=None, groups=1, first=0, fill=-1, counts=None, want_skipped=False):
        """alq_confusion_counts: adds counts[g][t][p] over the n elements of the device id tensors `pred` and `labels` (uint8,
        int32 or int64 each, contiguous, the same number of elements), g = ((first + i) // inner) % groups, to the int64 device
        tensor `counts` [groups, C, C] (None: a new zeroed one).  A label outside [0, C) reads as `fill` when 0 <= fill < C; an
        element whose label (after that) or prediction lies outside [0, C) is skipped.  inner None: the whole call is one group
        run (inner = n).  Returns counts, or (counts, skipped int64 device [1]) with want_skipped.  Nothing is copied back."""
        torch = self.torch
        self.bind_stream()
        types = {torch.uint8: 0, torch.int32: 1, torch.int64: 2}
        n = int(pred.numel())
        for t in (pred, labels):
            assert t.dtype in types and t.is_contiguous() and t.device == self.device and int(t.numel()) == n
        C, groups = int(C), int(groups)          # (the argument hides the module's ctypes alias here: _lib.C)
        inner = max(n, 1) if inner is None else int(inner)
        if counts is None:
            counts = torch.zeros((max(groups, 0), max(C, 0), max(C, 0)), dtype=torch.int64, device=self.device)
        assert counts.dtype == torch.int64 and counts.is_contiguous() and counts.device == self.device and \
            int(counts.numel()) == groups * C * C
        skipped = torch.zeros((1,), dtype=torch.int64, device=self.device) if want_skipped else None
        check(self.lib.alq_confusion_counts(self._ctx, _lib.C.c_void_p(pred.data_ptr()), types[pred.dtype], _lib.C.c_void_p(labels.data_ptr()),
                                            types[labels.dtype], n, int(first), inner, groups, C, int(fill), _lib.C.c_void_p(counts.data_ptr()),
                                            _lib.C.c_void_p(skipped.data_ptr()) if want_skipped else None))
        return (counts, skipped) if want_skipped else counts

    def unc_accumulate(self, post, sum_p, sum_h=None, first=False):
        """alq_unc_accumulate: one dropout pass `post` (float32 device [c, R], as the forward calls return it) into the float64
        device sums sum_p [c, R] (+= p) and sum_h [R] (+= -sum_j p_j log p_j; None: not kept).  first: assign instead of add."""
        torch = self.torch
        self.bind_stream()
        c, R = (int(v) for v in post.shape)
        assert post.dtype == torch.float32 and post.is_contiguous() and post.device == self.device
        for t, numel in ((sum_p, c * R), (sum_h, R)):
            assert t is None or (t.dtype == torch.float64 and t.is_contiguous() and t.device == self.device and int(t.numel()) == numel)
        check(self.lib.alq_unc_accumulate(self._ctx, C.c_void_p(post.data_ptr()), c, R, 1 if first else 0, C.c_void_p(sum_p.data_ptr()),
                                          C.c_void_p(sum_h.data_ptr()) if sum_h is not None else None))

    def slice_scores(self, kind, n_slices, V, c, T=1, sum_p=None, sum_h=None, f32=None, roi=None, scores=None, counts=None):
        """alq_slice_scores: per slice the SUM of the per-voxel value of `kind` (slice_query.KINDS: entropy of the float32
        posteriors f32 [c, R]; MC-entropy / BALD of the float64 sums of T passes; the float32 map f32 [R] itself) over the
        voxels whose `roi` byte (uint8 device [R], None: all) is non-zero, and their number: (scores float64, counts int64)
        device tensors [n_slices] (written into the ones given).  R = n_slices * V.  Nothing is copied back."""
        torch = self.torch
        self.bind_stream()
        n_slices, V, c = int(n_slices), int(V), int(c)
        R = n_slices * V
        if scores is None:
            scores = self.empty((max(n_slices, 0),), torch.float64)
        if counts is None:
            counts = self.empty((max(n_slices, 0),), torch.int64)
        for t, dt, numel in ((sum_p, torch.float64, c * R), (sum_h, torch.float64, R), (roi, torch.uint8, R), (scores, torch.float64, n_slices),
                             (counts, torch.int64, n_slices), (f32, torch.float32, None)):
            assert t is None or (t.dtype == dt and t.is_contiguous() and t.device == self.device and numel in (None, int(t.numel())))
        assert f32 is None or int(f32.numel()) in (R, c * R)

        def ptr(t):
            return C.c_void_p(t.data_ptr()) if t is not None else None
        check(self.lib.alq_slice_scores(self._ctx, int(kind), int(T), c, n_slices, V, ptr(sum_p), ptr(sum_h), ptr(f32), ptr(roi), ptr(scores),
                                        ptr(counts)))
        return scores, counts

    def cc_sizes(self, labels):
        """alq_cc_sizes: `labels` int32 device tensor as cc_label returns it -> int32 device tensor of its shape, the size of the
        component at every root voxel (the smallest raveled index of the component), 0 elsewhere."""
        torch = self.torch
        self.bind_stream()
        assert labels.dtype == torch.int32 and labels.is_contiguous() and labels.device == self.device
        sizes = self.empty(tuple(labels.shape), torch.int32)
        check(self.lib.alq_cc_sizes(self._ctx, C.c_void_p(labels.data_ptr()), int(labels.numel()), C.c_void_p(sizes.data_ptr())))
        return sizes

    def cc_relabel(self, labels, table=None, sizes=None, min_size=0):
        """alq_cc_relabel: with `table` (int32 device, one entry per voxel, read at the roots) the int32 image
        table[labels[v]] (0 where labels is -1); with `sizes` (cc_sizes) the uint8 mask sizes[labels[v]] >= min_size."""
        torch = self.torch
        self.bind_stream()
        if (table is None) == (sizes is None):
            raise ValueError('cc_relabel takes exactly one of table / sizes')
        n = int(labels.numel())
        for t in (labels, table, sizes):
            assert t is None or (t.dtype == torch.int32 and t.is_contiguous() and t.device == self.device and int(t.numel()) == n)
        out = self.empty(tuple(labels.shape), torch.int32 if table is not None else torch.uint8)
        check(self.lib.alq_cc_relabel(self._ctx, C.c_void_p(labels.data_ptr()), n, C.c_void_p(table.data_ptr()) if table is not None else None,
                                      C.c_void_p(sizes.data_ptr()) if sizes is not None else None, int(min_size),
                                      C.c_void_p(out.data_ptr()) if table is not None else None,
                                      C.c_void_p(out.data_ptr()) if table is None else None))
        return out

    # -- connected components, largest component, hole filling (csrc/ccl.hip) ---------------
    def _cc_args(self, seg, shape, out=None):
        torch = self.torch
        self.bind_stream()
        shape = tuple(int(v) for v in shape)
        if len(shape) == 2:
            shape = shape + (1,)
        assert len(shape) == 3 and min(shape) >= 1
        nvox = shape[0] * shape[1] * shape[2]
        for t in (seg, out):
            assert t is None or (t.dtype == torch.uint8 and t.is_contiguous() and t.device == self.device and int(t.numel()) == nvox)
        if nvox >= 2 ** 31:
            raise ValueError('volume %r has 2^31 voxels or more' % (shape,))
        return shape, nvox, (C.c_int64 * 3)(*shape)

    def _cc_work(self, dims):
        return self.empty((int(self.lib.alq_cc_work_bytes(dims)),), self.torch.uint8), self.empty((4,), self.torch.int64)

    def cc_label(self, seg, shape, connectivity=26, select_zero=False):
        """alq_cc_label: the canonical component labels of a uint8 device volume `seg` of `shape` [H, W, S] (or [H, W]): int32
        device tensor of that shape, for a selected voxel (!= 0; == 0 with select_zero) the smallest raveled index of its 6- /
        18- / 26-connected component, -1 elsewhere."""
        shape, nvox, dims = self._cc_args(seg, shape)
        labels = self.empty(shape, self.torch.int32)
        check(self.lib.alq_cc_label(self._ctx, C.c_void_p(seg.data_ptr()), dims, int(connectivity), 1 if select_zero else 0,
                                    C.c_void_p(labels.data_ptr())))
        return labels

    def cc_keep_largest(self, seg, shape, connectivity=26, skip_origin=True, out=None):
        """alq_cc_keep_largest: (mask, info) - the uint8 device mask (of `shape`; `out`, which may be `seg` itself, when given)
        of the largest component of the non-zero voxels, equal sizes -> the component that starts first in C order, without
        the component of voxel 0 when skip_origin; info = np.int64 [4] (candidates, winner's root or -1, its size, non-zero
        voxels), one copy of 32 bytes.  No candidate: an all-zero mask."""
        shape, nvox, dims = self._cc_args(seg, shape, out)
        if out is None:
            out = self.empty(shape, self.torch.uint8)
        work, info = self._cc_work(dims)
        check(self.lib.alq_cc_keep_largest(self._ctx, C.c_void_p(seg.data_ptr()), dims, int(connectivity), 1 if skip_origin else 0,
                                           C.c_void_p(out.data_ptr()), C.c_void_p(info.data_ptr()), C.c_void_p(work.data_ptr())))
        return out, info.cpu().numpy()

    def fill_holes(self, seg, shape, out=None):
        """alq_fill_holes: (mask, info) - uint8 device mask = seg != 0 or inside a 6-connected background component that
        touches no face of the volume (scipy's binary_fill_holes); info = np.int64 [4] (enclosed components, voxels filled,
        0, 0), one copy of 32 bytes.  `out` may be `seg` itself."""
        shape, nvox, dims = self._cc_args(seg, shape, out)
        if out is None:
            out = self.empty(shape, self.torch.uint8)
        work, info = self._cc_work(dims)
        check(self.lib.alq_fill_holes(self._ctx, C.c_void_p(seg.data_ptr()), dims, C.c_void_p(out.data_ptr()),
                                      C.c_void_p(info.data_ptr()), C.c_void_p(work.data_ptr())))
        return out, info.cpu().numpy()

    # -- surface distances: surface voxels, exact distance transform, masked reductions (csrc/edt.hip) ---
    def surface_mask(self, seg, shape, label=None, out=None):
        """alq_surface_mask: uint8 device mask (of `shape` [H, W, S] or [H, W]) of the foreground voxels of the uint8 device
        volume `seg` that have a 6-neighbour which is background or outside the volume; foreground is seg != 0 (label None or
        negative) or seg == label.  An axis of extent 1 is ignored.  `out` may not be `seg`."""
        shape, nvox, dims = self._cc_args(seg, shape, out)
        if out is None:
            out = self.empty(shape, self.torch.uint8)
        assert out.data_ptr() != seg.data_ptr() or nvox == 0
        check(self.lib.alq_surface_mask(self._ctx, C.c_void_p(seg.data_ptr()), dims, -1 if label is None else int(label),
                                        C.c_void_p(out.data_ptr())))
        return out

    def edt_sq(self, feat, shape, spacing=(1., 1., 1.), out=None):
        """alq_edt_sq: float64 device tensor of `shape` [H, W, S] (or [H, W]) = the exact squared Euclidean distance from every
        voxel to the nearest non-zero voxel of the uint8 device volume `feat` (+inf everywhere when there is none), voxel
        spacings `spacing` (h, w, z; two values for an image).  Bit-equal to surfdist.edt_sq_host."""
        torch = self.torch
        shape, nvox, dims = self._cc_args(feat, shape)
        sp = [np.float64(s) for s in spacing]
        if len(sp) == 2:
            sp.append(np.float64(1.))
        assert len(sp) == 3
        s2 = (C.c_double * 3)(*[float(s * s) for s in sp])
        if out is None:
            out = self.empty(shape, torch.float64)
        assert out.dtype == torch.float64 and out.is_contiguous() and out.device == self.device and int(out.numel()) == nvox
        work = self.empty((max(int(self.lib.alq_edt_work_bytes(dims)), 8),), torch.uint8)
        check(self.lib.alq_edt_sq(self._ctx, C.c_void_p(feat.data_ptr()), dims, s2, C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr())))
        return out

    # -- whole-volume inference by tiles: gather, blend, finalize (csrc/tile.hip; statement: tiled.py) ---
    @staticmethod
    def tile_lattice(dims, tile, stride):
        """The alq_tile_lattice_t of a volume `dims`, `tile` and `stride`, each (Z, H, W); ValueError with the library's message for a
        lattice it refuses."""
        lat = _lib.TileLattice((C.c_int32 * 3)(*[int(v) for v in dims]), (C.c_int32 * 3)(*[int(v) for v in tile]),
                               (C.c_int32 * 3)(*[int(v) for v in stride]))
        if _lib.lib().alq_tile_lattice_check(C.byref(lat)) != 0:
            raise ValueError(_lib.lib().alq_last_error().decode())
        return lat

    def tile_count(self, lat):
        return int(self.lib.alq_tile_count(C.byref(lat), None))

    def tile_gather(self, vol, lat, first, n, fill=0., out=None):
        """alq_tile_gather: the tiles first .. first + n - 1 of the packed float32 device volume `vol` [Z, H, W, m] as a float32
        device tensor [n, tz, th, tw, m] (`out` when given); what lies outside the volume is `fill`."""
        torch = self.torch
        self.bind_stream()
        m = int(vol.shape[-1])
        assert vol.dtype == torch.float32 and vol.is_contiguous() and vol.device == self.device
        assert tuple(int(v) for v in vol.shape[:3]) == tuple(lat.dims)
        shape = (max(int(n), 0),) + tuple(lat.tile) + (m,)
        if out is None:
            out = self.empty(shape, torch.float32)
        assert out.dtype == torch.float32 and out.is_contiguous() and out.device == self.device and tuple(out.shape) == shape
        check(self.lib.alq_tile_gather(self._ctx, C.c_void_p(vol.data_ptr()), m, C.byref(lat), int(first), int(n), float(fill),
                                       C.c_void_p(out.data_ptr())))
        return out

    def tile_blend(self, post, lat, first, n, windows, acc):
        """alq_tile_blend: adds the posteriors `post` (float32 device [c, n V], class-major planes as the forward calls return them)
        of the tiles first .. first + n - 1, weighted by the float32 device window tables `windows` = (wz, wh, ww), into the
        float32 device accumulator `acc` [c + 1, Z, H, W] (zeroed by the caller before the first call)."""
        torch = self.torch
        self.bind_stream()
        c, V = int(acc.shape[0]) - 1, int(np.prod(tuple(lat.tile)))
        for t, numel in ((post, c * int(n) * V), (acc, (c + 1) * int(np.prod(tuple(lat.dims))))) + tuple(zip(windows, tuple(lat.tile))):
            assert t.dtype == torch.float32 and t.is_contiguous() and t.device == self.device and int(t.numel()) == numel
        check(self.lib.alq_tile_blend(self._ctx, C.c_void_p(post.data_ptr()), c, C.byref(lat), int(first), int(n),
                                      *[C.c_void_p(t.data_ptr()) for t in windows], C.c_void_p(acc.data_ptr())))
        return acc

    def tile_finalize(self, acc, hwz=True, want_post=True, want_label=True, post=None, label=None):
        """alq_tile_finalize of the accumulator `acc` [c + 1, Z, H, W]: (posteriors float32 [c, H, W, Z] or None, labels uint8
        [H, W, Z] or None) with hwz, else [c, Z, H, W] / [Z, H, W]; written into `post` / `label` when given."""
        torch = self.torch
        self.bind_stream()
        c = int(acc.shape[0]) - 1
        Z, H, W = (int(v) for v in acc.shape[1:])
        assert acc.dtype == torch.float32 and acc.is_contiguous() and acc.device == self.device
        shape = (H, W, Z) if hwz else (Z, H, W)
        if post is None and want_post:
            post = self.empty((c,) + shape, torch.float32)
        if label is None and want_label:
            label = self.empty(shape, torch.uint8)
        for t, dt, numel in ((post, torch.float32, c * Z * H * W), (label, torch.uint8, Z * H * W)):
            assert t is None or (t.dtype == dt and t.is_contiguous() and t.device == self.device and int(t.numel()) == numel)
        check(self.lib.alq_tile_finalize(self._ctx, C.c_void_p(acc.data_ptr()), c, (C.c_int32 * 3)(Z, H, W), 1 if hwz else 0,
                                         C.c_void_p(post.data_ptr()) if post is not None else None,
                                         C.c_void_p(label.data_ptr()) if label is not None else None))
        return post, label

    def _masked_args(self, d2, mask):
        torch = self.torch
        self.bind_stream()
        n = int(d2.numel())
        assert d2.dtype == torch.float64 and d2.is_contiguous() and d2.device == self.device
        assert mask.dtype == torch.uint8 and mask.is_contiguous() and mask.device == self.device and int(mask.numel()) == n
        if n >= 2 ** 31:
            raise ValueError('2^31 elements or more')
        return n, self.empty((int(self.lib.alq_masked_work_bytes(n)),), torch.uint8)

    def masked_dist_stats(self, d2, mask):
        """alq_masked_dist_stats: np.float64 [4] = (count, sum of sqrt(d2), max of d2, min of d2) over the elements of the float64
        device tensor `d2` whose byte of the uint8 device tensor `mask` is non-zero (empty: 0, 0, -inf, +inf); one copy of 32
        bytes.  The same bits on every run."""
        n, work = self._masked_args(d2, mask)
        out = self.empty((4,), self.torch.float64)
        check(self.lib.alq_masked_dist_stats(self._ctx, C.c_void_p(d2.data_ptr()), C.c_void_p(mask.data_ptr()), n, C.c_void_p(out.data_ptr()),
                                             C.c_void_p(work.data_ptr())))
        return out.cpu().numpy()

    def masked_select(self, d2, mask, ranks):
        """alq_masked_select: np.float64 [len(ranks)] (at most 8) = the ranks[r]-th smallest (0-based) of the masked entries of
        `d2` (non-negative or +inf), NaN for a rank at or above the masked count; one copy of 8 bytes per rank."""
        n, work = self._masked_args(d2, mask)
        ranks = [int(r) for r in ranks]
        out = self.empty((len(ranks),), self.torch.float64)
        check(self.lib.alq_masked_select(self._ctx, C.c_void_p(d2.data_ptr()), C.c_void_p(mask.data_ptr()), n, (C.c_int64 * max(len(ranks), 1))(*ranks),
                                         len(ranks), C.c_void_p(out.data_ptr()), C.c_void_p(work.data_ptr())))
        return out.cpu().numpy()

    # -- dense CRF on a two-class posterior map (csrc/dcrf.hip) ------------------------------
    def dcrf2d(self, post, img, dims, params=None, want_q=False):
        """alq_dcrf2d: the dense CRF of DCRF_postprocess_2D (nnal_amd.dcrf states the model) on S independent slices,
        dims = [S, H, W] (or [H, W]: one slice).  `post`, `img`: class-1 posteriors and image, float32 device tensors of S H W
        elements (neither is written) or arrays, which are uploaded as float32; zeros of a NumPy `post` become 1e-10 in the
        caller's array, as the reference's call leaves them.  `params`: a dict of dcrf.DEFAULTS entries and / or `niter` to
        replace (None: the reference's values, 5 iterations).  Returns the uint8 device tensor [S, H, W] of MAP labels, or
        (labels, q1) with the float32 class-1 marginals after the last iteration when want_q.  Nothing is copied back."""
        from . import dcrf
        torch = self.torch
        self.bind_stream()
        dims = tuple(int(v) for v in dims)
        if len(dims) == 2:
            dims = (1,) + dims
        assert len(dims) == 3 and min(dims) >= 1
        n = dims[0] * dims[1] * dims[2]
        if isinstance(post, np.ndarray):
            post[post == 0] += 1e-10                      # PW_analyze_results.py:549
        tens = []
        for t in (post, img):
            if not isinstance(t, torch.Tensor):
                t = self.to_device(np.ascontiguousarray(t, dtype=np.float32), torch.float32)
            assert t.dtype == torch.float32 and t.is_contiguous() and t.device == self.device and int(t.numel()) == n
            tens.append(t)
        kw = dict(params or {})
        niter = int(kw.pop('niter', dcrf.NITER))
        par = dcrf.make_params(**kw)
        cpar = _lib.DcrfParams((C.c_float * 2)(*par['sdims_smooth']), (C.c_float * 2)(*par['sdims_app']), par['schan'],
                               par['compat_smooth'], par['compat_app'], niter)
        cdims = (C.c_int64 * 3)(*dims)
        work = self.empty((max(4, int(self.lib.alq_dcrf_work_bytes(cdims))),), torch.uint8)
        labels = self.empty(dims, torch.uint8)
        q1 = self.empty(dims, torch.float32) if want_q else None
        check(self.lib.alq_dcrf2d(self._ctx, C.c_void_p(tens[0].data_ptr()), C.c_void_p(tens[1].data_ptr()), cdims, C.byref(cpar),
                                  C.c_void_p(q1.data_ptr()) if want_q else None, C.c_void_p(labels.data_ptr()),
                                  C.c_void_p(work.data_ptr())))
        return (labels, q1) if want_q else labels

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
        assert t.dtype == self.torch.float64 and t.is_contiguous()
        self.bind_stream()
        check(self.lib.alq_allreduce_sum(self._ctx, C.c_void_p(t.data_ptr()), t.numel()))
        return t

    # -- A-optimal design of the `fi` query (csrc/aopt.hip) -------------------------------------
    # One method per launch: host scalars / vectors of size m in, the launch's O(m^2) reduction outputs back as host values
    # (one synchronising read-back each).  V [n, m], q, dq [n]: fp64 device tensors; work: aopt_work(n, L).
    def aopt_tile(self):
        return int(self.lib.alq_aopt_tile())

    def aopt_work(self, n, L):
        return self.empty((int(self.lib.alq_aopt_work_bytes(int(n), int(L))),), self.torch.uint8)

    def _aopt_args(self, *tensors):
        self.bind_stream()
        for t in tensors:
            assert t.dtype == self.torch.float64 and t.is_contiguous() and t.device == self.device
        return [C.c_void_p(t.data_ptr()) for t in tensors]

    @staticmethod
    def _h64(a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        return a, C.c_void_p(a.ctypes.data)

    def aopt_svec(self, A_dev):
        n, L = int(A_dev.shape[0]), int(A_dev.shape[1])
        V = self.empty((n, L * (L + 1) // 2), self.torch.float64)
        pA, pV = self._aopt_args(A_dev, V)
        check(self.lib.alq_aopt_svec(self._ctx, pA, n, L, pV))
        return V

    def aopt_stats(self, V, q, kvec, R, mu, obj, work):
        """alq_aopt_stats -> dict(G [m, m], h_r, h_1 [m], s_r, s_1, maxd)."""
        n, m = int(V.shape[0]), int(V.shape[1])
        ne = (m + 2) * (m + 3) // 2
        out = self.empty((ne + 1,), self.torch.float64)
        pV, pq, po = self._aopt_args(V, q, out)
        kvec, pk = self._h64(kvec)
        R, pR = self._h64(R)
        check(self.lib.alq_aopt_stats(self._ctx, pV, pq, n, m, pk, pR, float(mu), float(obj), po, C.c_void_p(work.data_ptr())))
        o = out.cpu().numpy()
        S = np.zeros((m + 2, m + 2))
        S[np.triu_indices(m + 2)] = o[:ne]
        G = S[:m, :m]
        return {'G': G + G.T - np.diag(np.diag(G)), 'h_r': S[:m, m].copy(), 'h_1': S[:m, m + 1].copy(), 's_r': float(S[m, m + 1]),
                's_1': float(S[m + 1, m + 1]), 'maxd': float(o[ne])}

    def aopt_direction(self, V, q, kvec, R, c_r, c_1, ratio, mu, obj, dq, work):
        """alq_aopt_direction: writes the device vector dq -> dict(dec, minratio, vdq [m])."""
        n, m = int(V.shape[0]), int(V.shape[1])
        out = self.empty((2 + m,), self.torch.float64)
        pV, pq, pd, po = self._aopt_args(V, q, dq, out)
        kvec, pk = self._h64(kvec)
        R, pR = self._h64(R)
        c_r, pcr = self._h64(c_r)
        c_1, pc1 = self._h64(c_1)
        check(self.lib.alq_aopt_direction(self._ctx, pV, pq, n, m, pk, pR, pcr, pc1, float(ratio), float(mu), float(obj), pd, po,
                                          C.c_void_p(work.data_ptr())))
        o = out.cpu().numpy()
        return {'dq': dq, 'dec': float(o[0]), 'minratio': float(o[1]), 'vdq': o[2:].copy()}

    def aopt_linesearch(self, q, dq, alphas, work):
        """alq_aopt_linesearch -> [J + 1]: sum log(q + alpha_j dq) for every j, then sum log q."""
        J = len(alphas)
        out = self.empty((J + 1,), self.torch.float64)
        pq, pd, po = self._aopt_args(q, dq, out)
        alphas, pa = self._h64(alphas)
        check(self.lib.alq_aopt_linesearch(self._ctx, pq, pd, int(q.numel()), pa, J, po, C.c_void_p(work.data_ptr())))
        return out.cpu().numpy()

    def aopt_update(self, q, dq, V, alpha, work):
        """alq_aopt_update: q <- (q + alpha dq) / sum, in place -> (sum before the division, sum_i q_i V_i [m])."""
        n, m = int(V.shape[0]), int(V.shape[1])
        out = self.empty((1 + m,), self.torch.float64)
        pq, pd, pV, po = self._aopt_args(q, dq, V, out)
        check(self.lib.alq_aopt_update(self._ctx, pq, pd, pV, n, m, float(alpha), po, C.c_void_p(work.data_ptr())))
        o = out.cpu().numpy()
        return float(o[0]), o[1:].copy()

    def aopt_design(self, A_dev, tol=1e-7, max_iter=500):
        """The query distribution of Fisher-information AL at lambda = 0 - min tr((sum q_i A_i)^-1) over the simplex - with the
        candidates on the device: the loop of NNAL_tools._aopt_newton, its O(n) work done by the four launches of csrc/aopt.hip
        and its L x L / m x m algebra (m = L(L+1)/2) in NumPy as there.  A_dev: fp64 device tensor [n, L, L]
        (fisher_device(..., want=('A',))).  Returns a dict like NNAL_tools.SDP_query_distribution's: 'x' = concat(q, t) on the
        host, 'q_device' the device vector, 'status', 'primal objective', 'gap', 'iterations', 'y'.  L > 8 (or a pool the
        library refuses) is solved by the host routine; 'status' says so."""
        from scipy.linalg import cho_factor, cho_solve
        from . import NNAL_tools
        torch = self.torch
        assert A_dev.dim() == 3 and A_dev.shape[1] == A_dev.shape[2] and A_dev.dtype == torch.float64 and A_dev.device == self.device
        A_dev = A_dev.contiguous()
        n, L = int(A_dev.shape[0]), int(A_dev.shape[1])
        m = L * (L + 1) // 2

        def on_host(why):
            soln = NNAL_tools.SDP_query_distribution(A_dev.cpu().numpy(), 0., [], None, tol=tol, max_iter=max_iter)
            soln['status'] += ' [solved on the host: %s]' % why
            soln['q_device'] = self.to_device(soln['x'][:n], torch.float64)
            return soln
        if L > 8 or n < 1 or n >= (1 << 31) // m:
            return on_host('n = %d, L = %d is outside the device solver' % (n, L))
        P = NNAL_tools._svec_basis(L)
        try:
            work = self.aopt_work(n, L)
            V = self.aopt_svec(A_dev)
        except _lib.AlqError as e:
            return on_host(str(e))

        def at(v):
            Mi = np.linalg.inv((P @ v).reshape(L, L))
            return Mi, float(np.trace(Mi))

        def factors(Mi):
            Mi2 = Mi @ Mi
            K = P.T @ (np.kron(Mi, Mi2) + np.kron(Mi2, Mi)) @ P
            return P.T @ Mi2.reshape(-1), np.linalg.cholesky(0.5 * (K + K.T))

        q = torch.full((n,), 1.0 / n, dtype=torch.float64, device=self.device)
        dq = torch.zeros((n,), dtype=torch.float64, device=self.device)
        _, vq = self.aopt_update(q, dq, V, 0.0, work)
        Mi, obj = at(vq)
        mu = obj / n
        status, steps, maxd = 'unknown', 0, None
        max_iter = min(int(max_iter), 500)
        while steps < max_iter:
            steps += 1
            kvec, R = factors(Mi)
            st = self.aopt_stats(V, q, kvec, R, mu, obj, work)
            maxd = st['maxd']
            if maxd <= obj * (1.0 + tol):                      # optimality condition d_i <= tr M^-1 for every i
                status = 'optimal'
                break
            S = cho_factor(np.eye(m) + st['G'])
            c_r, c_1 = cho_solve(S, st['h_r']), cho_solve(S, st['h_1'])
            ratio = (st['s_r'] - st['h_1'] @ c_r) / (st['s_1'] - st['h_1'] @ c_1)
            di = self.aopt_direction(V, q, kvec, R, c_r, c_1, ratio, mu, obj, dq, work)
            dec = di['dec']
            alphas = [min(1.0, 0.99 * di['minratio']) if np.isfinite(di['minratio']) else 1.0]
            while alphas[-1] >= 1e-12 and len(alphas) < 64:    # every step the halving loop could test, in one launch
                alphas.append(alphas[-1] * 0.5)
            ls = self.aopt_linesearch(q, dq, alphas, work)
            phi0 = obj - mu * ls[len(alphas)]
            slack = 1e-12 * abs(phi0)
            for j, alpha in enumerate(alphas):
                _, on = at(vq + alpha * di['vdq'])
                if on - mu * ls[j] <= phi0 - 0.25 * alpha * dec + slack or alpha < 1e-12:
                    break
            _, vq = self.aopt_update(q, dq, V, alpha, work)
            Mi, obj = at(vq)
            maxd = None
            if dec <= 0.05 * mu * n:                           # centred for this mu
                mu = max(0.2 * mu, 0.25 * tol * obj / n)
        if maxd is None:                                       # the step limit ended the loop: the gap of the last iterate
            kvec, R = factors(Mi)
            maxd = self.aopt_stats(V, q, kvec, R, mu, obj, work)['maxd']
        t = np.diag(Mi).copy()
        return {'x': np.concatenate((q.cpu().numpy(), t)), 'q_device': q,
                'status': '%s (log-barrier Newton A-optimal design on the device; not cvxopt)' % status,
                'primal objective': float(t.sum()), 'gap': float(maxd / t.sum() - 1.0), 'iterations': steps,
                'y': np.array([float(kvec @ vq)])}

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
        torch = self.torch
        t = torch.as_tensor(np.ascontiguousarray(arr))
        return t.to(device=self.device, dtype=dtype)

    def empty(self, shape, dtype):
        return self.torch.empty(shape, dtype=dtype, device=self.device)

    # -- sess.run compatibility -----------------------------------------------------------
    def run(self, fetch, feed_dict=None):
        """`sess.run(fetch, feed_dict={model.x: batch, model.keep_prob: p, model.y_: labels})` for the fetches the
        reference's query / fine-tune code uses: `model.posteriors`, `.prediction`, `.feature_layer` (PW_NN.py:522),
        `model.grad_posts[str(j)]` (PW_NNAL.py:773-807: list of 2L' gradient arrays of log posteriors[j, 0]) and
        `model.train_step` (PW_AL.py:1075-1080, :1140-1146); of the influence functions (Influence.py): `model.loss` (scalar
        mean cross-entropy, needs `model.y_`), `model.loss_grad` (NN.add_loss_grad) and `model.hess_vecp` with the entries of
        `model.v_placeholder` in the feed (Influence.get_hess_vec_product).  Per-sample loss weights fed under
        `model.input_weights` (or an `input_vox_weights` attribute of the model; the reference tests for one name and reads the
        other, NN_extended.py:1252-1255) multiply the weights of the cross-entropy; `model.LwF_train_step` (model_utils.get_LwF)
        takes `model.y__`, `model.lambda_o` and `model.T` as well; `model.labels` / `model.pt` are the label vector and the
        posterior of each sample's label as the two-class focal term reads them (NN_extended.py:1228-1231)."""
        model = getattr(fetch, 'model', None)
        if isinstance(fetch, list):
            model = getattr(fetch[0], 'model', None) if fetch else None
            if model is None:
                raise KeyError('unknown fetch list')
            x = feed_dict[model.x]
            kp = float(feed_dict.get(model.keep_prob, 1.))
            j = fetch[0].cls
            return model.grad_log_post(x, j, keep_prob=kp)
        if model is None:
            raise KeyError('unknown fetch %r' % (fetch,))
        if fetch.name == 'ema_apply':          # (NN_extended.py:1006-1008: run without a feed)
            return model.apply_ema()
        x = feed_dict[model.x]
        kp = float(feed_dict.get(model.keep_prob, 1.))
        iw = None
        for h in (getattr(model, 'input_weights', None), getattr(model, 'input_vox_weights', None)):
            if h is not None and h in feed_dict:
                iw = feed_dict[h]
        if getattr(model, 'dense', False):
            return model._run_dense(fetch, feed_dict, x, kp, iw)
        if fetch.name == 'LwF_train_step':
            lwf = (feed_dict[model.y__], float(feed_dict[model.lambda_o]), float(feed_dict[model.T]))
            return model.train_on_batch(x, feed_dict[model.y_], keep_prob=kp, input_weights=iw, lwf=lwf)
        if fetch.name == 'LwF_loss':
            lwf = (feed_dict[model.y__], float(feed_dict[model.lambda_o]), float(feed_dict[model.T]))
            return model.lwf_loss(x, feed_dict[model.y_], lwf, keep_prob=kp, input_weights=iw)
        if fetch.name in ('labels', 'pt'):
            lab = onehot_to_labels(feed_dict[model.y_], model.nclass)
            if fetch.name == 'labels':
                return lab
            post = model.forward(x, want=('posteriors',), keep_prob=kp)['posteriors']
            return np.where(lab == 1, post[1], post[0])
        if fetch.name == 'train_step':
            # NN_extended.get_optimizer (NN_extended.py:1441-1449): masks fed under model.par_placeholders hold for this step
            ph = getattr(model, 'par_placeholders', None)
            fed = [h in feed_dict for h in ph] if ph else []
            if any(fed):
                if not all(fed):
                    raise KeyError('a PFT step needs a mask for every entry of par_placeholders')
                return model.train_on_batch(x, feed_dict[model.y_], keep_prob=kp, pft_mask=[feed_dict[h] for h in ph], input_weights=iw)
            return model.train_on_batch(x, feed_dict[model.y_], keep_prob=kp, input_weights=iw)
        if fetch.name in ('loss', 'loss_grad', 'hess_vecp'):
            # the training-time graph nodes of the influence functions (NN.py:583-588, :862-871; Influence.py:126-166)
            if kp != 1.:
                raise NotImplementedError('%s at keep_prob < 1' % fetch.name)
            model._check_input_weights(iw)
            if model._obj is not None:
                # an NN_extended objective: soft targets are read as they are fed
                if fetch.name == 'hess_vecp':
                    model._require_default_objective('hess_vecp')
                if fetch.name == 'loss':
                    return model.mean_loss(x, None, targets=feed_dict[model.y_], input_weights=iw)
                return model.mean_loss_grad(x, None, fetch.layers, targets=feed_dict[model.y_], input_weights=iw)
            lab = onehot_to_labels(feed_dict[model.y_], model.nclass)
            if fetch.name == 'loss':
                return model.mean_loss(x, lab)
            if fetch.name == 'loss_grad':
                return model.mean_loss_grad(x, lab, fetch.layers)
            v = [feed_dict[h] for h in model.v_placeholder]
            return DeviceModel.hess_vecp(model, x, lab, v, layers=model.Hess_layers)
        res = model.forward(x, want=(fetch.name,), keep_prob=kp)
        return res[fetch.name]

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


# ------------------------------------------------------------------------------------------
def onehot_to_labels(y_onehot, nclass):
    """[c, n] one-hot columns (the reference's hot_labels, PW_NN.py:494-496) -> int32 labels; an all-zero column (a mask
    value that is no class) -> -1: the sample adds nothing to the loss, as its zero row does in the reference's sum."""
    y = np.asarray(y_onehot)
    if y.ndim != 2 or y.shape[0] != nclass:
        raise ValueError('labels must be [%d, n] one-hot columns, got %r' % (nclass, y.shape))
    return np.where(y.sum(0) > 0, y.argmax(0), -1).astype(np.int32)


def _is_extended(layer_dict):
    first = next(iter(layer_dict.values()))
    return isinstance(first[0], str)


def translate_layers(layer_dict, in_shape, skips=()):
    """Reference layer dict (either schema) -> list of dicts in alq_layer_t terms + bookkeeping.

    `in_shape` is the placeholder shape without batch, channels last: (H, W, C) for `NN.CNN`
    / 2-D `NN_extended.CNN`, (D, H, W, C) for 3-D.  Pure host logic (unit-tested on CPU)."""
    ext = _is_extended(layer_dict)
    nd = len(in_shape) - 1
    if nd not in (2, 3):
        raise ValueError('input must be [H,W,C] or [D,H,W,C], got %r' % (in_shape,))
    names = list(layer_dict.keys())

    def pad3(v, fill=1):
        v = list(v)
        return [fill] * (3 - len(v)) + v

    skip_src = {}
    for sk in skips:
        src, dsts, kind = sk
        if kind != 'con':
            raise NotImplementedError("skip type %r: only 'con' is on the scored path" % kind)
        for d in dsts:
            if d in skip_src:
                raise NotImplementedError('layer %d has more than one skip source' % d)
            skip_src[d] = src
    out = []
    for i, name in enumerate(names):
        spec = layer_dict[name]
        last = i == len(names) - 1
        if ext:
            ltype, lspec = spec[0], spec[1]
            order = spec[2] if len(spec) > 2 else 'M'
            if 'B' in order:
                raise NotImplementedError('batch-norm op in layer %s is outside the scored path' % name)
            if order.replace('A', '').replace('M', '') or not order.startswith('M'):
                raise NotImplementedError('op order %r of layer %s' % (order, name))
            relu = 1 if 'A' in order else 0
        else:
            ltype = spec[1]
            relu = 1 if (ltype == 'conv' or (ltype == 'fc' and not last)) else 0
        d = dict(name=name, relu=relu, skip_src=skip_src.get(i, -1), k=[1, 1, 1], s=[1, 1, 1], cout=0)
        if ltype == 'conv':
            d['type'] = ALQ_CONV
            if ext:
                d['cout'] = int(lspec[0])
                d['k'] = pad3(lspec[1])
                if len(lspec) > 2:
                    d['s'] = pad3(lspec[2])
            else:
                d['cout'] = int(spec[0])
                d['k'] = pad3(spec[2])
        elif ltype == 'conv_transpose':
            d['type'] = ALQ_CONVT
            d['cout'] = int(lspec[0])
            d['k'] = pad3(lspec[1])
            d['s'] = pad3(lspec[2])
        elif ltype == 'pool':
            d['type'] = ALQ_POOL
            if ext:
                d['k'] = pad3(lspec)
                d['s'] = pad3(lspec)
            else:
                w, s = spec[0]          # max_pool(x, pool_size[0], pool_size[1]), NN.py:333-335
                d['k'] = pad3([w] * nd)
                d['s'] = pad3([s] * nd)
        elif ltype == 'fc':
            d['type'] = ALQ_FC
            d['cout'] = int(lspec[0]) if ext else int(spec[0])
        else:
            raise ValueError("layer type %r" % (ltype,))
        out.append(d)
    return out


def tf_param_shapes(layers, in_shape):
    """TF variable shapes [(name, W_shape, b_shape)] of the parameterised layers, creation order
    (NN.py:272-277,313-318; NN_extended.py:397-404,436-441,555-561)."""
    nd = len(in_shape) - 1
    spatial = list(in_shape[:-1])
    ch = in_shape[-1]
    chans = {}
    flat = None
    out = []
    for i, d in enumerate(layers):
        if d['skip_src'] >= 0:
            ch += chans[d['skip_src']]
        if d['type'] == ALQ_CONV:
            out.append((d['name'], tuple(d['k'][3 - nd:]) + (ch, d['cout']), (d['cout'],)))
            ch = d['cout']
        elif d['type'] == ALQ_CONVT:
            out.append((d['name'], tuple(d['k'][3 - nd:]) + (d['cout'], ch), (d['cout'],)))
            spatial = [a * b for a, b in zip(spatial, d['s'][3 - nd:])]
            ch = d['cout']
        elif d['type'] == ALQ_POOL:
            spatial = [-(-a // b) for a, b in zip(spatial, d['s'][3 - nd:])]
        else:
            if flat is None:
                flat = int(np.prod(spatial)) * ch
            out.append((d['name'], (d['cout'], flat), (d['cout'], 1)))
            flat = d['cout']
        chans[i] = ch
    return out


def out_map_shape(layers, in_shape):
    """Spatial shape of the last layer's output map (SAME padding: pools round up, transposed convs multiply)."""
    nd = len(in_shape) - 1
    spatial = [int(v) for v in in_shape[:-1]]
    for d in layers:
        if d['type'] == ALQ_CONVT:
            spatial = [a * b for a, b in zip(spatial, d['s'][3 - nd:])]
        elif d['type'] == ALQ_POOL:
            spatial = [-(-a // b) for a, b in zip(spatial, d['s'][3 - nd:])]
    return tuple(spatial)


class LazyVarDict(OrderedDict):
    """`model.var_dict`: name -> [W, b] host arrays in TF layouts.  When the weights were last set from device memory
    (DeviceModel.set_weights_device, every training step) the host copies are stale: `refresh` - a callable that fetches
    them and stores them with `put` - is armed with `mark_stale` and runs once, on the first access that reads a value.
    Names, length and membership never need the device."""

    def __init__(self, *args, **kwargs):
        self._refresh = None
        OrderedDict.__init__(self, *args, **kwargs)

    def mark_stale(self, refresh):
        self._refresh = refresh

    def mark_fresh(self):
        self._refresh = None

    @property
    def stale(self):
        return self._refresh is not None

    def put(self, name, value):
        """Stores a value without touching the stale mark (what the refresh callable uses)."""
        OrderedDict.__setitem__(self, name, value)

    def _sync(self):
        fn = self._refresh
        if fn is not None:
            self._refresh = None          # first: the callable reads nothing through us, but an error must not loop
            try:
                fn()
            except Exception:
                self._refresh = fn
                raise

    def __getitem__(self, name):
        self._sync()
        return OrderedDict.__getitem__(self, name)

    def get(self, name, default=None):
        self._sync()
        return OrderedDict.get(self, name, default)

    def values(self):
        self._sync()
        return OrderedDict.values(self)

    def items(self):
        self._sync()
        return OrderedDict.items(self)

    def copy(self):
        self._sync()
        return OrderedDict(OrderedDict.items(self))


class DeviceModel(object):
    """The reference model protocol (`x, keep_prob, posteriors, prediction, feature_layer,
    grad_posts, var_dict, dropout_rate`) over a libalq model."""

    def __init__(self, sess, layer_dict, in_shape, skips=(), feature_layer=None, dropout=None,
                 max_batch=256, name='model', aleatoric=False, au_log_rel_coeff=0.1):
        self.sess = sess
        self.lib = sess.lib
        self.name = name
        self.layer_dict = layer_dict
        self.in_shape = tuple(int(v) for v in in_shape)
        self.skips = [list(s) for s in skips]
        self.max_batch = int(max_batch)
        self.layers = translate_layers(layer_dict, self.in_shape, skips)
        self.param_shapes = tf_param_shapes(self.layers, self.in_shape)
        self.var_names = [p[0] for p in self.param_shapes]
        nd = len(self.in_shape) - 1
        dims = [1] * (3 - nd) + list(self.in_shape[:-1]) + [self.in_shape[-1]]
        arr = (LayerT * len(self.layers))()
        for i, d in enumerate(self.layers):
            arr[i].type = d['type']
            arr[i].cout = d['cout']
            arr[i].k[:] = d['k']
            arr[i].s[:] = d['s']
            arr[i].relu = d['relu']
            arr[i].skip_src = d['skip_src']
        self._m = C.c_void_p()
        cd = (C.c_int32 * 4)(*dims)
        self._create_args = (arr, len(self.layers), cd)
        check(self.lib.alq_model_create(sess.ctx, arr, len(self.layers), cd, self.max_batch, C.byref(self._m)))
        _track(self)
        self.max_batch = int(self.lib.alq_model_max_batch(self._m))      # may be below the request: 32-bit tensor offsets (alq.h)
        # extra scoring pipelines (fisher_device): created at the first call that has that many device passes to run.  Default
        # since round 6: two (ALQ_LANES=1: one pipeline; up to 4: three measured no faster than two, four slower): outputs are
        # bit-identical; each costs a set of workspaces
        self.lanes = max(1, min(4, int(os.environ.get('ALQ_LANES', '2'))))
        self._xlanes = []                 # the extra pipelines (lanes - 1 of them once a call spans that many passes)
        self._create_env = {k: v for k, v in os.environ.items() if k.startswith('ALQ_')}     # engine switches are read at creation
        self.L = self.lib.alq_model_num_param_layers(self._m)
        self.nclass = self.layers[-1]['cout']
        # AU_4U (NN_extended.py:265-288): the head's last channel, through a ReLU, is a per-voxel log-variance; class_num = cout - 1
        self.AU_4U = bool(aleatoric)
        self.AU_log_rel_coeff = float(au_log_rel_coeff)
        if self.AU_4U:
            check(self.lib.alq_model_set_aleatoric(self._m, 1))
            self.nclass -= 1
        self.class_num = self.nclass
        # a fully-convolutional model (1x1 conv head, csrc/dense.hip): every voxel of the head's output map is a sample
        self.dense = self.layers[-1]['type'] == ALQ_CONV
        self.out_voxels = int(self.lib.alq_model_out_voxels(self._m))
        self.out_map_shape = out_map_shape(self.layers, self.in_shape) if self.dense else ()
        if self.dense and int(np.prod(self.out_map_shape)) != self.out_voxels:
            raise AssertionError('output map %r against %d voxels in the library' % (self.out_map_shape, self.out_voxels))
        self.elems_per_patch = int(np.prod(self.in_shape))
        # reference-style attributes
        self.x = Handle('x')
        self.keep_prob = Handle('keep_prob')
        if dropout:
            self.dropout_layers, self.dropout_rate = dropout[0], dropout[1]
        else:
            self.dropout_layers, self.dropout_rate = [], 1.
        self.posteriors = Handle('posteriors')
        self.prediction = Handle('prediction')
        self.feature_idx = feature_layer
        fdim = 0
        if feature_layer is not None:
            e = C.c_int64()
            check(self.lib.alq_model_layer_out_elems(self._m, int(feature_layer), C.byref(e)))
            fdim = e.value
        self.feature_dim = fdim
        self.feature_layer = Handle('feature_layer', (fdim,))
        for h in (self.posteriors, self.prediction, self.feature_layer):
            h.model = self
        if self.AU_4U:
            self.AU_vals, self.output = Handle('AU_vals'), Handle('output')          # [n, *spatial] and [n, *spatial, c + 1]
            self.AU_vals.model = self.output.model = self
        # 2L opaque entries per class, so that len(model.grad_posts['1'])/2 == L (PW_NNAL.py:751)
        self.var_dict = LazyVarDict((n, None) for n in self.var_names)
        # Weights that are already in device memory are packed there (alq_model_set_weights_device): per parameterised layer,
        # whether the library has device packers for it (wide fc layers) and the device tensors (W, b) its current weights were
        # packed from (None: host arrays only).  ALQ_HOST_REPACK=1 at creation (A/B, tests): everything through the host packers.
        self._host_repack = os.environ.get('ALQ_HOST_REPACK', '0') not in ('', '0')
        self._dev_pack = [self.lib.alq_model_layer_packs_on_device(self._m, t) == 1 for t in range(self.L)]
        self._dev_w = [None] * self.L
        self.grad_layers = []
        self._build_grad_handles()
        self.y_ = Handle('y_')
        self.loss = Handle('loss')        # mean softmax cross-entropy of a labelled batch (NN.py:583-588)
        self.loss.model = self
        self.train_step = None            # get_optimizer() creates it (NN.py:557-615)
        self._opt = None
        # NN_extended.set_hypers: None = the batch-mean cross-entropy of NN.py:583-588; else the objective of NN_extended.get_loss
        self.hypers = None
        self._obj = None
        self.input_weights = Handle('input_weights')      # per-sample loss weights [n], fed through feed_dict
        self.input_vox_weights = Handle('input_vox_weights', self.out_map_shape) if self.dense else None      # [n, *spatial] (get_FCN_loss)
        self.labels = Handle('labels')
        self.pt = Handle('pt')
        self.labels.model = self.pt.model = self
        self._weights_version = 0         # bumped by every set_weights: the optimiser's device copy follows it
        self.PFT_bflag = False            # set_PFT_mask: the summed gradient is multiplied by a binary mask (NN_extended.py:1441-1449)
        self._pft_mask = None             # float32 device [P]
        self._pft_layers = None           # parameterised layers with a non-zero mask entry
        self._drop_calls = 0
        self._mt = None                   # set_mean_teacher: the settings and state of mean-teacher training
        self.num_params = int(self.lib.alq_model_num_params(self._m))
        self._feature_perm = self._feature_permutation()

    # -- gradients of the log-posteriors (get_gradients, NN.py:621-645) -------------------
    def _build_grad_handles(self):
        """2L' opaque entries per class - L' = the layers of `grad_layers` (all when empty) - so that
        len(model.grad_posts['1'])/2 is the A-matrix size PW_NNAL.gen_A_matrices reads (PW_NNAL.py:751)."""
        names = list(self.grad_layers) if len(self.grad_layers) else list(self.var_names)
        for nme in names:
            if nme not in self.var_names:
                raise KeyError('grad layer %r is not a parameterised layer of the model' % (nme,))
        self.grad_layer_idx = [self.var_names.index(nme) for nme in names]
        self.grad_posts = {}
        for j in range(self.nclass):
            hs = []
            for t in self.grad_layer_idx:
                for part in ('W', 'b'):
                    h = Handle('grad_%d_%s_%s' % (j, self.var_names[t], part))
                    h.model, h.cls = self, j
                    hs.append(h)
            self.grad_posts[str(j)] = hs

    def get_gradients(self, grad_layers=[]):
        """NN.py:621-645 / NN_extended.py:1011-1035: the gradient lists cover `grad_layers` (all layers when empty)."""
        self.grad_layers = list(grad_layers)
        self._build_grad_handles()

    def unflatten(self, vec, layers=None):
        """Flat parameter-order vector [W_0, b_0, W_1, ...] -> list of arrays in TF variable shapes (of `layers`)."""
        out, off = [], 0
        keep = set(range(self.L)) if layers is None else set(layers)
        for t, (name, wshape, bshape) in enumerate(self.param_shapes):
            nw, nb = int(np.prod(wshape)), int(np.prod(bshape))
            if t in keep:
                out.append(vec[off:off + nw].reshape(wshape))
                out.append(vec[off + nw:off + nw + nb].reshape(bshape))
            off += nw + nb
        return out

    def flat_params(self):
        return np.concatenate([np.concatenate([np.asarray(W, np.float32).ravel(), np.asarray(b, np.float32).ravel()])
                               for W, b in self.var_dict.values()])

    def set_flat_params(self, vec):
        arrs = self.unflatten(np.asarray(vec, dtype=np.float32))
        self.set_weights({n: [arrs[2 * t], arrs[2 * t + 1]] for t, n in enumerate(self.var_names)})

    def _drop_args(self, keep_prob, seed):
        kp = float(keep_prob)
        lay = [int(v) for v in self.dropout_layers] if kp < 1. else []
        arr = (C.c_int32 * max(len(lay), 1))(*lay)
        if seed is None:
            # the reference's tf.nn.dropout draws a fresh mask per sess.run from TF's stream; here: a fresh seed per
            # call from the global NumPy stream (reproducible under np.random.seed like the rest of the query code)
            seed = int(np.random.randint(0, 2 ** 31 - 1)) if kp < 1. else 0
        return kp, arr, len(lay), int(seed)

    def param_grads_device(self, t, n, mode, cls=0, labels=None, loss_scale=1., keep_prob=1., seed=None, first_sample=0,
                           per_sample=True, want_post=False, want_loss=False):
        """alq_param_grads on n device patches (n <= max_batch): mode 0 = gradients of log posteriors[cls, .] per sample,
        mode 1 = gradient of loss_scale * sum CE.  Returns (grads [n, P] or [P], post [c, n] or None, loss or None)."""
        torch = self.sess.torch
        self.sess.bind_stream()
        if n > self.max_batch:
            raise ValueError('%d patches exceed max_batch = %d' % (n, self.max_batch))
        kp, arr, nl, seed = self._drop_args(keep_prob, seed)
        g = self.sess.empty((n, self.num_params) if per_sample else (self.num_params,), torch.float32)
        post = self.sess.empty((self.nclass, n), torch.float32) if want_post else None
        loss = self.sess.empty((1,), torch.float64) if want_loss else None
        lab = None
        if mode == 1:
            lab = labels if isinstance(labels, torch.Tensor) else self.sess.to_device(np.asarray(labels, dtype=np.int32), torch.int32)
        check(self.lib.alq_param_grads(
            self._m, C.c_void_p(t.data_ptr()), n, int(mode), int(cls), C.c_void_p(lab.data_ptr()) if lab is not None else None,
            float(loss_scale), kp, seed, int(first_sample), arr, nl, 1 if per_sample else 0, C.c_void_p(g.data_ptr()),
            C.c_void_p(post.data_ptr()) if post is not None else None, C.c_void_p(loss.data_ptr()) if loss is not None else None))
        return g, post, loss

    def grad_sqnorms_device(self, t, n, cls=-1, cls_per_sample=None):
        """alq_grad_sqnorms over device passes of max_batch patches: [n, 2L'] float64 on the device, column 2t' =
        ||dW||^2 and 2t' + 1 = ||db||^2 of the t'-th layer of `grad_layers` (all layers when empty).  cls = -1: the
        unit-cotangent gradient u = d(z0 - z1) / d theta of a two-class net; cls in [0, c): d log posteriors[cls] /
        d theta; cls_per_sample (int array or device int32 tensor [n]) overrides cls per sample.  Rows do not depend
        on the pass cut."""
        torch = self.sess.torch
        self.sess.bind_stream()
        L = self.L
        dc = None
        if cls_per_sample is not None:
            dc = cls_per_sample if isinstance(cls_per_sample, torch.Tensor) else \
                self.sess.to_device(np.asarray(cls_per_sample, dtype=np.int32).reshape(n), torch.int32)
            assert dc.dtype == torch.int32 and dc.is_contiguous() and int(dc.numel()) == n
        sq = self.sess.empty((n, 2 * L), torch.float64)
        for a in range(0, n, self.max_batch):
            b = min(n, a + self.max_batch)
            check(self.lib.alq_grad_sqnorms(self._m, C.c_void_p(t.data_ptr() + a * self.elems_per_patch * 4), b - a, int(cls),
                                            C.c_void_p(dc.data_ptr() + a * 4) if dc is not None else None, None,
                                            C.c_void_p(sq.data_ptr() + a * 2 * L * 8)))
        if list(self.grad_layer_idx) != list(range(L)):
            cols = [2 * i + h for i in self.grad_layer_idx for h in (0, 1)]
            sq = sq[:, cols].contiguous()
        return sq

    # -- Hessian-vector products (Influence.py:64-166) ---------------------------------------
    def hess_layer_idx(self, layers='all'):
        """Parameterised-layer indices of `layers`: 'all' / None, layer names (the reference's Hess_layers) or indices."""
        if layers is None or (isinstance(layers, str) and layers == 'all'):
            return list(range(self.L))
        idx = [self.var_names.index(l) if isinstance(l, str) else int(l) for l in layers]
        if len(idx) == 0 or len(set(idx)) != len(idx) or min(idx) < 0 or max(idx) >= self.L:
            raise KeyError('Hessian layers %r' % (layers,))
        return idx

    def _param_offsets(self):
        off, out = 0, []
        for _, wshape, bshape in self.param_shapes:
            nw, nb = int(np.prod(wshape)), int(np.prod(bshape))
            out.append((off, nw, nb))
            off += nw + nb
        return out

    def ravel_for_layers(self, v, idx):
        """`v` - a flat vector over all parameters, a flat vector over the layers `idx` (in that order) or a list
        [VW, Vb, ...] of arrays for them - as a flat float32 vector [P] in parameter order (zero outside `idx`)."""
        offs = self._param_offsets()
        if isinstance(v, (list, tuple)):
            if len(v) != 2 * len(idx):
                raise ValueError('expected %d arrays (W, b per layer), got %d' % (2 * len(idx), len(v)))
            v = np.concatenate([np.asarray(a, dtype=np.float32).ravel() for a in v])
        v = np.asarray(v, dtype=np.float32).ravel()
        if v.size == self.num_params:
            return np.ascontiguousarray(v)
        if v.size != sum(offs[t][1] + offs[t][2] for t in idx):
            raise ValueError('vector of %d entries fits neither all %d parameters nor the chosen layers' % (v.size, self.num_params))
        full = np.zeros(self.num_params, dtype=np.float32)
        c = 0
        for t in idx:
            o, nw, nb = offs[t]
            full[o:o + nw + nb] = v[c:c + nw + nb]
            c += nw + nb
        return full

    def _require_default_objective(self, what):
        """The exact R-operator (csrc/hvp.hip) is that of the batch-mean cross-entropy: a model whose loss set_hypers changed
        has no Hessian-vector product, whichever way it is asked for."""
        if self._obj is not None:
            raise NotImplementedError('%s of a non-default objective (set_hypers): the R-operator covers the batch-mean '
                                      'cross-entropy only' % what)

    def _check_input_weights(self, input_weights):
        """Per-sample weights belong to NN_extended.get_loss (NN_extended.py:1252-1255); NN.py's loss has none."""
        if input_weights is not None and self._obj is None and not self.dense:
            raise ValueError('input_weights on a model without training hypers: the batch-mean cross-entropy of NN.py:583-588 '
                             'takes no sample weights (build the NN_extended.CNN with loss_name=\'CE\' for the weighted mean)')

    def hess_vecp_device(self, t, n, labels, v, idx=None, loss_scale=1., out=None, want_loss=False):
        """alq_hess_vecp on n device patches (any n: passes of max_batch with the same loss_scale): `out` (float64 device
        [P]; created and overwritten when None) += H v, H the Hessian of loss_scale * sum CE over the layers `idx` (indices;
        None = all).  labels / v: int32 [n] / float32 [P] device tensors.  Returns (out, scaled loss of the passes or None)."""
        self._require_default_objective('hess_vecp')      # every caller: hess_vecp, sess.run, PW_NN.batch_eval, Influence
        torch = self.sess.torch
        self.sess.bind_stream()
        assert labels.dtype == torch.int32 and labels.is_contiguous() and int(labels.numel()) == n
        assert v.dtype == torch.float32 and v.is_contiguous() and int(v.numel()) == self.num_params
        on = None
        if idx is not None and sorted(idx) != list(range(self.L)):
            on = (C.c_uint8 * self.L)(*[1 if q in idx else 0 for q in range(self.L)])
        acc = out is not None
        if out is None:
            out = self.sess.empty((self.num_params,), torch.float64)
        assert out.dtype == torch.float64 and out.is_contiguous() and int(out.numel()) == self.num_params
        loss = self.sess.empty((1,), torch.float64) if want_loss else None
        total = torch.zeros((1,), dtype=torch.float64, device=self.sess.device) if want_loss else None
        for a in range(0, n, self.max_batch):
            b = min(n, a + self.max_batch)
            check(self.lib.alq_hess_vecp(self._m, C.c_void_p(t.data_ptr() + a * self.elems_per_patch * 4), b - a,
                                         C.c_void_p(labels.data_ptr() + a * 4), float(loss_scale), C.c_void_p(v.data_ptr()), on,
                                         1 if (acc or a > 0) else 0, C.c_void_p(out.data_ptr()),
                                         C.c_void_p(loss.data_ptr()) if want_loss else None))
            if want_loss:
                total += loss
        return out, total

    def hess_vecp(self, x, labels, v, layers='all', loss_scale=None, out=None):
        """H v for the Hessian of loss_scale * sum_n CE(softmax(z_n), labels[n]) (loss_scale None: 1 / n, the mean loss of
        NN.py:583-588) over the parameters of `layers` ('all', names or indices; the others are held constant).  `v`: see
        ravel_for_layers.  Returns the list [HW, Hb, ...] of the chosen layers in TF shapes, float64.  `out`: a float64
        device vector [P] the product is ADDED to (multi-pass sums); the list then holds the accumulated values."""
        self._require_default_objective('hess_vecp')
        torch = self.sess.torch
        t, n = self._as_device_batch(x)
        idx = self.hess_layer_idx(layers)
        lab = labels if isinstance(labels, torch.Tensor) else self.sess.to_device(np.asarray(labels, dtype=np.int32).reshape(n), torch.int32)
        vd = self.sess.to_device(self.ravel_for_layers(v, idx), torch.float32)
        hv, _ = self.hess_vecp_device(t, n, lab, vd, idx, 1. / n if loss_scale is None else loss_scale, out)
        return self.unflatten(hv.cpu().numpy(), idx)

    def mean_loss(self, x, labels, targets=None, input_weights=None):
        """`sess.run(model.loss, {x, y_})`: the mean softmax cross-entropy of the batch (unlabelled samples add 0 to the sum),
        or the model's own objective once set_hypers gave it one (forward passes + alq_loss_stats; `targets` [c, n]: the
        soft targets of CE_softclasses / GCE, one-hot columns of `labels` when None; `input_weights` [n])."""
        torch = self.sess.torch
        t, n = self._as_device_batch(x)
        self._check_input_weights(input_weights)
        if self._obj is not None or self.dense:
            y = self._onehot(labels, n * self.out_voxels) if targets is None else targets
            return self._objective_pass(t, n, y, 1., None, input_weights, None, want_grad=False)[1]
        lab = self.sess.to_device(np.asarray(labels, dtype=np.int32).reshape(n), torch.int32)
        loss = 0.
        for a in range(0, n, self.max_batch):
            b = min(n, a + self.max_batch)
            _, _, l = self.param_grads_device(t[a:b], b - a, 1, labels=lab[a:b], loss_scale=1. / n, per_sample=False, want_loss=True)
            loss += float(l.item()) * (b - a) / n
        return loss

    def mean_loss_grad(self, x, labels, layers='all', targets=None, input_weights=None):
        """`sess.run(model.loss_grad, {x, y_})` (NN.add_loss_grad, NN.py:862-871): gradient of the mean cross-entropy with
        respect to the variables of `layers`, TF shapes (alq_param_grads mode 1) - of the model's own objective once set_hypers
        gave it one (alq_param_grads_loss; `targets` / `input_weights` as in mean_loss)."""
        torch = self.sess.torch
        t, n = self._as_device_batch(x)
        self._check_input_weights(input_weights)
        if self._obj is not None or self.dense:
            y = self._onehot(labels, n * self.out_voxels) if targets is None else targets
            g, _ = self._objective_pass(t, n, y, 1., None, input_weights, None)
            return self.unflatten(g.cpu().numpy(), self.hess_layer_idx(layers))
        lab = self.sess.to_device(np.asarray(labels, dtype=np.int32).reshape(n), torch.int32)
        g = torch.zeros((self.num_params,), dtype=torch.float64, device=self.sess.device)
        for a in range(0, n, self.max_batch):
            b = min(n, a + self.max_batch)
            gp, _, _ = self.param_grads_device(t[a:b], b - a, 1, labels=lab[a:b], loss_scale=1. / n, per_sample=False)
            g += gp
        return self.unflatten(g.cpu().numpy().astype(np.float32), self.hess_layer_idx(layers))

    def grad_log_post(self, x, j, keep_prob=1.):
        """`sess.run(model.grad_posts[str(j)], {x: batch})`: gradients of log posteriors[j, 0] - sample 0 of the batch,
        like the reference's graph node (NN.py:639-645) - w.r.t. the variables of `grad_layers`, TF shapes."""
        t, n = self._as_device_batch(x)
        g, _, _ = self.param_grads_device(t, 1, 0, cls=j, keep_prob=keep_prob)
        return self.unflatten(g[0].cpu().numpy(), self.grad_layer_idx)

    # -- training step (get_optimizer / train_step, NN.py:557-615) --------------------------
    def set_hypers(self, hypers):
        """NN_extended.CNN.set_hypers (NN_extended.py:24-63) for the keys a device step reads (NN_extended.CNN.DEFAULT_HYPERS):
        from here on the model's loss is NN_extended.get_loss's (:1221-1277) and get_optimizer() takes no arguments."""
        from . import losses
        torch = self.sess.torch
        h = dict(hypers)
        kind = losses.KINDS[h.get('loss_name', 'CE')]
        bcw, gamma = h.get('bin_class_weights'), h.get('focal_gamma')
        if (bcw is not None or gamma is not None) and self.nclass != 2:
            raise ValueError('bin_class_weights / focal_gamma need a two-class net, got %d classes' % self.nclass)
        if kind == losses.GCE and float(h.get('q', 0.7)) == 0:
            raise ValueError('q cannot be equal to zero.')
        self.hypers = h
        self._obj = dict(kind=kind, divisor='nonzero', q=float(h.get('q', 0.7)),
                         gamma=float(gamma) if (gamma is not None and kind == losses.CE) else None,
                         class_w=self.sess.to_device(np.asarray(bcw, dtype=np.float32).reshape(2), torch.float32)
                         if (bcw is not None and kind == losses.CE) else None)

    def get_optimizer(self, learning_rate=None, train_layers=[], optimizer_name=None):
        """Mean softmax cross-entropy + SGD or Adam on all layers or on `train_layers` (NN.py:583-615).  Without arguments
        (NN_extended.get_optimizer, NN_extended.py:1380-1449): the optimiser - SGD, Adam(beta1, beta2) or RMSProp(decay, momentum,
        epsilon) - and the learning rate (`learning_rate`, else `lr_schedule(step)` evaluated on the host before every step,
        step = 0 before the first) of the model's hypers; `train_layers` as set on the model before the call, if at all."""
        h = self.hypers or {}
        if learning_rate is None and optimizer_name is None and not train_layers:
            if self.hypers is None:
                raise TypeError('get_optimizer() without arguments needs the hyper-parameters of an NN_extended.CNN')
            train_layers = list(getattr(self, 'train_layers', []))
        if optimizer_name is None:
            optimizer_name = h.get('optimizer_name', 'SGD')
        if optimizer_name not in ('SGD', 'Adam', 'RMSProp'):
            raise NotImplementedError('optimizer %r (SGD, Adam and RMSProp are known)' % (optimizer_name,))
        if self.AU_4U and self._mt is None:
            raise NotImplementedError('an AU_4U model trains with MT_SSL: its log-variance channel has a gradient only under the '
                                      'consistency term')
        schedule = None
        if learning_rate is None:
            learning_rate = h.get('learning_rate')
            if learning_rate is None:
                schedule = h.get('lr_schedule')
                if schedule is None:
                    raise ValueError('neither learning_rate nor lr_schedule is set')
                learning_rate = schedule(0)
        for nme in train_layers:
            if nme not in self.var_names:
                raise KeyError('train layer %r' % (nme,))
        self.train_layers = list(train_layers)
        self.train_step = Handle('train_step')
        self.train_step.model = self
        self._opt = dict(name=optimizer_name, lr=float(learning_rate), schedule=schedule, t=0, theta=None, m=None, v=None,
                         beta1=float(h.get('beta1', 0.9)), beta2=float(h.get('beta2', 0.999)), decay=float(h.get('decay', 0.9)),
                         momentum=float(h.get('momentum', 0.)), epsilon=float(h.get('epsilon', 1e-10)))
        if self._mt is not None:
            self._build_teacher()

    # -- mean-teacher consistency training (NN_extended.py:913-926, :1337-1396) -------------
    @property
    def global_step(self):
        """Optimiser steps taken so far (the reference's `global_step` variable)."""
        return self._opt['t'] if self._opt is not None else 0

    def set_mean_teacher(self, mt):
        """MT_SSL of NN_extended.CNN: `mt` holds output_perturbation_measure, MT_ema_decay_schedule, Gaussian_noise_std,
        rotation_angle, max_cons_coeff and rampup_length.  get_optimizer() then builds the teacher."""
        from . import mteach
        if not self.dense:
            raise NotImplementedError('mean-teacher training is defined for fully-convolutional models')
        if mt.get('rotation_angle') is not None and len(self.in_shape) != 3:
            raise ValueError('rotation_angle on a 3-D model')
        self._mt = dict(measure=mteach.MEASURES[mt['output_perturbation_measure']], decay=mt['MT_ema_decay_schedule'],
                        std=float(mt['Gaussian_noise_std'] or 0.), angle=mt.get('rotation_angle'),
                        max_coeff=float(mt['max_cons_coeff']), rampup=float(mt['rampup_length']), shadow=None, tver=0)
        self.cons_coeff = mteach.cons_coeff(0, self._mt['rampup'], self._mt['max_coeff'])

    def _build_teacher(self):
        """get_FCN_loss with MT_SSL (NN_extended.py:1337-1396): a second model over the same layers on the same session whose
        weights are the moving averages of this model's, its input `perturbed_x`, and the handles of the step."""
        drop = [self.dropout_layers, self.dropout_rate] if len(self.dropout_layers) else None
        if getattr(self, 'teacher', None) is not None:      # (a second get_optimizer(): a new teacher, as a new graph would hold)
            self.teacher.close()
        self.teacher = DeviceModel(self.sess, self.layer_dict, self.in_shape, self.skips, None, drop, self.max_batch,
                                   self.name + '_teacher', aleatoric=self.AU_4U, au_log_rel_coeff=self.AU_log_rel_coeff)
        self.perturbed_x = Handle('perturbed_x')
        for nme in ('ema_apply', 'labeled_loss', 'cons_loss'):
            h = Handle(nme)
            h.model = self
            setattr(self, nme, h)
        self._mt.update(shadow=None, tver=0)

    def _student_theta(self):
        """This model's weights as a flat device vector: the optimiser's own when it is current."""
        o = self._opt
        if o is not None and o['theta'] is not None and o.get('version') == self._weights_version:
            return o['theta']
        return self.sess.to_device(self.flat_params(), self.sess.torch.float32)

    def _mt_shadow(self):
        """The teacher's weights, flat fp32 on the device.  They start as a copy of this model's weights at the first use -
        of the teacher's own when teacher.set_weights / load_weights was called (again after every later such call)."""
        mt, T = self._mt, self.teacher
        if mt['shadow'] is None or T._weights_version != mt['tver']:
            src = self._student_theta() if T._weights_version == 0 else self.sess.to_device(T.flat_params(), self.sess.torch.float32)
            mt['shadow'] = src.clone()
            T.set_weights_device(mt['shadow'])
            mt['tver'] = T._weights_version
        return mt['shadow']

    def apply_ema(self):
        """`sess.run(model.ema_apply)`: shadow -= (shadow - theta) * (1 - decay) on the device (alq_ema_step), decay =
        MT_ema_decay_schedule(global_step) evaluated on the host; the teacher is repacked from the shadow vector."""
        if self._mt is None or self._opt is None:
            raise RuntimeError('ema_apply needs MT_SSL and get_optimizer()')
        mt = self._mt
        shadow = self._mt_shadow()
        theta = self._student_theta()
        self.sess.bind_stream()
        check(self.lib.alq_ema_step(self.sess.ctx, C.c_void_p(shadow.data_ptr()), C.c_void_p(theta.data_ptr()), self.num_params,
                                    float(mt['decay'](self.global_step))))
        self.teacher.set_weights_device(shadow)
        mt['tver'] = self.teacher._weights_version

    def perturb_device(self, t, n, seed, first_sample=0):
        """`model.perturbed_x` of n device patches (alq_perturb_input): Gaussian noise, then the rotation."""
        mt = self._mt
        out = self.sess.empty((n, self.elems_per_patch), self.sess.torch.float32)
        H, W, Cc = (self.in_shape if len(self.in_shape) == 3 else (self.in_shape[0] * self.in_shape[1],) + self.in_shape[2:])
        self.sess.bind_stream()
        check(self.lib.alq_perturb_input(self.sess.ctx, C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr()), n, H, W, Cc, mt['std'],
                                         int(seed), int(first_sample), int(mt['angle'] is not None), float(mt['angle'] or 0.)))
        return out

    def _mt_pass(self, t, n, y, keep_prob, seed, input_weights, want_grad, feed):
        """_objective_pass of a mean-teacher model: loss = L + cons_coeff * cons read as the vector [n], so
        the gradient is n grad L + cons_coeff sum_i grad cons_i.  Per cut of max_batch: perturb the cut, the teacher's forward
        pass at its own keep_prob, alq_param_grads_loss_mt.  `feed`: dict(kp = the teacher's keep_prob, px = a fed
        perturbed_x or None).  The labelled scale is n / (non-zero weights of the whole batch), the consistency scale
        cons_coeff 2 / (c V) per voxel (L2; CE adds to the value only).  An AU_4U model takes the _au entry points: the
        consistency value of a voxel is div exp(-a) + AU_log_rel_coeff a / 2 and its log-variance column has the scale
        cons_coeff / V under both measures.  Returns (gradient or None, loss) and leaves (L, mean_i cons_i, cons_coeff) in
        self._mt['last']."""
        from . import losses, mteach
        torch = self.sess.torch
        self.sess.bind_stream()
        mt, T = self._mt, self.teacher
        obj = self._obj or dict(q=0.7, gamma=None, class_w=None)          # (no hypers: the plain voxel-wise cross-entropy)
        c, V = self.nclass, self.out_voxels
        ns = n * V
        t = t.reshape(n, -1)
        counts = None
        if self._is_device_labels(y):
            lab, labd, counts = self._device_label_feed(y, ns, input_weights is not None)
        else:
            y = np.asarray(y)
            if y.shape != (c, ns):
                raise ValueError('labels must be [%d, %d] columns, got %r' % (c, ns, y.shape))
            lab = np.where(y.sum(0) > 0, y.argmax(0), -1).astype(np.int32)
            labd = self.sess.to_device(lab, torch.int32)
        sw = None if input_weights is None else np.asarray(input_weights, dtype=np.float32).reshape(ns)
        swd = None if sw is None else self.sess.to_device(sw, torch.float32)
        cw = obj['class_w']
        gamma = obj['gamma'] if (obj['gamma'] is not None and obj['gamma'] > 0) else None
        kp, arr, nl, seed = self._drop_args(keep_prob, seed)
        tkp, tarr, tnl, tseed = T._drop_args(feed.get('kp', 1.), None)            # the second draw of the seed stream
        px = feed.get('px')
        nseed = int(np.random.randint(0, 2 ** 31 - 1)) if (px is None and mt['std'] > 0) else 0      # ... and the third
        if px is not None:
            px, npx = self._as_device_batch(px)
            if npx != n:
                raise ValueError('perturbed_x holds %d patches, x %d' % (npx, n))
            px = px.reshape(n, -1)
        self._mt_shadow()
        coeff = mteach.cons_coeff(self.global_step, mt['rampup'], mt['max_coeff'])
        kscale = coeff * 2. / (c * V) if mt['measure'] == mteach.L2 else 0.
        au_on, kappa = self.AU_4U, self.AU_log_rel_coeff
        cuts = [(a, min(n, a + self.max_batch)) for a in range(0, n, self.max_batch)]
        xb = lambda src, a: C.c_void_p(src.data_ptr() + a * self.elems_per_patch * 4)
        spec = lambda a: LossT(losses.CE, -1. if gamma is None else gamma, obj['q'], 1., cw.data_ptr() if cw is not None else None,
                               swd.data_ptr() + a * V * 4 if swd is not None else None, None, None)

        def teacher_post(a, b):
            pin = px[a:b] if px is not None else (self.perturb_device(t[a:b], b - a, nseed, a) if (mt['std'] > 0 or mt['angle'] is not None)
                                                  else t[a:b])
            tq = self.sess.empty((c, (b - a) * V), torch.float32)
            check(self.lib.alq_forward_dropout(T._m, xb(pin, 0), b - a, tkp, tseed, a, tarr, tnl, C.c_void_p(tq.data_ptr()), None))
            return tq

        def student_post(a, b, want_au=False):
            pb = self.sess.empty((c, (b - a) * V), torch.float32)
            if want_au:
                au = self.sess.empty(((b - a) * V,), torch.float32)
                check(self.lib.alq_forward_au(self._m, xb(t, a), b - a, kp, seed, a, arr, nl, C.c_void_p(pb.data_ptr()), None,
                                              C.c_void_p(au.data_ptr()), None))
                return pb, au
            check(self.lib.alq_forward_dropout(self._m, xb(t, a), b - a, kp, seed, a, arr, nl, C.c_void_p(pb.data_ptr()), None))
            return pb

        stats = torch.zeros((len(cuts), 3), dtype=torch.float64, device=self.sess.device)
        if want_grad:
            if gamma is None and lab is None:
                cnt = float(self._count_from_class_counts(counts, cw))
            elif gamma is None:
                w = (lab >= 0).astype(np.float64)
                if cw is not None:
                    w = w * np.asarray(self.hypers['bin_class_weights'], dtype=np.float32).reshape(2)[np.where(lab == 1, 1, 0)]
                if sw is not None:
                    w = w * sw
                cnt = float(np.count_nonzero(w))
            else:      # the focal weight can vanish (pt == 1): the count comes from a statistics pass first
                for k, (a, b) in enumerate(cuts):
                    pb, L = student_post(a, b), spec(a)
                    check(self.lib.alq_loss_stats(self.sess.ctx, C.c_void_p(pb.data_ptr()), c, (b - a) * V,
                                                  C.c_void_p(labd.data_ptr() + a * V * 4), C.byref(L), C.c_void_p(stats.data_ptr() + k * 24)))
                cnt = float(stats[:, 1].sum().item())
            s = n / cnt if cnt else 0.
            gsum = torch.zeros((self.num_params,), dtype=torch.float32, device=self.sess.device)
            for k, (a, b) in enumerate(cuts):
                g = self.sess.empty((self.num_params,), torch.float32)
                tq, L = teacher_post(a, b), spec(a)
                if au_on:
                    check(self.lib.alq_param_grads_loss_mt_au(self._m, xb(t, a), b - a, C.c_void_p(labd.data_ptr() + a * V * 4), C.byref(L),
                                                              float(s), C.c_void_p(tq.data_ptr()), mt['measure'], float(kscale),
                                                              float(coeff / V), kappa, kp, seed, a, arr, nl, C.c_void_p(g.data_ptr()), None,
                                                              C.c_void_p(stats.data_ptr() + k * 24)))
                else:
                    check(self.lib.alq_param_grads_loss_mt(self._m, xb(t, a), b - a, C.c_void_p(labd.data_ptr() + a * V * 4), C.byref(L),
                                                           float(s), C.c_void_p(tq.data_ptr()), mt['measure'], float(kscale), kp, seed, a, arr,
                                                           nl, C.c_void_p(g.data_ptr()), None, C.c_void_p(stats.data_ptr() + k * 24)))
                gsum += g
        else:
            gsum = None
            for k, (a, b) in enumerate(cuts):
                tq, L = teacher_post(a, b), spec(a)
                if au_on:
                    pb, au = student_post(a, b, True)
                    check(self.lib.alq_mt_stats_au(self.sess.ctx, C.c_void_p(pb.data_ptr()), C.c_void_p(tq.data_ptr()), C.c_void_p(au.data_ptr()),
                                                   c, (b - a) * V, C.c_void_p(labd.data_ptr() + a * V * 4), C.byref(L), kappa, mt['measure'],
                                                   C.c_void_p(stats.data_ptr() + k * 24)))
                    continue
                pb = student_post(a, b)
                check(self.lib.alq_mt_stats(self.sess.ctx, C.c_void_p(pb.data_ptr()), C.c_void_p(tq.data_ptr()), c, (b - a) * V,
                                            C.c_void_p(labd.data_ptr() + a * V * 4), C.byref(L), mt['measure'],
                                            C.c_void_p(stats.data_ptr() + k * 24)))
        st = stats.cpu().numpy()
        cnt = st[:, 1].sum()
        labelled = float(st[:, 0].sum() / cnt) if cnt else 0.
        cons = float(st[:, 2].sum() / ns)
        mt['last'] = (labelled, cons, coeff)
        return gsum, labelled + coeff * cons

    def _train_mask(self):
        """1 on the parameters of `train_layers` (all when empty), flat order."""
        if not self.train_layers:
            return None
        mask = np.zeros(self.num_params, dtype=np.float32)
        off = 0
        for name, wshape, bshape in self.param_shapes:
            cnt = int(np.prod(wshape)) + int(np.prod(bshape))
            if name in self.train_layers:
                mask[off:off + cnt] = 1.
            off += cnt
        return mask

    # -- partial fine-tuning (PFT_bflag / par_placeholders, NN_extended.py:1441-1449) ------------
    def _flat_mask(self, mask):
        """A PFT mask - list [MW, Mb, ...] in variable shapes (grads_vars order) or a flat vector / device tensor [P] - as
        (float32 device tensor [P], layers with a non-zero entry)."""
        torch = self.sess.torch
        if isinstance(mask, torch.Tensor):
            if int(mask.numel()) != self.num_params:
                raise ValueError('mask of %d entries for %d parameters' % (int(mask.numel()), self.num_params))
            md = mask.to(device=self.sess.device, dtype=torch.float32).reshape(-1).contiguous()
        else:
            if isinstance(mask, (list, tuple)):
                if len(mask) != 2 * self.L:
                    raise ValueError('expected %d mask arrays (W, b per layer), got %d' % (2 * self.L, len(mask)))
                for q, (nme, wshape, bshape) in enumerate(self.param_shapes):
                    for a_, shp in ((mask[2 * q], wshape), (mask[2 * q + 1], bshape)):
                        if int(np.size(a_)) != int(np.prod(shp)):
                            raise ValueError('layer %s: mask of %d entries for a variable of shape %s' % (nme, np.size(a_), shp))
                mask = np.concatenate([np.asarray(a_, dtype=np.float32).ravel() for a_ in mask])
            mask = np.asarray(mask, dtype=np.float32).ravel()
            if mask.size != self.num_params:
                raise ValueError('mask of %d entries for %d parameters' % (mask.size, self.num_params))
            md = self.sess.to_device(mask, torch.float32)
        # which layers train: L flags cross to the host, not the mask
        flags = torch.stack([(md[o:o + nw + nb] != 0).any() for o, nw, nb in self._param_offsets()]).cpu().numpy()
        return md, [q for q in range(self.L) if flags[q]]

    def set_PFT_mask(self, mask):
        """Partial fine-tuning: every later train step multiplies the summed gradient by `mask` before the optimiser step (on
        top of `train_layers`).  `mask`: list in variable shapes, flat vector or flat device tensor [P] (pft_mask_device);
        None clears it.  Sets `PFT_bflag`.  The mask multiplies the gradient, as in the reference: under SGD a masked-out
        parameter does not move; under Adam it does not move if the mask held since the optimiser's first step, and otherwise
        goes on moving on the moments it has (they are not reset), as a TF variable would."""
        if mask is None:
            self.PFT_bflag, self._pft_mask, self._pft_layers = False, None, None
            return
        self._pft_mask, self._pft_layers = self._flat_mask(mask)
        self.PFT_bflag = True

    def get_par_placeholders(self):
        """NN_extended.py:1441-1449: one mask placeholder per variable in grads_vars order (W_0, b_0, W_1, ...); masks fed under
        them in `sess.run(model.train_step, feed_dict)` hold for that step."""
        self.par_placeholders = []
        for nme, wshape, bshape in self.param_shapes:
            for part, shp in (('W', wshape), ('b', bshape)):
                self.par_placeholders.append(Handle('par_placeholder_%s_%s' % (nme, part), shp))
        return self.par_placeholders

    def pft_mask_device(self, diagF_flat, k=None, thr=None):
        """The binary mask of partial fine-tuning from a flat float64 device vector (diagonal_fisher_device): k given - 1 on
        the k largest entries, ties at the k-th value to the lower index (alq_topk_mask; keep_k_largest_from_LoV); thr given -
        1 where the entry >= thr (alq_threshold_mask; threshold_LoV).  float32 device tensor of the same length."""
        torch = self.sess.torch
        if (k is None) == (thr is None):
            raise ValueError('give exactly one of k and thr')
        v = diagF_flat
        assert v.dtype == torch.float64 and v.is_contiguous() and v.device == self.sess.device
        self.sess.bind_stream()
        n = int(v.numel())
        mask = self.sess.empty((n,), torch.float32)
        if k is not None:
            work = self.sess.empty((self.lib.alq_topk_mask_work_bytes(n),), torch.uint8)
            check(self.lib.alq_topk_mask(self.sess.ctx, C.c_void_p(v.data_ptr()), n, int(k), C.c_void_p(mask.data_ptr()),
                                         C.c_void_p(work.data_ptr())))
        else:
            check(self.lib.alq_threshold_mask(self.sess.ctx, C.c_void_p(v.data_ptr()), n, float(thr), C.c_void_p(mask.data_ptr())))
        return mask

    def _onehot(self, labels, n):
        lab = np.asarray(labels).astype(np.int64).reshape(n)
        y = np.zeros((self.nclass, n), dtype=np.float32)
        ok = (lab >= 0) & (lab < self.nclass)
        y[lab[ok], np.nonzero(ok)[0]] = 1.
        return y

    @staticmethod
    def _is_device_labels(y):
        from .datasets.utils import DeviceLabels
        return isinstance(y, DeviceLabels)

    def _device_label_feed(self, dl, ns, want_host):
        """The label feed of a dense objective from a datasets.DeviceLabels: (host labels [ns] - only when per-voxel weights
        need them -, the int32 device labels [ns], the class counts).  No one-hot, no argmax, no upload."""
        torch = self.sess.torch
        if not self.dense:
            raise TypeError('DeviceLabels feed a fully-convolutional model; an fc-head model takes one-hot columns')
        if dl.C != self.nclass or int(dl.labels.numel()) != ns:
            raise ValueError('labels must be [%d, %d] columns, got DeviceLabels of %r' % (self.nclass, ns, dl.shape))
        labd = dl.labels.to(device=self.sess.device, dtype=torch.int32).contiguous().reshape(ns)
        return (labd.cpu().numpy() if want_host else None), labd, dl.counts

    def _count_from_class_counts(self, counts, cw):
        """The non-zero weights of a batch from its voxels per class: every labelled voxel, or - with bin_class_weights - those
        of the classes whose weight is not zero (the integer the host path counts voxel by voxel)."""
        if cw is None:
            return int(counts[:self.nclass].sum())
        bw = np.asarray(self.hypers['bin_class_weights'], dtype=np.float32).reshape(2)
        return int(counts[0]) * int(bw[0] != 0) + int(counts[1]) * int(bw[1] != 0)

    def _objective_pass(self, t, n, y, keep_prob, seed, input_weights, lwf, want_grad=True, mt_feed=None):
        """The model's objective (set_hypers; the batch-mean cross-entropy with divisor n when none is set) on n device patches
        over passes of max_batch: (gradient of the loss, float32 device [P] - None without `want_grad` - and the loss).
        y [c, n]: one-hot columns (all zero: unlabelled) or, for CE_softclasses / GCE, the soft targets; input_weights [n];
        lwf = (old logits [c, n], lambda_o, T) adds lambda_o * mean_n l'_n (model_utils.get_LwF).
        The weighted cross-entropy divides by the number of non-zero weights of the WHOLE batch (TF's SUM_BY_NONZERO_WEIGHTS):
        without the focal term that count is known on the host from labels and weights; with it the passes run unscaled and
        the summed gradient is divided by the count on the device (no read in between); focal with LwF - two terms with two
        divisors - takes the count from forward passes + alq_loss_stats first.  One read of the statistics at the end."""
        from . import losses
        if self._mt is not None and getattr(self, 'teacher', None) is not None:      # (before get_optimizer(): the labelled loss alone)
            if lwf is not None:
                raise NotImplementedError('MT_SSL with learning without forgetting')
            return self._mt_pass(t, n, y, keep_prob, seed, input_weights, want_grad, mt_feed or {})
        torch = self.sess.torch
        self.sess.bind_stream()
        # (a dense model: V samples per patch, always the non-zero-weight divisor of get_FCN_loss, NN_extended.py:1285-1335)
        obj = self._obj or dict(kind=losses.CE, divisor='nonzero' if self.dense else 'N', q=0.7, gamma=None, class_w=None)
        kind, c, V = obj['kind'], self.nclass, self.out_voxels
        ns = n * V
        counts = None
        if self._is_device_labels(y):
            if kind != losses.CE:
                raise TypeError('DeviceLabels are class ids: the objective reads soft targets')
            lab, labd, counts = self._device_label_feed(y, ns, input_weights is not None)
            tgd = None
        else:
            y = np.asarray(y)
            if y.shape != (c, ns):
                raise ValueError('labels must be [%d, %d] columns, got %r' % (c, ns, y.shape))
            lab = np.where(y.sum(0) > 0, y.argmax(0), -1).astype(np.int32)
            labd = self.sess.to_device(lab, torch.int32)
            tgd = self.sess.to_device(y.astype(np.float32), torch.float32) if kind != losses.CE else None
        sw = None if input_weights is None else np.asarray(input_weights, dtype=np.float32).reshape(ns)
        swd = None if sw is None else self.sess.to_device(sw, torch.float32)
        cw = obj['class_w']
        gamma = obj['gamma'] if (obj['gamma'] is not None and obj['gamma'] > 0) else None
        old, lam, T = None, 0., 1.
        if lwf is not None:
            old = self.sess.to_device(np.asarray(lwf[0], dtype=np.float32).reshape(c, ns), torch.float32)
            lam, T = float(lwf[1]), float(lwf[2])
        kp, arr, nl, seed = self._drop_args(keep_prob, seed)
        cuts = [(a, min(n, a + self.max_batch)) for a in range(0, n, self.max_batch)]

        def spec(a, b):
            keep = [None if v is None else v[:, a * V:b * V].contiguous() for v in (tgd, old)]
            L = LossT(kind, -1. if gamma is None else gamma, obj['q'], T, cw.data_ptr() if cw is not None else None,
                      swd.data_ptr() + a * V * 4 if swd is not None else None, keep[0].data_ptr() if keep[0] is not None else None,
                      keep[1].data_ptr() if keep[1] is not None else None)
            return L, keep

        def stats_only(dst):
            for k, (a, b) in enumerate(cuts):
                pb = self.sess.empty((c, (b - a) * V), torch.float32)
                check(self.lib.alq_forward_dropout(self._m, C.c_void_p(t.data_ptr() + a * self.elems_per_patch * 4), b - a, kp, seed, a,
                                                   arr, nl, C.c_void_p(pb.data_ptr()), None))
                L, keep = spec(a, b)
                check(self.lib.alq_loss_stats(self.sess.ctx, C.c_void_p(pb.data_ptr()), c, (b - a) * V, C.c_void_p(labd.data_ptr() + a * V * 4),
                                              C.byref(L), C.c_void_p(dst.data_ptr() + k * 24)))
                del keep

        stats = torch.zeros((len(cuts), 3), dtype=torch.float64, device=self.sess.device)
        post_scale = False
        if kind == losses.CE_SOFT:
            s = 1. / ns
        elif kind == losses.GCE:
            s = 1.           # reduce_mean over the classes leaves a vector over samples: the optimiser differentiates its sum
        elif obj['divisor'] == 'N':
            s = 1. / ns
        elif gamma is None and lab is None:
            cnt = self._count_from_class_counts(counts, cw)
            s = 1. / cnt if cnt else 0.
        elif gamma is None:
            w = (lab >= 0).astype(np.float64)
            if cw is not None:
                w = w * np.asarray(self.hypers['bin_class_weights'], dtype=np.float32).reshape(2)[np.where(lab == 1, 1, 0)]
            if sw is not None:
                w = w * sw
            cnt = int(np.count_nonzero(w))
            s = 1. / cnt if cnt else 0.
        elif want_grad and lwf is not None:
            stats_only(stats)
            cnt = float(stats[:, 1].sum().item())
            s = 1. / cnt if cnt else 0.
        else:
            s, post_scale = 1., True
        gsum = None
        if want_grad:
            gsum = torch.zeros((self.num_params,), dtype=torch.float32, device=self.sess.device)
            for k, (a, b) in enumerate(cuts):
                g = self.sess.empty((self.num_params,), torch.float32)
                L, keep = spec(a, b)
                check(self.lib.alq_param_grads_loss(self._m, C.c_void_p(t.data_ptr() + a * self.elems_per_patch * 4), b - a,
                                                    C.c_void_p(labd.data_ptr() + a * V * 4), C.byref(L), float(s), lam / ns, kp, seed, a,
                                                    arr, nl, C.c_void_p(g.data_ptr()), None, C.c_void_p(stats.data_ptr() + k * 24)))
                gsum += g
                del keep
            if post_scale:
                cnt_d = stats[:, 1].sum()
                gsum *= torch.where(cnt_d > 0, 1. / cnt_d.clamp(min=1.), torch.zeros_like(cnt_d)).to(torch.float32)
        else:
            stats_only(stats)
        st = stats.cpu().numpy()
        if kind == losses.CE and obj['divisor'] == 'N':
            loss = 0.
            for (a, b), row in zip(cuts, st):          # the arithmetic of the default step: per-pass means, weighted
                loss += float(row[0] / ((b - a) * V)) * ((b - a) * V) / ns
        elif kind == losses.CE:
            cnt = st[:, 1].sum()
            loss = float(st[:, 0].sum() / cnt) if cnt else 0.
        else:
            loss = float(st[:, 0].sum() / ns)      # GCE: the mean of the reference's per-sample loss vector
        if lwf is not None:
            loss = loss + lam * float(st[:, 2].sum() / ns)
        return gsum, loss

    def lwf_loss(self, x, y_onehot, lwf, keep_prob=1., seed=None, input_weights=None):
        """`sess.run(model.LwF_loss, ...)`: the value LwF_train_step minimises, loss + lambda_o * mean_n l'_n, without a step
        (forward passes + alq_loss_stats).  lwf = (old logits [c, n], lambda_o, T)."""
        self._check_input_weights(input_weights)
        t, n = self._as_device_batch(x)
        return self._objective_pass(t, n, y_onehot, keep_prob, seed, input_weights, lwf, want_grad=False)[1]

    def train_on_batch(self, x, y_onehot, keep_prob=1., seed=None, pft_mask=None, input_weights=None, lwf=None, mt_feed=None):
        """One `sess.run(model.train_step, {x, y_, keep_prob})`: gradient of the batch-mean cross-entropy (summed over
        device passes of max_batch patches), one optimiser step on the device, weights repacked.  y_onehot: [c, n]
        like the reference's hot_labels (PW_AL.py:1064-1067); an all-zero column is an unlabelled sample.
        A PFT mask (set_PFT_mask, or `pft_mask` for this step only) multiplies the summed gradient before the step.
        With hypers (set_hypers) or `lwf` = (old logits [c, n], lambda_o, T) the gradient and the loss are those of the model's
        objective (_objective_pass; alq_param_grads_loss); per-sample `input_weights` [n] need hypers (ValueError without).
        Returns the batch-mean loss before the step."""
        if self._opt is None:
            raise RuntimeError('get_optimizer() has not been called (NN.py:1354)')
        torch = self.sess.torch
        t, n = self._as_device_batch(x)
        if self._is_device_labels(y_onehot):          # (a dense model's labels from datasets: checked where they are read)
            if not self.dense:
                raise TypeError('DeviceLabels feed a fully-convolutional model; an fc-head model takes one-hot columns')
            y = y_onehot
        else:
            y = np.asarray(y_onehot)
            if y.shape != (self.nclass, n * self.out_voxels):
                raise ValueError('labels must be [%d, %d] one-hot columns, got %r' % (self.nclass, n * self.out_voxels, y.shape))
        self._check_input_weights(input_weights)
        if self._obj is not None or lwf is not None or self.dense:
            gsum, loss = self._objective_pass(t, n, y, keep_prob, seed, input_weights, lwf, mt_feed=mt_feed)
        else:
            lab = np.where(y.sum(0) > 0, y.argmax(0), -1).astype(np.int32)
            kp, _, _, seed = self._drop_args(keep_prob, seed)
            labd = self.sess.to_device(lab, torch.int32)
            gsum = torch.zeros((self.num_params,), dtype=torch.float32, device=self.sess.device)
            loss = 0.
            for a in range(0, n, self.max_batch):
                b = min(n, a + self.max_batch)
                g, _, l = self.param_grads_device(t[a:b], b - a, 1, labels=labd[a:b], loss_scale=1. / n, keep_prob=kp,
                                                  seed=seed, first_sample=a, per_sample=False, want_loss=True)
                gsum += g
                loss += float(l.item()) * (b - a) / n
        o = self._opt
        if o['theta'] is None or o.get('version') != self._weights_version:
            # the TF variables are the single state of the reference: weights loaded or assigned since the last step
            # (set_weights / load_weights / perform_assign_ops) are what the next step updates; Adam's slots persist
            fresh = o['theta'] is None
            o['theta'] = self.sess.to_device(self.flat_params(), torch.float32)
        else:
            fresh = False
        if fresh:
            o['m'] = torch.zeros_like(o['theta'])
            o['v'] = torch.zeros_like(o['theta'])
            if o['name'] == 'RMSProp':                  # TF 1.x: the rms slot starts at ones, the momentum slot at zeros
                o['ms'] = torch.ones_like(o['theta'])
                o['mom'] = torch.zeros_like(o['theta'])
            tm = self._train_mask()
            o['mask'] = self.sess.to_device(tm, torch.float32) if tm is not None else None
        if o.get('mask') is not None:
            gsum *= o['mask']
        pmask, players = (self._pft_mask, self._pft_layers) if pft_mask is None else self._flat_mask(pft_mask)
        if pmask is not None:
            gsum *= pmask
            if o['name'] == 'Adam' and len(players) < self.L:
                # The mask multiplies the gradient only (NN_extended.py:1441-1449): Adam's moments persist, so a layer whose
                # mask is all zero still moves unless its m and v are all zero BEFORE this step (then m stays 0 and the step is
                # 0 / eps = 0) - the case when the mask held since the optimiser's first step.  L flags cross to the host.
                offs = self._param_offsets()
                still = torch.stack([((o['m'][a_:a_ + nw + nb] == 0).all() & (o['v'][a_:a_ + nw + nb] == 0).all())
                                     for a_, nw, nb in offs]).cpu().numpy()
                players = [q for q in range(self.L) if q in players or not still[q]]
            if o['name'] == 'RMSProp' and o['momentum'] != 0. and len(players) < self.L:
                # likewise: a masked layer goes on moving on the momentum it has (momentum 0: mom = lr * 0 / sqrt(.) = 0, it stays)
                still = torch.stack([(o['mom'][a_:a_ + nw + nb] == 0).all() for a_, nw, nb in self._param_offsets()]).cpu().numpy()
                players = [q for q in range(self.L) if q in players or not still[q]]
        if o.get('schedule') is not None:
            o['lr'] = float(o['schedule'](o['t']))          # the step count before this step: 0 at the first
        o['t'] += 1
        P = self.num_params
        self.sess.bind_stream()
        if o['name'] == 'SGD':
            check(self.lib.alq_sgd_step(self.sess.ctx, C.c_void_p(o['theta'].data_ptr()), C.c_void_p(gsum.data_ptr()), P, o['lr']))
        elif o['name'] == 'RMSProp':
            check(self.lib.alq_rmsprop_step(self.sess.ctx, C.c_void_p(o['theta'].data_ptr()), C.c_void_p(gsum.data_ptr()),
                                            C.c_void_p(o['ms'].data_ptr()), C.c_void_p(o['mom'].data_ptr()), P, o['lr'],
                                            o['decay'], o['momentum'], o['epsilon']))
        else:
            check(self.lib.alq_adam_step(self.sess.ctx, C.c_void_p(o['theta'].data_ptr()), C.c_void_p(gsum.data_ptr()),
                                         C.c_void_p(o['m'].data_ptr()), C.c_void_p(o['v'].data_ptr()), P, o['lr'],
                                         o.get('beta1', 0.9), o.get('beta2', 0.999), 1e-8, o['t']))      # a parameter masked out since the first step keeps m = v = 0: its step is 0 / eps = 0
        if self._host_repack:
            self.set_flat_params(o['theta'].cpu().numpy())
        else:
            # the model is fed from the device vector; a layer outside `train_layers` kept its weights (masked gradient: SGD
            # subtracts 0, Adam's m = v = 0 step is 0 / eps = 0) and its packed forms.  A layer whose PFT mask is all zero is
            # left out only where this step provably did not move it: SGD, or Adam with that layer's moments all zero (`players`)
            only = [t for t, nme in enumerate(self.var_names) if nme in self.train_layers] if self.train_layers else None
            if pmask is not None:
                only = [t for t in (range(self.L) if only is None else only) if t in players]
            self.set_weights_device(o['theta'], only=only)
        o['version'] = self._weights_version
        if self._mt is not None:
            from . import mteach
            self.cons_coeff = mteach.cons_coeff(o['t'], self._mt['rampup'], self._mt['max_coeff'])
        return loss

    def diagonal_fisher_device(self, t, n, labels):
        """alq_diag_fisher over device passes of max_batch patches: the mean over the n samples of the squared gradient of
        log posteriors[labels[i], i], flat float64 device tensor [P] in parameter order.  No per-sample gradient rows are
        formed; labels: int array or int32 device tensor [n]."""
        torch = self.sess.torch
        self.sess.bind_stream()
        lab = labels if isinstance(labels, torch.Tensor) else self.sess.to_device(np.asarray(labels, dtype=np.int32).reshape(n), torch.int32)
        assert lab.dtype == torch.int32 and lab.is_contiguous() and int(lab.numel()) == n
        acc = torch.zeros((self.num_params,), dtype=torch.float64, device=self.sess.device)
        for a in range(0, n, self.max_batch):
            b = min(n, a + self.max_batch)
            check(self.lib.alq_diag_fisher(self._m, C.c_void_p(t.data_ptr() + a * self.elems_per_patch * 4), b - a,
                                           C.c_void_p(lab.data_ptr() + a * 4), C.c_void_p(acc.data_ptr())))
        return acc.div_(max(n, 1))

    def diagonal_fisher(self, x, labels=None, batch=None, fused=None):
        """model_utils.diagonal_Fisher (model_utils.py:294-330): mean over samples of the squared gradient of the
        log-likelihood of the sample's label (labels given) or of the model's own prediction (None), per parameter.
        Returns the list of arrays in variable shapes.  Default: the fused statistic (diagonal_fisher_device); fused=False or
        ALQ_DIAGF_ROWS=1: per-sample gradient rows squared and folded (alq_param_grads + alq_sq_accum), the A/B arm; `batch`
        caps the rows of one of its passes (the fused arm forms none and runs passes of max_batch)."""
        torch = self.sess.torch
        t, n = self._as_device_batch(x)
        if labels is None:
            post, pred, _ = self.forward_device(t, n, want_pred=True)
            labels = pred.cpu().numpy()
        labels = np.asarray(labels).astype(np.int64)
        if fused is None:
            fused = os.environ.get('ALQ_DIAGF_ROWS', '0') in ('', '0')
        if fused:
            return self.unflatten(self.diagonal_fisher_device(t.reshape(n, -1), n, labels.astype(np.int32)).cpu().numpy())
        return self.unflatten(self.diagonal_fisher_rows_device(t, n, labels, batch).cpu().numpy())

    def diagonal_fisher_rows_device(self, t, n, labels, batch=None):
        """The rows arm of diagonal_fisher on the device (A/B; tools/gpu_diagfisher.py): per class, the per-sample gradient rows
        of up to `batch` samples (alq_param_grads) squared and folded (alq_sq_accum).  labels: host int array [n].  Flat
        float64 device tensor [P], the mean over the n samples."""
        torch = self.sess.torch
        labels = np.asarray(labels).astype(np.int64)
        acc = torch.zeros((self.num_params,), dtype=torch.float64, device=self.sess.device)
        step = min(self.max_batch, batch or self.max_batch)
        for j in range(self.nclass):
            idx = np.nonzero(labels == j)[0]
            for a in range(0, len(idx), step):
                sel = self.sess.to_device(idx[a:a + step], torch.int64)
                xs = t.reshape(n, -1).index_select(0, sel)
                g, _, _ = self.param_grads_device(xs, int(sel.numel()), 0, cls=j)
                check(self.lib.alq_sq_accum(self.sess.ctx, C.c_void_p(g.data_ptr()), self.num_params, int(sel.numel()),
                                            C.c_void_p(acc.data_ptr())))
        return acc.div_(max(n, 1))

    # -- last-layer closed forms (NN.py:874-1029, PW_NNAL.py:851-881) -------------------------
    _LLFC_SLICE = 32768        # samples / columns per launch (alq.h: at most 65535; they are independent)

    def _require_llfc(self):
        """The closed forms take `feature_layer` as the input u of the last fc layer."""
        wshape = self.param_shapes[-1][1]
        if self.feature_idx is None or self.layers[-1]['type'] != ALQ_FC or self.feature_dim * self.nclass != int(np.prod(wshape)):
            raise ValueError('feature_layer (%r, %d values) is not the input of the last fc layer (weights %r)' %
                             (self.feature_idx, self.feature_dim, tuple(wshape)))

    def llfc_reference_order(self):
        """Index vector [P]: entry j*d + i of a reference-ordered last-layer vector (NN.py:296-301 flatten order) is entry
        idx[j*d + i] of the device's (feature-memory order); the biases keep their places."""
        d, c = self.feature_dim, self.nclass
        perm = self._feature_perm if self._feature_perm is not None else np.arange(d)
        return np.concatenate([(np.arange(c)[:, None] * d + np.asarray(perm)[None, :]).reshape(-1), c * d + np.arange(c)])

    def llfc_grads_device(self, feat, post, labels):
        """alq_llfc_grads: the gradients of log posteriors[labels[n], n] with respect to the last fc layer, float32 device
        tensor [n, (d+1)c] (W class-major, then b), from device tensors feat [n, d], post [c, n] (forward_device) and labels
        (int array or device tensor [n]).  Features in the device's memory order (llfc_reference_order)."""
        torch = self.sess.torch
        self._require_llfc()
        self.sess.bind_stream()
        n, d, c = int(feat.shape[0]), self.feature_dim, self.nclass
        lab = labels if isinstance(labels, torch.Tensor) else self.sess.to_device(np.asarray(labels).reshape(n), torch.int32)
        lab = lab.to(torch.int32).contiguous()
        assert feat.dtype == torch.float32 and feat.is_contiguous() and tuple(feat.shape) == (n, d)
        assert post.dtype == torch.float32 and tuple(post.shape) == (c, n) and int(lab.numel()) == n
        out = self.sess.empty((n, (d + 1) * c), torch.float32)
        for a in range(0, n, self._LLFC_SLICE):
            b = min(n, a + self._LLFC_SLICE)
            pb = post[:, a:b].contiguous()
            check(self.lib.alq_llfc_grads(self.sess.ctx, C.c_void_p(feat.data_ptr() + a * d * 4), C.c_void_p(pb.data_ptr()),
                                          C.c_void_p(lab.data_ptr() + a * 4), b - a, d, c, C.c_void_p(out.data_ptr() + a * (d + 1) * c * 4)))
        return out

    def _require_llfc_hess_fits(self):
        """Before anything is computed or allocated: the explicit matrix must stay under the library's byte cap."""
        self._require_llfc()
        P = (self.feature_dim + 1) * self.nclass
        cap = int(self.lib.alq_llfc_hess_max_bytes())
        if P * P * 8 > cap:
            raise ValueError('the explicit last-layer Hessian of (d+1)c = %d parameters takes %d bytes (cap %d): use the implicit '
                             'routes, PW_NNAL.stoch_approx_IF / DeviceModel.llfc_stoch_if_device' % (P, P * P * 8, cap))

    def llfc_hess_device(self, feat_one, post_one):
        """alq_llfc_hess: the explicit [(d+1)c, (d+1)c] float64 Hessian of one sample's loss in the last fc layer."""
        torch = self.sess.torch
        self._require_llfc_hess_fits()
        d, c = self.feature_dim, self.nclass
        P = (d + 1) * c
        self.sess.bind_stream()
        f = feat_one.reshape(-1).contiguous()
        p = post_one.reshape(-1).contiguous()
        assert f.dtype == torch.float32 and int(f.numel()) == d and p.dtype == torch.float32 and int(p.numel()) == c
        H = self.sess.empty((P, P), torch.float64)
        check(self.lib.alq_llfc_hess(self.sess.ctx, C.c_void_p(f.data_ptr()), C.c_void_p(p.data_ptr()), d, c, C.c_void_p(H.data_ptr())))
        return H

    def llfc_stoch_if_features_device(self, pool_feat, pool_post, pool_labels, tr_feat, tr_post, draws, scale, path=0):
        """alq_llfc_stoch_if on features that are already there: pool_feat [n_pool, d], pool_post [c, n_pool], tr_feat [n_tr, d],
        tr_post [c, n_tr] float32 device tensors, `draws` indices into the training rows.  float32 device tensor [n_pool, (d+1)c]."""
        torch = self.sess.torch
        self.sess.bind_stream()
        d, c = int(pool_feat.shape[1]), int(pool_post.shape[0])
        n_pool, n_tr = int(pool_feat.shape[0]), int(tr_feat.shape[0]) if tr_feat is not None else 0
        draws = np.asarray(draws, dtype=np.int64).reshape(-1)
        T = int(draws.size)
        if T and (n_tr < 1 or draws.min() < 0 or draws.max() >= n_tr):
            raise ValueError('draws outside the %d training samples' % n_tr)
        dr = self.sess.to_device(draws.astype(np.int32), torch.int32) if T else None
        lab = pool_labels.to(torch.int32).contiguous()
        for t_ in (pool_feat, tr_feat):
            assert t_ is None or (t_.dtype == torch.float32 and t_.is_contiguous() and int(t_.shape[1]) == d)
        tp = tr_post.contiguous() if tr_post is not None else None
        P = (d + 1) * c
        V = self.sess.empty((n_pool, P), torch.float32)

        def ptr(t_, off=0):
            return C.c_void_p(t_.data_ptr() + off) if t_ is not None else None
        for a in range(0, n_pool, self._LLFC_SLICE):
            b = min(n_pool, a + self._LLFC_SLICE)
            pb = pool_post[:, a:b].contiguous()
            work = self.sess.empty((max(int(self.lib.alq_llfc_if_work_bytes(b - a, c)), 8),), torch.uint8)
            check(self.lib.alq_llfc_stoch_if(self.sess.ctx, ptr(pool_feat, a * d * 4), ptr(pb), ptr(lab, a * 4), b - a, ptr(tr_feat), ptr(tp),
                                             n_tr, ptr(dr), T, float(scale), d, c, int(path), ptr(V, a * P * 4), ptr(work)))
        return V

    def llfc_stoch_if_device(self, pool_t, n_pool, tr_t, draws, scale, path=0):
        """The recursion of PW_NNAL.stoch_approx_IF on the device: V_0 = the last-layer gradients of the n_pool device patches
        `pool_t` at their predicted labels, then one step per entry of `draws` (row indices into the device patches `tr_t`).
        One forward pass over the pool and one over the training patches; nothing leaves the device.  Returns (V float32 device
        [n_pool, (d+1)c] in the device's feature order - llfc_reference_order - and the predicted labels, int64 device [n_pool])."""
        self._require_llfc()
        post, pred, feat = self.forward_device(pool_t, n_pool, want_pred=True, want_feat=True)
        tpost = tfeat = None
        if len(draws):
            n_tr = int(tr_t.numel()) // self.elems_per_patch
            tpost, _, tfeat = self.forward_device(tr_t, n_tr, want_feat=True)
        return self.llfc_stoch_if_features_device(feat, post, pred, tfeat, tpost, draws, scale, path), pred

    # -- weights ---------------------------------------------------------------------------
    def set_weights(self, pars):
        """`pars`: name -> [W, b] in TF layouts (HWIO / DHWIO, transpose [k..,out,in], fc [out,in],
        fc bias [out,1]); the weight interchange of NN.py:390-394 / :508-517 with numpy arrays in
        place of the HDF5 datasets (h5py is not in the image)."""
        staged = []
        for t, (name, wshape, bshape) in enumerate(self.param_shapes):
            W, b = pars[name]
            W = np.ascontiguousarray(np.asarray(W, dtype=np.float32))
            b = np.ascontiguousarray(np.asarray(b, dtype=np.float32))
            if tuple(W.shape) != tuple(wshape) or b.size != int(np.prod(bshape)):
                raise ValueError('layer %s: expected W%s b%s, got W%s b%s' % (name, wshape, bshape, W.shape, b.shape))
            staged.append((W, b))
        torch = self.sess.torch
        self.var_dict.mark_fresh()
        self.sess.bind_stream()
        for t, name in enumerate(self.var_names):
            W, b = staged[t]
            if self._dev_pack[t] and not self._host_repack:
                # a wide fc layer: the raw arrays are uploaded once and packed on the device; the extra pipelines' models are fed
                # from the same tensors (_extra_lanes)
                Wd, bd = self.sess.to_device(W, torch.float32), self.sess.to_device(b, torch.float32)
                check(self.lib.alq_model_set_weights_device(self._m, t, C.c_void_p(Wd.data_ptr()), C.c_void_p(bd.data_ptr())))
                self._dev_w[t] = (Wd, bd)
            else:
                check(self.lib.alq_model_set_weights(self._m, t, W.ctypes.data_as(C.c_void_p),
                                                     b.ctypes.data_as(C.c_void_p)))
                self._dev_w[t] = None
            self.var_dict[name] = [W, b]
        self._weights_version += 1

    def _device_slices(self, src):
        """[(W, b)] device fp32 tensors per parameterised layer from a flat parameter-order vector [P], a dict
        name -> (W, b) or a list of (W, b)."""
        torch = self.sess.torch
        if isinstance(src, torch.Tensor):
            if src.dtype != torch.float32 or not src.is_contiguous() or int(src.numel()) != self.num_params or not src.is_cuda:
                raise ValueError('expected a contiguous device fp32 vector of %d parameters' % self.num_params)
            flat = src.reshape(-1)
            pairs = self.unflatten(flat)
            return [(pairs[2 * t], pairs[2 * t + 1]) for t in range(self.L)]
        if isinstance(src, dict):
            src = [src[nme] for nme in self.var_names]
        if len(src) != self.L:
            raise ValueError('expected %d (W, b) pairs, got %d' % (self.L, len(src)))
        out = []
        for (name, wshape, bshape), (W, b) in zip(self.param_shapes, src):
            for a, shp in ((W, wshape), (b, bshape)):
                if not (isinstance(a, torch.Tensor) and a.is_cuda and a.dtype == torch.float32 and a.is_contiguous() and
                        int(a.numel()) == int(np.prod(shp))):
                    raise ValueError('layer %s: expected contiguous device fp32 tensors W%s b%s' % (name, wshape, bshape))
            out.append((W, b))
        return out

    def set_weights_device(self, theta_or_slices, only=None):
        """`set_weights` from DEVICE memory (alq_model_set_weights_device): a flat parameter-order fp32 vector [P] (what the
        optimiser step updates), a dict name -> (W, b) or a list of (W, b) device tensors in TF layouts.  The tensors must be
        ready on the current stream.  Wide fc layers are packed by device kernels, any other layer's slice takes the host
        packers; `var_dict` turns stale and is fetched on its next read.  `only`: the layer indices whose values changed
        (the rest of the model keeps its packed weights); the source still holds every layer.  The model keeps a reference
        to the tensors (they feed the extra scoring pipelines): the caller may update them in place only together with
        another call."""
        torch = self.sess.torch
        sl = self._device_slices(theta_or_slices)
        if self._host_repack:
            pars = OrderedDict((nme, [sl[t][0].cpu().numpy().reshape(self.param_shapes[t][1]),
                                      sl[t][1].cpu().numpy().reshape(self.param_shapes[t][2])])
                               for t, nme in enumerate(self.var_names))
            return self.set_weights(pars)
        if only is not None and any(v is None for v in OrderedDict.values(self.var_dict)) and not self.var_dict.stale:
            only = None          # nothing set yet: every layer needs its weights
        self.sess.bind_stream()
        for t in (range(self.L) if only is None else only):
            W, b = sl[t]
            check(self.lib.alq_model_set_weights_device(self._m, t, C.c_void_p(W.data_ptr()), C.c_void_p(b.data_ptr())))
        self._dev_w = list(sl)
        flat = theta_or_slices if isinstance(theta_or_slices, torch.Tensor) else None

        def refresh():
            if flat is not None:          # one copy of the whole vector, cut like set_flat_params cuts it
                arrs = self.unflatten(flat.reshape(-1).cpu().numpy())
            else:
                arrs = [a.cpu().numpy().reshape(shp) for (W, b), (_, ws, bs) in zip(sl, self.param_shapes)
                        for a, shp in ((W, ws), (b, bs))]
            for t, nme in enumerate(self.var_names):
                self.var_dict.put(nme, [arrs[2 * t], arrs[2 * t + 1]])
        self.var_dict.mark_stale(refresh)
        self._weights_version += 1

    def load_weights(self, path, session=None):
        """CNN.load_weights (NN.py:396-419; NN_extended.py:708-760): an HDF5 file of the reference - groups per layer, datasets
        `Weight` / `Bias` in TF layouts - when h5py is importable, or the .npz twin (keys '<layer>/Weight', '<layer>/Bias')."""
        from . import weights_io
        self.set_weights(weights_io.read_weights(path, self.var_names))

    def save_weights(self, path):
        """CNN.save_weights (NN.py:379-394): `.h5` -> the reference's HDF5 layout (needs h5py), anything else -> the .npz twin."""
        from . import weights_io
        weights_io.write_weights(path, self.var_dict)

    def add_assign_ops(self):
        """No graph to extend (NN.py:421-458): kept so loop code calls it unchanged."""

    def perform_assign_ops(self, file_path, sess=None):
        """NN.py:462-519: 'init' draws He-normal weights with the global np.random in variable
        creation order (std = sqrt(2/n), zero biases); otherwise loads a weight file."""
        if file_path != 'init':
            return self.load_weights(file_path)
        pars = OrderedDict()
        for name, wshape, bshape in self.param_shapes:
            n = int(np.prod(wshape[:-1])) if len(wshape) > 2 else wshape[1]
            pars[name] = [np.sqrt(2. / n) * np.random.randn(*wshape), np.zeros(bshape)]
        self.set_weights(pars)

    # -- evaluation ------------------------------------------------------------------------
    def _feature_permutation(self):
        """feature_layer of a conv/pool layer is flattened in the reference's order (full axis
        reversal, NN.py:296-301,337-340); the device returns memory order.  Identity after an fc."""
        if self.feature_idx is None:
            return None
        # re-derive the layer's output geometry
        nd = len(self.in_shape) - 1
        spatial = list(self.in_shape[:-1])
        ch = self.in_shape[-1]
        for i, d in enumerate(self.layers):
            if d['type'] == ALQ_CONV:
                ch = d['cout']
            elif d['type'] == ALQ_CONVT:
                spatial = [a * b for a, b in zip(spatial, d['s'][3 - nd:])]
                ch = d['cout']
            elif d['type'] == ALQ_POOL:
                spatial = [-(-a // b) for a, b in zip(spatial, d['s'][3 - nd:])]
            else:
                return None                      # at or after an fc: already a flat vector
            if i == self.feature_idx:
                mem = np.arange(int(np.prod(spatial)) * ch).reshape(spatial + [ch])
                return mem.transpose(*reversed(range(nd + 1))).reshape(-1)
        return None

    def _as_device_batch(self, x):
        torch = self.sess.torch
        if isinstance(x, torch.Tensor):
            t = x.to(device=self.sess.device, dtype=torch.float32).contiguous()
        else:
            t = self.sess.to_device(np.asarray(x), torch.float32)    # placeholder is tf.float32
        n = t.numel() // self.elems_per_patch
        if n * self.elems_per_patch != t.numel():
            raise ValueError('batch of %d elements is not a multiple of the patch size %d' % (t.numel(), self.elems_per_patch))
        return t, n

    def forward_dropout_device(self, t, n, keep_prob, seed=None, first_sample=0, want_pred=False):
        """Posteriors at keep_prob < 1 (MC strategies): alq_forward_dropout over device passes; masks keyed by sample id."""
        torch = self.sess.torch
        self.sess.bind_stream()
        kp, arr, nl, seed = self._drop_args(keep_prob, seed)
        V = self.out_voxels          # samples per patch: 1, or the voxels of a dense model's output map
        post = self.sess.empty((self.nclass, n * V), torch.float32)
        pred = self.sess.empty((n * V,), torch.int64) if want_pred else None
        for a in range(0, n, self.max_batch):
            b = min(n, a + self.max_batch)
            pb = self.sess.empty((self.nclass, (b - a) * V), torch.float32)
            check(self.lib.alq_forward_dropout(self._m, C.c_void_p(t.data_ptr() + a * self.elems_per_patch * 4), b - a, kp, seed,
                                               int(first_sample) + a, arr, nl, C.c_void_p(pb.data_ptr()),
                                               C.c_void_p(pred.data_ptr() + a * V * 8) if want_pred else None))
            post[:, a * V:b * V] = pb
        return post, pred

    def forward_device(self, t, n, want_pred=False, want_feat=False, rows=None):
        """t: device fp32 tensor of n patches - or, with `rows` (int64 device tensor [n]), a resident pool whose
        rows `rows` are the patches (alq_forward_rows: no gathered copy on the caller's side).
        Returns device tensors (post [c,n], pred, feat)."""
        torch = self.sess.torch
        self.sess.bind_stream()
        V = self.out_voxels          # samples per patch: 1, or the voxels of a dense model's output map
        if rows is not None and self.dense:
            raise NotImplementedError('forward_device(rows=...): not defined for a fully-convolutional model (1x1 conv head)')
        post = self.sess.empty((self.nclass, n * V), torch.float32)
        pred = self.sess.empty((n * V,), torch.int64) if want_pred else None
        feat = self.sess.empty((n, self.feature_dim), torch.float32) if want_feat else None
        if rows is not None:
            assert rows.dtype == torch.int64 and rows.is_contiguous() and int(rows.numel()) == n
        # one pipeline: forward-only passes leave no gaps a second one could fill (configs[4]'s filter: 0.3625 s per 200k patches
        # with two pipelines against 0.3601 s with one, same box)
        for a in range(0, n, self.max_batch):
            b = min(n, a + self.max_batch)
            pb = self.sess.empty((self.nclass, (b - a) * V), torch.float32)
            outs = (C.c_void_p(pb.data_ptr()),
                    C.c_void_p(pred.data_ptr() + a * V * 8) if want_pred else None,
                    C.c_void_p(feat.data_ptr() + a * self.feature_dim * 4) if want_feat else None,
                    self.feature_idx if want_feat else -1)
            if rows is None:
                check(self.lib.alq_forward(self._m, C.c_void_p(t.data_ptr() + a * self.elems_per_patch * 4), b - a, *outs))
            else:
                check(self.lib.alq_forward_rows(self._m, C.c_void_p(t.data_ptr()), C.c_void_p(rows.data_ptr() + a * 8),
                                                b - a, *outs))
            post[:, a * V:b * V] = pb
        return post, pred, feat

    def forward_maps_device(self, t, n, keep_prob=1., want_pred=False, seed=None, first_sample=0):
        """A dense model's outputs as maps, on the device: (posteriors [n, *spatial, c] float32 - `model.posteriors` of the
        reference's FCN branch, NN_extended.py:262-294 - and prediction [n, *spatial] int64 or None).  The posteriors are a view of
        the class-major planes [c, n V] the library wrote (`.movedim(-1, 0)` is that array again).  first_sample: the dropout keys
        of the samples are first_sample .. first_sample + n - 1 (keep_prob < 1)."""
        if not self.dense:
            raise NotImplementedError('forward_maps_device: the model has an fc head (no output map)')
        if float(keep_prob) < 1. and len(self.dropout_layers):
            post, pred = self.forward_dropout_device(t, n, keep_prob, seed=seed, first_sample=first_sample, want_pred=want_pred)
        else:
            post, pred, _ = self.forward_device(t, n, want_pred)
        maps = post.reshape((self.nclass, n) + self.out_map_shape).movedim(0, -1)
        return maps, (pred.reshape((n,) + self.out_map_shape) if pred is not None else None)

    def forward_au_device(self, t, n, keep_prob=1., seed=None, want_output=True):
        """An AU_4U model's `AU_vals` [n, *spatial] and `output` [n, *spatial, c + 1] (or None) on the device: alq_forward_au over
        passes of max_batch; keep_prob < 1 drops as forward_dropout_device does ('MC-sigma')."""
        if not self.AU_4U:
            raise NotImplementedError('forward_au_device: the model has no aleatoric-uncertainty head (AU_4U)')
        torch = self.sess.torch
        self.sess.bind_stream()
        kp, arr, nl, seed = self._drop_args(keep_prob, seed)
        V, ct = self.out_voxels, self.nclass + 1
        au = self.sess.empty((n * V,), torch.float32)
        out = self.sess.empty((n * V, ct), torch.float32) if want_output else None
        for a in range(0, n, self.max_batch):
            b = min(n, a + self.max_batch)
            check(self.lib.alq_forward_au(self._m, C.c_void_p(t.data_ptr() + a * self.elems_per_patch * 4), b - a, kp, seed, a, arr, nl,
                                          None, None, C.c_void_p(au.data_ptr() + a * V * 4),
                                          C.c_void_p(out.data_ptr() + a * V * ct * 4) if want_output else None))
        return au.reshape((n,) + self.out_map_shape), (out.reshape((n,) + self.out_map_shape + (ct,)) if want_output else None)

    def _run_dense(self, fetch, feed_dict, x, kp, iw):
        """sess.run of a dense model: `posteriors` [n, *spatial, c], `prediction` [n, *spatial], `feature_layer`, `loss` and
        `train_step` with `y_` one-hot [n, *spatial, c] (an all-zero row: unlabelled voxel, NN_extended.py:1291-1293) and
        `input_vox_weights` [n, *spatial].  A datasets.DeviceLabels under `y_` (labels [n, *spatial] built on the device) is read in
        place: no one-hot, no argmax, no upload; the non-zero-weight count comes from its class counts."""
        name = fetch.name
        if name in ('posteriors', 'prediction'):
            t, n = self._as_device_batch(x)
            maps, pred = self.forward_maps_device(t, n, kp, want_pred=name == 'prediction')
            return (pred if name == 'prediction' else maps.contiguous()).cpu().numpy()
        if name == 'feature_layer':
            return self.forward(x, want=(name,), keep_prob=kp)[name]
        if name in ('AU_vals', 'output') and self.AU_4U:
            t, n = self._as_device_batch(x)
            au, out = self.forward_au_device(t, n, kp, want_output=name == 'output')
            return (au if name == 'AU_vals' else out).cpu().numpy()
        mt_on = self._mt is not None and getattr(self, 'teacher', None) is not None
        if name not in ('loss', 'train_step') + (('labeled_loss', 'cons_loss') if mt_on else ()):
            raise NotImplementedError('sess.run(model.%s) is not defined for a fully-convolutional model (1x1 conv head)' % name)
        y = feed_dict[self.y_]
        on_device = self._is_device_labels(y)          # datasets.DeviceLabels: the labels stay where they are
        y = y if on_device else np.asarray(y)
        n = int(np.asarray(x).shape[0]) if not isinstance(x, self.sess.torch.Tensor) else int(x.shape[0])
        if tuple(y.shape) != (n,) + self.out_map_shape + (self.nclass,):
            raise ValueError('y_ must be one-hot %r, got %r' % ((n,) + self.out_map_shape + (self.nclass,), tuple(y.shape)))
        ycols = y if on_device else np.ascontiguousarray(y.reshape(-1, self.nclass).T)
        if iw is not None:
            iw = np.asarray(iw)
            if tuple(iw.shape) != (n,) + self.out_map_shape:
                raise ValueError('input_vox_weights must be %r, got %r' % ((n,) + self.out_map_shape, tuple(iw.shape)))
            iw = iw.reshape(-1)
        mt_feed = dict(kp=float(feed_dict.get(self.teacher.keep_prob, 1.)), px=feed_dict.get(self.perturbed_x)) if mt_on else None
        if name in ('loss', 'labeled_loss', 'cons_loss'):
            t, n = self._as_device_batch(x)
            loss = self._objective_pass(t, n, ycols, kp, None, iw, None, want_grad=False, mt_feed=mt_feed)[1]
            return loss if name == 'loss' else self._mt['last'][name == 'cons_loss']
        ph = getattr(self, 'par_placeholders', None)
        fed = [h in feed_dict for h in ph] if ph else []
        if any(fed) and not all(fed):
            raise KeyError('a PFT step needs a mask for every entry of par_placeholders')
        return self.train_on_batch(x, ycols, keep_prob=kp, pft_mask=[feed_dict[h] for h in ph] if any(fed) else None, input_weights=iw,
                                   mt_feed=mt_feed)

    def forward(self, x, want=('posteriors',), keep_prob=1.):
        t, n = self._as_device_batch(x)
        if float(keep_prob) < 1. and len(self.dropout_layers):
            if 'feature_layer' in want:
                raise NotImplementedError('feature_layer at keep_prob < 1')
            post, pred = self.forward_dropout_device(t, n, keep_prob, want_pred='prediction' in want)
            res = {'posteriors': post.cpu().numpy()}
            if pred is not None:
                res['prediction'] = pred.cpu().numpy()
            return res
        post, pred, feat = self.forward_device(t, n, 'prediction' in want, 'feature_layer' in want)
        res = {'posteriors': post.cpu().numpy()}
        if pred is not None:
            res['prediction'] = pred.cpu().numpy()
        if feat is not None:
            f = feat.cpu().numpy()
            if self._feature_perm is not None:
                f = f[:, self._feature_perm]
            res['feature_layer'] = np.ascontiguousarray(f.T)       # [F, n] like the reference
        return res

    def fisher_device(self, t, n, p1_in=None, diag_load=1e-5, want=('p1', 'g0', 'g1', 'A', 'trace', 'Asum'), rows=None):
        """Device-resident Fisher scoring of n patches (t: device fp32; with `rows`, rows of the resident pool `t`:
        alq_fisher_rows).  Returns device tensors; 'Asum' is the sum over the n patches (fixed summation order per
        launch).  'H' (Shannon entropy of the posteriors, alq_score_entropy) is produced on request."""
        torch = self.sess.torch
        self.sess.bind_stream()
        if rows is not None:
            assert rows.dtype == torch.int64 and rows.is_contiguous() and int(rows.numel()) == n
        L = self.L
        out = {}
        out['p1'] = self.sess.empty((n,), torch.float32) if 'p1' in want else None
        out['g0'] = self.sess.empty((n, L), torch.float64) if 'g0' in want else None
        out['g1'] = self.sess.empty((n, L), torch.float64) if 'g1' in want else None
        out['A'] = self.sess.empty((n, L, L), torch.float64) if 'A' in want else None
        out['trace'] = self.sess.empty((n,), torch.float64) if 'trace' in want else None
        asum = torch.zeros((L, L), dtype=torch.float64, device=self.sess.device) if 'Asum' in want else None
        part = self.sess.empty((L, L), torch.float64) if asum is not None else None

        def ptr(tn, off_elems, itemsize):
            return C.c_void_p(tn.data_ptr() + off_elems * itemsize) if tn is not None else None

        # Device passes of max_batch patches alternate between two PIPELINES (own libalq context = own stream pair, own
        # workspaces, the same weights): the tail of one pass (the last box-filter dot products, finalisation) and its
        # small kernels run beside the next pass's first launches instead of leaving the chip idle.  Each pass is the same
        # launches on the same data whichever pipeline runs it, so every per-patch output is bit-identical to ALQ_LANES=1;
        # the passes' partial sums of A are added in pass order after the join.
        # Pass sizes: an EVEN number of equal passes, so that two pipelines get the same work (100,000 patches at 2047 per pass are 49
        # passes: one pipeline ran 25 of them and the other idled through the last one: 268.0 against 272.7 k patches/s same-box,
        # three rounds).  Per-patch results do not depend on the cut (tests: any batch cut is bit-identical); the cut itself does not
        # depend on the number of pipelines, so the pass-ordered sum of A is the same bits with one, two or three.  (A multiple of 6
        # - equal shares for three pipelines as well - was tried: 50 ... 56 passes score the same within noise on NET-C, but NET-B
        # streams its 168 MB of fc weights once per pass and 16,384 patches became 12 passes instead of 8: ALQ_PASS_MULT=6.)
        step, starts = self.pass_cut(n)
        nl = min(self.lanes, len(starts))
        extra = self._extra_lanes(nl - 1) if nl > 1 else []
        part = self.sess.empty((max(len(starts), 1), L, L), torch.float64) if asum is not None else None
        cur = torch.cuda.current_stream(self.sess.device)
        # with several pipelines whole passes overlap: the per-context side streams (the statistics kernels of a layer beside its
        # contraction) then only add streams competing for the same gaps (274.4 -> 277.8 k patches/s without them, same box,
        # three rounds); a single pipeline keeps its side stream (+3.4 %, round 4).  Same kernels, same results either way.
        side_on = 0 if (extra and not os.environ.get('ALQ_LANES_SIDE_STREAM')) else 1
        check(self.lib.alq_ctx_use_side_stream(self.sess.ctx, side_on))
        for ln in extra:
            check(self.lib.alq_ctx_use_side_stream(ln['sess'].ctx, side_on))
            ln['stream'].wait_stream(cur)          # inputs, output buffers and the weights are ordered on the caller's stream
        for k, a in enumerate(starts):
            b = min(n, a + step)
            outs = (ptr(p1_in, a, 4), float(diag_load), ptr(out['p1'], a, 4), ptr(out['g0'], a * L, 8),
                    ptr(out['g1'], a * L, 8), ptr(out['A'], a * L * L, 8), ptr(out['trace'], a, 8),
                    C.c_void_p(part.data_ptr() + k * L * L * 8) if part is not None else None)

            def launch(m):
                if rows is None:
                    check(self.lib.alq_fisher(m, C.c_void_p(t.data_ptr() + a * self.elems_per_patch * 4), b - a, *outs))
                else:
                    check(self.lib.alq_fisher_rows(m, C.c_void_p(t.data_ptr()), C.c_void_p(rows.data_ptr() + a * 8), b - a, *outs))
            which = k % nl
            if which:
                ln = extra[which - 1]
                with torch.cuda.stream(ln['stream']):
                    ln['sess'].bind_stream()
                    launch(ln['m'])
            else:
                launch(self._m)
        for ln in extra:
            cur.wait_stream(ln['stream'])
        if not side_on:
            check(self.lib.alq_ctx_use_side_stream(self.sess.ctx, 1))
        if asum is not None:
            for k in range(len(starts)):
                asum += part[k]
        out['Asum'] = asum
        if 'H' in want or 'absdev' in want:
            if out['p1'] is None:
                raise ValueError("'H' / 'absdev' need 'p1' in `want`")
            out['H'] = self.sess.empty((n,), torch.float32) if 'H' in want else None
            out['absdev'] = self.sess.empty((n,), torch.float64) if 'absdev' in want else None
            check(self.lib.alq_score_entropy(self.sess.ctx, C.c_void_p(out['p1'].data_ptr()), n,
                                             ptr(out['absdev'], 0, 8), ptr(out['H'], 0, 4)))
        return out

    def _creation_env(self):
        """The ALQ_* engine switches are read when a model is created and when its weights are packed: the second pipeline's
        model is built under the ones the first was created with."""
        import contextlib

        @contextlib.contextmanager
        def cm():
            now = {k: v for k, v in os.environ.items() if k.startswith('ALQ_')}
            for k in now:
                del os.environ[k]
            os.environ.update(self._create_env)
            try:
                yield
            finally:
                for k in self._create_env:
                    os.environ.pop(k, None)
                os.environ.update(now)
        return cm()

    def pass_cut(self, n):
        """How fisher_device cuts n patches into device passes: (patches per pass, first patch of every pass)."""
        step = self.max_batch
        if n > self.max_batch and not os.environ.get('ALQ_NO_PASS_BALANCE'):
            P = -(-n // self.max_batch)
            mult = int(os.environ.get('ALQ_PASS_MULT', '2'))          # (tuning experiments)
            P = -(-P // mult) * mult if P >= mult else P + (P & 1)
            step = -(-n // P)
        return step, list(range(0, n, step))

    @property
    def _lane2(self):
        """The first extra pipeline (None until a call needed one): what the tests of round 5 look at."""
        return self._xlanes[0] if self._xlanes else None

    def _extra_lanes(self, count):
        """`count` extra scoring pipelines of fisher_device: each a libalq context on its own torch stream and a model of the same
        layers on it; their weights follow `set_weights` / `set_weights_device`: wide fc layers from the device tensors the first
        model was fed from, the other layers from the host copies in var_dict."""
        torch = self.sess.torch
        while len(self._xlanes) < count:
            stream = torch.cuda.Stream(self.sess.device)
            with torch.cuda.stream(stream):
                sess2 = DeviceSession(self.sess.device.index)
            m = C.c_void_p()
            arr, nl, cd = self._create_args
            with self._creation_env():
                check(self.lib.alq_model_create(sess2.ctx, arr, nl, cd, self.max_batch, C.byref(m)))
            if int(self.lib.alq_model_max_batch(m)) != self.max_batch:
                self.lib.alq_model_destroy(m)
                raise _lib.AlqError('extra pipeline: the library granted another batch size')
            self._xlanes.append(dict(sess=sess2, stream=stream, m=m, version=None))
        for ln in self._xlanes[:count]:
            if ln['version'] != self._weights_version:
                if not self.var_dict.stale and any(v is None for v in self.var_dict.values()):
                    raise RuntimeError('set_weights() has not been called')
                # the pipeline's context runs on its own stream: what fills the device tensors (an upload, the optimiser step) is
                # ordered on the caller's
                ln['stream'].wait_stream(torch.cuda.current_stream(self.sess.device))
                with self._creation_env():
                    for ti, name in enumerate(self.var_names):
                        if self._dev_pack[ti] and self._dev_w[ti] is not None and not self._host_repack:
                            Wd, bd = self._dev_w[ti]
                            with torch.cuda.stream(ln['stream']):
                                ln['sess'].bind_stream()
                                check(self.lib.alq_model_set_weights_device(ln['m'], ti, C.c_void_p(Wd.data_ptr()), C.c_void_p(bd.data_ptr())))
                            continue
                        W, b = self.var_dict[name]
                        check(self.lib.alq_model_set_weights(ln['m'], ti, W.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)))
                ln['version'] = self._weights_version
        return self._xlanes[:count]

    def fisher(self, x, p1=None, diag_load=1e-5):
        t, n = self._as_device_batch(x)
        p1_in = None
        if p1 is not None:
            p1_in = self.sess.to_device(np.asarray(p1, dtype=np.float32), self.sess.torch.float32)
        out = self.fisher_device(t, n, p1_in, diag_load)
        return {k: (v.cpu().numpy() if v is not None else None) for k, v in out.items()}

    def shrunk_class_gradients(self, x):
        """g [n, c, L'] float64: shrink_gradient(d log posteriors[j, sample] / d theta, 'sum') for every sample and class -
        what the reference obtains with one session.run(model.grad_posts[str(j)]) per sample and class plus a host
        reduction (NNAL.py:381-405, NNAL_tools.py:784-796).  Per device pass: alq_param_grads (mode 0, per-sample rows)
        for class j, alq_shrink_sum on the rows; nothing of size |theta| reaches the host.  L' = the layers of
        `grad_layers` (all when empty).  Also returns the posteriors [c, n] of these passes (device fp32).
        The A/B arm of the query since class_layer_sums_device (fisher_classes(..., fused=False), ALQ_FI_ROWS=1)."""
        torch = self.sess.torch
        t, n = self._as_device_batch(x)
        c, L = self.nclass, self.L
        elems = (C.c_int64 * L)(*[int(np.prod(w)) + int(np.prod(b)) for _, w, b in self.param_shapes])
        g = self.sess.empty((n, c, L), torch.float64)
        post = self.sess.empty((c, n), torch.float32)
        tmp = self.sess.empty((min(n, self.max_batch), L), torch.float64)
        flat = t.reshape(n, -1)
        for a in range(0, n, self.max_batch):
            b = min(n, a + self.max_batch)
            for j in range(c):
                rows, pb, _ = self.param_grads_device(flat[a:b], b - a, 0, cls=j, want_post=(j == 0))
                if j == 0:
                    post[:, a:b] = pb
                check(self.lib.alq_shrink_sum(self.sess.ctx, C.c_void_p(rows.data_ptr()), b - a, self.num_params, elems, L,
                                              C.c_void_p(tmp.data_ptr())))
                g[a:b, j, :] = tmp[:b - a]
        idx = list(self.grad_layer_idx)
        if idx != list(range(L)):
            g = g[:, :, idx].contiguous()
        return g, post

    def class_layer_sums_device(self, t, n, classes):
        """alq_class_layer_sums over device passes of max_batch samples: g [n, J, L'] float64 on the device, g[i, j] =
        shrink_gradient(d log posteriors[classes[i, j], i] / d theta, 'sum') over the layers of `grad_layers` (all when
        empty), like shrunk_class_gradients but for the class slots given per sample and with nothing of the size of theta
        formed: per pass one forward pass, one field launch per layer, then per slot a backward-data sweep with the fused
        mask + channel-sum + dot kernels (csrc/lsum.hip).  classes: int array [n, J], entries in [0, c); the slots of a pass
        are uploaded with it.  Rows do not depend on the pass cut."""
        torch = self.sess.torch
        self.sess.bind_stream()
        classes = np.asarray(classes)
        if classes.ndim != 2 or classes.shape[0] != n or not 1 <= classes.shape[1] <= 64:
            raise ValueError('classes must be [n = %d, J] with 1 <= J <= 64, got %r' % (n, classes.shape))
        J, L = int(classes.shape[1]), self.L
        g = self.sess.empty((n, J, L), torch.float64)
        flat = t.reshape(n, -1)
        for a in range(0, n, self.max_batch):
            b = min(n, a + self.max_batch)
            dc = self.sess.to_device(np.ascontiguousarray(classes[a:b].T, dtype=np.int32), torch.int32)      # [J][b - a]
            check(self.lib.alq_class_layer_sums(self._m, C.c_void_p(flat[a:b].data_ptr()), b - a, J, C.c_void_p(dc.data_ptr()), None,
                                                C.c_void_p(g.data_ptr() + a * J * L * 8)))
        idx = list(self.grad_layer_idx)
        if idx != list(range(L)):
            g = g[:, :, idx].contiguous()
        return g

    @staticmethod
    def class_slots(W):
        """The slot form of per-sample class weights W [n, c] (0 = class not kept): (classes [n, J] int, weights [n, J]) with
        J the largest kept-class count over the samples; slot j of sample i is its j-th kept class in ascending class order,
        spare slots repeat class 0 with weight 0.  sum_j weights[i, j] g(classes[i, j]) g(..)^T = sum_c W[i, c] g(c) g(c)^T."""
        W = np.asarray(W, dtype=np.float64)
        n = W.shape[0]
        kept = [np.flatnonzero(W[i] != 0.) for i in range(n)]
        J = max(1, max(len(k) for k in kept)) if n else 1
        classes = np.zeros((n, J), dtype=np.int64)
        weights = np.zeros((n, J))
        for i, k in enumerate(kept):
            classes[i, :len(k)] = k
            weights[i, :len(k)] = W[i, k]
        return classes, weights

    def fisher_classes(self, x, W, diag, fused=None):
        """A [n, L', L'] float64 = sum_j W[i, j] g_ij g_ij^T + diag[i] I (alq_fisher_classes).  fused (default; None = on unless
        ALQ_FI_ROWS=1): only the classes with a non-zero weight are differentiated, as class slots (class_slots) through
        class_layer_sums_device, and alq_fisher_classes runs over the J slots.  Otherwise the gradients of all c classes come
        from shrunk_class_gradients (alq_param_grads rows + alq_shrink_sum per class): the A/B arm."""
        torch = self.sess.torch
        if fused is None:
            fused = os.environ.get('ALQ_FI_ROWS', '0') in ('', '0')
        if fused:
            t, n = self._as_device_batch(x)
            classes, W = self.class_slots(np.asarray(W, dtype=np.float64).reshape(n, self.nclass))
            g = self.class_layer_sums_device(t, n, classes)
        else:
            g, _ = self.shrunk_class_gradients(x)
        n, c, L = [int(v) for v in g.shape]
        Wd = self.sess.to_device(np.asarray(W, dtype=np.float64).reshape(n, c), torch.float64)
        dd = self.sess.to_device(np.asarray(diag, dtype=np.float64).reshape(n), torch.float64)
        A = self.sess.empty((n, L, L), torch.float64)
        self.sess.bind_stream()
        check(self.lib.alq_fisher_classes(self.sess.ctx, C.c_void_p(g.data_ptr()), C.c_void_p(Wd.data_ptr()), C.c_void_p(dd.data_ptr()),
                                          n, c, L, C.c_void_p(A.data_ptr())))
        return A.cpu().numpy()

    def debug_tensor(self, layer_idx, what, n):
        """Test hook (alq_model_debug_copy): internal tensor of the last forward/fisher call."""
        torch = self.sess.torch
        cap = {0: None, 1: None}
        e = C.c_int64()
        # size query by over-allocation: the largest activation of a patch is bounded by 64x input
        buf = self.sess.empty((n * max(self.elems_per_patch * 64, 1 << 16),), torch.float32)
        check(self.lib.alq_model_debug_copy(self._m, int(layer_idx), int(what), int(n),
                                            C.c_void_p(buf.data_ptr()), C.byref(e)))
        del cap
        return buf[:e.value].cpu().numpy()

    def close(self):
        for ln in getattr(self, '_xlanes', []):
            self.lib.alq_model_destroy(ln['m'])
            ln['sess'].close()
        self._xlanes = []
        if getattr(self, 'teacher', None) is not None:
            self.teacher.close()
        if self._m:
            self.lib.alq_model_destroy(self._m)
            self._m = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass



def _fc_only(fn):
    """The method is defined for fc-head models: on a fully-convolutional one it raises before it touches the device."""
    @functools.wraps(fn)
    def guarded(self, *args, **kwargs):
        if getattr(self, 'dense', False):
            raise NotImplementedError('%s: not defined for a fully-convolutional model (1x1 conv head)' % fn.__name__)
        return fn(self, *args, **kwargs)
    return guarded


for _name in ('get_gradients', 'grad_log_post', 'param_grads_device', 'grad_sqnorms_device', 'hess_vecp_device', 'hess_vecp',
              'fisher_device', 'fisher', 'shrunk_class_gradients', 'class_layer_sums_device', 'fisher_classes',
              'diagonal_fisher_device', 'diagonal_fisher', 'diagonal_fisher_rows_device', 'llfc_reference_order', 'llfc_grads_device',
              'llfc_hess_device', 'llfc_stoch_if_features_device', 'llfc_stoch_if_device'):
    setattr(DeviceModel, _name, _fc_only(getattr(DeviceModel, _name)))
del _name
