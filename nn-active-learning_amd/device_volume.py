"""Session operations on whole volumes, a mixin of device.DeviceSession: connected components (csrc/ccl.hip), surface voxels,
distance transform and masked reductions (edt.hip), tiled inference (tile.hip), the dense CRF (dcrf.hip)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, check_tensor, ptr


class VolumeOps(object):
    def cc_sizes(self, labels):
        """alq_cc_sizes: `labels` int32 device tensor as cc_label returns it -> int32 device tensor of its shape, the size of the
        component at every root voxel (the smallest raveled index of the component), 0 elsewhere."""
        torch = self.torch
        self.bind_stream()
        check_tensor(labels, torch.int32, device=self.device)
        sizes = self.empty(tuple(labels.shape), torch.int32)
        check(self.lib.alq_cc_sizes(self._ctx, ptr(labels), int(labels.numel()), ptr(sizes)))
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
            check_tensor(t, torch.int32, n, self.device, optional=True)
        out = self.empty(tuple(labels.shape), torch.int32 if table is not None else torch.uint8)
        check(self.lib.alq_cc_relabel(self._ctx, ptr(labels), n, ptr(table), ptr(sizes), int(min_size),
                                      ptr(out) if table is not None else None, ptr(out) if table is None else None))
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
            check_tensor(t, torch.uint8, nvox, self.device, optional=True)
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
        check(self.lib.alq_cc_label(self._ctx, ptr(seg), dims, int(connectivity), 1 if select_zero else 0, ptr(labels)))
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
        check(self.lib.alq_cc_keep_largest(self._ctx, ptr(seg), dims, int(connectivity), 1 if skip_origin else 0, ptr(out), ptr(info), ptr(work)))
        return out, info.cpu().numpy()

    def fill_holes(self, seg, shape, out=None):
        """alq_fill_holes: (mask, info) - uint8 device mask = seg != 0 or inside a 6-connected background component that
        touches no face of the volume (scipy's binary_fill_holes); info = np.int64 [4] (enclosed components, voxels filled,
        0, 0), one copy of 32 bytes.  `out` may be `seg` itself."""
        shape, nvox, dims = self._cc_args(seg, shape, out)
        if out is None:
            out = self.empty(shape, self.torch.uint8)
        work, info = self._cc_work(dims)
        check(self.lib.alq_fill_holes(self._ctx, ptr(seg), dims, ptr(out), ptr(info), ptr(work)))
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
        check(self.lib.alq_surface_mask(self._ctx, ptr(seg), dims, -1 if label is None else int(label), ptr(out)))
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
        check_tensor(out, torch.float64, nvox, self.device)
        work = self.empty((max(int(self.lib.alq_edt_work_bytes(dims)), 8),), torch.uint8)
        check(self.lib.alq_edt_sq(self._ctx, ptr(feat), dims, s2, ptr(out), ptr(work)))
        return out

    def _masked_args(self, d2, mask):
        torch = self.torch
        self.bind_stream()
        n = int(d2.numel())
        check_tensor(d2, torch.float64, device=self.device)
        check_tensor(mask, torch.uint8, n, self.device)
        if n >= 2 ** 31:
            raise ValueError('2^31 elements or more')
        return n, self.empty((int(self.lib.alq_masked_work_bytes(n)),), torch.uint8)

    def masked_dist_stats(self, d2, mask):
        """alq_masked_dist_stats: np.float64 [4] = (count, sum of sqrt(d2), max of d2, min of d2) over the elements of the float64
        device tensor `d2` whose byte of the uint8 device tensor `mask` is non-zero (empty: 0, 0, -inf, +inf); one copy of 32
        bytes.  The same bits on every run."""
        n, work = self._masked_args(d2, mask)
        out = self.empty((4,), self.torch.float64)
        check(self.lib.alq_masked_dist_stats(self._ctx, ptr(d2), ptr(mask), n, ptr(out), ptr(work)))
        return out.cpu().numpy()

    def masked_select(self, d2, mask, ranks):
        """alq_masked_select: np.float64 [len(ranks)] (at most 8) = the ranks[r]-th smallest (0-based) of the masked entries of
        `d2` (non-negative or +inf), NaN for a rank at or above the masked count; one copy of 8 bytes per rank."""
        n, work = self._masked_args(d2, mask)
        ranks = [int(r) for r in ranks]
        out = self.empty((len(ranks),), self.torch.float64)
        check(self.lib.alq_masked_select(self._ctx, ptr(d2), ptr(mask), n, (C.c_int64 * max(len(ranks), 1))(*ranks), len(ranks), ptr(out), ptr(work)))
        return out.cpu().numpy()

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
        check_tensor(vol, torch.float32, device=self.device)
        assert tuple(int(v) for v in vol.shape[:3]) == tuple(lat.dims)
        shape = (max(int(n), 0),) + tuple(lat.tile) + (m,)
        if out is None:
            out = self.empty(shape, torch.float32)
        check_tensor(out, torch.float32, device=self.device)
        assert tuple(out.shape) == shape
        check(self.lib.alq_tile_gather(self._ctx, ptr(vol), m, C.byref(lat), int(first), int(n), float(fill), ptr(out)))
        return out

    def tile_blend(self, post, lat, first, n, windows, acc):
        """alq_tile_blend: adds the posteriors `post` (float32 device [c, n V], class-major planes as the forward calls return them)
        of the tiles first .. first + n - 1, weighted by the float32 device window tables `windows` = (wz, wh, ww), into the
        float32 device accumulator `acc` [c + 1, Z, H, W] (zeroed by the caller before the first call)."""
        torch = self.torch
        self.bind_stream()
        c, V = int(acc.shape[0]) - 1, int(np.prod(tuple(lat.tile)))
        for t, numel in ((post, c * int(n) * V), (acc, (c + 1) * int(np.prod(tuple(lat.dims))))) + tuple(zip(windows, tuple(lat.tile))):
            check_tensor(t, torch.float32, numel, self.device)
        check(self.lib.alq_tile_blend(self._ctx, ptr(post), c, C.byref(lat), int(first), int(n), *[ptr(t) for t in windows], ptr(acc)))
        return acc

    def tile_finalize(self, acc, hwz=True, want_post=True, want_label=True, post=None, label=None):
        """alq_tile_finalize of the accumulator `acc` [c + 1, Z, H, W]: (posteriors float32 [c, H, W, Z] or None, labels uint8
        [H, W, Z] or None) with hwz, else [c, Z, H, W] / [Z, H, W]; written into `post` / `label` when given."""
        torch = self.torch
        self.bind_stream()
        c = int(acc.shape[0]) - 1
        Z, H, W = (int(v) for v in acc.shape[1:])
        check_tensor(acc, torch.float32, device=self.device)
        shape = (H, W, Z) if hwz else (Z, H, W)
        if post is None and want_post:
            post = self.empty((c,) + shape, torch.float32)
        if label is None and want_label:
            label = self.empty(shape, torch.uint8)
        check_tensor(post, torch.float32, c * Z * H * W, self.device, optional=True)
        check_tensor(label, torch.uint8, Z * H * W, self.device, optional=True)
        check(self.lib.alq_tile_finalize(self._ctx, ptr(acc), c, (C.c_int32 * 3)(Z, H, W), 1 if hwz else 0, ptr(post), ptr(label)))
        return post, label

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
            check_tensor(t, torch.float32, n, self.device)
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
        check(self.lib.alq_dcrf2d(self._ctx, ptr(tens[0]), ptr(tens[1]), cdims, C.byref(cpar), ptr(q1), ptr(labels), ptr(work)))
        return (labels, q1) if want_q else labels
