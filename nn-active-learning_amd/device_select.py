"""Session operations of selection and evaluation: top-k, committee scoring, confusion counts, uncertainty sums and slice
scores (csrc/topk.hip, committee.hip, evalcounts.hip, confusion.hip, sliceq.hip).  A mixin of device.DeviceSession."""
from ._lib import check, check_tensor, ptr


class SelectOps(object):
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
        check(self.lib.alq_topk_uncertain(self._ctx, ptr(keys), n, int(B), ptr(out), ptr(work)))
        return out

    def committee_update(self, p1, member, mode, mean_p, mean_h=None, keys=None):
        """alq_committee_update: member `member` (0-based, in order) of the ensemble (mode 0) or QBC-JS (mode 1) committee,
        p1 = its class-1 posteriors (float32 device [n]); updates the float64 device running means mean_p (and mean_h,
        QBC-JS) in place and, when `keys` is given, writes the float64 top-k keys for topk_smallest into it."""
        torch = self.torch
        self.bind_stream()
        n = int(p1.numel())
        for t, dt in ((p1, torch.float32), (mean_p, torch.float64), (mean_h, torch.float64), (keys, torch.float64)):
            check_tensor(t, dt, n, self.device, optional=True)
        check(self.lib.alq_committee_update(self._ctx, ptr(p1), n, int(member), int(mode), ptr(mean_p), ptr(mean_h), ptr(keys)))

    def eval_counts(self, pred, inds, mask, counts, seg=None):
        """alq_eval_counts: adds the confusion counts (P, N, TP, FP, TN, FN; get_preds_stats) of the predictions `pred` (int64
        device [n]) against the labels mask[inds] - `mask` the subject's un-padded mask volume on the device (float32 or
        float64, NaN = ignored), `inds` int64 device [n] raveled indices into it, or None when `mask` is the label vector
        itself - to the int64 device totals `counts` [6]; with `seg` (uint8 device, the mask's size) also seg[inds] = pred."""
        torch = self.torch
        self.bind_stream()
        n = int(pred.numel())
        check_tensor(mask, (torch.float32, torch.float64), device=self.device)
        check_tensor(counts, torch.int64, 6, self.device)
        for t in (pred, inds):
            check_tensor(t, torch.int64, n, self.device, optional=True)
        elems = int(mask.numel())
        assert inds is not None or elems >= n
        check_tensor(seg, torch.uint8, device=self.device, optional=True)
        assert seg is None or int(seg.numel()) >= (elems if inds is not None else n)
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
            check_tensor(t, tuple(types), n, self.device)
        C, groups = int(C), int(groups)
        inner = max(n, 1) if inner is None else int(inner)
        if counts is None:
            counts = torch.zeros((max(groups, 0), max(C, 0), max(C, 0)), dtype=torch.int64, device=self.device)
        check_tensor(counts, torch.int64, groups * C * C, self.device)
        skipped = torch.zeros((1,), dtype=torch.int64, device=self.device) if want_skipped else None
        check(self.lib.alq_confusion_counts(self._ctx, ptr(pred), types[pred.dtype], ptr(labels), types[labels.dtype], n, int(first),
                                            inner, groups, C, int(fill), ptr(counts), ptr(skipped)))
        return (counts, skipped) if want_skipped else counts

    def unc_accumulate(self, post, sum_p, sum_h=None, first=False):
        """alq_unc_accumulate: one dropout pass `post` (float32 device [c, R], as the forward calls return it) into the float64
        device sums sum_p [c, R] (+= p) and sum_h [R] (+= -sum_j p_j log p_j; None: not kept).  first: assign instead of add."""
        torch = self.torch
        self.bind_stream()
        c, R = (int(v) for v in post.shape)
        check_tensor(post, torch.float32, device=self.device)
        check_tensor(sum_p, torch.float64, c * R, self.device)
        check_tensor(sum_h, torch.float64, R, self.device, optional=True)
        check(self.lib.alq_unc_accumulate(self._ctx, ptr(post), c, R, 1 if first else 0, ptr(sum_p), ptr(sum_h)))

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
            check_tensor(t, dt, numel, self.device, optional=True)
        assert f32 is None or int(f32.numel()) in (R, c * R)
        check(self.lib.alq_slice_scores(self._ctx, int(kind), int(T), c, n_slices, V, ptr(sum_p), ptr(sum_h), ptr(f32), ptr(roi), ptr(scores),
                                        ptr(counts)))
        return scores, counts
