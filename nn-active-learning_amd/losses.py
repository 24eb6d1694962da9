"""Plain NumPy fp64 restatement of the training objectives that csrc/loss.hip evaluates at the logits: per-sample losses,
cotangent rows and the three statistics of alq_loss_stats, from posteriors, labels and a loss description.  Host code: the
reference of the kernel tests and the documentation of the formulas (include/alq.h, alq_loss_t)."""
import numpy as np

CE, CE_SOFT, GCE = 0, 1, 2
KINDS = {'CE': CE, 'CE_softclasses': CE_SOFT, 'GCE': GCE}


def _logp(p):
    """log p as the device takes it: log((double)max(p, 1e-38f))."""
    return np.log(np.maximum(p, p.dtype.type(1e-38)).astype(np.float64))


def evaluate(post, labels=None, kind=CE, class_w=None, sample_w=None, focal_gamma=None, targets=None, q=0.7, old_logits=None,
             T=1., loss_scale=1., lwf_scale=1.):
    """post [c, N], labels int [N] (outside [0, c): unlabelled), class_w [c], sample_w [N], targets / old_logits [c, N].
    float32 posteriors are taken as the values the head wrote and the device's fp32 steps are kept (1 - pt and the GCE clip
    bounds are formed in fp32); float64 posteriors are evaluated in fp64 throughout (the form checked against autograd).
    Returns dict(rows [N, c] float64 = loss_scale * d sum_n l_n / dz + lwf_scale * d sum_n l'_n / dz, loss [N], weight [N],
    lwf [N], stats = (sum l, number of non-zero weights, sum l'))."""
    p32 = np.asarray(post)          # the posteriors in their own precision ("32": the device's case)
    if p32.dtype != np.float32:
        p32 = p32.astype(np.float64)
    one = p32.dtype.type
    c, N = p32.shape
    p = p32.astype(np.float64)
    lp = _logp(p32)
    rows = np.zeros((N, c))
    loss = np.zeros(N)
    w = np.ones(N)
    if kind == CE:
        y = np.asarray(labels).astype(np.int64).reshape(N)
        lab = (y >= 0) & (y < c)
        ys = np.where(lab, y, 0)
        cols = np.arange(N)
        pt32 = p32[ys, cols]
        pt, lpt = pt32.astype(np.float64), lp[ys, cols]
        base = lab.astype(np.float64)
        if class_w is not None:
            base = base * np.asarray(class_w, dtype=np.float64)[ys]
        if sample_w is not None:
            base = base * np.asarray(sample_w, dtype=np.float64).reshape(N)
        f, fac = np.ones(N), np.ones(N)
        if focal_gamma is not None and focal_gamma > 0:
            g = float(focal_gamma)
            om = (one(1.) - pt32).astype(np.float64)          # fp32 posteriors: 1 - pt in fp32, like tf.pow(1. - model.pt, gamma)
            sat = pt32 == one(1.)
            oms = np.where(sat, 1., om)
            f = np.where(sat, 0., oms ** g)
            fac = np.where(sat, 0., oms ** g - g * oms ** (g - 1.) * pt * lpt)
        w = base * f
        loss = -w * lpt
        onehot = np.zeros((N, c))
        onehot[cols, ys] = 1.
        rows = loss_scale * (base * fac)[:, None] * (p.T - onehot)
    elif kind == CE_SOFT:
        t = np.asarray(targets, dtype=np.float64)
        loss = -(t * lp).sum(0)
        rows = loss_scale * (p * t.sum(0, keepdims=True) - t).T
    elif kind == GCE:
        t = np.asarray(targets, dtype=np.float64)
        qq = float(q)
        if qq == 0:
            raise ValueError('q cannot be equal to zero.')
        lo, hi = one(1e-4), one(1.) - one(1e-4)
        pc = np.clip(p32, lo, hi).astype(np.float64)
        loss = (t * (1. - pc ** qq) / qq).sum(0) / c
        own = np.where((p32 >= lo) & (p32 <= hi), t * p ** qq, 0.)
        rows = (-(loss_scale / c) * (own - p * own.sum(0, keepdims=True))).T
    else:
        raise ValueError('loss kind %r' % (kind,))
    lwf = np.zeros(N)
    if old_logits is not None:
        TT = float(T)
        if TT <= 0:
            raise ValueError('LwF temperature %r' % (T,))
        a = lp / TT
        a = a - a.max(0, keepdims=True)
        lpi = a - np.log(np.exp(a).sum(0, keepdims=True))
        o = np.asarray(old_logits, dtype=np.float64) / TT
        o = o - o.max(0, keepdims=True)
        tau = np.exp(o - np.log(np.exp(o).sum(0, keepdims=True)))
        lwf = -(tau * lpi).sum(0)
        rows = rows + lwf_scale * ((np.exp(lpi) - tau) / TT).T
    count = float(np.count_nonzero(w)) if kind == CE else float(N)
    return dict(rows=rows, loss=loss, weight=w, lwf=lwf, stats=(float(loss.sum()), count, float(lwf.sum())))
