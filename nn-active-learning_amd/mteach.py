"""Plain NumPy restatement of what csrc/mteach.hip computes for mean-teacher consistency training (NN_extended.py:913-926,
:1337-1396, :1535-1560): the consistency value and its cotangent rows in fp64, the teacher's moving average in fp32, the
counter-based input noise and the nearest-neighbour rotation.  Host code: the reference of the kernel tests and the
documentation of the formulas (include/alq.h)."""
import numpy as np

from . import losses

L2, CE = 0, 1
MEASURES = {'L2': L2, 'CE': CE}


def cons_coeff(step, rampup_length, max_cons_coeff):
    """sigmoid_rampup(global_step, rampup_length) * max_cons_coeff (NN_extended.py:1372-1375), step = the count before the step."""
    from .NN_extended import sigmoid_rampup
    return sigmoid_rampup(step, rampup_length) * float(max_cons_coeff)


def consistency(post, tpost, measure, cons_scale=0.):
    """Student posteriors p and teacher posteriors q, [c, R]: (div [R], rows [R, c]) in fp64.
    L2: div = mean_j (p_j - q_j)^2, rows_k = cons_scale p_k (d_k - sum_j p_j d_j), d = p - q: the gradient of
    (cons_scale c / 2) sum_v div_v at the student's logits.  CE: div = -sum_j p_j log q_j (log as the device takes it) and no
    rows: TF does not differentiate the labels of softmax_cross_entropy_with_logits, and the teacher is a constant."""
    p, q = np.asarray(post), np.asarray(tpost)
    c = p.shape[0]
    p64 = p.astype(np.float64)
    if measure == L2:
        d = p64 - q.astype(np.float64)
        div = (d * d).sum(0) / c
        rows = (float(cons_scale) * p64 * (d - (p64 * d).sum(0, keepdims=True))).T
    elif measure == CE:
        div = -(p64 * losses._logp(q if q.dtype == np.float32 else q.astype(np.float64))).sum(0)
        rows = np.zeros(p.shape[::-1])
    else:
        raise ValueError('output-perturbation measure %r' % (measure,))
    return div, rows


def evaluate(post, tpost, labels, measure, loss_scale=1., cons_scale=0., class_w=None, sample_w=None, focal_gamma=None):
    """The rows [R, c] and statistics alq_mt_cotangent writes: losses.evaluate's weighted / focal cross-entropy rows at
    loss_scale plus the consistency rows at cons_scale.  dict(rows, labelled_rows, cons_rows, div [R], stats = (sum l, number of
    non-zero weights, sum div))."""
    lab = losses.evaluate(post, labels, losses.CE, class_w=class_w, sample_w=sample_w, focal_gamma=focal_gamma, loss_scale=loss_scale)
    div, crow = consistency(post, tpost, measure, cons_scale)
    return dict(rows=lab['rows'] + crow, labelled_rows=lab['rows'], cons_rows=crow, div=div,
                stats=(lab['stats'][0], lab['stats'][1], float(div.sum())))


def consistency_au(post, tpost, au, measure, cons_scale=0., au_scale=0., kappa=0.1):
    """The consistency term of a head with an aleatoric-uncertainty channel (AU_4U, NN_extended.py:265-288, :1551-1554): au [R]
    is the student's log-variance a = relu(z_c) >= 0 and, with e = exp(-a), a voxel's value is cons = div e + kappa a / 2.
    (div [R], cons [R], rows [R, c + 1]) in fp64: columns k < c are consistency's rows times e (CE: zero), column c is
    au_scale (kappa / 2 - div e) where a > 0 and 0 elsewhere (TF's ReluGrad is g * (x > 0))."""
    a = np.asarray(au)
    a64 = a.astype(np.float64)
    e = np.exp(-a64)
    div, _ = consistency(post, tpost, measure)
    kap = float(np.float32(kappa))
    p64 = np.asarray(post).astype(np.float64)
    rows = np.zeros((a.shape[0], p64.shape[0] + 1))
    if measure == L2:          # the order of the products is the device's: ((cons_scale e) p_k) (d_k - sum_j p_j d_j)
        d = p64 - np.asarray(tpost).astype(np.float64)
        rows[:, :-1] = (float(cons_scale) * e * p64 * (d - (p64 * d).sum(0, keepdims=True))).T
    rows[:, -1] = np.where(a > 0, float(au_scale) * (0.5 * kap - div * e), 0.)
    return div, div * e + (0.5 * kap) * a64, rows


def evaluate_au(post, tpost, au, labels, measure, loss_scale=1., cons_scale=0., au_scale=0., kappa=0.1, class_w=None, sample_w=None,
                focal_gamma=None):
    """The rows [R, c + 1] and statistics alq_mt_cotangent_au writes: the labelled rows of `evaluate` on the c clean logits (the
    log-variance column gets none) plus consistency_au's.  dict(rows, labelled_rows, cons_rows, div [R], cons [R], stats = (sum l,
    number of non-zero weights, sum cons))."""
    lab = losses.evaluate(post, labels, losses.CE, class_w=class_w, sample_w=sample_w, focal_gamma=focal_gamma, loss_scale=loss_scale)
    div, cons, crow = consistency_au(post, tpost, au, measure, cons_scale, au_scale, kappa)
    lrow = np.concatenate([lab['rows'], np.zeros((crow.shape[0], 1))], axis=1)
    return dict(rows=lrow + crow, labelled_rows=lrow, cons_rows=crow, div=div, cons=cons,
                stats=(lab['stats'][0], lab['stats'][1], float(cons.sum())))


def ema_step(shadow, theta, decay):
    """tf.train.ExponentialMovingAverage's update in fp32, every operation rounded: shadow - (shadow - theta) * (1 - decay)."""
    s, t = np.asarray(shadow, dtype=np.float32), np.asarray(theta, dtype=np.float32)
    omd = np.float32(1.) - np.float32(decay)
    return (s - ((s - t) * omd).astype(np.float32)).astype(np.float32)


# ---- the teacher's input (perturb_input, NN_extended.py:1337-1351) -------------------------------
_M64 = (1 << 64) - 1
NOISE_TAG = 0xFF << 56          # the dropout masks carry their layer index (< 64) there


def _splitmix64(x):
    with np.errstate(over='ignore'):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def noise_uniforms(seed, sample_ids, per):
    """The two 24-bit uniforms of every element: u1 in (0, 1], u2 in [0, 1), float32 [len(sample_ids), per], from the generator
    of the dropout masks keyed (seed, NOISE_TAG, sample id, element in memory order)."""
    keys = np.array([(int(seed) ^ ((int(i) * 0xD1B54A32D192ED03) & _M64) ^ NOISE_TAG) & _M64 for i in sample_ids], dtype=np.uint64)
    with np.errstate(over='ignore'):
        h = _splitmix64(_splitmix64(keys)[:, None] + np.arange(per, dtype=np.uint64)[None, :])
    u1 = ((h >> np.uint64(40)).astype(np.float64) + 1.) / 16777216.
    u2 = ((h >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) / 16777216.
    return u1.astype(np.float32), u2.astype(np.float32)


def noise(seed, sample_ids, per):
    """Standard normal draws z [len(sample_ids), per] in fp64: Box-Muller on noise_uniforms."""
    u1, u2 = noise_uniforms(seed, sample_ids, per)
    return np.sqrt(-2. * np.log(u1.astype(np.float64))) * np.cos(2. * np.pi * u2.astype(np.float64))


def rotation_sources(H, W, angle):
    """tf.contrib.image.rotate's NEAREST transform in fp32: (ys, xs) float32 [H, W], the source coordinates of every output
    pixel BEFORE rounding.  (TF 1.x's angles_to_projective_transforms, restated: not checked against TensorFlow.)"""
    f = np.float32
    ca, sa = np.cos(f(angle)).astype(f), np.sin(f(angle)).astype(f)
    w1, h1 = f(W - 1), f(H - 1)
    xo = (w1 - (ca * w1 - sa * h1)) / f(2)
    yo = (h1 - (sa * w1 + ca * h1)) / f(2)
    y, x = np.meshgrid(np.arange(H, dtype=f), np.arange(W, dtype=f), indexing='ij')
    return (sa * x + ca * y) + yo, (ca * x - sa * y) + xo


def _round_half_away(v):
    r = np.trunc(v)
    return r + np.where(np.abs(v - r) >= 0.5, np.sign(v), 0.).astype(v.dtype)


def rotation_indices(H, W, angle):
    """(iy, ix, inside): integer source indices [H, W] (0 where outside) and the mask of output pixels whose source is in the image."""
    ys, xs = rotation_sources(H, W, angle)
    ry, rx = _round_half_away(ys), _round_half_away(xs)
    inside = (ry >= 0) & (ry <= H - 1) & (rx >= 0) & (rx <= W - 1)
    return np.where(inside, ry, 0).astype(np.int64), np.where(inside, rx, 0).astype(np.int64), inside


def perturb(x, noise_std=0., seed=0, first_sample=0, angle=None):
    """alq_perturb_input on x [N, H, W, C] (a 3-D batch [N, D, H, W, C] with angle None): noise first, rotation after, as one
    gather; (out float64, the part of it that is noise).  The device forms x + noise_std * z in fp32."""
    x = np.asarray(x)
    N = x.shape[0]
    per = int(np.prod(x.shape[1:]))
    eps = np.zeros((N, per))
    if noise_std:
        eps = float(np.float32(noise_std)) * noise(seed, int(first_sample) + np.arange(N), per)
    eps = eps.reshape(x.shape)
    out = x.astype(np.float64) + eps
    if angle is None:
        return out, eps
    if x.ndim != 4:
        raise ValueError('rotation applies to 2-D inputs [N, H, W, C]')
    iy, ix, inside = rotation_indices(x.shape[1], x.shape[2], angle)
    m = inside[None, :, :, None]
    return np.where(m, out[:, iy, ix, :], 0.), np.where(m, eps[:, iy, ix, :], 0.)
