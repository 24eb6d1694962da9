"""The aleatoric-uncertainty head (AU_4U; csrc/dense.hip dense_head_fwd_au_kernel, csrc/mteach.hip mt_cotangent_au_kernel) restated
in NumPy fp64 for tests/test_aleatoric_host.py and tests/test_gpu_aleatoric.py, on top of tests/dense_head_ref.py.

    z = b + x W  [R, c + 1]     post = softmax(z[:, :c]) as planes [c, R]     pred = first maximum of z[:, :c]     au = max(z[:, c], 0)
    F(z) = s sum_v l_v + k sum_v (div_v exp(-a_v) + kappa a_v / 2),   a = relu(z[:, c]),  l and div on softmax(z[:, :c])

F is the scalar whose gradient at z the cotangent rows are when cons_scale = 2 k / c and au_scale = k (L2; under CE TF does not
differentiate the labels, so only the log-variance column is F's gradient)."""
import numpy as np

from tests import dense_head_ref as ref


def forward_au(x, W, b):
    """W [Ci, c + 1], b [c + 1]: dict(z [R, c + 1], post [c, R], pred [R], au [R])."""
    z = ref.logits(x, W, b)
    c = z.shape[1] - 1
    return dict(z=z, post=ref.softmax_planes(z[:, :c]), pred=ref.first_argmax(z[:, :c]), au=np.maximum(z[:, c], 0.))


def split(z):
    """Logits [R, c + 1] -> (posteriors [c, R], log-variances [R]) in fp64."""
    z = ref.f64(z)
    return ref.softmax_planes(z[:, :-1]), np.maximum(z[:, -1], 0.)


def objective(z, tpost, labels, measure, s, k, kappa):
    """F(z) above, through nnal_amd.mteach / nnal_amd.losses on fp64 posteriors (unweighted labelled term)."""
    from nnal_amd import losses, mteach
    post, a = split(z)
    lab = losses.evaluate(post, labels, losses.CE)
    div, _ = mteach.consistency(post, ref.f64(tpost), measure)
    return s * lab['stats'][0] + k * float((div * np.exp(-a) + 0.5 * kappa * a).sum())


def central_differences(z, h, tpost, labels, *args):
    """dF / dz [R, c + 1] by central differences of step h, one logit at a time (F is a sum over voxels: the difference is
    taken on the voxel's own term)."""
    z = ref.f64(z)
    g = np.zeros_like(z)
    for r in range(z.shape[0]):
        for j in range(z.shape[1]):
            zp, zm = z[r:r + 1].copy(), z[r:r + 1].copy()
            zp[0, j] += h
            zm[0, j] -= h
            own = (np.asarray(tpost)[:, r:r + 1], np.asarray(labels)[r:r + 1]) + args
            g[r, j] = (objective(zp, *own) - objective(zm, *own)) / (2 * h)
    return g


def draw_logits(R, c, seed0, margin=1e-3, tries=200):
    """The first seed >= seed0 whose unit-scale logits [R, c + 1] keep the raw log-variance channel `margin` away from the kink
    of the ReLU: (z, seed)."""
    for seed in range(seed0, seed0 + tries):
        z = np.random.RandomState(seed).randn(R, c + 1)
        if np.abs(z[:, c]).min() > margin:
            return z, seed
    raise AssertionError('no seed in [%d, %d) keeps |z_c| above %g' % (seed0, seed0 + tries, margin))
