"""Host restatement of the dense CRF of PW_analyze_results.DCRF_postprocess_2D (reference :539-591): 2 labels, a smoothness and
an appearance Gaussian kernel, NORMALIZE_SYMMETRIC, Potts compatibilities, mean-field inference, arg-max.  NumPy only; the
oracle of csrc/dcrf.hip (alq_dcrf2d) and of its tests.  The model, for one slice `img` [H, W] and class-1 posteriors `post`
[H, W], pixels raveled in C order:

  unary      post[post == 0] += 1e-10 (in place, on the caller's array); nl = -log(post); U = float32([1 - nl, nl]) - the
             reference's lines :549-553 as they stand: label 0 gets 1 + log p, not -log(1 - p)
  kernels    k(i, j) = exp(-|f_i - f_j|^2 / 2), the pixel itself included, with f = (row, column) / sdims for the smoothness
             kernel (create_pairwise_gaussian) and (row / sdims, column / sdims, img / schan) for the appearance kernel
             (create_pairwise_bilateral)
  norm       n_i = 1 / sqrt(sum_j k(i, j) + 1e-20) per kernel; (K~ Q)_i = n_i sum_j k(i, j) n_j Q_j
  inference  Q = softmax(-U), then niter times Q = softmax(-U + compat_smooth K~_smooth Q + compat_app K~_app Q)
  MAP        argmax over the two labels, a tie gives label 0

`window=None` forms the kernels over all pairs as dense matrices (slices of a few thousand pixels); `window='cutoff'` evaluates
them on |d row|, |d column| <= ceil(sdims sqrt(48 ln 2)) (6 and 29 for the reference's values), where the spatial weight
dropped is at most 2^-24 of the peak - the form the device computes - with the normalisation sums over the same window.
pydensecrf itself filters on a permutohedral lattice, an approximation of these sums: this file states the model, not the
library's approximation of it."""
import numpy as np

DEFAULTS = dict(sdims_smooth=(1., 1.), sdims_app=(5., 5.), schan=1., compat_smooth=20., compat_app=30.)
NITER = 5


def make_params(**kw):
    """The reference's parameter values with `kw` replacing some of them; a scalar sdims is taken for both axes."""
    p = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in p:
            raise KeyError('unknown dense-CRF parameter %r' % k)
        p[k] = v
    for k in ('sdims_smooth', 'sdims_app'):
        v = p[k]
        p[k] = (float(v), float(v)) if np.isscalar(v) else (float(v[0]), float(v[1]))
    return p


def window_radius(sd):
    """ceil(sd sqrt(2 * 24 ln 2)): beyond it exp(-d^2 / (2 sd^2)) < 2^-24."""
    return int(np.ceil(float(sd) * np.sqrt(48. * np.log(2.))))


def unary(post):
    """PW_analyze_results.py:549-553, literally: the zero guard in place on `post`, U float32 [2, H W]."""
    post[post == 0] += 1e-10
    nl = -np.log(post)
    U = np.float32(np.array([1 - nl, nl]))
    return U.reshape((2, -1))


def _softmax(E):
    """softmax over axis 0 of the negated energies E [2, n] (DenseCRF's expAndNormalize: the maximum is subtracted first)."""
    E = E - E.max(axis=0, keepdims=True)
    Q = np.exp(E)
    return Q / Q.sum(axis=0, keepdims=True)


def _dense_kernels(img, par, dtype):
    """The two all-pairs kernel matrices [n, n] in `dtype`."""
    H, W = img.shape
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing='ij')
    r = r.ravel().astype(dtype)
    c = c.ravel().astype(dtype)
    v = np.asarray(img, dtype=dtype).ravel()
    half = dtype(0.5)

    def sqd(f):
        return (f[:, None] - f[None, :]) ** 2

    ss, sa = par['sdims_smooth'], par['sdims_app']
    Ks = np.exp(-half * (sqd(r / dtype(ss[0])) + sqd(c / dtype(ss[1]))))
    D = sqd(r / dtype(sa[0]))
    D += sqd(c / dtype(sa[1]))
    D += sqd(v / dtype(par['schan']))
    Ka = np.exp(-half * D)
    return Ks, Ka


class _DenseFilter(object):
    """K~ of both kernels as matrices: apply(Q [2, n]) -> (K~_smooth Q, K~_app Q)."""

    def __init__(self, img, par, dtype):
        self.K = []
        for K in _dense_kernels(img, par, dtype):
            n = dtype(1.) / np.sqrt(K.sum(axis=1) + dtype(1e-20))
            self.K.append((K, n))

    def matrices(self):
        return [n[:, None] * K * n[None, :] for K, n in self.K]

    def apply(self, Q):
        return [n[None, :] * ((n[None, :] * Q) @ K.T) for K, n in self.K]


class _WindowFilter(object):
    """The same two filters on the cut-off windows, clipped to the slice, by shifted array sums (any slice size)."""

    def __init__(self, img, par, dtype):
        self.dtype = dtype
        self.shape = img.shape
        self.img = np.asarray(img, dtype=dtype)
        self.spec = []
        for sd, schan in ((par['sdims_smooth'], None), (par['sdims_app'], par['schan'])):
            R = (window_radius(sd[0]), window_radius(sd[1]))
            spec = dict(R=R, sd=(dtype(sd[0]), dtype(sd[1])), schan=None if schan is None else dtype(schan))
            ones = np.ones(self.shape, dtype=dtype)
            spec['n'] = dtype(1.) / np.sqrt(self._sum(spec, ones[None])[0] + dtype(1e-20))
            self.spec.append(spec)

    def _sum(self, spec, V):
        """out[l, i] = sum over the window of k(i, j) V[l, j]; V [L, H, W]."""
        H, W = self.shape
        Ry, Rx = spec['R']
        dtype = self.dtype
        half = dtype(0.5)
        Vp = np.zeros((V.shape[0], H + 2 * Ry, W + 2 * Rx), dtype=dtype)
        Vp[:, Ry:Ry + H, Rx:Rx + W] = V
        if spec['schan'] is not None:
            Ip = np.zeros((H + 2 * Ry, W + 2 * Rx), dtype=dtype)
            Ip[Ry:Ry + H, Rx:Rx + W] = self.img
            a = self.img / spec['schan']
        out = np.zeros(V.shape, dtype=dtype)
        for dy in range(-Ry, Ry + 1):
            for dx in range(-Rx, Rx + 1):
                d2 = (dtype(dy) / spec['sd'][0]) ** 2 + (dtype(dx) / spec['sd'][1]) ** 2
                if spec['schan'] is not None:
                    k = np.exp(-half * (d2 + (a - Ip[Ry + dy:Ry + dy + H, Rx + dx:Rx + dx + W] / spec['schan']) ** 2))
                else:
                    k = np.exp(-half * d2)
                out += k * Vp[:, Ry + dy:Ry + dy + H, Rx + dx:Rx + dx + W]
        return out

    def apply(self, Q):
        H, W = self.shape
        res = []
        for spec in self.spec:
            n = spec['n']
            res.append((n[None] * self._sum(spec, n[None] * Q.reshape(2, H, W))).reshape(2, -1))
        return res


def make_filter(img, dtype=np.float64, window=None, params=None):
    """The normalised filters of one image, reusable over calls with different posteriors or iteration counts."""
    dtype = np.dtype(dtype).type
    par = make_params(**(params or {}))
    img = np.asarray(img)
    if img.ndim != 2:
        raise ValueError('img must be [H, W]')
    if window is None:
        return _DenseFilter(img, par, dtype), par
    if window == 'cutoff':
        return _WindowFilter(img, par, dtype), par
    raise ValueError("window must be None (all pairs) or 'cutoff'")


def meanfield_host(post, img, dtype=np.float64, window=None, niter=NITER, params=None, _filter=None):
    """[Q_0, Q_1, ..., Q_niter]: the marginals [2, H W] in `dtype` before the first and after every mean-field iteration
    (niter + 1 arrays; Q_0 = softmax(-U)).  Mutates zeros of `post` to 1e-10 as the reference does.  `params`: a dict of
    DEFAULTS entries to replace.  `_filter`: make_filter(...)'s result for the same image, dtype, window and params."""
    flt, par = _filter if _filter is not None else make_filter(img, dtype, window, params)
    dtype = np.dtype(dtype).type
    if tuple(np.shape(post)) != tuple(np.shape(img)):
        raise ValueError('post %r and img %r differ in shape' % (np.shape(post), np.shape(img)))
    E = -unary(post).astype(dtype)
    ws, wa = dtype(par['compat_smooth']), dtype(par['compat_app'])
    Q = _softmax(E)
    out = [Q]
    for _ in range(int(niter)):
        Fs, Fa = flt.apply(Q)
        Q = _softmax(E + ws * Fs + wa * Fa)
        out.append(Q)
    return out


def map_host(post, img, dtype=np.float64, window=None, niter=NITER, params=None, _filter=None):
    """The MAP image [H, W] (int64): argmax over the labels of the last marginals, a tie giving label 0."""
    Q = meanfield_host(post, img, dtype, window, niter, params, _filter)[-1]
    return np.argmax(Q, axis=0).reshape(np.shape(img))
