"""The 1x1 conv head of a fully-convolutional model (csrc/dense.hip) restated in NumPy fp64, and the inputs of its kernel-level
tests (tests/test_gpu_dense_head.py; checked without a GPU by tests/test_dense_head_host.py).

    z = b + x W   [R, c]        post = softmax(z) as class-major planes [c, R]        pred = the FIRST maximal class (tf.argmax)
    dX = delta W^T [R, Ci]      dW = x^T delta [Ci, c]      db = sum_r delta_r [c]     -> [dW, db] flat, as the device writes it

Everything is computed in fp64 from the fp32 (or integer) values handed in.  For integer inputs below 2^53 every figure but the
softmax is exact."""
import numpy as np

U24 = 2. ** -24          # half an ulp of fp32, relative: one rounding to nearest


def f64(a):
    return np.asarray(a, dtype=np.float64)


def logits(x, W, b):
    return f64(x) @ f64(W) + f64(b)[None, :]


def softmax_planes(z):
    """[R, c] logits -> [c, R] posteriors."""
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return np.ascontiguousarray((e / e.sum(axis=1, keepdims=True)).T)


def first_argmax(z):
    """The first maximal class of every row, spelt out: a later class wins only when it is strictly larger."""
    z = f64(z)
    best = np.zeros(z.shape[0], np.int64)
    top = z[:, 0].copy()
    for j in range(1, z.shape[1]):
        m = z[:, j] > top
        best[m] = j
        top[m] = z[m, j]
    return best


def forward(x, W, b):
    z = logits(x, W, b)
    return dict(z=z, post=softmax_planes(z), pred=first_argmax(z), spread=z.max(1) - z.min(1))


def backward(x, delta, W):
    x, delta, W = f64(x), f64(delta), f64(W)
    return dict(dX=delta @ W.T, dW=x.T @ delta, db=delta.sum(0))


def flat_grad(ref):
    return np.concatenate([ref['dW'].reshape(-1), ref['db']])


# ---- bounds (per element; derived from the arithmetic of the kernels, not from their output)
def post_rel_bound(c):
    """Relative bound on a posterior whose logits are exact: expf within 1 ulp (2 U24) on the numerator and on every term of the
    denominator, c - 1 additions and one division, one rounding each."""
    return (4 + c) * U24


def logit_bound(x, W, b):
    """A chain of Ci fused multiply-adds started at b: (Ci + 1) roundings of partial sums no larger than |b| + sum |x||W|."""
    Ci = np.asarray(x).shape[1]
    return (Ci + 1) * U24 * (np.abs(f64(b))[None, :] + np.abs(f64(x)) @ np.abs(f64(W)))


def grad_bounds(x, delta, W, ref):
    """dW / db: 64 rows of a lane summed in fp32 (a product and an addition each: 65 roundings bound the chain), folded in fp64, and
    one rounding of the total to fp32.  dX: c fused multiply-adds."""
    x, delta, W = np.abs(f64(x)), np.abs(f64(delta)), np.abs(f64(W))
    c = delta.shape[1]
    dW = 65 * U24 * (x.T @ delta) + U24 * np.abs(ref['dW'])
    db = 65 * U24 * delta.sum(0) + U24 * np.abs(ref['db'])
    return dict(dX=(c + 1) * U24 * (delta @ W.T), g=np.concatenate([dW.reshape(-1), db]))


# ---- inputs
def backward_ints(R, Ci, c, seed):
    """x in [-4, 4], delta in [-3, 3], W in [-4, 4], integers as float32."""
    rs = np.random.RandomState(seed)
    return (rs.randint(-4, 5, size=(R, Ci)).astype(np.float32), rs.randint(-3, 4, size=(R, c)).astype(np.float32),
            rs.randint(-4, 5, size=(Ci, c)).astype(np.float32))


def tie_bias(c):
    """b = [0, 1, 1, ...]: with x = 0 classes 1 and 2 tie (c > 2) and the first wins."""
    return np.asarray([0.] + [1.] * (c - 1), np.float32)


def forward_ints(R, Ci, c, seed, wide=False):
    """Integer x, W, b with exact logits, and rows of x = 0 (logits = b = [0, 1, 1, ...]: for c > 2 classes 1 and 2 tie, the
    first wins) at the start, the end and scattered in between.
    wide = False: every class reads at most 9 channels with weight +-1, |x| <= 4, so |z - b| <= 36 and the spread of a voxel's
    logits is at most 73 by construction: every posterior is a normal float.  wide = True: W in [-4, 4] everywhere."""
    rs = np.random.RandomState(seed)
    x = rs.randint(-4, 5, size=(R, Ci)).astype(np.float32)
    if wide:
        W = rs.randint(-4, 5, size=(Ci, c)).astype(np.float32)
    else:
        W = np.zeros((Ci, c), np.float32)
        for j in range(c):
            ch = rs.permutation(Ci)[:min(Ci, 9)]
            W[ch, j] = rs.choice([-1., 1.], size=len(ch))
    zero = np.unique(np.concatenate([[0, R - 1], rs.randint(0, R, size=max(1, R // 8))]))
    x[zero] = 0
    return x, W, tie_bias(c)


def tie_case(Ci, c, j, R=24):
    """Rows whose logits are exactly: b (x = 0); a tie of classes j and j + 1 above the rest (x = e_0); all classes equal
    (x = e_1); a strict maximum at the last class (x = e_2).  W and b are integers, so the device's chain of fused
    multiply-adds gives these logits exactly."""
    rs = np.random.RandomState(97 * Ci + 11 * c + j)
    b = rs.randint(-3, 4, size=c).astype(np.float32)
    W = rs.randint(-4, 5, size=(Ci, c)).astype(np.float32)
    pat = -np.abs(np.arange(c) - j).astype(np.float32)
    pat[j + 1] = pat[j]
    last = np.zeros(c, np.float32)
    last[c - 1] = 2
    W[0], W[1], W[2] = pat - b, 5 - b, last - b
    x = np.zeros((R, Ci), np.float32)
    kinds = np.arange(R) % 4          # 0: x = 0, k > 0: x = e_{k-1}
    for k in (1, 2, 3):
        x[kinds == k, k - 1] = 1
    want = np.empty(R, np.int64)
    want[kinds == 0] = first_argmax(b[None, :])[0]
    want[kinds == 1], want[kinds == 2], want[kinds == 3] = j, 0, c - 1
    return x, W, b, want


def triple_loop(x, delta, W, b):
    """The same statements as plain loops over rows, channels and classes (fp64 Python floats): the witness of this module."""
    R, Ci = x.shape
    c = W.shape[1]
    z = [[float(b[j]) for j in range(c)] for _ in range(R)]
    dX = [[0.] * Ci for _ in range(R)]
    dW = [[0.] * c for _ in range(Ci)]
    db = [0.] * c
    for r in range(R):
        for j in range(c):
            for i in range(Ci):
                z[r][j] += float(x[r, i]) * float(W[i, j])
                dX[r][i] += float(delta[r, j]) * float(W[i, j])
                dW[i][j] += float(x[r, i]) * float(delta[r, j])
            db[j] += float(delta[r, j])
    post = [[0.] * R for _ in range(c)]
    pred = [0] * R
    for r in range(R):
        mx = max(z[r])
        e = [np.exp(v - mx) for v in z[r]]
        for j in range(c):
            post[j][r] = e[j] / sum(e)
        for j in range(c):
            if z[r][j] == mx:
                pred[r] = j
                break
    return dict(z=np.asarray(z), post=np.asarray(post), pred=np.asarray(pred), dX=np.asarray(dX), dW=np.asarray(dW), db=np.asarray(db))
