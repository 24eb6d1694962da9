"""SLIC super-pixel over-segmentation: the NumPy statement of csrc/slic.hip.  Host code: the reference of the kernel tests and of
tools/gpu_slic.py, and what regions.oversegment runs without a session.

NOT skimage.  The reference makes its over-segmentation with skimage.segmentation.slic (PW_AL.py:2), which this project can
neither import nor match bit for bit; there is no reference counterpart here, this module DEFINES the algorithm and the device
equals it byte for byte whatever order its workgroups run in.  It is a SLIC in the gSLIC form, per axial slice, 2-D, m modalities:

  quantise   per channel q = clamp(rint((double(v) - lo_c) * scale_c), 0, 65535), v the float32 a resident volume holds, every
             operation rounded on its own.  A pixel with a non-finite value in any channel, or outside the mask, is OUT: label 0,
             never assigned, never counted.  From here on every cluster sum is a 64-bit INTEGER sum: any order gives the same
             centres.
  grid       gh x gw cells; cluster k = i gw + j starts at pixel (((2i+1) H) // (2 gh), ((2j+1) W) // (2 gw)) with its q (zeros if
             that pixel is out); home cell of (y, x) = (y gh // H, x gw // W); the candidates of a pixel are the clusters of the up
             to nine cells around its home cell, for the whole run.
  iterate    T times: assign every in pixel, then update every centre.  d = sum_c (q_c - mu_c)^2 + w ((y - cy)^2 + (x - cx)^2) in
             fp64, channels ascending, the spatial term last, every product and sum rounded on its own; the smallest d among the
             candidates in ascending k with a strict <.  mu_c = double(sum q_c) / double(n), likewise cy, cx; n = 0 keeps the
             centre.  T = 0: every in pixel belongs to its home cell.
  connect    1. 4-connected components of equal cluster label among the in pixels; root = smallest raveled pixel index.
             2. per cluster its largest component (ties: lowest root) is KEPT if its size >= min_size (0: no threshold); every
                other component is an ORPHAN.
             3. adoption rounds until nothing changes: an orphan that is 4-adjacent to a pixel of a kept region joins the region
                of the lowest-indexed such pixel; all orphans of a round decide on the regions as they stood when it began.
             3b. orphans that no round adopted - walled in by out pixels, or in a slice without any kept region - merge with the
                unadopted orphans they touch:
                every 4-connected set of unadopted orphan pixels is one region.  Without it two such orphans could touch and both
                be smaller than min_size, which property (d) forbids.
             4. regions of a slice are numbered 1 .. n_z by their first pixel in raster order.

Properties (tests/test_slic_host.py): (a) a pure function of its inputs; (b) every label of a slice is one 4-connected set of in
pixels; (c) labels are exactly 1 .. n_z by first pixel, 0 exactly on out pixels; (d) with min_size > 0 no region that touches
another region is smaller than min_size; (e) a constant image, T >= 1, w > 0, no mask, min_size = 0 gives the home cells, n_z =
gh gw - PROVIDED no pixel is equidistant from its own cell's start pixel and a lower-indexed neighbour's.  That holds e.g. for
9 x 11 / 2 x 3 and 20 x 28 / 3 x 4; it fails where a cell has an even number of rows or columns that 2 gh (2 gw) divides, e.g.
H = 4, gh = 2: start rows 1 and 3, and row 2 (home cell 1) ties between them and goes to cluster 0 for good.  The start pixels
and the tie rule are kept simple rather than bent around that case; it is stated here and pinned by a test.

grid_for / spatial_weight derive gh, gw and w from skimage-style arguments; that derivation is only skimage-LIKE (see there)."""
import numpy as np

QMAX = 65535
_BIG = np.iinfo(np.int64).max


def grid_for(H, W, n_segments):
    """(gh, gw) for about n_segments cells per slice: square cells of side step = sqrt(H W / n_segments), gh = rint(H / step),
    gw = rint(W / step), each clamped to [1, axis].  skimage-like only: skimage places its seeds on a grid of that step too, but
    rounds differently and lets clusters move without bound."""
    H, W, n_segments = int(H), int(W), int(n_segments)
    if H < 1 or W < 1 or n_segments < 1:
        raise ValueError('grid_for: H, W, n_segments >= 1')
    step = np.sqrt(H * W / float(n_segments))
    gh = int(min(max(np.rint(H / step), 1), H))
    gw = int(min(max(np.rint(W / step), 1), W))
    return gh, gw


def spatial_weight(compactness, H, W, gh, gw):
    """w of the distance d = |q - mu|^2 + w |p - c|^2.  skimage's slic compares |I - mu|^2 / compactness^2 + |p - c|^2 / step^2 on
    an image scaled to [0, 1]; times compactness^2, with I = q / 65535 and step^2 = (H / gh) (W / gw), the area of a cell:
    w = (compactness * 65535)^2 / ((H / gh) (W / gw)).  skimage-like only (its step is one number for a square grid)."""
    c = float(compactness)
    if not np.isfinite(c) or c < 0:
        raise ValueError('spatial_weight: compactness must be finite and >= 0')
    return (c * QMAX) ** 2 / ((float(H) / gh) * (float(W) / gw))


def as_modalities(vol):
    """-> list of m float32 arrays [H, W, S] from one 3-D array, an array [m, H, W, S] or a list of 3-D arrays."""
    if isinstance(vol, (list, tuple)):
        arrs = [np.asarray(v) for v in vol]
    else:
        a = np.asarray(vol)
        arrs = [a] if a.ndim == 3 else [a[i] for i in range(a.shape[0])] if a.ndim == 4 else None
    if not arrs or any(a.ndim != 3 or a.shape != arrs[0].shape for a in arrs):
        raise ValueError('a volume [H, W, S], an array [m, H, W, S] or a list of m volumes of one shape expected')
    return [a.astype(np.float32) for a in arrs]


def quant_range(mods, mask=None):
    """(lo [m], scale [m]) from the subject's minimum and maximum over the finite in-mask values of every channel:
    scale = 65535 / (double(max) - double(min)), 0 where max = min or nothing is finite."""
    lo, scale = [], []
    for a in mods:
        ok = np.isfinite(a) if mask is None else (np.isfinite(a) & np.asarray(mask, dtype=bool))
        if not ok.any():
            lo.append(0.0)
            scale.append(0.0)
            continue
        mn, mx = float(a[ok].min()), float(a[ok].max())
        lo.append(mn)
        scale.append(QMAX / (mx - mn) if mx > mn else 0.0)
    return np.array(lo, dtype=np.float64), np.array(scale, dtype=np.float64)


def quantise(mods, lo, scale, mask=None):
    """-> (q int64 [H, W, S, m], inn bool [H, W, S])."""
    inn = np.ones(mods[0].shape, dtype=bool) if mask is None else np.asarray(mask, dtype=bool).copy()
    q = np.zeros(mods[0].shape + (len(mods),), dtype=np.int64)
    for c, a in enumerate(mods):
        fin = np.isfinite(a)
        inn &= fin
        v = np.where(fin, a, np.float32(0)).astype(np.float64)
        t = (v - float(lo[c])) * float(scale[c])
        q[..., c] = np.clip(np.rint(t), 0, QMAX).astype(np.int64)
    return q, inn


def start_centres(q, inn, gh, gw):
    """-> (mu [K, m], cy [K], cx [K]) float64 of one slice (q [H, W, m])."""
    H, W, m = q.shape
    iy = ((2 * np.arange(gh) + 1) * H) // (2 * gh)
    ix = ((2 * np.arange(gw) + 1) * W) // (2 * gw)
    mu = q[iy][:, ix].reshape(gh * gw, m).astype(np.float64)
    mu[~inn[iy][:, ix].reshape(-1)] = 0.0
    return mu, np.repeat(iy.astype(np.float64), gw), np.tile(ix.astype(np.float64), gh)


def assign_iterate(q, inn, gh, gw, w, T):
    """The T iterations on one slice: -> cluster index int64 [H, W] (meaningful on in pixels)."""
    H, W, m = q.shape
    K = gh * gw
    hy = (np.arange(H) * gh) // H
    hx = (np.arange(W) * gw) // W
    lab = (hy[:, None] * gw + hx[None, :]).astype(np.int64)
    mu, cy, cx = start_centres(q, inn, gh, gw)
    qd = q.astype(np.float64)
    Y = np.broadcast_to(np.arange(H, dtype=np.float64)[:, None], (H, W))
    X = np.broadcast_to(np.arange(W, dtype=np.float64)[None, :], (H, W))
    w = np.float64(w)
    for _ in range(int(T)):
        best = np.full((H, W), np.inf)
        for di in (-1, 0, 1):
            ci = hy + di
            for dj in (-1, 0, 1):
                cj = hx + dj
                valid = ((ci >= 0) & (ci < gh))[:, None] & ((cj >= 0) & (cj < gw))[None, :]
                k = np.clip(ci, 0, gh - 1)[:, None] * gw + np.clip(cj, 0, gw - 1)[None, :]
                t = qd[:, :, 0] - mu[k, 0]
                acc = t * t
                for c in range(1, m):
                    t = qd[:, :, c] - mu[k, c]
                    acc = acc + t * t
                dy = Y - cy[k]
                dx = X - cx[k]
                s = dy * dy + dx * dx
                d = acc + w * s
                upd = valid & (d < best)
                best = np.where(upd, d, best)
                lab = np.where(upd, k, lab)
        li = lab[inn]
        n = np.bincount(li, minlength=K)
        ys, xs = np.nonzero(inn)
        nz = n > 0
        nd = n[nz].astype(np.float64)
        # integer sums (each below 2^53, so bincount's float64 accumulation holds them exactly)
        cy[nz] = np.bincount(li, weights=ys, minlength=K).astype(np.int64)[nz].astype(np.float64) / nd
        cx[nz] = np.bincount(li, weights=xs, minlength=K).astype(np.int64)[nz].astype(np.float64) / nd
        for c in range(m):
            mu[nz, c] = np.bincount(li, weights=q[:, :, c][inn], minlength=K).astype(np.int64)[nz].astype(np.float64) / nd
    return lab


def _components(sel_h, sel_v, H, W):
    """root [H W] = the smallest raveled index of the component of every pixel, edges (y, x)-(y, x+1) where sel_h, (y, x)-(y+1, x)
    where sel_v."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    idx = np.arange(H * W).reshape(H, W)
    a = np.concatenate([idx[:, :-1][sel_h], idx[:-1, :][sel_v]])
    b = np.concatenate([idx[:, 1:][sel_h], idx[1:, :][sel_v]])
    g = coo_matrix((np.ones(len(a), dtype=np.int8), (a, b)), shape=(H * W, H * W))
    _, comp = connected_components(g, directed=False)
    _, first = np.unique(comp, return_index=True)
    return first[comp]


def _neighbour_pairs(H, W):
    """(p, n) raveled index pairs of every pixel p and each of its up to four neighbours n."""
    idx = np.arange(H * W).reshape(H, W)
    ps = [idx[:, 1:], idx[:, :-1], idx[1:, :], idx[:-1, :]]
    ns = [idx[:, :-1], idx[:, 1:], idx[:-1, :], idx[1:, :]]
    return np.concatenate([p.reshape(-1) for p in ps]), np.concatenate([n.reshape(-1) for n in ns])


def enforce_connectivity(lab, inn, K, min_size=0, stats=None):
    """Steps 1 to 4 on one slice: cluster indices [H, W] + in mask -> (labels int32 [H, W], n_z).  `stats` (a dict) receives
    orphans (components that step 2 did not keep), rounds (adoption rounds that changed something) and unadopted (orphan
    components left to step 3b)."""
    H, W = lab.shape
    HW = H * W
    same_h = inn[:, :-1] & inn[:, 1:] & (lab[:, :-1] == lab[:, 1:])
    same_v = inn[:-1, :] & inn[1:, :] & (lab[:-1, :] == lab[1:, :])
    innf = inn.reshape(-1)
    reg = np.where(innf, _components(same_h, same_v, H, W), -1).astype(np.int64)
    roots = np.flatnonzero(reg == np.arange(HW))
    size = np.bincount(reg[innf], minlength=HW)
    cl = lab.reshape(-1)[roots]
    key = (size[roots].astype(np.int64) << 32) | (0xffffffff - roots)
    ckey = np.zeros(K, dtype=np.int64)
    np.maximum.at(ckey, cl, key)
    keep = (ckey[cl] == key) & (size[roots] >= int(min_size))
    kept = np.zeros(HW + 1, dtype=bool)          # kept[-1]: an out pixel is no kept region
    kept[roots[keep]] = True
    P, N = _neighbour_pairs(H, W)
    rounds = 0
    while True:
        orphan = (reg >= 0) & ~kept[reg]
        cond = orphan[P] & kept[reg[N]]
        best = np.full(HW, _BIG, dtype=np.int64)
        np.minimum.at(best, reg[P[cond]], N[cond])
        adopt = np.flatnonzero(orphan & (best[np.maximum(reg, 0)] != _BIG))
        if len(adopt) == 0:
            break
        reg[adopt] = reg[best[reg[adopt]]]
        rounds += 1
    orphan = ((reg >= 0) & ~kept[reg]).reshape(H, W)
    unadopted = len(np.unique(reg[orphan.reshape(-1)]))
    if unadopted:
        merged = _components(orphan[:, :-1] & orphan[:, 1:], orphan[:-1, :] & orphan[1:, :], H, W)
        reg = np.where(orphan.reshape(-1), merged, reg)
    if stats is not None:
        stats.update(orphans=int(len(roots) - keep.sum()), rounds=rounds, unadopted=int(unadopted))
    out = np.zeros(HW, dtype=np.int32)
    pos = np.flatnonzero(reg >= 0)
    if len(pos) == 0:
        return out.reshape(H, W), 0
    u, fi, inv = np.unique(reg[pos], return_index=True, return_inverse=True)
    num = np.empty(len(u), dtype=np.int32)
    num[np.argsort(pos[fi], kind='stable')] = np.arange(1, len(u) + 1, dtype=np.int32)
    out[pos] = num[inv.reshape(-1)]
    return out.reshape(H, W), int(len(u))


def slic_host(vol, gh, gw, w, T=10, min_size=0, mask=None, lo=None, scale=None, threads=1):
    """-> (labels int32 [H, W, S], n_per_slice int32 [S]).  vol: see as_modalities (values are taken as float32); mask: bool
    [H, W, S], True = in; lo / scale [m]: the quantisation (default: quant_range of the subject); threads: slices in flight."""
    mods = as_modalities(vol)
    H, W, S = mods[0].shape
    gh, gw, T, min_size = int(gh), int(gw), int(T), int(min_size)
    if not (1 <= gh <= H and 1 <= gw <= W):
        raise ValueError('slic: grid %d x %d outside [1, %d] x [1, %d]' % (gh, gw, H, W))
    if T < 0 or min_size < 0 or not np.isfinite(w) or w < 0:
        raise ValueError('slic: T >= 0, min_size >= 0, w finite and >= 0')
    if mask is not None and np.asarray(mask).shape != (H, W, S):
        raise ValueError('slic: mask shape %r, volume %r' % (np.asarray(mask).shape, (H, W, S)))
    if lo is None or scale is None:
        lo, scale = quant_range(mods, mask)
    q, inn = quantise(mods, lo, scale, mask)
    labels = np.zeros((H, W, S), dtype=np.int32)
    counts = np.zeros(S, dtype=np.int32)

    def one(z):
        qz, iz = np.ascontiguousarray(q[:, :, z, :]), np.ascontiguousarray(inn[:, :, z])
        lab = assign_iterate(qz, iz, gh, gw, w, T)
        labels[:, :, z], counts[z] = enforce_connectivity(lab, iz, gh * gw, min_size)

    if threads > 1 and S > 1:
        from concurrent.futures import ThreadPoolExecutor
        with ThreadPoolExecutor(int(threads)) as ex:
            list(ex.map(one, range(S)))
    else:
        for z in range(S):
            one(z)
    return labels, counts
