"""Shared by tests/test_slic_host.py and tests/test_gpu_slic.py: a plain-loop restatement of nnal_amd/slic.py (pure Python, one
pixel and one candidate at a time, breadth-first components) and the small subjects both files run.  No GPU, no test in here."""
import numpy as np


# ---------------------------------------------------------------------------------------------------- the plain-loop restatement
def naive_slice(q, inn, gh, gw, w, T, min_size):
    """One slice: q int [H, W, m], inn bool [H, W] -> (labels [H, W], n)."""
    H, W, m = q.shape
    K = gh * gw
    w = float(w)
    mu = [[0.0] * m for _ in range(K)]
    cy, cx = [0.0] * K, [0.0] * K
    for i in range(gh):
        for j in range(gw):
            y, x = ((2 * i + 1) * H) // (2 * gh), ((2 * j + 1) * W) // (2 * gw)
            k = i * gw + j
            cy[k], cx[k] = float(y), float(x)
            if inn[y, x]:
                mu[k] = [float(q[y, x, c]) for c in range(m)]
    lab = [[(y * gh // H) * gw + (x * gw // W) for x in range(W)] for y in range(H)]
    for _ in range(T):
        for y in range(H):
            for x in range(W):
                if not inn[y, x]:
                    continue
                hi, hj = y * gh // H, x * gw // W
                best = float('inf')
                for di in (-1, 0, 1):
                    for dj in (-1, 0, 1):
                        ci, cj = hi + di, hj + dj
                        if ci < 0 or ci >= gh or cj < 0 or cj >= gw:
                            continue
                        k = ci * gw + cj
                        acc = None
                        for c in range(m):
                            t = float(q[y, x, c]) - mu[k][c]
                            acc = t * t if acc is None else acc + t * t
                        dy, dx = float(y) - cy[k], float(x) - cx[k]
                        s = dy * dy + dx * dx
                        d = acc + w * s
                        if d < best:
                            best, lab[y][x] = d, k
        n, sy, sx = [0] * K, [0] * K, [0] * K
        sq = [[0] * m for _ in range(K)]
        for y in range(H):
            for x in range(W):
                if inn[y, x]:
                    k = lab[y][x]
                    n[k] += 1
                    sy[k] += y
                    sx[k] += x
                    for c in range(m):
                        sq[k][c] += int(q[y, x, c])
        for k in range(K):
            if n[k]:
                cy[k], cx[k] = float(sy[k]) / float(n[k]), float(sx[k]) / float(n[k])
                mu[k] = [float(sq[k][c]) / float(n[k]) for c in range(m)]

    def nbrs(y, x):
        for yy, xx in ((y - 1, x), (y, x - 1), (y, x + 1), (y + 1, x)):
            if 0 <= yy < H and 0 <= xx < W:
                yield yy, xx

    def flood(seed, member, mark, tag):
        todo, cells = [seed], [seed]
        mark[seed] = tag
        while todo:
            y, x = todo.pop()
            for p in nbrs(y, x):
                if p not in mark and member(p, seed):
                    mark[p] = tag
                    todo.append(p)
                    cells.append(p)
        return cells

    # 1. components in raster order: the seed is the smallest raveled index of its component
    comp, members = {}, {}
    for y in range(H):
        for x in range(W):
            if inn[y, x] and (y, x) not in comp:
                members[(y, x)] = flood((y, x), lambda p, s: inn[p] and lab[p[0]][p[1]] == lab[s[0]][s[1]], comp, (y, x))
    # 2. kept components
    winner = {}
    for root, cells in members.items():
        k = lab[root[0]][root[1]]
        if k not in winner or (len(cells), -root[0] * W - root[1]) > (len(members[winner[k]]), -winner[k][0] * W - winner[k][1]):
            winner[k] = root
    kept = set(r for r in winner.values() if len(members[r]) >= min_size)
    region = dict(comp)          # pixel -> root of its region
    orphans = [r for r in members if r not in kept]
    # 3. adoption rounds
    while True:
        snapshot = dict(region)
        moved = []
        for r in orphans:
            offers = [p for c in members[r] for p in nbrs(*c) if inn[p] and snapshot[p] in kept]
            if offers:
                target = snapshot[min(offers, key=lambda p: p[0] * W + p[1])]
                for c in members[r]:
                    region[c] = target
                moved.append(r)
        if not moved:
            break
        orphans = [r for r in orphans if r not in moved]
    # 3b. unadopted orphans that touch merge
    left = set(c for r in orphans for c in members[r])
    merged = {}
    for y in range(H):
        for x in range(W):
            if (y, x) in left and (y, x) not in merged:
                flood((y, x), lambda p, s: p in left, merged, (y, x))
    region.update(merged)
    # 4. numbers by first pixel
    out = np.zeros((H, W), dtype=np.int32)
    number = {}
    for y in range(H):
        for x in range(W):
            if inn[y, x]:
                out[y, x] = number.setdefault(region[(y, x)], len(number) + 1)
    return out, len(number)


def naive_slic(vol, gh, gw, w, T=10, min_size=0, mask=None):
    from nnal_amd import slic
    mods = slic.as_modalities(vol)
    q, inn = slic.quantise(mods, *slic.quant_range(mods, mask), mask=mask)
    H, W, S = mods[0].shape
    labels, counts = np.zeros((H, W, S), dtype=np.int32), np.zeros(S, dtype=np.int32)
    for z in range(S):
        labels[:, :, z], counts[z] = naive_slice(q[:, :, z], inn[:, :, z], gh, gw, w, T, min_size)
    return labels, counts


# ---------------------------------------------------------------------------------------------------------------- the subjects
def _smooth(rs, shp, m=1, noise=0.3):
    """m modalities: a few plateaus of differing intensity plus noise (super-pixels then follow edges, and noise makes orphans)."""
    H, W, S = shp
    out = []
    for c in range(m):
        base = np.zeros(shp)
        for _ in range(4):
            y0, x0 = rs.randint(0, H), rs.randint(0, W)
            base[y0:y0 + rs.randint(3, H), x0:x0 + rs.randint(3, W)] += rs.rand() * 4
        out.append((base + noise * rs.randn(*shp)).astype(np.float32))
    return out


def checkerboard(shp=(16, 18, 2)):
    """Two intensities in 2 x 2 blocks: with a small w a cluster takes the blocks of one intensity around it, which touch only at
    corners - many 4-connected components per cluster, all but one of them orphans."""
    y, x = np.arange(shp[0])[:, None, None], np.arange(shp[1])[None, :, None]
    return [np.broadcast_to((((y // 2) + (x // 2)) % 2) * 100.0, shp).astype(np.float32)]


def walled_pocket(shp=(14, 16, 2)):
    """A ring of out pixels around a 2 x 2 pocket in the corner of a home cell: with T = 0 the pocket is a component of that
    cell's cluster, smaller than the rest of the cell, and touches nothing but the wall."""
    mask = np.ones(shp, dtype=bool)
    mask[1:5, 1:5] = False
    mask[2:4, 2:4] = True
    rs = np.random.RandomState(12)
    return [rs.rand(*shp).astype(np.float32)], mask


def cases():
    """name -> dict(vol, gh, gw, w, T, min_size, mask): the subjects of the byte-equality tests, each at the smallest shape that
    still takes the path its name says."""
    rs = np.random.RandomState(2024)
    odd = _smooth(rs, (20, 28, 3))                       # 20 x 28 with 3 x 4: neither axis a multiple of the grid or of the 16-pixel tile
    c = {}
    c['odd'] = dict(vol=odd, gh=3, gw=4, w=40.0, T=3, min_size=0, mask=None)
    c['T0'] = dict(c['odd'], T=0)
    c['T1'] = dict(c['odd'], T=1)
    c['min_size'] = dict(c['odd'], w=2.0, min_size=7)
    c['m3'] = dict(vol=_smooth(rs, (20, 28, 2), m=3), gh=3, gw=4, w=25.0, T=2, min_size=5, mask=None)
    c['one_cell'] = dict(vol=_smooth(rs, (12, 10, 2)), gh=1, gw=1, w=1.0, T=2, min_size=0, mask=None)
    c['pixel_cells'] = dict(vol=_smooth(rs, (6, 9, 2)), gh=6, gw=3, w=10.0, T=2, min_size=0, mask=None)
    c['one_slice'] = dict(vol=_smooth(rs, (17, 19, 1)), gh=4, gw=4, w=30.0, T=3, min_size=3, mask=None)
    c['tie'] = dict(vol=[np.full((9, 11, 2), 3.0, dtype=np.float32)], gh=2, gw=3, w=1.0, T=1, min_size=0, mask=None)
    m = np.ones((20, 28, 3), dtype=bool)
    m[:14, :14] = False                                   # the pixel window of cluster (0, 0): cells 0..1 x 0..1
    c['empty_cluster'] = dict(c['odd'], mask=m)
    holes = rs.rand(20, 28, 3) > 0.15
    bad = [v.copy() for v in odd]
    bad[0][3, 5, 0], bad[0][10, 20, 1], bad[0][19, 27, 2] = np.nan, np.inf, -np.inf
    c['mask_nan'] = dict(c['odd'], vol=bad, mask=holes, min_size=4)
    c['nan_only'] = dict(c['odd'], vol=bad)
    c['rounds'] = dict(vol=_smooth(rs, (32, 32, 2), noise=1.5), gh=4, gw=4, w=0.5, T=4, min_size=10, mask=None)
    c['checkerboard'] = dict(vol=checkerboard(), gh=2, gw=2, w=0.01, T=2, min_size=0, mask=None)
    pv, pm = walled_pocket()
    c['pocket'] = dict(vol=pv, gh=2, gw=2, w=1.0, T=0, min_size=0, mask=pm)
    c['all_small'] = dict(c['odd'], min_size=10000)      # no component is kept: everything merges in step 3b
    return c


def slice_stats(case, z=0):
    """(cluster labels after the iterations, in mask, stats of enforce_connectivity) of slice z of a case."""
    from nnal_amd import slic
    mods = slic.as_modalities(case['vol'])
    q, inn = slic.quantise(mods, *slic.quant_range(mods, case['mask']), mask=case['mask'])
    lab = slic.assign_iterate(q[:, :, z], inn[:, :, z], case['gh'], case['gw'], case['w'], case['T'])
    st = {}
    slic.enforce_connectivity(lab, inn[:, :, z], case['gh'] * case['gw'], case['min_size'], st)
    return lab, inn[:, :, z], st
