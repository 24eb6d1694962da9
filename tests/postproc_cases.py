"""Inputs shared by tests/test_postproc_host.py and tests/test_gpu_postproc.py: the random volumes of the post-processing issue,
volumes built by hand together with the labels / masks they must give (written down from their construction, not computed by
the code under test), and a literal restatement of the reference's connected_component_analysis_3d on top of
regions.cc_label_host.  TEST INFRASTRUCTURE, no test in here."""
import functools
import itertools

import numpy as np

BOX = (21, 19, 70)          # 70 slices: more than one wave along z and a partial one
SMALL = (13, 11, 9)         # several rows per wave
FLAT = (17, 13, 1)          # a 2-D image
BIG = (128, 128, 64)
DENSITIES = (0.05, 0.12, 0.2, 0.35)
FILL_DENSITIES = (0.6, 0.75, 0.9)
CONNS = (6, 18, 26)
MAXNZ = {6: 1, 18: 2, 26: 3}


@functools.lru_cache(maxsize=None)
def random_volume(shape, d):
    """RandomState(1101 + int(100 d)), rand < d, voxel 0 cleared (read-only)."""
    seg = (np.random.RandomState(1101 + int(100 * d)).rand(*shape) < d).astype(np.uint8)
    seg.reshape(-1)[0] = 0
    seg.setflags(write=False)
    return seg


@functools.lru_cache(maxsize=None)
def fill_volume(shape, d):
    seg = (np.random.RandomState(1201 + int(100 * d)).rand(*shape) < d).astype(np.uint8)
    seg.setflags(write=False)
    return seg


@functools.lru_cache(maxsize=None)
def host_labels(shape, d, conn, select_zero):
    from nnal_amd import regions
    lab = regions.cc_label_host(random_volume(shape, d), conn, select_zero)
    lab.setflags(write=False)
    return lab


def serpentine(shape=BOX):
    """A one-voxel-wide path through the whole box: full z-runs in the rows (i, j) with i and j even, joined at alternating
    z ends by one voxel in the odd row between them, planes joined the same way.  -> the path as a list of (i, j, z), every
    step a face step, no two voxels further apart than one step on the path adjacent under any connectivity."""
    H, W, S = shape
    path = []
    up = True                       # direction of the next z-run
    fwd = True                      # direction of the next sweep over j
    for i in range(0, H, 2):
        js = list(range(0, W, 2))
        if not fwd:
            js.reverse()
        for n, j in enumerate(js):
            zs = range(S) if up else range(S - 1, -1, -1)
            path.extend((i, j, z) for z in zs)
            zend = S - 1 if up else 0
            up = not up
            if n + 1 < len(js):
                path.append((i, (j + js[n + 1]) // 2, zend))
            elif i + 2 < H:
                path.append((i + 1, j, zend))
        fwd = not fwd
    return path


def path_volume(shape, path):
    seg = np.zeros(shape, dtype=np.uint8)
    for p in path:
        seg[p] = 1
    return seg


def path_labels(shape, parts):
    """Expected labels of disjoint, mutually non-adjacent paths: the smallest raveled index of each."""
    lab = np.full(shape, -1, dtype=np.int32)
    for part in parts:
        idx = np.ravel_multi_index(tuple(np.array(part).T), shape)
        lab.reshape(-1)[idx] = idx.min()
    return lab


def built_label_cases():
    """[(name, seg, {connectivity: expected labels of the non-zero voxels})]."""
    cases = []
    path = serpentine()
    assert len(set(path)) == len(path)
    cases.append(('serpentine', path_volume(BOX, path), {c: path_labels(BOX, [path]) for c in CONNS}))
    cut = len(path) // 2
    while not (20 < path[cut][2] < 50):      # inside a z-run, far from the joints: its two path neighbours are not adjacent
        cut += 1
    parts = [path[:cut], path[cut + 1:]]
    cases.append(('serpentine cut', path_volume(BOX, parts[0] + parts[1]), {c: path_labels(BOX, parts) for c in CONNS}))
    # two voxels that touch across a face, an edge or a corner: one component exactly when the connectivity reaches that far
    for off in itertools.product((-1, 0, 1), repeat=3):
        nz = sum(1 for v in off if v)
        if nz == 0:
            continue
        a, b = (2, 2, 2), (2 + off[0], 2 + off[1], 2 + off[2])
        exp = {c: path_labels((5, 5, 5), [[a, b]] if nz <= MAXNZ[c] else [[a], [b]]) for c in CONNS}
        cases.append(('pair %r' % (off,), path_volume((5, 5, 5), [a, b]), exp))
    # neighbours in memory that are no neighbours in the volume: the end of a row and the start of the next one, the last
    # row of a plane and the first row of the next plane
    lone = [(1, 1, 5), (1, 2, 0), (0, 3, 2), (1, 0, 2), (2, 3, 5), (0, 0, 0)]
    cases.append(('row ends', path_volume((3, 4, 6), lone), {c: path_labels((3, 4, 6), [[p] for p in lone]) for c in CONNS}))
    # one z-run across lanes 63 / 64 of a wave, and one that ends on lane 63 next to one that starts on lane 64 of another row
    run = [(0, 0, z) for z in range(58, 71)]
    cases.append(('lane 63/64', path_volume((2, 2, 100), run), {c: path_labels((2, 2, 100), [run]) for c in CONNS}))
    r1, r2 = [(0, 0, z) for z in range(50, 64)], [(0, 1, z) for z in range(0, 9)]
    exp = {6: path_labels((2, 3, 64), [r1, r2]), 18: path_labels((2, 3, 64), [r1, r2]), 26: path_labels((2, 3, 64), [r1, r2])}
    cases.append(('row end on lane 63', path_volume((2, 3, 64), r1 + r2), exp))
    ones = np.ones(SMALL, dtype=np.uint8)
    cases.append(('all ones', ones, {c: np.zeros(SMALL, dtype=np.int32) for c in CONNS}))
    cases.append(('all zero', np.zeros(SMALL, dtype=np.uint8), {c: np.full(SMALL, -1, dtype=np.int32) for c in CONNS}))
    return cases


def _shell(shape=(9, 9, 9), lo=2, hi=6):
    seg = np.zeros(shape, dtype=np.uint8)
    seg[lo:hi + 1, lo:hi + 1, lo:hi + 1] = 1
    seg[lo + 1:hi, lo + 1:hi, lo + 1:hi] = 0
    return seg


def built_fill_cases():
    """[(name, seg, expected mask, expected info)]."""
    cases = []
    shell = _shell()
    solid = np.zeros_like(shell)
    solid[2:7, 2:7, 2:7] = 1
    cases.append(('closed shell', shell, solid, [1, 27, 0, 0]))
    tunnel = shell.copy()
    tunnel[2, 4, 4] = 0                                          # a face-connected way out of the cavity
    cases.append(('tunnel', tunnel, tunnel.copy(), [0, 0, 0, 0]))
    leak = shell.copy()
    leak[2, 2, 2] = 0                                            # touches the cavity's corner voxel (3, 3, 3) by a corner only
    want = solid.copy()
    want[2, 2, 2] = 0
    cases.append(('diagonal leak', leak, want, [1, 27, 0, 0]))
    edge = shell.copy()
    edge[2, 2, 4] = 0                                            # touches cavity voxel (3, 3, 4) across an edge only
    want = solid.copy()
    want[2, 2, 4] = 0
    cases.append(('edge leak', edge, want, [1, 27, 0, 0]))
    cup = np.zeros((9, 9, 9), dtype=np.uint8)
    cup[0:5, 2:7, 2:7] = 1
    cup[0:4, 3:6, 3:6] = 0                                       # a cavity that opens on the volume face i = 0
    cases.append(('open to a face', cup, cup.copy(), [0, 0, 0, 0]))
    two = np.zeros((9, 9, 20), dtype=np.uint8)
    two[2:7, 2:7, 2:7] = _shell()[2:7, 2:7, 2:7]
    two[2:7, 2:7, 12:17] = _shell()[2:7, 2:7, 2:7]
    want = two.copy()
    want[3:6, 3:6, 3:6] = 1
    want[3:6, 3:6, 13:16] = 1
    cases.append(('two cavities', two, want, [2, 54, 0, 0]))
    cases.append(('all ones', np.ones(SMALL, dtype=np.uint8), np.ones(SMALL, dtype=np.uint8), [0, 0, 0, 0]))
    cases.append(('all zero', np.zeros(SMALL, dtype=np.uint8), np.zeros(SMALL, dtype=np.uint8), [0, 0, 0, 0]))
    return cases


def reference_cca(seg):
    """post_processing.connected_component_analysis_3d of the reference, line by line, with regions.cc_label_host standing
    in for skimage.measure.label (labels 1.. in the order of each component's first voxel, 0 = background) and a stable
    argsort for the size ties the reference leaves open."""
    from nnal_amd import regions
    seg = np.asarray(seg)
    lab = regions.cc_label_host(seg, 26)
    roots = np.unique(lab[lab >= 0])
    CC_labels = np.where(lab >= 0, np.searchsorted(roots, lab) + 1, 0)
    bkg_label = CC_labels[0, 0, 0]
    comp_labels = list(np.unique(CC_labels))
    comp_labels.remove(bkg_label)
    vols = np.zeros(len(comp_labels))
    for i, l in enumerate(comp_labels):
        vols[i] = np.sum(CC_labels == l)
    largest_comp_label = comp_labels[np.argsort(-vols, kind='stable')[0]]
    cc_seg = np.zeros(seg.shape, dtype=np.uint32)
    cc_seg[CC_labels == largest_comp_label] = 1
    return cc_seg


def wrapper_cases():
    """[(name, seg)] for connected_component_analysis_3d: both origin branches, the tie of the zero set."""
    cases = [('origin 0, sparse', np.array(random_volume(BOX, 0.12))), ('origin 0, tie of 8', np.array(random_volume(SMALL, 0.05)))]
    sparse = np.array(random_volume(SMALL, 0.2))
    sparse[0, 0, 0] = 1
    cases.append(('origin set, zero set larger', sparse))                       # 1053 zeros against a component of 222
    dense = np.array(fill_volume(BOX, 0.75))
    dense[0:2, 0:2, 0:2] = 0
    dense[0, 0, 0] = 1                                                          # the origin's component is that voxel alone
    cases.append(('origin set, a foreground component larger', dense))
    tie = np.array([1, 0, 0, 1, 1], dtype=np.uint8).reshape(1, 1, 5)            # two zeros, a component of two: label 0 first
    cases.append(('origin set, zero set ties', tie))
    return cases
