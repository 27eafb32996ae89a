"""Plain numpy fp64 references, and the case builders, that tests/test_gpu_angle_mse_edges.py and tests/test_gpu_kabsch_edges.py
hold csrc/angle_mse.hip and csrc/kabsch.hip against.  No torch autograd, no GPU; pinned by tests/test_metric_ref.py.

Angle MSE (the header comment of csrc/angle_mse.hip, oracle.losses.mse_over_angles): a row of the [T, 24] truth is selected for a
column slice - full 0..23, backbone 0..11, side chain 12..23 - when any truth element OF THAT SLICE is != 0 (NaN counts as
non-zero, -0.0 as zero); NaN truth elements of a selected row are dropped; the rest enter a plain sum of squared differences
and a count.

Superposed RMSD: by EXPLICIT superposition (centre, SVD of H, rotate, residuals), not by the trace identity
rmsd^2 = (sum |a|^2 + sum |b|^2 - 2 (s1 + s2 + d s3)) / n that the kernel evaluates - so it does not share the kernel's
cancellation.  `present_atoms` is the one restatement of which slots the kernel must use.
"""
import numpy as np

PAD_ID = 20
NUM_SLOTS = 14
SLICES = (("full", slice(0, 24)), ("bb", slice(0, 12)), ("sc", slice(12, 24)))
EPS64 = 2.0 ** -52


# --------------------------------------------------------------------------- angle MSE
def mse_masks(true):
    """true [..., 24] -> {slice name: bool [T, 24]}: the elements that enter the slice's sum"""
    t = np.asarray(true, dtype=np.float64).reshape(-1, 24)
    out = {}
    for name, sl in SLICES:
        selected = (t[:, sl] != 0).any(axis=1)                   # NaN != 0 is True, -0.0 != 0 is False
        m = np.zeros(t.shape, bool)
        m[:, sl] = selected[:, None] & ~np.isnan(t[:, sl])
        out[name] = m
    return out


def mse_sums_ref(pred, true):
    """-> (sums [6] float64 in the kernel's layout {sum, count} x {full, bb, sc}, the three counts as exact ints)"""
    p = np.asarray(pred, dtype=np.float64).reshape(-1, 24)
    t = np.asarray(true, dtype=np.float64).reshape(-1, 24)
    masks = mse_masks(t)
    sums, counts = np.zeros(6), []
    for k, (name, _) in enumerate(SLICES):
        m = masks[name]
        d = p[m] - t[m]
        sums[2 * k], sums[2 * k + 1] = float(np.sum(d * d)), float(m.sum())
        counts.append(int(m.sum()))
    return sums, tuple(counts)


def mse_grad_ref(pred, true, coef, count):
    """d(coef * sum_full / count) / d(pred): coef 2 (p - t) / count on the selected, non-NaN elements of the FULL slice, exactly 0
    elsewhere (float64, pred's shape).  `count` is whatever the caller normalises with (the global count under data parallelism)."""
    p = np.asarray(pred, dtype=np.float64)
    t = np.asarray(true, dtype=np.float64)
    m = mse_masks(t)["full"].reshape(p.shape)
    g = np.zeros(p.shape)
    g[m] = float(coef) * 2.0 * (p[m] - t[m]) / float(count)
    return g


# the row classes of the angle-MSE cases: name -> (in full, in bb, in sc, non-NaN elements in bb, in sc)
ROW_CLASSES = {
    "ordinary": (True, True, True, 12, 12),
    "padding": (False, False, False, 12, 12),                    # all-zero truth
    "bb_zero": (True, False, True, 12, 12),                      # backbone all zero, side chain not
    "sc_zero": (True, True, False, 12, 12),                      # side chain all zero, backbone not
    "some_nan": (True, True, True, 9, 7),
    "all_nan": (True, True, True, 0, 0),                         # selected, contributes nothing
    "bb_zero_one_nan": (True, True, True, 11, 12),               # backbone zero except one NaN: the NaN selects it
    "neg_zero": (False, False, False, 12, 12),                   # a row of -0.0
    "denormal": (True, False, True, 12, 12),                     # the only non-zero element is 1e-40 (side chain, column 17)
}
HEAVY = 8.0                                                      # |p - t| of every element of the heavy row
LIGHT = 0.5                                                      # |p - t| <= LIGHT elsewhere


def make_truth_rows(cls, k, rng):
    """k truth rows [k, 24] (float64) of one class"""
    t = rng.uniform(0.1, 1.0, (k, 24)) * rng.choice([-1.0, 1.0], (k, 24))
    if cls == "padding":
        t[:] = 0.0
    elif cls == "bb_zero":
        t[:, :12] = 0.0
    elif cls == "sc_zero":
        t[:, 12:] = 0.0
    elif cls == "some_nan":
        t[:, [0, 5, 11, 12, 13, 19, 22, 23]] = np.nan
    elif cls == "all_nan":
        t[:] = np.nan
    elif cls == "bb_zero_one_nan":
        t[:, :12] = 0.0
        t[:, 7] = np.nan
    elif cls == "neg_zero":
        t[:] = -0.0
    elif cls == "denormal":
        t[:] = 0.0
        t[:, 17] = 1e-40
    else:
        assert cls == "ordinary"
    return t


def make_mse_case(T, heavy_row, seed):
    """pred, true [T, 24] fp32 and the class name of every row.  A third of the rows (at least 9, where T allows), at shuffled
    positions, cycle through ROW_CLASSES, the others are `ordinary`; the last row is padding from T = 36 on; every element has
    |p - t| <= LIGHT (a NaN truth element faces a finite prediction).  `heavy_row`: see set_heavy_row."""
    rng = np.random.default_rng(seed)
    names = list(ROW_CLASSES)
    classes = np.array(["ordinary"] * T, dtype=object)
    special = rng.permutation(T)[:max(T // 3, min(T, len(names)))]
    for k, r in enumerate(special):
        classes[r] = names[k % len(names)]
    if T >= 4 * len(names):
        classes[T - 1] = "padding"
    true = np.zeros((T, 24))
    for cls in names:
        rows = np.nonzero(classes == cls)[0]
        true[rows] = make_truth_rows(cls, len(rows), rng)
    true = true.astype(np.float32)
    pred = (np.nan_to_num(true.astype(np.float64), nan=0.3) + rng.uniform(-LIGHT, LIGHT, (T, 24))).astype(np.float32)
    d = np.abs(pred.astype(np.float64) - np.nan_to_num(true.astype(np.float64), nan=0.3))
    assert np.all(d <= LIGHT + 1e-6)                             # what the fp32 rounding left of the bound
    if heavy_row is not None:
        return set_heavy_row(pred, true, classes, heavy_row, seed)
    return pred, true, classes


def set_heavy_row(pred, true, classes, row, seed=0):
    """copies of the case with `row` made an ordinary row with |p - t| = HEAVY on every element (to the fp32 rounding of p)"""
    rng = np.random.default_rng([seed, row])
    pred, true, classes = pred.copy(), true.copy(), classes.copy()
    classes[row] = "ordinary"
    true[row] = make_truth_rows("ordinary", 1, rng)[0].astype(np.float32)
    pred[row] = (true[row].astype(np.float64) + HEAVY * rng.choice([-1.0, 1.0], 24)).astype(np.float32)
    assert np.all(np.abs(np.abs(pred[row].astype(np.float64) - true[row]) - HEAVY) < 1e-5)
    return pred, true, classes


def check_row_classes(true, classes):
    """asserts that every row is of the class it is labelled with: membership in the three slices and the non-NaN counts"""
    t = np.asarray(true, dtype=np.float64).reshape(-1, 24)
    masks = mse_masks(t)
    for r, cls in enumerate(classes):
        full, bb, sc, n_bb, n_sc = ROW_CLASSES[cls]
        got = (bool((t[r] != 0).any()), bool((t[r, :12] != 0).any()), bool((t[r, 12:] != 0).any()))
        assert got == (full, bb, sc), (r, cls, got)
        ok = ~np.isnan(t[r])
        assert (int(ok[:12].sum()), int(ok[12:].sum())) == (n_bb, n_sc), (r, cls)
        want = ((n_bb + n_sc) * full, n_bb * bb, n_sc * sc)
        assert tuple(int(masks[name][r].sum()) for name, _ in SLICES) == want, (r, cls)


# --------------------------------------------------------------------------- superposed RMSD
def superposed_rmsd_ref(a, b):
    """a, b [n, 3] -> (rmsd, sigma [3] descending, n, M): the RMSD of `a` optimally superposed on `b`, the singular values of the
    centred H = sum a_i b_i^T, the atom count and the UNCENTRED second moment M = sum |a|^2 + sum |b|^2.  fp64 throughout.
    NaN for n = 0 and for a non-finite coordinate (sigma and M are NaN then, too)."""
    a = np.asarray(a, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(b, dtype=np.float64).reshape(-1, 3)
    n = a.shape[0]
    assert b.shape[0] == n
    nan = float("nan")
    if n == 0 or not (np.isfinite(a).all() and np.isfinite(b).all()):
        return nan, np.full(3, nan), n, nan
    M = float((a * a).sum() + (b * b).sum())
    ac, bc = a - a.mean(0), b - b.mean(0)
    u, s, vt = np.linalg.svd(ac.T @ bc)
    d = 1.0 if np.linalg.det(u) * np.linalg.det(vt) >= 0 else -1.0
    rot = u @ np.diag([1.0, 1.0, d]) @ vt                         # row vectors: a_i rot is a_i turned onto b_i
    res = ac @ rot - bc
    return float(np.sqrt((res * res).sum() / n)), s, n, M


def kabsch_bar(want, sigma, n, M):
    """The bar on |got^2 - want^2| for the kernel's fp32 answer `got` (module docstring of tests/test_gpu_kabsch_edges.py)."""
    s1, s2, s3 = (float(x) for x in sigma)
    den = s2 if s2 <= RANK1_TOL * s1 else s3                      # rank-1 H: sigma_2 in place of sigma_3
    root = np.sqrt(16 * EPS64) * s1
    third = root if den == 0.0 else min(root, 16 * EPS64 * s1 * s1 / den)
    return 2.0 ** -22 * want * want + 64 * EPS64 * M / n + 6 * third / n


RANK1_TOL = 1e-5                                                 # fp32 inputs: a collinear set rounds to sigma_2 / sigma_1 ~ 1e-7


def present_atoms(pred, true, seq):
    """pred, true [L*14, 3], seq [L] -> bool [L*14]: the slots the kernel must use - the residue is not PAD_ID and no TRUE
    coordinate of the atom is NaN (one NaN coordinate removes the atom).  What the prediction holds never decides presence."""
    true = np.asarray(true)
    seq = np.asarray(seq)
    assert true.shape == np.asarray(pred).shape == (seq.shape[0] * NUM_SLOTS, 3)
    return np.repeat(seq != PAD_ID, NUM_SLOTS) & ~np.isnan(true).any(axis=1)


def protein_ref(pred, true, seq):
    """superposed_rmsd_ref over the present atoms of one protein"""
    m = present_atoms(pred, true, seq)
    return superposed_rmsd_ref(np.asarray(pred)[m], np.asarray(true)[m])


def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


N_GEO = 40
NOISE = 0.5


def geometry_cases():
    """name -> (a, b, exact): prediction a and truth b, [n, 3] float32, and whether a is an exact rigid motion of b in fp64 (before
    the rounding to fp32).  Every geometry of the Kabsch suite, once exact and once with NOISE A of isotropic noise on a."""
    rng = np.random.default_rng(11)
    q, shift = rotation(rng), np.array([30.0, -7.0, 110.0])
    move = lambda x: x @ q.T + shift                              # noqa: E731
    general = rng.normal(0, 8, (N_GEO, 3))
    planar = general * np.array([1.0, 1.0, 0.0])
    planar_rot = planar @ rotation(rng).T
    bumps = planar + np.outer(rng.choice([-3.0, 3.0], N_GEO) * rng.uniform(0.5, 1.0, N_GEO), [0.0, 0.0, 1.0])
    line = np.outer(rng.normal(0, 8, N_GEO), np.array([2.0, -1.0, 0.5]) / np.linalg.norm([2.0, -1.0, 0.5])) + [1.0, 2.0, 3.0]
    cube = 3.0 * np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64)
    mirror = np.array([1.0, 1.0, -1.0])
    base = {                                                     # name -> (truth, prediction before noise, rigid?)
        "general": (general, move(general), True),
        "planar-axis": (planar, move(planar), True),
        "planar-rotated": (planar_rot, move(planar_rot), True),
        "planar-vs-3d": (planar, move(bumps), False),
        "collinear": (line, move(line), True),
        "one-point": (general, np.tile(shift, (N_GEO, 1)), False),
        "mirror": (general, general * mirror, False),
        "mirror-rotated": (general, move(general * mirror), False),
        "mirror-cube": (cube, cube * mirror, False),
        "mirror-cube-rotated": (cube, move(cube * mirror), False),
        "offset-1e3": (general + 1e3, move(general) + 1e3, True),
        "offset-1e4-opposite": (general - 1e4, move(general) + 1e4, True),
    }
    out = {}
    for name, (b, a, rigid) in base.items():
        out[name] = (a.astype(np.float32), b.astype(np.float32), rigid)
        noisy = a + rng.normal(0, NOISE, a.shape) if name != "one-point" else a + 1e3    # (the point, elsewhere)
        out[name + "+noise"] = (noisy.astype(np.float32), b.astype(np.float32), False)
    return out


# what test_metric_ref.py asserts of the cases, from the reference's own singular values: name -> rank of the centred H
GEOMETRY_RANK = {"general": 3, "planar-axis": 2, "planar-rotated": 2, "planar-vs-3d": 2, "collinear": 1, "one-point": 0,
                 "mirror": 3, "mirror-rotated": 3, "mirror-cube": 3, "mirror-cube-rotated": 3, "offset-1e3": 3,
                 "offset-1e4-opposite": 3}


def embed(a, b, L=None, slots=None, rng=None):
    """a, b [n, 3] -> (pred [L*14, 3], true [L*14, 3], seq [L]) fp32 / int64 with the n atoms at `slots` (default: the first n), NaN
    truth at every other slot and finite garbage in the prediction there."""
    n = len(a)
    L = L or max(1, -(-n // NUM_SLOTS))
    slots = np.arange(n) if slots is None else np.asarray(slots)
    assert len(slots) == n and (n == 0 or slots.max() < L * NUM_SLOTS)
    rng = rng or np.random.default_rng(n + L)
    pred = rng.normal(0, 50, (L * NUM_SLOTS, 3)).astype(np.float32)
    true = np.full((L * NUM_SLOTS, 3), np.nan, np.float32)
    pred[slots], true[slots] = a, b
    return pred, true, np.zeros(L, np.int64)


SLOT_LS = (1, 18, 19, 37, 74)
SLOT_EDGES = (0, 63, 64, 255, 256, 511, 512)


def sparse_slot_sets(L):
    """the sparse proteins of a length: sets of 4 - 6 present slots out of SLOT_EDGES and the last slot, every existing edge in at
    least one set (L = 1 has two of them: the sets are filled up with their neighbours)"""
    last = L * NUM_SLOTS - 1
    edges = sorted({s for s in SLOT_EDGES if s < last} | {last})
    if len(edges) < 4:
        edges = sorted(set(edges) | {1, last - 1})[:6]
    if len(edges) <= 6:
        return [edges]
    inner = edges[:-1]
    return [inner[:4] + [last], inner[3:] + [last]]
