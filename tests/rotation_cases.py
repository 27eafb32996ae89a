"""Degenerate geometry for the three kernels that call tm_rotation::solve (csrc/tm_rotation.h): csrc/kabsch_loss.hip,
csrc/ensemble.hip and csrc/tmscore.hip.  The cases, their classes, the fp64 yardsticks and the host-side moments, shared by
tests/test_rotation_cases.py, tests/test_rotation_host.py (no GPU) and tests/test_gpu_rotation_degenerate.py.  TEST INFRASTRUCTURE
ONLY.  Nothing is re-derived here: the point sets come from metric_ref.geometry_cases, the references are
kabsch_loss_ref.kabsch_loss_reference, ensemble_ref.reference and tm_ref.tm_ref.

CLASSES, by the reference's gap g = (sigma2 + sign(det S) sigma3) / sigma1 of the centred correlation matrix S (tm_ref's min_gap; it
is what separates the two largest eigenvalues of Horn's matrix):
  unique      g >= GAP_UNIQUE = 1e-5.  The rotation is determined; an fp64 solve errs by ~2.2e-16 x O(100) / g <= 2e-9, far below
              every fp32-output bar, so everything is compared at the kernels' existing bars.
  free        g == 0 exactly, by construction: sets on coordinate axes with coordinates that are multiples of 1/64 (exact in fp32,
              sums exact in fp64), moved by signed axis permutations and shifts that are multiples of 0.25 - collinearity and the
              cube's symmetry survive every rounding.  A whole family of rotations is optimal (free_family); only what is the same
              for every member is compared (FREE_KINDS says what that is per kind of family, test_rotation_cases.py checks it).
  value-only  0 < g < 1e-5: VALUE_ONLY, three cases of metric_ref.geometry_cases and nothing else.  `collinear` (g 2.0e-16) and
              `collinear+noise` (2.3e-10: S = sum a_k b_k^T has the rank of the TRUTH, whatever noise the prediction carries) are
              lines rotated off the axes and rounded to fp32; `mirror-cube-rotated` (1.0e-7) is the cube's equal singular values
              split by that rounding.  The rotation is formally unique and numerically arbitrary: the optimum (loss, rmsd) is
              compared, the rotation and what depends on it is not.

FREE FAMILIES (R maps the prediction onto the truth, column vectors; R0 the SVD's answer):
  line    the truth is collinear along u (and the prediction may be, along v): Rot(u, s) R0 Rot(v, t).  Rot(u) fixes every centred
          true atom, Rot(v) every centred predicted one, so EVERY residual keeps its length: loss, rmsd, each C-alpha's deviation
          and each TM distance are invariant; atoms that are not on the lines (the all-atom rmsf column) are not.
  pline   the prediction is collinear along v, the truth is not: R0 Rot(v, t); the same invariants.
  point   every predicted atom on one point: S = 0, any rotation; the residual is -(b_k - bbar) for all of them - the same invariants.
  cube    sigma1 = sigma2 = sigma3, det S < 0: V W diag(1, 1, -1) W^T U^T for any rotation W, a two-parameter family.  Only the SUM
          of squared residuals is invariant (loss, rmsd); single residuals are not, so neither rmsf column is compared.
For every member g = R^T r / (n loss) satisfies sum g = 0 and sum |g|^2 = 1 / n: that needs R orthogonal, nothing more."""
import functools

import numpy as np

import ensemble_ref as ER
import kabsch_loss_ref as KR
import metric_ref as M
import tm_ref as T

GAP_UNIQUE = 1e-5
VALUE_ONLY = ("collinear", "collinear+noise", "mirror-cube-rotated")
FREE_KINDS = {"line": ("loss", "per-atom"), "pline": ("loss", "per-atom"), "point": ("loss", "per-atom"), "cube": ("loss",)}
GRID = 64.0                                                      # coordinates of the free sets are multiples of 1 / GRID


def gap(a, b):
    """prediction a, truth b [n,3] -> (g, singular values, sign of det S) of the centred S, in fp64; g = 0 where S = 0"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    u, s, vt = np.linalg.svd((a - a.mean(0)).T @ (b - b.mean(0)))
    sign = 1.0 if np.linalg.det(vt.T @ u.T) >= 0 else -1.0
    return (0.0 if s[0] == 0 else float((s[1] + sign * s[2]) / s[0])), s, sign


def class_of(name, a, b):
    g = gap(a, b)[0]
    if g >= GAP_UNIQUE:
        return "unique"
    return "free" if g == 0.0 else "value-only"


def signed_permutation(perm, signs):
    q = np.zeros((3, 3))
    for i, (p, s) in enumerate(zip(perm, signs)):
        q[i, p] = s
    assert abs(np.linalg.det(q) - 1.0) < 1e-15                   # a proper one
    return q


Q_XY = signed_permutation((1, 0, 2), (1, -1, 1))                 # x -> -y ... : quarter turn about z
Q_CYC = signed_permutation((1, 2, 0), (1, 1, 1))                 # cyclic
Q_FLIP = signed_permutation((2, 1, 0), (-1, -1, -1))


def on_grid(x):
    return np.round(np.asarray(x) * GRID) / GRID


@functools.lru_cache(maxsize=None)
def cases():
    """name -> dict(a, b [n,3] fp32: prediction and truth; rigid: a is an exact motion of b; cls; kind: the free family or None).
    The 24 cases of metric_ref.geometry_cases and the new ones of this file."""
    out = {}
    for name, (a, b, rigid) in M.geometry_cases().items():
        kind = {"one-point": "point", "one-point+noise": "point", "mirror-cube": "cube"}.get(name)
        out[name] = dict(a=a, b=b, rigid=rigid, kind=kind)
    rng = np.random.default_rng(2024)
    n = M.N_GEO
    ex, mirror = np.array([1.0, 0.0, 0.0]), np.array([1.0, 1.0, -1.0])
    line = np.outer(on_grid(rng.normal(0, 8, n)), ex) + [1.25, -2.5, 7.0]
    stretched = line + np.outer(on_grid(rng.uniform(-2, 2, n)), ex)
    cloud = rng.normal(0, 8, (n, 3))
    cube = 3.0 * np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float64)
    tri = np.array([[0.0, 0.0, 0.0], [3.8, 0.0, 0.0], [5.1, 3.5, 0.0]]) @ M.rotation(rng).T
    q, shift = M.rotation(rng), np.array([-12.0, 40.0, 3.0])
    move = lambda x: x @ q.T + shift                              # noqa: E731

    def near_line(scatter, m=12):                                # a short strand: 12 atoms over ~6 A, `scatter` A off the line
        t = np.linspace(-3.0, 3.0, m) + rng.normal(0, 0.2, m)
        u = np.array([2.0, -1.0, 0.5]) / np.linalg.norm([2.0, -1.0, 0.5])
        off = rng.normal(0, scatter, (m, 3))
        return np.outer(t, u) + off - np.outer(off @ u, u) + [4.0, 5.0, 6.0]

    def add(name, a, b, rigid, kind=None):
        out[name] = dict(a=np.asarray(a).astype(np.float32), b=np.asarray(b).astype(np.float32), rigid=rigid, kind=kind)

    # ---- free: exact in fp32 by construction
    add("axis-line", line @ Q_XY.T + [0.25, -3.0, 10.5], line, True, "line")
    add("axis-line-stretched", stretched @ Q_CYC.T + [-7.75, 0.5, 2.0], line, False, "line")
    add("axis-line-vs-3d", cloud, line @ Q_FLIP.T + [3.0, 3.25, -1.5], False, "line")
    add("3d-vs-axis-line", line @ Q_CYC.T, cloud, False, "pline")
    add("axis-mirror-cube-moved", (cube * mirror) @ Q_CYC.T + [5.25, -0.75, 2.0], cube, False, "cube")
    add("axis-one-point", np.tile([2.5, -1.25, 8.0], (n, 1)), on_grid(cloud), False, "point")
    # ---- unique: three atoms, and lines with a little scatter
    add("three", move(tri) + rng.normal(0, 0.3, tri.shape), tri, False)
    add("three-exact", move(tri.astype(np.float32).astype(np.float64)), tri, True)
    for k, scatter in ((2, 1e-2), (1, 1e-1)):
        b = near_line(scatter)
        add(f"near-line-1e-{k}", move(b) + rng.normal(0, 0.2, b.shape), b, False)
        add(f"near-line-1e-{k}-exact", move(b.astype(np.float32).astype(np.float64)), b, True)
    for name, c in out.items():
        c["cls"] = class_of(name, c["a"], c["b"])
        c["gap"] = gap(c["a"], c["b"])[0]
    return out


def grid_lines():
    """[(direction, x [20,3] fp32)]: lines along every integer direction with entries in -3 .. 3 (first entry >= 0), positions
    on the 1/64 grid: EXACTLY collinear in fp32, off the coordinate axes.  Against itself such a set has sigma2 = sigma3 = 0 and
    the identity ties with the half turn about the line; on 22 of the 195 the sweeps of csrc/tm_rotation.h round the half turn's
    eigenvalue above trace S, and a strict comparison then returned the half turn."""
    import itertools
    rng = np.random.default_rng(5)
    out = []
    for d in itertools.product(range(-3, 4), repeat=3):
        if any(d) and d[0] >= 0:
            x = np.outer(on_grid(rng.normal(0, 8, 20)), d) + np.round(rng.normal(0, 10, 3) * 4) / 4
            assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
            out.append((d, x.astype(np.float32)))
    return out


def rot(axis, angle):
    return ER._rotation(np.asarray(axis, np.float64) / np.linalg.norm(axis) * angle)


def direction(x):
    """the unit vector along a collinear set [n,3] (fp64)"""
    xc = x - x.mean(0)
    v = xc[np.abs(xc).sum(1).argmax()]
    return v / np.linalg.norm(v)


def free_family(a, b, kind, count=7):
    """[R0, R1 .. R_count]: the SVD rotation of kabsch_loss_ref.svd_rotation and `count` further optimal rotations of the family."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    ac, bc = a - a.mean(0), b - b.mean(0)
    R0 = KR.svd_rotation(ac, bc)
    rng = np.random.default_rng(99)
    out = [R0]
    for j in range(count):
        s, t = rng.uniform(0.3, 2 * np.pi - 0.3, 2)
        if kind == "line":
            R = rot(direction(b), s) @ R0
            if gap(a, a)[1][1] == 0.0:                            # the prediction is collinear as well
                R = R @ rot(direction(a), t)
        elif kind == "pline":
            R = R0 @ rot(direction(a), t)
        elif kind == "point":
            R = M.rotation(rng)
        else:
            assert kind == "cube", kind
            u, _, vt = np.linalg.svd(ac.T @ bc)
            W = M.rotation(rng)
            R = vt.T @ W @ np.diag([1.0, 1.0, -1.0]) @ W.T @ u.T
        assert abs(np.linalg.det(R) - 1.0) < 1e-12
        out.append(R)
    return out


def residuals(R, a, b):
    """r_k = R (a_k - abar) - (b_k - bbar), [n,3] fp64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (a - a.mean(0)) @ R.T - (b - b.mean(0))


# ----------------------------------------------------------------------------- the superposition loss
def straddling_slots(n, L=37):
    """n slots of a row of L = 37 residues (518 slots): half around slot 256, half around slot 512 - both round edges of the
    kernel's 256-thread sweeps lie inside the set"""
    h = n // 2 if n >= 4 else 1
    m = n - h
    lo = 256 - (h + 1) // 2
    hi = min(512 - m // 2, L * M.NUM_SLOTS - m)
    s = list(range(lo, lo + h)) + list(range(hi, hi + m))
    assert len(set(s)) == n and lo < 256 <= s[h - 1] + (h == 1) and hi <= 512
    return s


@functools.lru_cache(maxsize=None)
def loss_inputs(name, layout):
    """(pred, true, seq) of one case: `dense` at L = 3, `straddle` at L = 37 on straddling_slots"""
    c = cases()[name]
    if layout == "dense":
        return M.embed(c["a"], c["b"], L=3)
    return M.embed(c["a"], c["b"], L=37, slots=straddling_slots(len(c["a"])))


@functools.lru_cache(maxsize=None)
def loss_reference(name, layout):
    return KR.kabsch_loss_reference(*loss_inputs(name, layout))


ORIGIN_FIRST = (63, 64, 128, 191, 255, 256, 511, 512, "last")    # (128 and 191 are this file's: no edge of the issue is in wavefront 2)


def origin_cases():
    """(L, first) -> (pred, true, seq): the slots of metric_ref.sparse_slot_sets(L) from `first` on, filled up with the slots that
    follow `first` to four atoms where the row has them; the atoms are those of `general+noise`.
    The origin search of kabsch_loss_kernel runs in rounds of 256 slots, four wavefronts of 64 each.  First present slot ->
    (round, wavefront): 63 -> (0, 0), 64 -> (0, 1), 128 -> (0, 2), 191 -> (0, 2), 255 -> (0, 3), 256 -> (1, 0), 511 -> (1, 3),
    512 -> (2, 0); the last slot is 517 -> (2, 0) at L = 37 and 1035 -> (4, 0) at L = 74.  So 256 and 511 reach round 1, 512 and the
    last slots reach round 2 and beyond, 64 reaches wavefront 1, 128 and 191 wavefront 2, 255 and 511 wavefront 3."""
    a, b, _ = M.geometry_cases()["general+noise"]
    out = {}
    for L in (37, 74):
        last = L * M.NUM_SLOTS - 1
        edges = sorted({s for group in M.sparse_slot_sets(L) for s in group} | {128, 191})
        for first in ORIGIN_FIRST:
            f = last if first == "last" else first
            slots = [s for s in edges if s >= f]
            fill = f + 1
            while len(slots) < 4 and fill <= last:
                if fill not in slots:
                    slots.append(fill)
                fill += 1
            slots = sorted(slots)
            assert slots[0] == f
            out[(L, first)] = M.embed(a[:len(slots)], b[:len(slots)], L=L, slots=slots)
    return out


# ----------------------------------------------------------------------------- the ensemble spread
ENSEMBLE_LS = (40, 65)
ENSEMBLE_BASES = ("general", "planar-axis", "planar-rotated", "planar-vs-3d", "collinear", "one-point", "mirror", "mirror-rotated",
                  "mirror-cube", "mirror-cube-rotated", "offset-1e3", "offset-1e4-opposite", "axis-line", "axis-line-stretched",
                  "axis-line-vs-3d", "3d-vs-axis-line", "axis-mirror-cube-moved", "axis-one-point", "three", "near-line-1e-2",
                  "near-line-1e-1")


def ensemble_samples(base):
    """The K = 3 C-alpha sets fitted on the truth of a base case: the case's prediction, a noisy form of it, its mirror image."""
    cs = cases()
    a = cs[base]["a"]
    if base + "+noise" in cs:
        noisy = cs[base + "+noise"]["a"]
    else:
        rng = np.random.default_rng(len(base))
        noisy = (a.astype(np.float64) + rng.normal(0, M.NOISE, a.shape)).astype(np.float32)
    return [a, noisy, a * np.array([1.0, 1.0, -1.0], np.float32)]


def ensemble_compared(base):
    """(rmsd compared per sample [3], C-alpha column compared, all-atom column compared) from the class of each of the three fits"""
    b = cases()[base]["b"]
    kinds = []
    for k, s in enumerate(ensemble_samples(base)):
        cls = class_of(base, s, b)
        if cls == "unique":
            kinds.append("unique")
        elif cls == "value-only":
            kinds.append("value-only")
        else:
            kinds.append(free_kind(s, b))
    per_atom = all(k == "unique" or (k in FREE_KINDS and "per-atom" in FREE_KINDS[k]) for k in kinds)
    return kinds, per_atom, all(k == "unique" for k in kinds)


def free_kind(a, b):
    """the family of a pair whose gap is exactly 0, from its singular values"""
    _, s, sign = gap(a, b)
    if s[0] == 0:
        return "point" if gap(a, a)[1][0] == 0 else "line"        # (S = 0 without a one-point prediction: not among the cases)
    if s[1] == 0:
        return "line" if gap(b, b)[1][1] == 0 else "pline"
    assert sign < 0 and s[0] == s[1] == s[2]
    return "cube"


@functools.lru_cache(maxsize=None)
def ensemble_inputs(L):
    """(bases, ref [B, L*14, 3], samples [B, 3, L*14, 3], seq [B, L], extent [B]) fp32 / int64: the truth of each base as the
    C-alphas of n residues - the first n of the row at L = 40, the LAST n at L = 65 (the rmsf kernel's second tile of 64 residues)
    - every other residue padding; the other atoms a residue's type has are finite clouds of 1.5 A around the C-alpha (the
    sample's: the reference's cloud carried along unrotated, plus 0.3 A), the slots it does not have are NaN."""
    rng = np.random.default_rng(500 + L)
    B = len(ENSEMBLE_BASES)
    ref = np.full((B, L, ER.SLOTS, 3), np.nan, np.float32)
    samples = np.full((B, 3, L, ER.SLOTS, 3), np.nan, np.float32)
    seq = np.full((B, L), ER.PAD_ID, np.int64)
    extent = np.zeros(B)
    for i, base in enumerate(ENSEMBLE_BASES):
        b = cases()[base]["b"]
        n = len(b)
        at = np.arange(n) if L == 40 else np.arange(L - n, L)
        seq[i, at] = rng.integers(0, 20, n)
        mask = ER.atom_mask(seq[i])[at]                           # [n, 14]
        offs = rng.normal(0, 1.5, (n, ER.SLOTS, 3))
        offs[:, ER.CA] = 0.0
        ref[i, at] = np.where(mask[:, :, None], b[:, None, :].astype(np.float64) + offs, np.nan)
        for k, s in enumerate(ensemble_samples(base)):
            cloud = s[:, None, :].astype(np.float64) + offs + rng.normal(0, 0.3, offs.shape) * (np.arange(ER.SLOTS) != ER.CA)[None, :, None]
            samples[i, k, at] = np.where(mask[:, :, None], cloud, np.nan)
        assert np.array_equal(ref[i, at, ER.CA], b) and all(np.array_equal(samples[i, k, at, ER.CA], s)
                                                            for k, s in enumerate(ensemble_samples(base)))
        extent[i] = ER.extent_of(ref[i], samples[i])
    return ENSEMBLE_BASES, ref.reshape(B, -1, 3), samples.reshape(B, 3, -1, 3), seq, extent


@functools.lru_cache(maxsize=None)
def ensemble_reference(L):
    _, ref, samples, seq, _ = ensemble_inputs(L)
    return ER.reference(ref, samples, seq)


# ----------------------------------------------------------------------------- TM-score
TM_NS = (5, 20, 65, 130)
TM_STEP = 3.75                                                   # A between neighbours on the line; exact in fp32


def tm_line_line(n, seed):
    """exact collinear against collinear: the truth on the x axis, the prediction on the y axis with every residue displaced
    along the line by up to 3 A.  The coordinates ACROSS the lines are constants on the 1/64 grid, so both sets stay exactly
    collinear in fp32; the displacements along the line are whatever fp32 holds (on the grid a distance would sit ON a cutoff)"""
    rng = np.random.default_rng(seed)
    t = TM_STEP * np.arange(n)
    q = np.outer(t, [1.0, 0.0, 0.0]) + [2.0, -4.25, 0.5]
    p = np.outer(t + rng.uniform(-3, 3, n), [0.0, 1.0, 0.0]) + [-1.5, 0.25, 3.0]
    return T.embed(p, q)


def tm_line_3d(n, seed):
    """collinear truth (z axis) against a 3-D prediction: the line plus 0.3 - 3 A of isotropic noise per residue, turned"""
    rng = np.random.default_rng(seed)
    q = np.outer(TM_STEP * np.arange(n), [0.0, 0.0, 1.0]) + [0.25, 8.0, -3.5]
    sigma = rng.uniform(0.3, 3.0, (n, 1)) / np.sqrt(3.0)
    return T.embed((q + sigma * rng.normal(size=q.shape)) @ T.rotation(rng).T + rng.normal(size=3) * 10.0, q)


def tm_zigzag(n, seed):
    """a planar zig-zag strand (3.8 A between neighbours, 1.9 A across) against a copy with in-plane noise of 0.3 - 3 A, turned"""
    rng = np.random.default_rng(seed)
    k = np.arange(n)
    q = np.stack([3.3 * k, 0.95 * (-1.0) ** k, np.zeros(n)], 1)
    noise = rng.uniform(0.3, 3.0, (n, 1)) / np.sqrt(2.0) * rng.normal(size=(n, 3)) * [1.0, 1.0, 0.0]
    return T.embed((q + noise) @ T.rotation(rng).T + rng.normal(size=3) * 10.0, q @ M.rotation(rng).T)


def tm_three_collinear():
    """N = 3 on a line, truth and prediction on different axes with different spacing"""
    q = np.outer([0.0, 3.75, 7.5], [0.0, 1.0, 0.0]) + [1.0, 2.0, 3.0]
    p = np.outer([0.0, 4.5, 7.25], [0.0, 0.0, 1.0]) + [-2.0, 0.5, 0.25]
    return T.embed(p, q)


# name -> builder of ONE protein, in the style of tm_ref.GPU_CASES.  They are NOT in that table: tests/test_tm_ref.py requires
# min_rank >= 1e-3 of every entry of it, and rank 1 is the point of these; tests/test_rotation_cases.py holds them to the margin
# condition instead.  The seeds are the first, counting up from 3000 + n, whose smallest margin is >= TM_MARGIN.
TM_MARGIN = 1e-6
TM_CASES = {**{f"line-line{n}": functools.partial(tm_line_line, n, 3000 + n) for n in TM_NS},
            **{f"line-3d{n}": functools.partial(tm_line_3d, n, 3000 + n) for n in TM_NS},
            **{f"zigzag{n}": functools.partial(tm_zigzag, n, 3000 + n) for n in TM_NS},
            "three-collinear": tm_three_collinear}
TM_RANK1 = tuple(k for k in TM_CASES if not k.startswith("zigzag"))


@functools.lru_cache(maxsize=None)
def tm_case_with_reference(name):
    pred, true, seq = TM_CASES[name]()
    return pred, true, seq, T.tm_ref(pred, true, seq)


# ----------------------------------------------------------------------------- moments, as the kernels form them
def raw_moments(a, b):
    """(n, the 15 moments of csrc/tm_rotation.h) of the pairs relative to the FIRST pair, fp64, summed in order - what
    csrc/tmscore.hip hands to solve() (csrc/ensemble.hip does the same without the origin)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    p, q = a - a[0], b - b[0]
    return len(a), np.concatenate([p.sum(0), q.sum(0), (p.T @ q).reshape(-1)])


def centred_moments(a, b):
    """... and what csrc/kabsch_loss.hip hands to it: zero sums, S = M - (sum a)(sum b)^T / n with the product formed first"""
    n, m = raw_moments(a, b)
    S = m[6:].reshape(3, 3) - np.outer(m[:3], m[3:6]) * (1.0 / n)
    return n, np.concatenate([np.zeros(6), S.reshape(-1)])
