"""fp64 numpy restatement of the frame-aligned error matrix (include/ptamd.h, `ptamd_aligned_error`), for
tests/test_aligned_error_ref.py, tests/test_gpu_aligned_error.py, tests/test_gpu_predict_pae.py and tests/test_gpu_score_ae.py.
TEST INFRASTRUCTURE ONLY: the product never imports it.

Two forms of the same definition: `reference` (vectorised over the samples, frames and points of a protein) and `reference_loops`
(a plain loop over protein, sample, frame and point), which the CPU test holds against each other.  Both work on the fp32 inputs
the kernel gets, in fp64, the frame included (the kernel rounds its frame to fp32).  `emulate32` restates the kernel's ARITHMETIC
in numpy float32 - it is how the bound below is checked without a device.

THE BOUND ON AN FP32 ENTRY.  u = 2^-24, eps32 = 2 u, X = the largest |coordinate| of the reference and the samples, K <= 8.
For one structure and one component c of x_ij = E_i (p_j - t_i), with r = p_j - t_i, |r_c| <= 2 X, |r| <= 2 sqrt(3) X = 3.47 X:
  * the frame is fp64 arithmetic on the fp32 inputs (1e-16: invisible) rounded to fp32 once: the three entries of a row of E,
    each at most 1, move by u each, times |r_x| + |r_y| + |r_z| <= 6 X:                                         6 u X;
  * r_c is one fp32 subtraction, u |r_c| <= 2 u X per component, times the row of E (sum |e_c| <= sqrt 3):      3.47 u X;
  * one multiplication and two fused multiply-adds, every intermediate at most |e| |r| <= 3.47 X:              10.4 u X;
together 19.9 u X, for the sample and for the reference: 39.8 u X; the fp32 subtraction of the two local coordinates, its result
at most 6.93 X: 6.93 u X.  So 46.7 u X per component, 46.7 sqrt(3) = 80.9 u X on the difference vector, and by the triangle
inequality on its norm.  The norm itself (a multiplication, two fused multiply-adds, a correctly rounded root: 2.5 u relative on a
value of at most 6.93 X): 17.3 u X.  The fp32 sum over k of K such norms, divided by K': at most (K + 1) / 2 roundings of a partial
sum's share, 6.93 u X each - 31.2 u X at K = 8 -; the fp32 division: 6.93 u X.  In all 136.3 u X = 68.2 eps32 X:
    |gpu - ref| <= tol(X) = 72 x 2^-23 x X   for K <= 8.
The MEAN is an fp64 sum of such entries rounded to fp32 once (6.93 u X, inside the 7.7 u X the figure above leaves): its bound is
`tol` itself.  The TM STAT averages f(x) = 1 / (1 + x^2) of x = ae / d0; |f'| <= 3 sqrt(3) / 8 = 0.6495, so |d tm| <= 0.65 tol / d0
(`tol_tm`), the fp64 arithmetic and the final rounding vanishing in the 0.0005 tol / d0 that 0.65 leaves."""
import numpy as np

from ensemble_ref import extent_of, present_of, random_chain, random_rigid   # noqa: F401  (shared, not copied)

SLOTS = 14
N_SLOT, CA, C_SLOT = 0, 1, 2
EPS32 = 2.0 ** -23
MULT = 72.0
MAX_K = 8
CRD_MAX = 1.0e18
DEGENERATE = 1.0e-8


def tol(extent, K=MAX_K):
    """Bound on |gpu - fp64| of an entry of `ae` and of the mean (module docstring); `extent` = the largest |coordinate|."""
    assert K <= MAX_K
    return MULT * EPS32 * extent


def d0_of(n):
    return 1.24 * np.cbrt(max(int(n), 19) - 15.0) - 1.8


def tol_tm(extent, n, K=MAX_K):
    """Bound on |gpu - fp64| of the TM stat of a protein with n points."""
    return 0.65 * tol(extent, K) / d0_of(n)


def _usable(p):
    """[..., 3] -> bool [...]: finite and within CRD_MAX."""
    with np.errstate(invalid="ignore"):
        return (np.abs(p) <= CRD_MAX).all(-1)


def frames_of(crd):
    """crd [..., L, 14, 3] fp64 -> (E [..., L, 3, 3] rows e1 e2 e3, t [..., L, 3], spans [..., L]): algorithm 21 from N, CA, C."""
    n, a, c = crd[..., N_SLOT, :], crd[..., CA, :], crd[..., C_SLOT, :]
    with np.errstate(all="ignore"):
        v1, v2 = c - a, n - a
        q1 = (v1 * v1).sum(-1)
        e1 = v1 / np.sqrt(q1)[..., None]
        u = v2 - e1 * (e1 * v2).sum(-1)[..., None]
        q2 = (u * u).sum(-1)
        e2 = u / np.sqrt(q2)[..., None]
        e3 = np.cross(e1, e2)
        spans = (q1 > DEGENERATE) & (q2 > DEGENERATE)
    return np.stack([e1, e2, e3], -2), a, spans


def validity(ref, samples, seq):
    """One protein: ref [L, 14, 3], samples [K, L, 14, 3], seq [L] -> (frame [L], point [L], usable [K]) bool."""
    pres = present_of(seq)
    _, _, spans = frames_of(ref)
    point = pres & _usable(ref[:, CA])
    frame = point & _usable(ref[:, N_SLOT]) & _usable(ref[:, C_SLOT]) & spans
    _, _, s_spans = frames_of(samples)
    s_point = _usable(samples[:, :, CA])
    s_frame = s_point & _usable(samples[:, :, N_SLOT]) & _usable(samples[:, :, C_SLOT]) & s_spans
    usable = (s_frame | ~frame[None]).all(1) & (s_point | ~point[None]).all(1)
    return frame, point, usable


def stats_of(ae, frame, point):
    """ae [L, L] with NaN where undefined -> (mean, tm) in fp64; NaN when no entry is defined."""
    defined = np.isfinite(ae)
    if not defined.any():
        return np.nan, np.nan
    n = int(point.sum())
    d0 = d0_of(n)
    rows = ae[frame][:, point]
    return float(rows.mean()), float((1.0 / (1.0 + (rows / d0) ** 2)).sum(1).max() / n)


def _shape(ref, samples, seq):
    seq = np.asarray(seq)
    B, L = seq.shape
    K = np.asarray(samples).shape[1]
    return seq, B, L, K


def reference(ref, samples, seq):
    """ref [B, L*14, 3], samples [B, K, L*14, 3] (fp32), seq [B, L] -> (ae [B, L, L], stats [B, 2], usable [B]) in fp64."""
    seq, B, L, K = _shape(ref, samples, seq)
    ref = np.asarray(ref, np.float64).reshape(B, L, SLOTS, 3)
    samples = np.asarray(samples, np.float64).reshape(B, K, L, SLOTS, 3)
    ae = np.full((B, L, L), np.nan)
    stats = np.full((B, 2), np.nan)
    usable = np.zeros(B, np.int64)
    for b in range(B):
        frame, point, ok = validity(ref[b], samples[b], seq[b])
        usable[b] = ok.sum()
        if not ok.any():
            continue
        with np.errstate(all="ignore"):
            E, t, _ = frames_of(ref[b])
            xr = np.einsum("icd,ijd->ijc", E, ref[b][None, :, CA] - t[:, None])                   # [L, L, 3]
            Es, ts, _ = frames_of(samples[b][ok])
            xs = np.einsum("kicd,kijd->kijc", Es, samples[b][ok][:, None, :, CA] - ts[:, :, None])
            d = np.sqrt(((xs - xr[None]) ** 2).sum(-1)).mean(0)
        ae[b] = np.where(frame[:, None] & point[None, :], d, np.nan)
        stats[b] = stats_of(ae[b], frame, point)
    return ae, stats, usable


def reference_loops(ref, samples, seq):
    """The same definition as plain loops over protein, sample, frame and point."""
    seq, B, L, K = _shape(ref, samples, seq)
    ref = np.asarray(ref, np.float64).reshape(B, L, SLOTS, 3)
    samples = np.asarray(samples, np.float64).reshape(B, K, L, SLOTS, 3)
    ae = np.full((B, L, L), np.nan)
    stats = np.full((B, 2), np.nan)
    usable = np.zeros(B, np.int64)

    def frame_of(res):
        ok = all(np.isfinite(res[s]).all() and (np.abs(res[s]) <= CRD_MAX).all() for s in (N_SLOT, CA, C_SLOT))
        if not ok:
            return None
        v1, v2 = res[C_SLOT] - res[CA], res[N_SLOT] - res[CA]
        if v1 @ v1 <= DEGENERATE:
            return None
        e1 = v1 / np.sqrt(v1 @ v1)
        u = v2 - e1 * (e1 @ v2)
        if u @ u <= DEGENERATE:
            return None
        e2 = u / np.sqrt(u @ u)
        return np.array([e1, e2, np.cross(e1, e2)]), res[CA]

    def point_of(res):
        return bool(np.isfinite(res[CA]).all() and (np.abs(res[CA]) <= CRD_MAX).all())

    for b in range(B):
        pres = [0 <= seq[b, i] < 20 for i in range(L)]
        frames = {i: frame_of(ref[b, i]) for i in range(L) if pres[i] and frame_of(ref[b, i]) is not None}
        points = [j for j in range(L) if pres[j] and point_of(ref[b, j])]
        total = {(i, j): 0.0 for i in frames for j in points}
        for k in range(K):
            mine = {i: frame_of(samples[b, k, i]) for i in frames}
            if any(f is None for f in mine.values()) or not all(point_of(samples[b, k, j]) for j in points):
                continue
            usable[b] += 1
            for i in frames:
                for j in points:
                    x_ref = frames[i][0] @ (ref[b, j, CA] - frames[i][1])
                    x_smp = mine[i][0] @ (samples[b, k, j, CA] - mine[i][1])
                    total[(i, j)] += float(np.sqrt(((x_smp - x_ref) ** 2).sum()))
        if usable[b] == 0 or not total:
            continue
        for (i, j), v in total.items():
            ae[b, i, j] = v / usable[b]
        n = len(points)
        stats[b, 0] = sum(total.values()) / usable[b] / len(total)
        stats[b, 1] = max(sum(1.0 / (1.0 + (ae[b, i, j] / d0_of(n)) ** 2) for j in points) / n for i in frames)
    return ae, stats, usable


def _fma32(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 numbers is exact in fp64."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _local32(E, t, p):
    """E [L, 3, 3], t [L, 3] fp32 frames, p [L, 3] fp32 points -> x [L, L, 3] fp32 as `backbone_frame::local_coords` rounds."""
    r = (p[None, :, :] - t[:, None, :]).astype(np.float32)                                     # one fp32 subtraction
    e = np.broadcast_to(E[:, None], (E.shape[0], p.shape[0], 3, 3))
    m = (e[..., 0] * r[..., 0, None]).astype(np.float32)                                       # __fmul_rn(e[0], rx)
    return _fma32(e[..., 2], r[..., 2, None], _fma32(e[..., 1], r[..., 1, None], m))


def emulate32(ref, samples, seq):
    """The kernel's arithmetic in numpy float32 -> ae [B, L, L] float32: fp64 frames rounded once, fp32 local coordinates, fp32
    difference, fp32 norm, fp32 sum over the usable samples in the order k = 0 .. K - 1, one fp32 division."""
    seq, B, L, K = _shape(ref, samples, seq)
    ref = np.asarray(ref, np.float32).reshape(B, L, SLOTS, 3)
    samples = np.asarray(samples, np.float32).reshape(B, K, L, SLOTS, 3)
    ae = np.full((B, L, L), np.nan, np.float32)
    for b in range(B):
        frame, point, ok = validity(ref[b].astype(np.float64), samples[b].astype(np.float64), seq[b])
        if not ok.any():
            continue
        with np.errstate(all="ignore"):
            E, _, _ = frames_of(ref[b].astype(np.float64))
            xr = _local32(E.astype(np.float32), ref[b][:, CA], ref[b][:, CA])
            acc = np.zeros((L, L), np.float32)
            for k in np.flatnonzero(ok):
                Es, _, _ = frames_of(samples[b, k].astype(np.float64))
                e = (_local32(Es.astype(np.float32), samples[b, k][:, CA], samples[b, k][:, CA]) - xr).astype(np.float32)
                sq = _fma32(e[..., 2], e[..., 2], _fma32(e[..., 1], e[..., 1], (e[..., 0] * e[..., 0]).astype(np.float32)))
                acc = (acc + np.sqrt(sq, dtype=np.float32)).astype(np.float32)
            d = (acc / np.float32(ok.sum())).astype(np.float32)
        ae[b] = np.where(frame[:, None] & point[None, :], d, np.float32(np.nan))
    return ae


# ---- structures the CPU and the GPU tests share
def hinge(crd, h, degrees=60.0, axis=(0.3, -0.5, 0.8)):
    """crd [L*14, 3] -> (the chain with residues >= h rotated about an axis through the C-alpha of h, the distance [L] of every
    C-alpha from that axis), fp64.  2 sin(30 deg) = 1: at 60 degrees a C-alpha moves by exactly its distance from the axis."""
    crd = np.asarray(crd, np.float64).reshape(-1, SLOTS, 3)
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(degrees)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    c = crd[h, CA]
    out = crd.copy()
    out[h:] = (crd[h:] - c) @ R.T + c
    rel = crd[:, CA] - c
    perp = np.linalg.norm(rel - np.outer(rel @ axis, axis), axis=1)
    return out.reshape(-1, 3), perp * 2.0 * np.sin(th / 2.0)


def moved_copy_slack(ref, n, extent):
    """What the fp64 definition itself may give for a rigidly moved copy of `ref` ([L*14, 3], n residues) that was ROUNDED TO FP32:
    such a copy is not a rigid image.  Every coordinate is off by at most u X, every atom by a = sqrt(3) u X.  C - CA = v1 and the
    rejection u2 of N - CA = v2 from it are off by 2 a and 2 a (1 + |v2| / |v1|), so e1 and e2 tilt by d1 = 2 a / |v1| and
    d2 = 2 a (1 + |v2| / |v1|) / |u2|, e3 = e1 x e2 by d1 + d2, the frame as a matrix by at most 2 (d1 + d2); a point at distance
    D from the frame's origin moves by that times D in the frame's coordinates, plus 2 a for the point and the origin themselves.
    -> the largest such figure over the frames of the protein (first order in u).  It is a bound on the REFERENCE's value for
    these inputs, added to `tol` where a test asserts that a moved copy gives zero."""
    r = np.asarray(ref, np.float64).reshape(-1, SLOTS, 3)[:n]
    a = np.sqrt(3.0) * 2.0 ** -24 * extent
    v1, v2 = r[:, C_SLOT] - r[:, CA], r[:, N_SLOT] - r[:, CA]
    l1 = np.linalg.norm(v1, axis=1)
    e1 = v1 / l1[:, None]
    u2 = np.linalg.norm(v2 - e1 * (e1 * v2).sum(1)[:, None], axis=1)
    tilt = 2.0 * (2.0 * a / l1 + 2.0 * a * (1.0 + np.linalg.norm(v2, axis=1) / l1) / u2)
    reach = np.linalg.norm(r[:, None, CA] - r[None, :, CA], axis=-1).max(1)
    return float((tilt * reach).max() + 2.0 * a)


def mirror(crd):
    return np.asarray(crd, np.float64) * np.array([1.0, 1.0, -1.0])


# ---- the cases of tests/test_gpu_aligned_error.py, built on the host so that tests/test_aligned_error_ref.py can hold
# `emulate32` against `reference` on every one of them before anything runs on a device
LENGTHS = (1, 3, 63, 64, 65, 129)
KS = (1, 3)
KINDS = ("noise", "identical", "rigid", "hinge", "mirror")
PAD_ID = 20
_cases = {}


def lens_of(L):
    """Three proteins per batch: a full row, one padded by a residue, one of at most five residues."""
    return [L, max(1, L - 1), min(L, 5)]


def make_case(L, K, kind="noise"):
    """-> dict(ref [3, L*14, 3], samples [3, K, L*14, 3] fp32, seq [3, L], extent, lens, want = `reference` of them, and for
    `hinge` the residue h and the analytic distances per protein); built once.  Slots a residue type does not have and padded
    residues hold NaN in both structures: they must never reach a result."""
    key = (L, K, kind)
    if key in _cases:
        return _cases[key]
    from ensemble_ref import atom_mask
    rng = np.random.default_rng(7000 + 10 * L + K)
    lens = lens_of(L)
    seq = np.full((3, L), PAD_ID, np.int64)
    ref = np.zeros((3, L * SLOTS, 3), np.float32)
    samples = np.zeros((3, K, L * SLOTS, 3), np.float32)
    moved = []
    for b, n in enumerate(lens):
        seq[b, :n] = rng.integers(0, 20, n)
        ref[b, :n * SLOTS] = random_chain(rng, seq[b, :n])
        r64 = ref[b].astype(np.float64)
        h, dist = n // 2, None
        for k in range(K):
            R, t = random_rigid(rng)
            if kind == "identical":
                s = r64
            elif kind == "rigid":
                s = r64 @ R.T + t
            elif kind == "hinge":
                s, dist = hinge(r64, h)
            elif kind == "mirror":
                s = mirror(r64)
            else:
                s = r64 @ R.T + t + rng.normal(0, 1.5, r64.shape)
            samples[b, k] = s.astype(np.float32)
        moved.append((h, dist))
    have = np.array([atom_mask(seq[b]).reshape(-1) for b in range(3)])                       # [3, L*14]
    extent = extent_of(ref[have], samples[np.repeat(have[:, None], K, 1)])
    ref[~have] = np.nan
    samples[~np.repeat(have[:, None], K, 1)] = np.nan
    case = dict(ref=ref, samples=samples, seq=seq, extent=extent, lens=lens, hinge=moved, K=K, L=L)
    case["want"] = reference(ref, samples, seq)
    _cases[key] = case
    return case


def spoiled(case, what):
    """A copy of a `noise` case with one thing wrong in protein 0 (and, for `all_samples`, in every protein):
      ref_n_nan, ref_ca_nan, ref_degenerate   residue 1 of the reference: N = NaN; CA = NaN; C = CA;
      smp_n_nan, smp_ca_huge, smp_c_nan, smp_degenerate   the same residue of sample 0: NaN / 1e19 / C = CA;
      smp_side_chain  a NaN in a side-chain slot of sample 0 (changes nothing);
      all_samples     a NaN C-alpha in every sample of every protein.
    -> (ref, samples, seq) fp32 copies.  Needs L >= 3."""
    ref, samples, seq = case["ref"].copy(), case["samples"].copy(), case["seq"]
    r3, s4 = ref.reshape(3, -1, SLOTS, 3), samples.reshape(3, samples.shape[1], -1, SLOTS, 3)
    i = 1
    if what == "ref_n_nan":
        r3[0, i, N_SLOT, 1] = np.nan
    elif what == "ref_ca_nan":
        r3[0, i, CA, 0] = np.nan
    elif what == "ref_degenerate":
        r3[0, i, C_SLOT] = r3[0, i, CA]
    elif what == "smp_n_nan":
        s4[0, 0, i, N_SLOT, 2] = np.nan
    elif what == "smp_ca_huge":
        s4[0, 0, i, CA, 0] = 1.0e19
    elif what == "smp_c_nan":
        s4[0, 0, i, C_SLOT, 1] = np.nan
    elif what == "smp_degenerate":
        s4[0, 0, i, C_SLOT] = s4[0, 0, i, CA]
    elif what == "smp_side_chain":
        s4[0, 0, 0, 4:, :] = np.nan
    elif what == "all_samples":
        s4[:, :, 0, CA, 0] = np.nan
    else:
        raise KeyError(what)
    return ref, samples, seq


SPOILS = ("ref_n_nan", "ref_ca_nan", "ref_degenerate", "smp_n_nan", "smp_ca_huge", "smp_c_nan", "smp_degenerate", "smp_side_chain",
          "all_samples")
