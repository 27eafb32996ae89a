"""fp64 numpy restatement of the side-chain accuracy metric (include/ptamd.h, `ptamd_sidechain`), for tests/test_sidechain_ref.py,
tests/test_gpu_sidechain.py and tests/test_score_cli.py.  TEST INFRASTRUCTURE ONLY: the product never imports it.

Two forms of the same definition: `reference` (vectorised over the residues of a protein) and `reference_loops` (a plain loop over
residue, chi and atom), which the CPU test holds against each other.  Both work on the fp32 inputs the kernel gets, in fp64.

THE BOUND ON THE FP32 DIHEDRAL (EPS_CHI, degrees).  u = 2^-24.  Conditions, asserted by `well_posed` on prediction and truth of
every case: coordinates within +-64 A, bonds of 1 .. 2 A, bond angles of 60 .. 150 degrees (sin >= 1/2) along every scored chi.
  * a bond vector b = p' - p of two fp32 points: one rounding, relative error u per component (whatever the coordinates are);
  * a component of n = b x b' is a b - c d: the inputs carry 2 u, a product u, the difference u, so its error is at most
    4 u (|a b| + |c d|) <= 4 u |b| |b'|, the vector's at most 4 sqrt(3) u |b| |b'| = 4 sqrt(3) u |n| / sin <= 13.9 u |n|;
  * x = n1 . n2: 2 * 13.9 u from the normals and 3 u from the three-term dot product: at most 31 u |n1| |n2|;
  * y = |b2| (b1 . n2): b1 . n2 is off by at most (1 + 13.9 + 3) u |b1| |n2|, |b2| by 3 u (three squares, a sum, a root),
    the product by u: at most 22 u |b1| |b2| |n2| = 22 u |n1| |n2| / sin <= 44 u |n1| |n2|;
  * (x, y) has length |n1| |n2|, so its direction is off by at most sqrt(31^2 + 44^2) u <= 54 u radians, and atan2f returns it
    within 4 ulp of a value below pi (ulp = 2^-22): 16 u.  One chi: 70 u radians;
  * Delta = |chi_p - chi_t| wrapped: two chi, the subtraction and the wrap 2 pi - d at 4 u each (half an ulp of a value below
    2 pi): 148 u radians; the conversion to degrees and, for chi_mae, the rounding of the mean: 2 u + 2 u relative to 180.
EPS_CHI = 148 u (180 / pi) + 4 u 180 = 5.5e-4 degrees.  A fused multiply-add in place of a product and a sum only removes a
rounding.  The symmetric fold min(D, 180 - D) adds a subtraction from 180: one more u 180, inside the 4 u 180 above for per_res.

THE BOUND ON THE LOCAL-FRAME RMSD (EPS_RMS, Angstrom).  The frame's rows are unit vectors rounded once from fp64 (u each); r = p -
CA carries u; a local coordinate e . r is three multiply-adds: at most (1 + 1 + 3) u |r| sqrt(3) <= 9 u |r|; the difference of
the two structures' local coordinates 18 u |r| + u |r|; the root of a mean of squares is off by at most the largest component
error times sqrt(3) (triangle inequality), plus u of itself for the sum, the division and the root, 4 u: with |r| <= R_MAX = 16 A
(`well_posed` asserts it) EPS_RMS = (19 sqrt(3) + 4) u R_MAX = 3.6e-5 A.  A prediction equal to the truth gives exactly 0.

Under `well_posed` (no Delta within EPS_CHI of the threshold, no true |n|^2 or frame |v|^2 within a factor 4 of 1e-8) the counts
are exact: that is the condition under which the GPU test demands equality."""
import math

import numpy as np

from rename_ref import PAD_ID, SLOTS, SWAPS

AA = "ACDEFGHIKLMNPQRSTVWY"
NSC = (1, 2, 4, 5, 7, 0, 6, 4, 5, 4, 4, 4, 3, 5, 7, 2, 3, 3, 10, 8)        # side-chain atoms per type (csrc/nerf_tables.h)
NCHI = (0, 1, 2, 3, 2, 0, 2, 2, 4, 2, 3, 2, 2, 3, 4, 1, 1, 1, 2, 2)
CHI_SLOTS = ((0, 1, 4, 5), (1, 4, 5, 6), (4, 5, 6, 7), (5, 6, 7, 8))
SYM_CHI = {r: col - 6 for r, (_, col) in SWAPS.items()}                       # type -> k of the chi with interchangeable far atoms
DEGENERATE = 1.0e-8
U = 2.0 ** -24
EPS_CHI = 148 * U * 180 / math.pi + 4 * U * 180
R_MAX = 16.0
EPS_RMS = (19 * math.sqrt(3) + 4) * U * R_MAX
SCORES = ("chi1", "chi12", "chi_mae", "sc_rmsd")


def dihedral(p0, p1, p2, p3):
    """[..., 3] fp64 each -> (chi in radians, |n1|^2, |n2|^2)."""
    b1, b2, b3 = p1 - p0, p2 - p1, p3 - p2
    n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
    y = np.linalg.norm(b2, axis=-1) * (b1 * n2).sum(-1)
    return np.arctan2(y, (n1 * n2).sum(-1)), (n1 * n1).sum(-1), (n2 * n2).sum(-1)


def frames(n, ca, c):
    """Algorithm 21: [..., 3] fp64 each -> (R [..., 3, 3] with rows e1, e2, e3, |v1|^2, |u2|^2)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        v1, v2 = c - ca, n - ca
        q1 = (v1 * v1).sum(-1)
        e1 = v1 / np.sqrt(q1)[..., None]
        u2 = v2 - e1 * (e1 * v2).sum(-1)[..., None]
        q2 = (u2 * u2).sum(-1)
        e2 = u2 / np.sqrt(q2)[..., None]
    return np.stack([e1, e2, np.cross(e1, e2)], axis=-2), q1, q2


def wrap_deg(d):
    """|difference of two angles| in radians -> degrees in [0, 180]"""
    d = np.abs(d)
    return np.degrees(np.where(d > math.pi, 2 * math.pi - d, d))


def reference(pred, truth, seq, threshold=40.0):
    """One protein: pred, truth [L*14, 3] fp32, seq [L] -> dict(score [4], counts [12] int, per_res [L, 5], bad, scored [L, 4],
    counted [L], delta [L, 4], d2 [L], chi_pred / chi_true [L, 4], margins: the quantities `well_posed` looks at)."""
    L = len(seq)
    seq = np.asarray(seq)
    p, t = np.asarray(pred, np.float64).reshape(L, SLOTS, 3), np.asarray(truth, np.float64).reshape(L, SLOTS, 3)
    known = (seq >= 0) & (seq < 20)
    typ = np.where(known, seq, 0)
    nchi, nsc = np.where(known, np.array(NCHI)[typ], 0), np.where(known, np.array(NSC)[typ], 0)
    delta, scored = np.full((L, 4), np.nan), np.zeros((L, 4), bool)
    chi_p, chi_t, nsq = np.full((L, 4), np.nan), np.full((L, 4), np.nan), np.full((L, 4, 2), np.nan)
    bad = np.zeros(L, bool)
    with np.errstate(invalid="ignore"):
        for k, sl in enumerate(CHI_SLOTS):
            ct, q1, q2 = dihedral(*(t[:, s] for s in sl))
            cp, _, _ = dihedral(*(p[:, s] for s in sl))
            ok = (nchi > k) & ~np.isnan(t[:, sl]).any((1, 2)) & (q1 > DEGENERATE) & (q2 > DEGENERATE)
            d = wrap_deg(cp - ct)
            sym = np.array([SYM_CHI.get(int(s)) == k + 1 for s in typ]) & known
            d = np.where(sym, np.minimum(d, 180.0 - d), d)
            scored[:, k], delta[:, k] = ok, np.where(ok & np.isfinite(p[:, sl]).all((1, 2)), d, np.nan)
            chi_p[:, k], chi_t[:, k] = cp, ct
            nsq[:, k, 0], nsq[:, k, 1] = np.where(nchi > k, q1, np.nan), np.where(nchi > k, q2, np.nan)
            bad |= ok & ~np.isfinite(p[:, sl]).all((1, 2))
    hit = scored & (delta <= threshold)
    # the side chain in the residue's own frame
    Rt, t1, t2 = frames(t[:, 0], t[:, 1], t[:, 2])
    Rp, p1, p2 = frames(p[:, 0], p[:, 1], p[:, 2])
    slot = np.arange(SLOTS)[None, :]
    sc = (slot >= 4) & (slot < 4 + nsc[:, None])                                  # [L, 14]: the side-chain slots of the type
    with np.errstate(invalid="ignore"):
        counted = (nsc > 0) & ~(np.isnan(t).any(-1) & (sc | (slot < 3))).any(1) & (t1 > DEGENERATE) & (t2 > DEGENERATE)
        usable = np.isfinite(p).all(-1) | ~(sc | (slot < 3))
        pred_ok = usable.all(1) & (p1 > DEGENERATE) & (p2 > DEGENERATE)
        xt = np.einsum("lij,lsj->lsi", Rt, t - t[:, 1:2])
        perm = np.tile(np.arange(SLOTS), (L, 1))
        for r in np.nonzero(known)[0]:
            for a, b in SWAPS.get(int(seq[r]), ((), 0))[0]:
                perm[r, [a, b]] = b, a
        xp = np.einsum("lij,lsj->lsi", Rp, p - p[:, 1:2])
        xo = np.take_along_axis(xp, perm[:, :, None], axis=1)
        plain = np.where(sc, ((xp - xt) ** 2).sum(-1), 0.0).sum(1)
        other = np.where(sc, ((xo - xt) ** 2).sum(-1), 0.0).sum(1)
        d2 = np.where(counted & pred_ok, np.minimum(plain, other), np.nan)
        reach = np.where(sc & counted[:, None], np.maximum(np.linalg.norm(t - t[:, 1:2], axis=-1), np.linalg.norm(p - p[:, 1:2], axis=-1)), 0.0)
    bad |= counted & ~pred_ok
    rms = np.where(counted, np.sqrt(d2 / np.maximum(nsc, 1)), np.nan)
    per_res = np.concatenate([delta, rms[:, None]], axis=1)
    any_bad = bool(bad.any())
    counts = np.zeros(12, np.int64)
    for k in range(4):
        counts[2 * k], counts[2 * k + 1] = scored[:, k].sum(), 0 if any_bad else hit[:, k].sum()
    both = scored[:, 0] & scored[:, 1]
    counts[8], counts[9] = both.sum(), 0 if any_bad else (both & hit[:, 0] & hit[:, 1]).sum()
    counts[10], counts[11] = counted.sum(), nsc[counted].sum()
    score = np.full(4, np.nan)
    if not any_bad:
        nscored = scored.sum()
        score[0] = hit[:, 0].sum() / counts[0] if counts[0] else np.nan
        score[1] = (both & hit[:, 0] & hit[:, 1]).sum() / counts[8] if counts[8] else np.nan
        score[2] = delta[scored].sum() / nscored if nscored else np.nan
        score[3] = math.sqrt(d2[counted].sum() / counts[11]) if counts[11] else np.nan
    return dict(score=score, counts=counts, per_res=per_res, bad=any_bad, scored=scored, counted=counted, delta=delta, d2=d2,
                chi_pred=chi_p, chi_true=chi_t, hit=hit, nsq=nsq, frame_sq=np.stack([t1, t2], 1), nsc=nsc, reach=reach)


def reference_loops(pred, truth, seq, threshold=40.0):
    """The same numbers by plain loops over residue, chi and atom: (score [4], counts [12], per_res [L, 5])."""
    L = len(seq)
    p, t = np.asarray(pred, np.float64).reshape(L, SLOTS, 3), np.asarray(truth, np.float64).reshape(L, SLOTS, 3)
    per_res = np.full((L, 5), np.nan)
    c = [0] * 12
    sum_delta = sum_d2 = 0.0
    bad = False

    def one_dihedral(x, sl):
        b1, b2, b3 = x[sl[1]] - x[sl[0]], x[sl[2]] - x[sl[1]], x[sl[3]] - x[sl[2]]
        n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
        return math.atan2(math.sqrt(b2 @ b2) * (b1 @ n2), n1 @ n2), n1 @ n1, n2 @ n2

    def one_frame(x):
        v1, v2 = x[2] - x[1], x[0] - x[1]
        q1 = v1 @ v1
        if not q1 > DEGENERATE:
            return None
        e1 = v1 / math.sqrt(q1)
        u2 = v2 - e1 * (e1 @ v2)
        q2 = u2 @ u2
        if not q2 > DEGENERATE:
            return None
        e2 = u2 / math.sqrt(q2)
        return np.stack([e1, e2, np.cross(e1, e2)])

    for r in range(L):
        s = int(seq[r])
        if s < 0 or s > 19:
            continue
        hits = []
        for k in range(NCHI[s]):
            sl = CHI_SLOTS[k]
            if np.isnan(t[r, sl]).any():
                continue
            ct, q1, q2 = one_dihedral(t[r], sl)
            if not (q1 > DEGENERATE and q2 > DEGENERATE):
                continue
            c[2 * k] += 1
            if not np.isfinite(p[r, sl]).all():
                bad = True
                hits.append((k, False))
                continue
            cp = one_dihedral(p[r], sl)[0]
            d = abs(cp - ct)
            d = math.degrees(2 * math.pi - d if d > math.pi else d)
            if SYM_CHI.get(s) == k + 1:
                d = min(d, 180.0 - d)
            per_res[r, k] = d
            sum_delta += d
            hits.append((k, d <= threshold))
            c[2 * k + 1] += d <= threshold
        got = dict(hits)
        if 0 in got and 1 in got:
            c[8] += 1
            c[9] += got[0] and got[1]
        n = NSC[s]
        atoms = list(range(4, 4 + n))
        if n == 0 or np.isnan(t[r, [0, 1, 2] + atoms]).any():
            continue
        Rt = one_frame(t[r])
        if Rt is None:
            continue
        c[10] += 1
        c[11] += n
        Rp = one_frame(p[r]) if np.isfinite(p[r, [0, 1, 2] + atoms]).all() else None
        if Rp is None:
            bad = True
            continue
        partner = {a: a for a in atoms}
        for a, b in SWAPS.get(s, ((), 0))[0]:
            partner[a], partner[b] = b, a
        plain = other = 0.0
        for a in atoms:
            xt = Rt @ (t[r, a] - t[r, 1])
            plain += ((Rp @ (p[r, a] - p[r, 1]) - xt) ** 2).sum()
            other += ((Rp @ (p[r, partner[a]] - p[r, 1]) - xt) ** 2).sum()
        d2 = min(plain, other)
        per_res[r, 4] = math.sqrt(d2 / n)
        sum_d2 += d2
    nscored = c[0] + c[2] + c[4] + c[6]
    score = np.full(4, np.nan)
    if bad:
        c[1] = c[3] = c[5] = c[7] = c[9] = 0
    else:
        score[0] = c[1] / c[0] if c[0] else np.nan
        score[1] = c[9] / c[8] if c[8] else np.nan
        score[2] = sum_delta / nscored if nscored else np.nan
        score[3] = math.sqrt(sum_d2 / c[11]) if c[11] else np.nan
    return score, np.array(c, np.int64), per_res


# ------------------------------------------------------------------------------------------------ when the counts are exact
def bond_geometry(x, seq, scored):
    """(shortest bond, longest bond, smallest and largest bond angle in degrees) along the scored chi of x [L, 14, 3] fp64."""
    bonds, angles = [], []
    for r, k in zip(*np.nonzero(scored)):
        pts = x[r, list(CHI_SLOTS[k])]
        b = np.diff(pts, axis=0)
        bonds += list(np.linalg.norm(b, axis=1))
        for i in range(2):
            cosv = -(b[i] @ b[i + 1]) / (np.linalg.norm(b[i]) * np.linalg.norm(b[i + 1]))
            angles.append(math.degrees(math.acos(max(-1.0, min(1.0, cosv)))))
    if not bonds:
        return 1.5, 1.5, 109.0, 109.0
    return min(bonds), max(bonds), min(angles), max(angles)


def well_posed(pred, truth, seq, threshold=40.0, name=""):
    """Assert the conditions of the module docstring on one protein; returns its `reference`."""
    ref = reference(pred, truth, seq, threshold)
    L = len(seq)
    d = ref["delta"][ref["scored"]]
    d = d[np.isfinite(d)]
    assert not (np.abs(d - threshold) <= EPS_CHI).any(), (name, "a Delta within EPS_CHI of the threshold")
    for q in (ref["nsq"], ref["frame_sq"][(np.asarray(seq) >= 0) & (np.asarray(seq) < 20) & (ref["nsc"] > 0)]):
        q = q[np.isfinite(q)]
        assert not ((q > DEGENERATE / 4) & (q < DEGENERATE * 4)).any(), (name, "a |n|^2 or |v|^2 within a factor 4 of 1e-8")
    for which, x in (("pred", pred), ("truth", truth)):
        x = np.asarray(x, np.float64).reshape(L, SLOTS, 3)
        live = ref["scored"] & np.isfinite(x[:, :9]).all((1, 2))[:, None]
        lo, hi, amin, amax = bond_geometry(x, seq, live)
        assert 1.0 <= lo and hi <= 2.0 and 60.0 <= amin and amax <= 150.0, (name, which, lo, hi, amin, amax)
        used = x[np.isfinite(x).all(-1) & (np.asarray(seq) != PAD_ID)[:, None]]
        assert used.size == 0 or np.abs(used).max() <= 64.0, (name, which, "coordinates beyond 64 A")
    assert ref["reach"][np.isfinite(ref["reach"])].max(initial=0.0) <= R_MAX, (name, "a side-chain atom farther than R_MAX from its C-alpha")
    return ref


# ------------------------------------------------------------------------------------------------------------ case builders
def build(seq, ang):
    """[L*14, 3] fp64 coordinates of seq (ids) from ang [L, 12] radians, by the oracle's NeRF in fp64; slots a residue type does
    not have are NaN.  The chain is built behind one more residue (an ALA) that is then dropped: the build hangs the CB of its
    FIRST residue on other parents (csrc/nerf_tables.h), with an N-CA-CB angle that depends on a torsion, and needs two residues."""
    import torch
    from oracle import batched
    seq = np.asarray(seq)
    lead = np.array([[-1.05, -0.75, math.pi, 1.94, 2.03, 2.12, -2.1, 0, 0, 0, 0, 0]])
    ang, ids = np.concatenate([lead, np.asarray(ang, np.float64)]), np.concatenate([[0], seq])
    crd = batched.generate_coords_batched(torch.as_tensor(ang)[None], torch.as_tensor(ids)[None], torch.float64)
    crd = crd[0].numpy().reshape(len(ids), SLOTS, 3)[1:].copy()
    for r, s in enumerate(seq):
        crd[r, 4 + NSC[int(s)]:] = np.nan
    return crd.reshape(-1, 3)


def angles(L, seed, chi=None):
    """Angles of a random coil (phi and psi uniform: 129 residues stay within +-64 A of their centre, which `well_posed`
    asserts), random chi; `chi` [L, 4] overrides columns 7 .. 10 (chi1 .. chi4)."""
    rng = np.random.default_rng(seed)
    a = np.zeros((L, 12))
    a[:, 0], a[:, 1], a[:, 2] = rng.uniform(-3.1, 3.1, L), rng.uniform(-3.1, 3.1, L), rng.normal(math.pi, 0.03, L)
    a[:, 3], a[:, 4], a[:, 5] = rng.normal(1.94, 0.03, L), rng.normal(2.03, 0.03, L), rng.normal(2.12, 0.03, L)
    a[:, 6] = rng.normal(-2.1, 0.05, L)            # where CB goes: the torsion (C', N, CA, CB) of an L amino acid
    a[:, 7:] = rng.uniform(-3.1, 3.1, (L, 5))
    if chi is not None:
        a[:, 7:11] = chi
    return a


def centred(crd):
    return crd - np.nanmean(crd, axis=0, keepdims=True)


def rigid(crd, seed):
    """crd rotated by a random proper rotation and shifted by a few Angstrom."""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return crd @ q.T + rng.normal(0, 3.0, 3)


def swap_symmetric(crd, seq, types=None):
    """The symmetric slots of `types` (default: ASP, GLU, PHE, TYR) exchanged - or, for any other type listed in `types` with at
    least four side-chain atoms, its slots 6 and 7 (LEU CD1 / CD2 ...; VAL: 5 and 6)."""
    out = np.array(crd).reshape(len(seq), SLOTS, 3).copy()
    for r, s in enumerate(seq):
        s = int(s)
        if types is None and s not in SWAPS:
            continue
        if types is not None and s not in types:
            continue
        pairs = SWAPS[s][0] if s in SWAPS else (((5, 6),) if NSC[s] == 3 else ((6, 7),))
        for a, b in pairs:
            out[r, [a, b]] = out[r, [b, a]]
    return out.reshape(-1, 3)


ALL_TYPES = np.arange(20)


def pair_case(L, seed, spread=0.5):
    """(pred, truth, seq) fp32 / int64 of one protein of L residues that cycles through all twenty types: the truth from random
    chi, the prediction from chi moved by a normal of `spread` radians (so that hits and misses both occur) and its backbone
    angles by a little, then rigidly moved."""
    rng = np.random.default_rng(seed)
    seq = (np.arange(L) + seed) % 20
    a = angles(L, seed)
    b = a.copy()
    b[:, 7:] += rng.normal(0, spread, (L, 5))
    b[:, :6] += rng.normal(0, 0.01, (L, 6))
    truth = centred(build(seq, a))
    pred = rigid(centred(build(seq, b)), seed + 1)
    return pred.astype(np.float32), truth.astype(np.float32), seq.astype(np.int64)


def batch_of(items, L_pad=None):
    """[(pred, truth, seq)] -> (pred [B, Lp*14, 3], truth, seq [B, Lp]): rows padded with PAD_ID, zeros in the truth (what the
    data loader leaves there) and a poison in the prediction that no result may depend on."""
    Lp = max(len(s) for _, _, s in items) if L_pad is None else L_pad
    B = len(items)
    pred = np.full((B, Lp * SLOTS, 3), 7.5e3, np.float32)
    truth = np.zeros((B, Lp * SLOTS, 3), np.float32)
    seq = np.full((B, Lp), PAD_ID, np.int64)
    for b, (p, t, s) in enumerate(items):
        n = len(s)
        pred[b, :n * SLOTS], truth[b, :n * SLOTS], seq[b, :n] = p, t, s
    return pred, truth, seq


# ------------------------------------------------------------------------------------------------ the cases of the GPU test
SIZES = (1, 63, 64, 65, 128, 129)


def first_of(seq, types, start=0):
    """The first residue at or behind `start` whose type is in `types` (None without one)."""
    hit = [r for r in range(start, len(seq)) if int(seq[r]) in types]
    return hit[0] if hit else None


def with_gaps(item):
    """The truth of a protein with, where it is long enough to have such residues: a NaN on each of the four atoms of a chi2 in
    turn (four residues with two chi or more), a NaN on the last side-chain atom of a LYS (its chi4 and its RMSD go, chi1 .. chi3
    stay), a missing C (the chi stay, the RMSD goes), and an unknown residue id 21.  Returns (item, notes)."""
    pred, truth, seq = (x.copy() for x in item)
    t = truth.reshape(len(seq), SLOTS, 3)
    notes = {}
    two = [r for r in range(len(seq)) if NCHI[int(seq[r])] >= 2]
    for j, r in enumerate(two[:4]):
        t[r, CHI_SLOTS[1][j], j % 3] = np.nan
        notes[f"chi2-atom{j}"] = r
    r = first_of(seq, (8,), start=two[3] + 1 if len(two) >= 4 else len(seq))
    if r is not None:
        t[r, 8, 0] = np.nan
        notes["lys-nz"] = r
        r2 = first_of(seq, (8, 14, 3, 10), start=r + 1)
        if r2 is not None:
            t[r2, 2, 1] = np.nan
            notes["no-c"] = r2
            if r2 + 1 < len(seq):
                seq[r2 + 1] = 21
                notes["id21"] = r2 + 1
    return (pred, truth, seq), notes


def sparse_case(L, at, seed):
    """A protein of GLY and ALA with one LYS at residue `at`: the only scored chi of the protein."""
    pred, truth, seq = pair_case(L, seed)
    seq = np.where(np.arange(L) % 2 == 0, 5, 0).astype(np.int64)
    seq[at] = 8
    a = angles(L, seed)
    b = a.copy()
    b[:, 7:] += 0.4
    truth = centred(build(seq, a)).astype(np.float32)
    pred = rigid(centred(build(seq, b)), seed).astype(np.float32)
    return pred, truth, seq


def empty_row():
    return np.zeros((SLOTS, 3), np.float32), np.zeros((SLOTS, 3), np.float32), np.full(1, PAD_ID, np.int64)


_CASES = {}


def gpu_cases():
    """name -> (items, L_pad): every L of SIZES alone (B = 1) and in a batch of three whose rows have different true lengths and
    whose last row is all pad; the proteins cycle through all twenty types and carry the gaps of `with_gaps`; then the proteins
    whose only scored chi sits in tile 0, in tile 1 and on the last residue of a row of 129, and the unusable predictions."""
    if _CASES:
        return _CASES
    for L in SIZES:
        whole, _ = with_gaps(pair_case(L, 100 + L))
        _CASES[f"single-{L}"] = ([whole], L)
        short, _ = with_gaps(pair_case(max(1, L // 2), 200 + L))
        _CASES[f"batch-{L}"] = ([whole, short, empty_row()], L)
    _CASES["only-chi"] = ([sparse_case(129, 3, 301), sparse_case(129, 100, 302), sparse_case(129, 128, 303)], 129)
    base = [pair_case(65, 410 + i) for i in range(3)]
    p = base[1][0].copy()
    r = first_of(base[1][2], (8,))
    p[r * SLOTS + 6, 1] = np.nan                                  # CD of a LYS: on chi2, chi3, chi4 and in its RMSD
    _CASES["nonfinite-1-of-3"] = ([base[0], (p, base[1][1], base[1][2]), base[2]], 65)
    small = [pair_case(6, 500 + i) for i in range(3)]
    p0, p2 = small[0][0].copy(), small[2][0].copy()
    p0[0 * SLOTS + 0, 0] = np.inf                                 # an N: on chi1 and in the frame (residue 0 of seed 500 is not GLY)
    r = first_of(small[2][2], tuple(s for s in range(20) if NSC[s] > 0))
    p2[r * SLOTS + 2] = p2[r * SLOTS + 1]                         # C on CA: finite, and no frame
    _CASES["unusable-frames"] = ([(p0, small[0][1], small[0][2]), small[1], (p2, small[2][1], small[2][2])], 6)
    for name, (items, _) in _CASES.items():
        for b, (pred, truth, seq) in enumerate(items):
            well_posed(pred, truth, seq, name=f"{name}[{b}]")
    return _CASES
