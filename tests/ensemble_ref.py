"""fp64 numpy restatement of the superposed ensemble spread (include/ptamd.h, `ptamd_ensemble_spread`), for
tests/test_ensemble_ref.py, tests/test_gpu_ensemble.py and tests/test_gpu_predict.py.  TEST INFRASTRUCTURE ONLY: the product never
imports it.

Two forms of the same definition: `reference` (vectorised over the samples, residues and atoms of a protein) and
`reference_loops` (a plain loop over protein, sample, residue and atom), which the CPU test holds against each other.  Both work
on the fp32 inputs the kernel gets, in fp64; the fit is an SVD with the determinant correction (Kabsch), where the kernel takes
Horn's quaternion - two routes to the one minimiser.

THE BOUND ON THE FP32 RESULTS.  u = 2^-24, eps32 = 2 u, X = the largest |coordinate| of the reference and the samples.  The inputs
are exact in fp32 and the moments are fp64 (the fitted (R, t) is within 1e-12 X of the minimiser: five orders below what
follows), so the error comes from applying (R, t) and summing squares in fp32.  Per component c of e = R s + t - r:
  * the nine entries of R, |R_ij| <= 1, are rounded to fp32 once: u each, times |s_x| + |s_y| + |s_z| <= 3 X: 3 u X;
  * t = rbar - R sbar has |t_c| <= (1 + sqrt 3) X and is rounded once: 2.74 u X;
  * three fused multiply-adds, every intermediate at most |t_c| + 3 X = 5.74 X: 17.2 u X;
  * the subtraction of r_c, its result at most 6.74 X: 6.74 u X;
together 29.7 u X per component, 29.7 sqrt(3) u X = 25.7 eps32 X on the vector e.  rmsd, rmsf[..., 0] and rmsf[..., 1] are
weighted root mean squares of such vectors with weights that sum to 1 (1 / n_b; 1 / K'; 1 / (K' |A_ki|)), so by the triangle
inequality each moves by at most the largest error of a vector: ABS_MULT = 32 >= 25.7 multiples of eps32 X.  RELATIVE to the
result come: the three-term fp32 sum of squares (3 u on d^2, 1.5 u on its root), the fp32 sum over at most 14 atoms (14 u on the
sum, 7 u on the root), the final rounding to fp32 (u); the fp64 sums and the fp64 root add nothing visible: 9.5 u = 4.75 eps32 <
REL_MULT = 8 multiples of eps32.  So |gpu - ref| <= tol(ref, X) = ABS_MULT eps32 X + REL_MULT eps32 ref.

A root near zero amplifies an error of its square, so the tests compare the SQUARES: |gpu^2 - ref^2| = |gpu - ref| (gpu + ref)
<= tol_sq(ref, X) = tol (2 ref + tol), whose absolute term at ref = 0 is the square of the bound on the root."""
import numpy as np

AA = "ACDEFGHIKLMNPQRSTVWY"
NSC = (1, 2, 4, 5, 7, 0, 6, 4, 5, 4, 4, 4, 3, 5, 7, 2, 3, 3, 10, 8)        # side-chain atoms per type (csrc/nerf_tables.h)
PAD_ID = 20
SLOTS = 14
CA = 1
EPS32 = 2.0 ** -23
ABS_MULT = 32.0
REL_MULT = 8.0


def tol(ref, extent):
    """Bound on |gpu - ref| of rmsd / rmsf values (module docstring); `extent` = the largest finite |coordinate|."""
    return ABS_MULT * EPS32 * extent + REL_MULT * EPS32 * np.abs(ref)


def tol_sq(ref, extent):
    """Bound on |gpu^2 - ref^2|."""
    t = tol(ref, extent)
    return t * (2.0 * np.abs(ref) + t)


def extent_of(*arrays):
    return max(float(np.abs(a[np.isfinite(a)]).max()) for a in arrays)


def present_of(seq):
    seq = np.asarray(seq)
    return (seq >= 0) & (seq < 20)


def atom_mask(seq):
    """[L] ids -> bool [L, 14]: the slots a present residue's type has."""
    seq = np.asarray(seq)
    nsc = np.array(NSC + (0,))[np.where(present_of(seq), seq, 20)]
    return present_of(seq)[:, None] & (np.arange(SLOTS)[None, :] < 4 + nsc[:, None])


def kabsch(s, r):
    """s, r [n, 3] fp64 -> (R [3, 3], t [3]): the proper rotation and translation minimising sum |R s_i + t - r_i|^2."""
    sb, rb = s.mean(0), r.mean(0)
    U, _, Vt = np.linalg.svd((s - sb).T @ (r - rb))
    d = np.sign(np.linalg.det(Vt.T @ U.T))
    R = Vt.T @ np.diag([1.0, 1.0, d if d != 0 else 1.0]) @ U.T
    return R, rb - R @ sb


def reference(ref, samples, seq):
    """ref [B, L*14, 3], samples [B, K, L*14, 3] (fp32), seq [B, L] -> (rmsd [B, K], rmsf [B, L, 2], usable [B]) in fp64."""
    seq = np.asarray(seq)
    B, L = seq.shape
    K = samples.shape[1]
    ref = np.asarray(ref, np.float64).reshape(B, L, SLOTS, 3)
    samples = np.asarray(samples, np.float64).reshape(B, K, L, SLOTS, 3)
    rmsd = np.full((B, K), np.nan)
    rmsf = np.full((B, L, 2), np.nan)
    usable = np.zeros(B, np.int64)
    for b in range(B):
        pres = present_of(seq[b])
        n = int(pres.sum())
        r, s = ref[b], samples[b]
        ok = np.isfinite(s[:, pres, CA]).all((1, 2)) & bool(np.isfinite(r[pres, CA]).all()) & (n >= 3)
        usable[b] = ok.sum()
        if not ok.any():
            continue
        s = s[ok]                                                                  # [K', L, 14, 3]
        sb, rb = s[:, pres, CA].mean(1), r[pres, CA].mean(0)
        H = np.einsum("kni,nj->kij", s[:, pres, CA] - sb[:, None], r[pres, CA] - rb)
        U, _, Vt = np.linalg.svd(H)
        V, Ut = Vt.transpose(0, 2, 1), U.transpose(0, 2, 1)
        d = np.sign(np.linalg.det(V @ Ut))
        D = np.zeros((len(s), 3, 3))
        D[:, 0, 0] = D[:, 1, 1] = 1.0
        D[:, 2, 2] = np.where(d != 0, d, 1.0)
        R = V @ D @ Ut
        t = rb - np.einsum("kij,kj->ki", R, sb)
        with np.errstate(invalid="ignore", divide="ignore"):
            e = np.einsum("kij,klaj->klai", R, s) + t[:, None, None] - r
            d2 = (e * e).sum(-1)                                                   # [K', L, 14]
            rmsd[b, ok] = np.sqrt(d2[:, pres, CA].mean(1))
            fin = atom_mask(seq[b])[None] & np.isfinite(s).all(-1) & np.isfinite(r).all(-1)[None]
            term = np.where(fin, d2, 0.0).sum(-1) / fin.sum(-1)                    # [K', L]; 0 / 0 = NaN: no atom left
            rmsf[b, pres, 0] = np.sqrt(d2[:, pres, CA].mean(0))
            rmsf[b, pres, 1] = np.sqrt(term[:, pres].mean(0))
    return rmsd, rmsf, usable


def reference_loops(ref, samples, seq):
    """The same definition as plain loops over protein, sample, residue and atom."""
    seq = np.asarray(seq)
    B, L = seq.shape
    K = samples.shape[1]
    ref = np.asarray(ref, np.float64).reshape(B, L, SLOTS, 3)
    samples = np.asarray(samples, np.float64).reshape(B, K, L, SLOTS, 3)
    rmsd = np.full((B, K), np.nan)
    rmsf = np.full((B, L, 2), np.nan)
    usable = np.zeros(B, np.int64)
    for b in range(B):
        pres = [i for i in range(L) if 0 <= seq[b, i] < 20]
        sum_ca, sum_all = np.zeros(L), np.zeros(L)
        for k in range(K):
            if len(pres) < 3:
                continue
            if not all(np.isfinite(samples[b, k, i, CA]).all() and np.isfinite(ref[b, i, CA]).all() for i in pres):
                continue
            usable[b] += 1
            R, t = kabsch(np.array([samples[b, k, i, CA] for i in pres]), np.array([ref[b, i, CA] for i in pres]))
            total = 0.0
            for i in pres:
                acc, cnt = 0.0, 0
                for a in range(4 + NSC[seq[b, i]]):
                    s, r = samples[b, k, i, a], ref[b, i, a]
                    if not (np.isfinite(s).all() and np.isfinite(r).all()):
                        continue                                                   # left out of its own term
                    e = R @ s + t - r
                    acc += float(e @ e)
                    cnt += 1
                    if a == CA:
                        total += float(e @ e)
                        sum_ca[i] += float(e @ e)
                sum_all[i] += acc / cnt if cnt else np.nan
            rmsd[b, k] = np.sqrt(total / len(pres))
        if usable[b]:
            for i in pres:
                rmsf[b, i, 0] = np.sqrt(sum_ca[i] / usable[b])
                rmsf[b, i, 1] = np.sqrt(sum_all[i] / usable[b])
    return rmsd, rmsf, usable


def _rotation(v):
    """Rotation vector [3] -> matrix (Rodrigues)."""
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def brute_force_rmsd(s, r, rng, starts=3000, steps=3000):
    """The smallest RMSD a search over PROPER rotations finds for s on r ([n, 3]): `starts` random rotations (the best
    translation for a rotation joins the centroids), then a random descent from the best of them with a shrinking step."""
    sc, rc = s - s.mean(0), r - r.mean(0)
    cost = lambda R: float(np.sqrt(((sc @ R.T - rc) ** 2).sum(1).mean()))              # noqa: E731
    q = rng.normal(size=(starts, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    Rs = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                   2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                   2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).reshape(starts, 3, 3)
    costs = np.sqrt(((np.einsum("kij,nj->kni", Rs, sc) - rc) ** 2).sum(2).mean(1))
    best, best_cost = Rs[int(costs.argmin())], float(costs.min())
    step = 0.3
    for _ in range(steps):
        cand = _rotation(rng.normal(size=3) * step) @ best
        c = cost(cand)
        if c < best_cost:
            best, best_cost = cand, c
        else:
            step = max(step * 0.995, 1e-9)
    assert abs(np.linalg.det(best) - 1.0) < 1e-9
    return best_cost


def random_chain(rng, seq):
    """A chain for the CPU tests, [L*14, 3] fp32: C-alphas 3.8 A apart on a random walk, the other atoms of a residue within a
    few A of its C-alpha, zeros in the slots its type does not have and in padded residues (what the NeRF build leaves there)."""
    seq = np.asarray(seq)
    L = len(seq)
    steps = rng.normal(size=(L, 3))
    ca = np.cumsum(3.8 * steps / np.linalg.norm(steps, axis=1, keepdims=True), 0)
    crd = ca[:, None, :] + rng.normal(0, 1.5, (L, SLOTS, 3))
    crd[:, CA] = ca
    return np.where(atom_mask(seq)[:, :, None], crd, 0.0).astype(np.float32).reshape(L * SLOTS, 3)


def random_rigid(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q, rng.normal(0, 20, 3)
