"""The yardstick of the TM-score / GDT kernel (csrc/tmscore.hip): the definition of include/ptamd.h restated in plain numpy fp64,
by another route than the kernel's - every superposition is an SVD with the determinant correction (Kabsch), not a quaternion
eigenvector; distances are compared as distances, not as squares; the widening of a selection is the literal loop.  It also
measures how close any of its decisions came to flipping (`min_margin`, `min_rank`, `min_gap`) - the condition under which a
correct fp64 kernel must reproduce its integers - and holds the case builders of tests/test_gpu_tm.py.

Zhang & Skolnick, Proteins 57:702-710 (2004); the search is that of the public TMscore program.  No TM-score binary is at hand
(PARITY UNPINNED): tests/test_tm_ref.py pins this file by known answers."""
import functools

import numpy as np

PAD_ID = 20
NUM_SLOTS = 14
CA_SLOT = 1
GDT_CUTS = (0.5, 1.0, 2.0, 4.0, 8.0)
MAX_REFINE = 20


def d0_of(n):
    return max(1.24 * np.cbrt(n - 15.0) - 1.8, 0.5) if n > 21 else 0.5


def d_search_of(n):
    return min(8.0, max(4.5, d0_of(n)))


def seed_list(n):
    """[(length, start)] in seed order."""
    lengths = []
    for raw in (n, n >> 1, n >> 2, n >> 3, n >> 4, 4):
        ell = min(max(raw, 4), n)
        if ell not in lengths:
            lengths.append(ell)
    return [(ell, s) for ell in lengths for s in range(n - ell + 1)]


def kabsch(p, q):
    """(R, t, singular values, sign) of the proper rotation with R p + t ~ q in the least-squares sense."""
    pb, qb = p.mean(0), q.mean(0)
    U, S, Vt = np.linalg.svd((p - pb).T @ (q - qb))
    d = 1.0 if np.linalg.det(Vt.T @ U.T) >= 0 else -1.0
    R = Vt.T @ np.diag([1.0, 1.0, d]) @ U.T
    return R, qb - R @ pb, S, d


def distances(R, t, p, q):
    return np.sqrt((((p @ R.T + t) - q) ** 2).sum(1))


def tm_of(d, d0):
    return float(np.mean(1.0 / (1.0 + (d / d0) ** 2)))


def ca_pairs(pred, true, seq):
    """The compacted (p, q) C-alpha pairs of ONE protein: pred, true [L*14, 3], seq [L] -> fp64 [N,3], [N,3]."""
    L = len(seq)
    p = np.asarray(pred, np.float64).reshape(L, NUM_SLOTS, 3)[:, CA_SLOT]
    q = np.asarray(true, np.float64).reshape(L, NUM_SLOTS, 3)[:, CA_SLOT]
    ok = (np.asarray(seq) != PAD_ID) & ~np.isnan(q).any(1)
    return p[ok], q[ok]


def tm_ref(pred, true, seq):
    """One protein -> dict(score [3] = tm, gdt_ts, gdt_ha; counts [6] = N, c0.5, c1, c2, c4, c8; xform [3,4] = (R | t);
    min_margin, min_rank, min_gap; visited).  Diagnostics over every decision made: min_margin the smallest |d_i - threshold|
    over all selection cutoffs tried and the five GDT cutoffs on all visited superpositions, min_rank the smallest sigma2 / sigma1
    of a superposed set, min_gap the smallest (sigma2 + sign sigma3) / sigma1 - the relative gap that makes the best PROPER
    rotation unique (it is what separates the two largest eigenvalues of the quaternion matrix)."""
    p, q = ca_pairs(pred, true, seq)
    n = len(p)
    nan = float("nan")
    out = dict(score=np.full(3, nan), counts=np.array([n, 0, 0, 0, 0, 0]), xform=np.full((3, 4), nan), min_margin=np.inf,
               min_rank=np.inf, min_gap=np.inf, visited=0)
    if n < 3 or not np.isfinite(p).all():
        return out
    d0, ds = d0_of(n), d_search_of(n)
    best_tm, best_xform, best_c = -1.0, None, np.zeros(5, np.int64)
    margin, rank, gap, visited = np.inf, np.inf, np.inf, 0

    def select(d, cut):
        nonlocal margin
        while True:
            margin = min(margin, np.abs(d - cut).min())
            sel = d < cut
            if sel.sum() >= 3:
                return sel
            cut += 0.5

    def visit(sel):
        nonlocal best_tm, best_xform, best_c, margin, rank, gap, visited
        R, t, S, sign = kabsch(p[sel], q[sel])
        rank, gap = min(rank, S[1] / S[0]), min(gap, (S[1] + sign * S[2]) / S[0])
        d = distances(R, t, p, q)
        visited += 1
        tm = tm_of(d, d0)
        if tm > best_tm:
            best_tm, best_xform = tm, np.concatenate([R, t[:, None]], 1)
        for k, cut in enumerate(GDT_CUTS):
            margin = min(margin, np.abs(d - cut).min())
            best_c[k] = max(best_c[k], int((d <= cut).sum()))
        return d

    for ell, s in seed_list(n):
        sel = np.zeros(n, bool)
        sel[s:s + ell] = True
        d = visit(sel)
        sel = select(d, ds - 1.0)
        for _ in range(MAX_REFINE):
            d = visit(sel)
            new = select(d, ds + 1.0)
            same = np.array_equal(new, sel)
            sel = new
            if same:
                break
    c = best_c
    out.update(score=np.array([best_tm, (c[1] + c[2] + c[3] + c[4]) / (4.0 * n), (c[0] + c[1] + c[2] + c[3]) / (4.0 * n)]),
               counts=np.array([n, *c]), xform=best_xform, min_margin=float(margin), min_rank=float(rank), min_gap=float(gap),
               visited=visited)
    return out


# ----------------------------------------------------------------------------- case builders
def embed(p, q, L=None, missing=(), seq_fill=0):
    """C-alpha chains p (prediction), q (truth) [n,3] -> fp32 (pred [L*14,3], true [L*14,3], seq [L]): residue r of the first n
    carries them in slot 1; every other slot of the truth is NaN (absent), of the prediction zero.  `missing`: residues whose true
    C-alpha is NaN and whose prediction is garbage; residues from n on are padding (zeros in the truth, as collate pads)."""
    n = len(p)
    L = L or n
    pred = np.zeros((L, NUM_SLOTS, 3), np.float32)
    true = np.full((L, NUM_SLOTS, 3), np.nan, np.float32)
    seq = np.full(L, PAD_ID, np.int64)
    seq[:n] = seq_fill
    pred[:n, CA_SLOT], true[:n, CA_SLOT] = p, q
    true[n:] = 0.0
    for r in missing:
        true[r, CA_SLOT] = np.nan
        pred[r, CA_SLOT] = (1e30, -3e7, 12345.0)
    return pred.reshape(-1, 3), true.reshape(-1, 3), seq


def random_walk(n, rng, step=3.8):
    v = rng.normal(size=(n, 3))
    return np.cumsum(step * v / np.linalg.norm(v, axis=1, keepdims=True), axis=0)


def rotation(rng):
    A = np.linalg.qr(rng.normal(size=(3, 3)))[0]
    return A * np.sign(np.linalg.det(A))


def noisy_chain(n, seed, missing=()):
    """A 3.8 A random walk as the truth; the prediction is the truth plus per-residue noise of 0.5-4 A, turned and shifted."""
    rng = np.random.default_rng(seed)
    q = random_walk(n + len(missing), rng)
    sigma = rng.uniform(0.5, 4.0, size=(len(q), 1)) / np.sqrt(3.0)
    p = (q + sigma * rng.normal(size=q.shape)) @ rotation(rng).T + rng.normal(size=3) * 20.0
    return embed(p, q, missing=missing)


def hinge_chains():
    """80 residues; the prediction is the truth with residues 50..79 turned by 90 degrees about an axis through residue 50."""
    rng = np.random.default_rng(80)
    q = random_walk(80, rng)
    axis = np.array([0.0, 0.0, 1.0])
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R90 = np.eye(3) + K + K @ K                                # Rodrigues at 90 degrees
    p = q.copy()
    p[50:] = (q[50:] - q[50]) @ R90.T + q[50]
    return p, q


def hinge_case():
    return embed(*hinge_chains())


def mirror_case(n=40, seed=7):
    rng = np.random.default_rng(seed)
    q = random_walk(n, rng)
    return embed(q * np.array([1.0, 1.0, -1.0]), q)


def mirror_control_case(n=40, seed=7):
    """The chain of `mirror_case` against a noised copy of itself (1 A per residue)."""
    rng = np.random.default_rng(seed)
    q = random_walk(n, rng)
    return embed(q + rng.normal(size=q.shape) / np.sqrt(3.0), q)


def rigid_case(n=30, seed=3, offset=1e3):
    """An exact rigid motion of the truth, far from the origin.  In fp32 the moved copy is exact to ~6e-5 A at 1e3."""
    rng = np.random.default_rng(seed)
    q = random_walk(n, rng) + offset
    return embed(q.astype(np.float32).astype(np.float64) @ rotation(rng).T + rng.normal(size=3) * 5.0, q)


def stack(cases):
    """[(pred, true, seq)] of different lengths -> one batch [B, L*14, 3], [B, L*14, 3], [B, L], padded as collate pads."""
    L = max(len(c[2]) for c in cases)
    pred = np.zeros((len(cases), L * NUM_SLOTS, 3), np.float32)
    true = np.zeros_like(pred)
    seq = np.full((len(cases), L), PAD_ID, np.int64)
    for b, (p, t, s) in enumerate(cases):
        pred[b, :len(p)], true[b, :len(t)], seq[b, :len(s)] = p, t, s
    return pred, true, seq


# name -> builder of ONE protein; the GPU cases of tests/test_gpu_tm.py (tests/test_tm_ref.py checks their margins on the CPU)
LENGTHS = (3, 4, 5, 7, 8, 9, 63, 64, 65)
GPU_CASES = {**{f"walk{n}": functools.partial(noisy_chain, n, 1000 + n) for n in LENGTHS},
             "walk129_missing": functools.partial(noisy_chain, 129, 1129, missing=(0, 17, 64, 65, 130)),
             "walk20": functools.partial(noisy_chain, 20, 1020),
             "hinge": hinge_case, "mirror": mirror_case, "rigid1e3": rigid_case}


@functools.lru_cache(maxsize=None)
def case_with_reference(name):
    pred, true, seq = GPU_CASES[name]()
    return pred, true, seq, tm_ref(pred, true, seq)
