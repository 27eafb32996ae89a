"""fp64 numpy restatement of the batched dRMSD loss (include/ptamd.h, `ptamd_drmsd_fwd_bwd` and `ptamd_drmsd_bb_fwd_bwd`), for
tests/test_drmsd_ref.py and tests/test_gpu_drmsd_edges.py.  TEST INFRASTRUCTURE ONLY: the product never imports it.

Written from the definition, not from the kernels: one protein at a time, the present atoms as one list, every ordered pair
(i, j != i) visited from atom i's side in row blocks, so that n ~ 2000 needs a block x n x 3 array and never n x n x 3.

    d_ij = |x_i - x_j| (prediction),  tau_ij = |t_i - t_j| (truth),  both sqrt(max(. , 1e-30)) as losses.py:252 clamps them
    D    = sqrt( sum_{i<j} (d_ij - tau_ij)^2 / P ),   P = n (n - 1) / 2
    d(D / n)/d x_i = scale * sum_{j != i} (d_ij - tau_ij) / d_ij * (x_i - x_j),   scale = 1 / (n P D)

Besides the statistics and the gradient it returns what the per-atom bars of the GPU test are made of:

    unit_i         = 2^-24 * scale * sum_{j != i} (d_ij + tau_ij)   one fp32 rounding (half an ulp) of every d and tau of atom i,
                                                                   carried through cf (x_i - x_j): |(x_i - x_j) / d_ij| = 1
    pairmove_ij    = scale * |d_ij - tau_ij|                        the length of pair (i, j)'s term in atom i's gradient
    pairmove_p10_i = the smallest value that at least 90 % of atom i's pairmove_ij are >= (n >= 3; NaN below): losing or doubling
                     any of those pairs moves g_i by at least that much

and, for the four statistics, the same rounding model carried through D (d D / D = sum e de / sum e^2 with e = d - tau):

    stat_unit      = 2^-24 * (sum_{i<j} |e_ij| (d_ij + tau_ij) / sum_{i<j} e_ij^2 + k)   relative; k = 1 for D and D_bb (the result is
                     rounded to fp32 once), 2 for D/n and D_bb/n_bb (and divided in fp32).  At n = 2 this is the cancellation of
                     d - tau itself; it does not shrink with n as the error of a sum of random roundings does.
"""
import numpy as np

PAD_ID, SLOTS, BB = 20, 14, 3
EPS_SQ = 1e-30
HALF_ULP = 2.0 ** -24


def protein_len(seq):
    """`len` of a protein: the count of its non-pad ids (its residues are the first `len`)."""
    return int((np.asarray(seq) != PAD_ID).sum())


def present_slots(true, seq, spr=SLOTS):
    """-> (slots into pred [L*spr], slots into true [L*14], is_backbone), slot order: the atoms of the first `len` residues whose
    three true coordinates are all non-NaN; spr = 3 looks at the slots s % 14 < 3 of the truth alone."""
    assert spr in (SLOTS, BB)
    n_res = protein_len(seq)
    t = np.asarray(true, np.float64).reshape(-1, SLOTS, 3)[:n_res]
    ok = ~np.isnan(t).any(-1)                                     # [len, 14]
    if spr == BB:
        ok[:, BB:] = False
    res, slot = np.nonzero(ok)
    return res * spr + slot, res * SLOTS + slot, slot < BB


def _dist(a, b):
    diff = a[:, None, :] - b[None, :, :]
    return diff, np.sqrt(np.maximum((diff * diff).sum(-1), EPS_SQ))


def pair_sums(p, t, block=256):
    """p, t [n, 3] fp64 -> (sum_{i<j} (d - tau)^2, G [n, 3] = sum_j (d - tau) / d (x_i - x_j), W [n] = sum_j (d + tau),
    p10 [n] = per atom the smallest |d - tau| that at least 90 % of its pairs reach, sum_{i<j} |d - tau| (d + tau)), row block by
    row block."""
    n = len(p)
    sq, G, W, p10, lever = 0.0, np.zeros((n, 3)), np.zeros(n), np.full(n, np.nan), 0.0
    k = (n - 1) // 10                         # at most 10 % of an atom's n - 1 pairs may lie below the value
    for i0 in range(0, n, block):
        i1 = min(n, i0 + block)
        diff, d = _dist(p[i0:i1], p)
        tau = _dist(t[i0:i1], t)[1]
        e = d - tau
        own = (np.arange(i0, i1)[:, None] == np.arange(n)[None, :])
        e[own] = 0.0
        sq += 0.5 * float((e * e).sum())
        lever += 0.5 * float((np.abs(e) * (d + tau)).sum())
        G[i0:i1] = ((e / d)[:, :, None] * diff).sum(1)
        W[i0:i1] = np.where(own, 0.0, d + tau).sum(1)
        if n >= 3:
            a = np.where(own, np.inf, np.abs(e))                  # the atom's own column leaves the ranking
            p10[i0:i1] = np.partition(a, k, axis=1)[:, k]
    return sq, G, W, p10, lever


def _drmsd_of(sq, n):
    with np.errstate(invalid="ignore", divide="ignore"):
        P = n * (n - 1) / 2.0
        return np.sqrt(np.float64(sq) / np.float64(P))            # n < 2: 0 / 0, the NaN of a mean over an empty set


def drmsd_reference(pred, true, seq, spr=SLOTS, block=256):
    """One protein.  pred [L*spr, 3], true [L*14, 3] (NaN = absent), seq [L]; whatever they hold they are read as fp64.
    -> dict(stats [8] fp64 = {D, D/n, D_bb, D_bb/n_bb, n, n_bb, 0, 0}, grad [L*spr, 3] = d(D/n)/d pred (exact zeros in absent and
    padded slots and for a protein with fewer than two present atoms), slots [n] (the present atoms' slots in pred), unit [n],
    pairmove_p10 [n], stat_unit [4] (relative, for the first four statistics), scale, n, n_bb)."""
    pred = np.asarray(pred, np.float64).reshape(-1, 3)
    true = np.asarray(true, np.float64).reshape(-1, 3)
    ps, ts, bb = present_slots(true, seq, spr)
    p, t = pred[ps], true[ts]
    n, n_bb = len(ps), int(bb.sum())
    grad = np.zeros_like(pred)
    sq, G, W, a10, lever = pair_sums(p, t, block)
    D = _drmsd_of(sq, n)
    sq_bb, lever_bb = sq, lever
    if n_bb != n:
        sq_bb, _, _, _, lever_bb = pair_sums(p[bb], t[bb], block)
    D_bb = _drmsd_of(sq_bb, n_bb)
    with np.errstate(invalid="ignore", divide="ignore"):
        stats = np.array([D, D / n if n else np.nan, D_bb, D_bb / n_bb if n_bb else np.nan, n, n_bb, 0.0, 0.0])
        scale = 1.0 / (n * (n * (n - 1) / 2.0) * D) if n >= 2 else 0.0
        if n >= 2:
            grad[ps] = scale * G                                  # D == 0: inf * 0, the NaN of sqrt'(0) times a zero sum
        unit, move = HALF_ULP * scale * W, scale * a10
        a, b = np.float64(lever) / np.float64(sq), np.float64(lever_bb) / np.float64(sq_bb)
        stat_unit = HALF_ULP * np.array([a + 1, a + 2, b + 1, b + 2])
    return dict(stats=stats, grad=grad, slots=ps, unit=unit, pairmove_p10=move, scale=scale, n=n, n_bb=n_bb, stat_unit=stat_unit)


# ---- how the library cuts a batch (csrc/drmsd.hip: tri_layout(), layout()).  Unlike everything above this IS a restatement of
# the implementation: the tests need it to choose budgets that force passes and to know which chunk width a (B, L) takes;
# tests/test_drmsd_ref.py holds its byte count against ptamd_drmsd[_bb]_workspace_bytes_budget.
TS, STRIP_TILES, RS = 64, 4, 256
MAX_CHUNK_TILES, MIN_CHUNK_TILES, TARGET_ITEMS = 8, 4, 2560
PARTIAL_BUDGET = 200 << 20


def tri_layout(nmax, B):
    tiles = -(-nmax // TS)
    strips = -(-tiles // STRIP_TILES)
    chunk_tiles = MAX_CHUNK_TILES
    while True:
        chunks = -(-tiles // chunk_tiles)
        if strips * (chunks + 1) // 2 * B >= TARGET_ITEMS or chunk_tiles <= MIN_CHUNK_TILES:
            return dict(tiles=tiles, strips=strips, chunks=chunks, chunk_tiles=chunk_tiles)
        chunk_tiles >>= 1


def layout(B, L, budget=0, spr=SLOTS):
    """-> tri_layout plus per_strip (bytes of row and column partials one strip adds: layout(),
    `per_strip = B * (chunks * RS + tiles * TS) * sizeof(float4)`), spp (strips per pass) and total (workspace bytes)."""
    nmax = L * spr
    BN = B * nmax
    t = tri_layout(nmax, B)
    budget = budget or PARTIAL_BUDGET
    per_strip = B * (t["chunks"] * RS + t["tiles"] * TS) * 16
    spp = t["strips"]
    if per_strip * t["strips"] > budget:
        spp = max(1, budget // per_strip)
    passes = spp < t["strips"]
    parts = [BN * 16, BN * 32, B * spp * t["chunks"] * RS * 16, B * spp * t["tiles"] * TS * 16, BN * 16 if passes else 0,
             BN * 16 if passes else 0, BN * 4, B * 16, B * t["strips"] * t["chunks"] * 2 * 8]
    return dict(t, per_strip=per_strip, spp=spp, total=sum((p + 255) & ~255 for p in parts))


def drmsd_loops(pred, true, seq, spr=SLOTS):
    """The same statistics and gradient by a plain double loop over atoms (small proteins only): (stats [8], grad)."""
    pred = np.asarray(pred, np.float64).reshape(-1, 3)
    true = np.asarray(true, np.float64).reshape(-1, 3)
    ps, ts, bb = present_slots(true, seq, spr)
    n, n_bb = len(ps), int(bb.sum())
    sq = sq_bb = 0.0
    G = np.zeros((n, 3))
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            x = pred[ps[i]] - pred[ps[j]]
            y = true[ts[i]] - true[ts[j]]
            d, tau = np.sqrt(max(x @ x, EPS_SQ)), np.sqrt(max(y @ y, EPS_SQ))
            G[i] += (d - tau) / d * x
            if i < j:
                sq += (d - tau) ** 2
                if bb[i] and bb[j]:
                    sq_bb += (d - tau) ** 2
    D, D_bb = _drmsd_of(sq, n), _drmsd_of(sq_bb, n_bb)
    grad = np.zeros_like(pred)
    if n >= 2:
        grad[ps] = G / (n * (n * (n - 1) / 2.0) * D)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.array([D, D / n if n else np.nan, D_bb, D_bb / n_bb if n_bb else np.nan, n, n_bb, 0.0, 0.0]), grad
