"""The yardstick of the secondary-structure kernel (csrc/dssp.hip): the definition of include/ptamd.h - DSSP simplified: every
hydrogen bond under the threshold counts, three states - restated in numpy fp64, twice: vectorised (`hbonds`, `states_from_bits`)
and as a plain loop over residues and pairs (`hbonds_loop`, `states_from_bits_loop`); tests/test_ss_ref.py compares the two.  It
also holds the fixtures of tests/test_gpu_ss.py and measures how close any bond decision came to flipping (`min_margin`).

Kabsch & Sander, Biopolymers 22:2577-2637 (1983).  No DSSP binary is at hand (PARITY UNPINNED): the file is pinned by the
structures it must label - an ideal alpha-helix, an antiparallel and a parallel two-strand ladder.

THE EXCLUSION BAND.  The kernel decides E < -0.5 in fp32, this file in fp64, both on the same fp32 coordinates; they must agree
wherever the fp64 energy is farther from -0.5 than the kernel's error.  That error, for coordinates within +-64 A:
  * a difference of two fp32 coordinates is rounded once (relative 2^-24), so a distance between two INPUT atoms (O-N, C-N) is
    known to a relative 4 * 2^-24 = 2.4e-7 after the three squares, their sum and the 1-ulp v_rsq_f32;
  * the amide hydrogen is COMPUTED and stored as fp32: H = N + unit(C' - O') lies within +-65 A, where fp32 numbers are 2^-17
    apart, so each coordinate is off by up to 2^-18 = 3.8e-6 A from the rounding and ~4e-7 A from the unit vector: 4.2e-6 A per
    coordinate, 7.3e-6 A as a vector.  This is the term the coordinate range sets: at +-1000 A it would be 16 times larger;
  * with every distance >= 0.5 A (the clamp), 1/r <= 2 and d(1/r) = (1/r)(dr/r + 2.4e-7): <= 2 (1.46e-5 + 2.4e-7) = 3.0e-5 for the
    two H terms, <= 4.8e-7 for the two N terms; the three additions of terms <= 2 add 3 * 4 * 2^-24 = 7e-7:
    2 * 3.0e-5 + 2 * 4.8e-7 + 7e-7 = 6.2e-5, times 27.888 (and its own rounding, <= 7e-6) = 1.73e-3 kcal/mol.
BAND = 2e-3 kcal/mol covers it.  Every fixture keeps every candidate pair's fp64 energy farther than BAND from -0.5 (seeds are
chosen so that this file alone shows it); inside that condition the GPU tests demand exact equality of bits, states and counts."""
import functools

import numpy as np

PAD_ID = 20
NUM_SLOTS = 14
SLOT_N, SLOT_CA, SLOT_C, SLOT_O = 0, 1, 2, 3
Q_KCAL = 27.888
E_BOND = -0.5
R_MIN = 0.5
ST_H, ST_E, ST_C = 0, 1, 2
BAND = 2.0e-3
COORD_MAX = 64.0


# ----------------------------------------------------------------------------- the definition, vectorised
def presence(true, seq):
    """true [L*14,3], seq [L] -> bool [L]: not pad, no NaN among the four true backbone atoms."""
    L = len(seq)
    bb = np.asarray(true, np.float64).reshape(L, NUM_SLOTS, 3)[:, :4]
    return (np.asarray(seq) != PAD_ID) & ~np.isnan(bb).any((1, 2))


def backbone(crd, present):
    """crd [L*14,3] -> fp64 [L,4,3] (N, CA, C, O), absent residues zeroed: nothing they hold is read."""
    L = len(present)
    bb = np.asarray(crd, np.float64).reshape(L, NUM_SLOTS, 3)[:, :4].copy()
    bb[~present] = 0.0
    return bb


def hydrogens(bb, present):
    """(H [L,3], has_h [L]): H_j = N_j + unit(C_{j-1} - O_{j-1}) where j-1 and j are present."""
    has_h = present.copy()
    has_h[0] = False
    has_h[1:] &= present[:-1]
    u = np.zeros_like(bb[:, 0])
    u[1:] = bb[:-1, SLOT_C] - bb[:-1, SLOT_O]
    with np.errstate(invalid="ignore", divide="ignore"):
        h = bb[:, SLOT_N] + u / np.sqrt((u ** 2).sum(1))[:, None]
    h[~has_h] = 0.0
    return h, has_h


def energies(bb, present):
    """(E [L,L] fp64 kcal/mol, candidate [L,L] bool): E[i,j] for the C=O of i and the N-H of j; candidate = both present, j has
    an H, |i - j| >= 2."""
    L = len(present)
    h, has_h = hydrogens(bb, present)

    def inv(a, b):
        with np.errstate(invalid="ignore"):
            return 1.0 / np.maximum(np.sqrt(((a[:, None, :] - b[None, :, :]) ** 2).sum(2)), R_MIN)

    o, c, n = bb[:, SLOT_O], bb[:, SLOT_C], bb[:, SLOT_N]
    e = Q_KCAL * (inv(o, n) + inv(c, h) - inv(o, h) - inv(c, n))
    idx = np.arange(L)
    cand = present[:, None] & has_h[None, :] & (np.abs(idx[:, None] - idx[None, :]) >= 2)
    return e, cand


def hbonds(bb, present):
    e, cand = energies(bb, present)
    with np.errstate(invalid="ignore"):
        return cand & (e < E_BOND)


def _shift(m, a, b):
    """out[i,j] = m[i+a, j+b], False outside."""
    L = m.shape[0]
    out = np.zeros_like(m)
    i0, i1, j0, j1 = max(0, -a), min(L, L - a), max(0, -b), min(L, L - b)
    if i0 < i1 and j0 < j1:
        out[i0:i1, j0:j1] = m[i0 + a:i1 + a, j0 + b:j1 + b]
    return out


def states_from_bits(hb, present):
    """hb [L,L] bool, present [L] -> int8 [L] (ST_H / ST_E / ST_C, -1 absent): the pattern logic alone."""
    L = len(present)
    absent = np.concatenate([[0], np.cumsum(~present)])
    helix = {}
    for n in (3, 4, 5):
        turn = np.zeros(L, bool)
        k = np.arange(max(L - n, 0))
        if len(k):
            turn[k] = hb[k, k + n] & (absent[k + n + 1] - absent[k] == 0)
        start = np.zeros(L, bool)
        start[1:] = turn[1:] & turn[:-1]
        inside = np.zeros(L, bool)
        for d in range(min(n, L)):
            inside[d:] |= start[:L - d]
        helix[n] = inside
    ok3 = np.zeros(L, bool)
    if L >= 3:
        ok3[1:-1] = present[:-2] & present[1:-1] & present[2:]
    t = hb.T
    par = (_shift(hb, -1, 0) & _shift(t, 1, 0)) | (_shift(t, 0, -1) & _shift(hb, 0, 1))
    anti = (hb & t) | (_shift(hb, -1, 1) & _shift(t, 1, -1))
    idx = np.arange(L)
    strand = ((par | anti) & ok3[:, None] & ok3[None, :] & (np.abs(idx[:, None] - idx[None, :]) >= 3)).any(1)
    state = np.where(helix[4], ST_H, np.where(strand, ST_E, np.where(helix[3] | helix[5], ST_H, ST_C)))
    return np.where(present, state, -1).astype(np.int8)


# ----------------------------------------------------------------------------- the definition, as a plain loop
def hbonds_loop(bb, present):
    L = len(present)
    dist = lambda a, b: max(float(np.sqrt(((a - b) ** 2).sum())), R_MIN)      # noqa: E731
    hb = np.zeros((L, L), bool)
    for j in range(1, L):
        if not (present[j] and present[j - 1]):
            continue
        u = bb[j - 1, SLOT_C] - bb[j - 1, SLOT_O]
        h = bb[j, SLOT_N] + u / np.sqrt((u ** 2).sum())
        for i in range(L):
            if not present[i] or abs(i - j) < 2:
                continue
            o, c, n = bb[i, SLOT_O], bb[i, SLOT_C], bb[j, SLOT_N]
            e = Q_KCAL * (1 / dist(o, n) + 1 / dist(c, h) - 1 / dist(o, h) - 1 / dist(c, n))
            hb[i, j] = e < E_BOND
    return hb


def states_from_bits_loop(hb, present):
    L = len(present)
    p = lambda r: 0 <= r < L and bool(present[r])                             # noqa: E731
    run = lambda lo, hi: all(p(r) for r in range(lo, hi + 1))                 # noqa: E731
    b = lambda i, j: 0 <= i < L and 0 <= j < L and bool(hb[i, j])             # noqa: E731
    turn = lambda n, i: run(i, i + n) and b(i, i + n)                         # noqa: E731
    state = np.full(L, -1, np.int8)
    for r in range(L):
        if not present[r]:
            continue
        helix = {n: any(turn(n, i - 1) and turn(n, i) for i in range(r - n + 1, r + 1)) for n in (3, 4, 5)}
        strand = False
        if run(r - 1, r + 1):
            for j in range(L):
                if abs(r - j) < 3 or not run(j - 1, j + 1):
                    continue
                i = r
                par = (b(i - 1, j) and b(j, i + 1)) or (b(j - 1, i) and b(i, j + 1))
                anti = (b(i, j) and b(j, i)) or (b(i - 1, j + 1) and b(j - 1, i + 1))
                strand = strand or par or anti
        state[r] = ST_H if helix[4] else ST_E if strand else ST_H if (helix[3] or helix[5]) else ST_C
    return state


# ----------------------------------------------------------------------------- scores, and one protein end to end
def confusion_of(states, present, bad=False):
    """states [L,2] = {pred, true} -> int32 [3,3], true x pred."""
    c = np.zeros((3, 3), np.int32)
    if not bad:
        for p, t in states[present]:
            c[t, p] += 1
    return c


def scores_of(c, bad=False):
    """int [3,3] -> fp32 [3] = {q3, h, e}: ratios of integers, rounded once; NaN where the denominator is 0."""
    c = np.asarray(c, np.int64)
    ratio = lambda a, b: np.float32(np.float64(a) / np.float64(b)) if b > 0 and not bad else np.float32(np.nan)   # noqa: E731
    return np.array([ratio(np.trace(c), c.sum()), ratio(c[ST_H, ST_H], c[ST_H].sum()), ratio(c[ST_E, ST_E], c[ST_E].sum())],
                    np.float32)


def reference(pred, true, seq):
    """One protein: dict(present [L], hb [2,L,L] = {pred, true}, states [L,2] = {pred, true}, confusion [3,3], score [3], bad)."""
    present = presence(true, seq)
    L = len(seq)
    pbb = np.asarray(pred, np.float64).reshape(L, NUM_SLOTS, 3)[:, :4]
    bad = bool((~np.isfinite(pbb[present])).any())
    hb = np.stack([hbonds(backbone(x, present), present) for x in (pred, true)])
    states = np.stack([states_from_bits(hb[s], present) for s in (0, 1)], 1)
    if bad:
        states[:, 0] = -1
    c = confusion_of(states, present, bad)
    return dict(present=present, hb=hb, states=states, confusion=c, score=scores_of(c, bad), bad=bad)


def min_margin(crd, true, seq):
    """The smallest |E + 0.5| over the candidate pairs of the structure `crd` under the presence of `true`: inf without a pair."""
    present = presence(true, seq)
    e, cand = energies(backbone(crd, present), present)
    e = e[cand & np.isfinite(e)]
    return float(np.abs(e - E_BOND).min()) if e.size else float("inf")


def pack_bits(hb):
    """bool [L,L] -> uint64 [L, ceil(L/64)]: bit (j & 63) of word j >> 6 of row i = hb[i,j]."""
    L = hb.shape[0]
    W = (L + 63) // 64
    padded = np.zeros((L, W * 64), np.uint64)
    padded[:, :L] = hb
    return (padded.reshape(L, W, 64) << np.arange(64, dtype=np.uint64)).sum(2, dtype=np.uint64)


def unpack_bits(words, L):
    """uint64 [R, W] -> bool [R, L]."""
    words = np.asarray(words).astype(np.uint64)
    bits = (words[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(words.shape[0], -1)[:, :L].astype(bool)


# ----------------------------------------------------------------------------- fixtures
def _deg(*a):
    return [np.deg2rad(x) for x in a]


def segment(phi_psi, seed=None):
    """A poly-alanine backbone of len(phi_psi) residues from (phi, psi) in degrees, built by oracle.geometry with ideal bond angles
    and omega = 180: fp32 [n*14, 3], centred on its centroid."""
    import torch

    from oracle import geometry
    n = len(phi_psi)
    ang = torch.zeros(n, 12)
    ang[:, 0], ang[:, 1] = (torch.tensor([np.deg2rad(x[k]) for x in phi_psi], dtype=torch.float32) for k in (0, 1))
    ang[:, 2] = np.pi
    ang[:, 3], ang[:, 4], ang[:, 5] = _deg(111.0, 116.2, 121.7)
    crd = geometry.generate_coords(ang, torch.zeros(n, dtype=torch.int64)).numpy().astype(np.float64)
    atoms = crd.reshape(n, NUM_SLOTS, 3)[:, :5]
    return (crd - atoms.reshape(-1, 3).mean(0)).astype(np.float32)


def helix_segment(n):
    return segment([(-57.0, -47.0)] * n)


def coil_segment(n, seed):
    """A random-walk chain: phi in [-180, -40], psi in [-180, 180], uniformly."""
    rng = np.random.default_rng(seed)
    return segment(list(zip(rng.uniform(-180, -40, n), rng.uniform(-180, 180, n))))


def rotation(rotvec):
    """Rodrigues: the rotation by |rotvec| radians about rotvec."""
    v = np.asarray(rotvec, np.float64)
    th = np.sqrt((v ** 2).sum())
    if th < 1e-12:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


STRAND = 8                       # residues per strand of a ladder
STRAND_PHI_PSI = {"anti": (-139.0, 135.0), "par": (-119.0, 113.0)}
# strand B = rotation(rotvec) @ strand A + shift, A centred on its centroid: found by a CPU search (random restarts, then
# coordinate descent on the sum of the inter-strand bond energies) that maximises the residues labelled E; numbers committed
LADDER = {
    "anti": dict(rotvec=(1.3552, -2.266, 1.6509), shift=(-2.8199, 3.1551, -2.1874)),
    "par": dict(rotvec=(0.9917, 0.737, -0.0858), shift=(-1.1789, 3.0372, -3.1843)),
}


def ladder_segments(kind, placement=None):
    """(strand A, strand B) of a two-strand ladder, fp32 [STRAND*14, 3] each."""
    a = segment([STRAND_PHI_PSI[kind]] * STRAND).astype(np.float64)
    p = placement or LADDER[kind]
    b = a @ rotation(p["rotvec"]).T + np.asarray(p["shift"], np.float64)
    return a.astype(np.float32), b.astype(np.float32)


def assemble(L, pieces):
    """A chain of L residues from pieces [(first residue, coordinates [n*14,3], centre (x,y,z))]: every residue no piece covers is
    ABSENT (NaN truth): pieces are separated by chain breaks.  Returns (true [L*14,3] fp32, seq [L] int64)."""
    true = np.full((L, NUM_SLOTS, 3), np.nan, np.float32)
    for first, crd, centre in pieces:
        n = len(crd) // NUM_SLOTS
        assert 0 <= first and first + n <= L
        assert np.isnan(true[max(first - 1, 0):first + n + 1]).all(), "pieces must be separated by an absent residue"
        true[first:first + n] = (crd.reshape(n, NUM_SLOTS, 3).astype(np.float64) + np.asarray(centre, np.float64)).astype(np.float32)
    return true.reshape(L * NUM_SLOTS, 3), np.zeros(L, np.int64)


def noised(true, seed, sigma=0.25):
    """A prediction: the truth with Gaussian noise of `sigma` A on every coordinate; absent atoms get finite junk."""
    rng = np.random.default_rng(seed)
    out = np.asarray(true, np.float64) + rng.normal(0.0, sigma, true.shape)
    junk = rng.uniform(-50, 50, true.shape)
    return np.where(np.isnan(true), junk, out).astype(np.float32)


def helix_case(n=24):
    return assemble(n, [(0, helix_segment(n), (0, 0, 0))])


def ladder_case(kind):
    a, b = ladder_segments(kind)
    return assemble(2 * STRAND + 1, [(0, a, (0, 0, 0)), (STRAND + 1, b, (0, 0, 0))])


def walk_case(n=40, seed=3):
    return assemble(n, [(0, coil_segment(n, seed), (0, 0, 0))])


_CORNERS = [(x, y, z) for x in (-32.0, 32.0) for y in (-32.0, 32.0) for z in (-32.0, 32.0)]


def edge_case(L):
    """A chain whose bonds cross the boundaries of the 64-residue tiles: for L >= 128 an antiparallel ladder with strand A at
    residues 51..58 and strand B at 60..67 (pairs 64-54, 65-53, 66-52, 67-51: bonds across residue 64 in BOTH directions), a helix
    on the last 16 residues (its i -> i+4 bonds cross residue 128 when L = 129, residue 64 when L = 65 .. 79), random-walk
    filler elsewhere.  Shorter chains: the ladder at 10..17 / 19..26."""
    a, b = ladder_segments("anti")
    la = 51 if L >= 128 else 10
    pieces = [(la, a, _CORNERS[0]), (la + STRAND + 1, b, _CORNERS[0]), (L - 16, helix_segment(16), _CORNERS[1])]
    k = 0
    for lo, hi in ((0, la - 1), (la + 2 * STRAND + 2, L - 17)):      # free residues lo .. hi-1, a break behind them
        first = lo
        while hi - first >= 2:                   # filler pieces of at most 16 residues, each in a corner of its own
            n = min(16, hi - first)
            pieces.append((first, coil_segment(n, 1000 * L + k), _CORNERS[2 + k]))
            first, k = first + n + 1, k + 1
    return assemble(L, pieces)


@functools.lru_cache(maxsize=None)
def cases():
    """{name: (pred, true, seq)}: every fixture with a noised copy as its prediction, and the fixtures themselves as predictions
    of their noised copies' truth where that matters (the random walk predicts the helix)."""
    out = {}
    for k, (name, (true, seq)) in enumerate([("helix", helix_case()), ("anti", ladder_case("anti")), ("par", ladder_case("par")),
                                            ("walk", walk_case())]):
        out[name] = (noised(true, 22 + k), true, seq)
    ht, hs = helix_case(24)
    wt, _ = walk_case(24, seed=5)
    out["walk_as_helix"] = (np.where(np.isnan(ht), 0, wt).astype(np.float32), ht, hs)
    out["exact_helix"] = (np.where(np.isnan(ht), 0, ht).astype(np.float32), ht, hs)
    return out


EDGE_LENGTHS = (63, 64, 65, 128, 129)
_EDGE_NOISE_SEED = {63: 113, 64: 114, 65: 115, 128: 301, 129: 300}      # chosen for their margins (tests/test_ss_ref.py)


@functools.lru_cache(maxsize=None)
def edge_cases():
    return {L: (lambda ts: (noised(ts[0], _EDGE_NOISE_SEED[L], sigma=0.1), ts[0], ts[1]))(edge_case(L)) for L in EDGE_LENGTHS}


def batch_of(items, L_pad=None):
    """[(pred, true, seq)] -> (pred [B,Lp*14,3], true, seq [B,Lp]) padded to the longest (or L_pad) with pad residues and zeros."""
    Lp = L_pad or max(len(s) for _, _, s in items)
    B = len(items)
    pred = np.zeros((B, Lp * NUM_SLOTS, 3), np.float32)
    true = np.zeros((B, Lp * NUM_SLOTS, 3), np.float32)
    seq = np.full((B, Lp), PAD_ID, np.int64)
    for b, (p, t, s) in enumerate(items):
        pred[b, :len(p)], true[b, :len(t)], seq[b, :len(s)] = p, t, s
    return pred, true, seq
