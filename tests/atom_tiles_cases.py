"""Cases at the tile, strip, chunk, box and compaction-share edges of the kernels that read the compacted 64-atom tiles of
csrc/atom_tiles.h, with the CPU-side conditions that make them well posed: tests/test_atom_tiles_cases.py checks the cases on
any machine, tests/test_gpu_atom_tiles_edges.py runs them on the device.

The fp64 references are imported, not restated: `slddt_reference` (tests/test_gpu_slddt.py), `lddt_reference`
(tests/test_gpu_lddt.py), `clash_reference` (tests/clash_ref.py) and `fape_reference` with `well_posed_clamp`
(tests/test_gpu_fape.py; `fape_table` takes the per-pair terms, frame side included, from autograd of the same functions).  They return a gradient per protein; the per-atom bar
needs more - what every single pair adds to every atom - so `slddt_pairs` and `clash_pairs` write the analytic pair term down
once more, and `reference` asserts that the sum of the pair terms IS the imported reference's gradient (to 1e-9 of the atom's
scale).  The pair table serves two ends: scale_i = sum over the atom's pairs of |pair term|, and the mutations of
`mutations` (a pair dropped, a tile pair culled, a gradient moved to the next slot, a sign flipped), each of which the bar
must reject by a factor of ten.

Conditions on the inputs (asserted by `Case.check` or while the case is built):
  * no true inter-residue distance within 1e-3 A of the cutoff of 15 A - twice the half-gap that `well_posed_cutoff` of
    tests/test_gpu_slddt.py asks for; `settle_truth` moves the atoms of such pairs, truth and prediction alike, by 0.05 A
    until none is left, and `assert_cutoff_well_posed` checks it;
  * no included pair with |delta - t| <= 1.2 EPS for t in {0, 0.5, 1, 2, 4}, EPS = 2.5e-4 A the bracket of
    tests/test_gpu_lddt.py: the lDDT counts are then one number (lo == hi, asserted), and no pair sits on delta = 0 where the
    sign of the smooth-lDDT gradient is rounding (1e-5 A is the rule of tests/test_gpu_slddt.py; 3e-4 A is stricter).
    `settle` moves the prediction of the atoms of such pairs by 0.1 A until none is left;
  * no candidate clash pair within clash_ref.MARGIN of the kink (`settle_clash`, then `clash_reference` asserts it).

Atoms are compacted in slot order, so with 8 atoms per residue (slots 0..7) a tile is 8 consecutive residues."""
import functools

import numpy as np

import clash_ref
from test_gpu_lddt import EPS as LDDT_EPS, lddt_reference
from test_gpu_slddt import PAD, SLOTS, THRESHOLDS, cloud, present_atoms, slddt_reference, true_distances

TS, STRIP_TILES, CHUNK_TILES, LDDT_CHUNK_TILES, NWAVE = 64, 4, 8, 32, 16
PER_RES = 8
TAU = 1.0
CUTOFF = 15.0                                                          # every case is made well posed for it
EPS32 = 2.0 ** -24
EIGHT_ATOM_TYPES = [clash_ref.AA.index(c) for c in "DILMN"]        # residue types of exactly 8 atoms (slots 0..7)

# K of the bar err_i <= K scale_i + floor_i: 8 x the worst err_i / scale_i measured on an MI355X over every case below
# (profiles/atom_tiles/NOTES.md has the figures per case)
MEASURED = {"slddt": 7.656e-6, "clash": 6.321e-5, "fape": 2.538e-6}   # shares-147[0]; shares-147-clash[0]; fape-grid-128[8]
K = {k: 8 * v for k, v in MEASURED.items()}


# ----------------------------------------------------------------------------- building blocks
def place(slots, xyz_true, xyz_pred, L, rng, n_res=None):
    """One protein with the given present slots: (pred, true, seq); absent slots are NaN in the truth and finite garbage in
    the prediction, residues from `n_res` on are batch padding (zeros behind pad ids)."""
    n_res = L if n_res is None else n_res
    true = np.full((L * SLOTS, 3), np.nan, np.float32)
    pred = rng.normal(0, 5.0, (L * SLOTS, 3)).astype(np.float32)
    true[slots], pred[slots] = xyz_true, xyz_pred
    true[n_res * SLOTS:] = 0.0
    seq = np.full(L, PAD, np.int64)
    seq[:n_res] = rng.integers(0, 20, n_res)
    return pred, true, seq


def dense_slots(n_atoms):
    """Slots of n_atoms atoms, PER_RES per residue from slot 0 on."""
    k = np.arange(n_atoms)
    return (k // PER_RES) * SLOTS + k % PER_RES


def stack(items):
    return tuple(np.stack([it[k] for it in items]) for k in range(3))


def tile_boxes(xyz):
    """(lo, hi) [tiles, 3] fp64 of the tiles of 64 consecutive rows of xyz."""
    tiles = -(-len(xyz) // TS)
    lo = np.array([xyz[t * TS:(t + 1) * TS].min(0) for t in range(tiles)], np.float64)
    hi = np.array([xyz[t * TS:(t + 1) * TS].max(0) for t in range(tiles)], np.float64)
    return lo, hi


def box_gaps(lo, hi):
    """[tiles, tiles, 3]: the signed gap between the boxes of two tiles along every axis (negative: they overlap there)."""
    return np.maximum(lo[:, None] - hi[None], lo[None] - hi[:, None])


def near_matrix(xyz, reach):
    """Which tile pairs the sweep must visit: the Euclidean gap of the boxes, negative gaps counting as 0, within `reach`."""
    g = np.maximum(box_gaps(*tile_boxes(xyz)), 0.0)
    return (g ** 2).sum(-1) <= reach * reach


def kept_matrix(near):
    """[strips, tiles]: strip s touches column tile J - a row tile I <= J of the strip is near J."""
    tiles = len(near)
    strips = -(-tiles // STRIP_TILES)
    upper = near & (np.arange(tiles)[:, None] <= np.arange(tiles)[None])
    return np.array([upper[s * STRIP_TILES:(s + 1) * STRIP_TILES].any(0) for s in range(strips)])


def assert_cutoff_well_posed(true, seq, cutoff):
    for b in range(len(seq)):
        _, dt, other = true_distances(true[b], seq[b])
        d = dt[np.triu(other, 1)]
        assert d.size == 0 or np.abs(d - cutoff).min() >= 1e-3, b


def settle_truth(pred, true, seq, cutoff, rng):
    """Moves the atoms (truth and prediction alike) of inter-residue pairs whose true distance lies within 1.2e-3 A of the cutoff
    by 0.05 A until none is left; in place."""
    for b in range(len(seq)):
        for _ in range(200):
            idx, dt, other = true_distances(true[b], seq[b])
            atoms = np.nonzero((other & (np.abs(dt - cutoff) < 1.2e-3)).any(1))[0]
            if len(atoms) == 0:
                break
            move = rng.normal(0, 0.05, (len(atoms), 3)).astype(np.float32)
            true[b, idx[atoms]] += move
            pred[b, idx[atoms]] += move
        else:
            raise AssertionError(f"row {b} does not settle")


def ambiguous_pairs(pred, true, seq, cutoff):
    """Positions (in the present atoms) of the atoms of included pairs whose delta lies within 1.2 EPS of 0 or a threshold."""
    idx, dt, other = true_distances(true, seq)
    p = np.asarray(pred, np.float64)[idx]
    dp = np.sqrt(((p[:, None] - p[None]) ** 2).sum(-1))
    delta = np.abs(dp - dt)
    amb = np.zeros_like(other)
    for t in (0.0,) + THRESHOLDS:
        amb |= np.abs(delta - t) <= 1.2 * LDDT_EPS
    amb &= other & (dt < cutoff)
    return idx, np.nonzero(amb.any(1))[0]


def settle(pred, true, seq, cutoff, rng):
    """Moves the predicted atoms of ambiguous pairs by 0.1 A until no pair is ambiguous (module docstring); in place."""
    for b in range(len(seq)):
        for _ in range(200):
            idx, atoms = ambiguous_pairs(pred[b], true[b], seq[b], cutoff)
            if len(atoms) == 0:
                break
            pred[b, idx[atoms]] += rng.normal(0, 0.1, (len(atoms), 3)).astype(np.float32)
        else:
            raise AssertionError(f"row {b} does not settle")
    return pred


def clash_margins(crd, seq):
    idx, rad, ii, jj = clash_ref.candidate_pairs(seq)
    x = np.asarray(crd, np.float64)[idx]
    d = np.sqrt(((x[ii] - x[jj]) ** 2).sum(-1) + 1e-30)
    return idx, ii, jj, rad[ii] + rad[jj] - clash_ref.TOLERANCE - d


def settle_clash(crd, seq, rng, keep=()):
    """Moves the atoms of candidate pairs within 2 MARGIN of the kink by 0.01 A until none is left; in place.  `keep`: slots
    that are never moved (their partner is)."""
    for b in range(len(seq)):
        for _ in range(200):
            idx, ii, jj, over = clash_margins(crd[b], seq[b])
            bad = np.abs(over) < 2 * clash_ref.MARGIN
            if not bad.any():
                break
            atoms = np.unique(np.concatenate([ii[bad], jj[bad]]))
            atoms = atoms[~np.isin(idx[atoms], keep)]
            crd[b, idx[atoms]] += rng.normal(0, 0.01, (len(atoms), 3)).astype(np.float32)
        else:
            raise AssertionError(f"row {b} does not settle")
    return crd


# ----------------------------------------------------------------------------- the case record
class Case:
    """A batch.  kind "truth": pred, true, seq, cutoff for slddt and lddt (`kernels` says which); kind "clash": pred, seq (the
    truth is not an argument).  `with_pairs`: how many proteins have at least one included pair (or one atom, for clash) - the
    others must come back as NaN and zeros.  `facts(case)` asserts what the case was built for.  `designed`: per row the slots
    of the one cross-tile pair the case is about, or None."""

    def __init__(self, name, kind, kernels, pred, true, seq, cutoff, atoms, with_pairs, facts, designed=None):
        self.name, self.kind, self.kernels, self.cutoff = name, kind, kernels, cutoff
        self.pred, self.true, self.seq = pred, true, seq
        self.atoms, self.with_pairs, self.facts, self.designed = atoms, with_pairs, facts, designed or [None] * len(seq)
        for a in (pred, true, seq):
            if a is not None:
                a.setflags(write=False)

    @property
    def B(self):
        return self.seq.shape[0]

    @property
    def L(self):
        return self.seq.shape[1]

    def present(self, b):
        """Slot indices of protein b's atoms, in slot order (= compaction order)."""
        if self.kind == "clash":
            return clash_ref.atoms_of(self.seq[b])[0]
        return present_atoms(self.true[b], self.seq[b])

    def boxed(self, b):
        """The coordinate the kernel boxes, of the present atoms: the truth, or for clash the prediction."""
        return (self.pred if self.kind == "clash" else self.true)[b][self.present(b)].astype(np.float64)

    def reach(self):
        return 2 * 1.8 - clash_ref.TOLERANCE if self.kind == "clash" else self.cutoff

    def check(self):
        assert [len(self.present(b)) for b in range(self.B)] == list(self.atoms), self.name
        if self.kind == "truth" and set(self.kernels) & {"slddt", "lddt"}:
            assert_cutoff_well_posed(self.true, self.seq, self.cutoff)
            for b in range(self.B):
                assert len(ambiguous_pairs(self.pred[b], self.true[b], self.seq[b], self.cutoff)[1]) == 0, (self.name, b)
        self.facts(self)

    def stale_batch(self, rng):
        """The batch that goes through the workspace immediately before, for the `stale` state: the rows in reverse order, the
        one with the most atoms replaced by a protein that fills every slot of the row."""
        order = list(range(self.B))[::-1]
        full = int(np.argmax(self.atoms))
        pred, seq = self.pred[order].copy(), self.seq[order].copy()
        true = None if self.true is None else self.true[order].copy()
        k = order.index(full)
        n = self.L * SLOTS
        xyz = rng.normal(0, 9.0, (n, 3)).astype(np.float32)
        pred[k] = xyz + rng.normal(0, 1.0, (n, 3)).astype(np.float32)
        seq[k] = clash_ref.AA.index("W")                               # 14 atoms: every slot exists
        if true is not None:
            true[k] = xyz
        return pred, true, seq


# ----------------------------------------------------------------------------- B1: counts at the strip and chunk edges
def _counts_truth(name, counts, kernels, seed):
    rng = np.random.default_rng(seed)
    L = -(-max(counts) // PER_RES)
    pred, true, seq = stack([cloud(n, PER_RES, rng, L=L, line=3.8) for n in counts])
    lone = max(counts) < 1024                                          # one more row without a pair: a single residue
    if lone:
        pred, true, seq = stack(list(zip(pred, true, seq)) + [cloud(PER_RES, PER_RES, rng, L=L)])
        counts = tuple(counts) + (PER_RES,)
    cutoff = CUTOFF
    settle_truth(pred, true, seq, cutoff, rng)
    settle(pred, true, seq, cutoff, rng)

    def facts(c):
        tiles = [-(-n // TS) for n in c.atoms[:len(c.atoms) - lone]]
        if max(counts) < 1024:
            assert tiles == [4, 4, 5, 8, 8, 9]                         # the strip edge (4 tiles) and the chunk edge (8 tiles)
        else:
            assert tiles == [32, 32, 33]                               # the lDDT chunk (32 tiles)
    return Case(name, "truth", kernels, pred, true, seq, cutoff, counts, len(counts) - lone, facts)


def _counts_clash(seed):
    counts = (255, 256, 257, 511, 512, 513)
    rng = np.random.default_rng(seed)
    seqs = [clash_ref.sequence_with_atoms(n, rng) for n in counts]
    L = max(len(s) for s in seqs)
    rows = [clash_ref.build_chain(s, rng, L_pad=L) for s in seqs]
    one = (rng.normal(0, 3.0, (L * SLOTS, 3)).astype(np.float32), np.full(L, PAD, np.int64))
    one[1][0] = clash_ref.AA.index("W")                                # a single residue: 14 atoms, no candidate pair
    rows += [one, (np.zeros((L * SLOTS, 3), np.float32), np.full(L, PAD, np.int64))]     # and a fully padded row: no atom
    pred, seq = np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])
    settle_clash(pred, seq, rng)

    def facts(c):
        assert [-(-n // TS) for n in c.atoms[:6]] == [4, 4, 5, 8, 8, 9]
        assert [r["npairs"] > 0 for r in reference(c, "clash")] == [True] * 6 + [False] * 2    # every chain does clash
    return Case("counts-clash", "clash", ("clash",), pred, None, seq, None, counts + (14, 0), 7, facts)


# ----------------------------------------------------------------------------- B2: the box cull, two tiles
CUTOFF_B2 = CUTOFF
INSIDE = 5e-3                                                          # the designed pair: this far inside the cutoff


def _two_tiles(variant, control, rng):
    """Tile A: 63 atoms in [0,2]^3 (nested: [0,2] x [0,3]^2) and one designed atom a* on the box's face (corner); tile B: its
    designed atom b* first, displaced from a* along x (axis, nested) or along (1,1,1) (diagonal) so that |a* b*| = cutoff -
    INSIDE, and 63 atoms at least 1 A farther along every displaced axis.  `control`: tile B moved 1 A farther along every
    displaced axis - no cross pair is left and the tile pair is culled.  The prediction is the truth plus 0.25 A of noise, tile
    B moved 3 A farther still: a cull on the predicted boxes loses the designed pair."""
    diag = variant == "diagonal"
    axes = np.array([1.0, 1.0, 1.0]) if diag else np.array([1.0, 0.0, 0.0])
    g = (CUTOFF_B2 - INSIDE) / np.sqrt(axes.sum())
    A = rng.uniform(0, 2, (TS, 3))
    if variant == "nested":
        A[:, 1:] = rng.uniform(0, 3, (TS, 2))
    a_star = np.array([3.0, 3.0, 3.0]) if diag else np.array([3.0, 1.5, 1.5])
    A[TS - 1] = a_star                                                 # the last atom of tile A
    Bt = a_star + axes * (g + 1.0) + rng.uniform(0, 2, (TS, 3)) * axes + (1 - axes) * rng.uniform(-1.5, 1.5, (TS, 3))
    if variant == "nested":
        Bt[:, 1:] = a_star[1:] + rng.uniform(-0.5, 0.5, (TS, 2))       # B's box inside A's along y and z
    Bt[0] = a_star + axes * g                                          # the first atom of tile B
    if control:
        Bt += axes
    xyz = np.concatenate([A, Bt]).astype(np.float32)
    pred = xyz + rng.normal(0, 0.25, xyz.shape).astype(np.float32)
    pred[TS:] += (3.0 * axes).astype(np.float32)
    slots = dense_slots(2 * TS)
    return place(slots, xyz, pred, 2 * TS // PER_RES, rng), (int(slots[TS - 1]), int(slots[TS]))


def _box_cull(seed):
    rng = np.random.default_rng(seed)
    names = [(v, c) for c in (False, True) for v in ("axis", "diagonal", "nested")]
    built = [_two_tiles(v, c, rng) for v, c in names]
    pred, true, seq = stack([b[0] for b in built])
    settle(pred, true, seq, CUTOFF_B2, rng)
    designed = [None if c else b[1] for (v, c), b in zip(names, built)]

    def facts(case):
        for b, (variant, control) in enumerate(names):
            idx, dt, other = true_distances(case.true[b], case.seq[b])
            assert other[:TS, TS:].all()                               # the tiles share no residue
            cross = np.sort(dt[:TS, TS:].ravel())
            gaps = box_gaps(*tile_boxes(case.boxed(b)))[0, 1]
            pgap = np.maximum(box_gaps(*tile_boxes(case.pred[b][idx].astype(np.float64)))[0, 1], 0)
            assert (pgap ** 2).sum() > CUTOFF_B2 ** 2 * 1.001          # a cull on the predicted boxes drops the tile pair
            if control:
                assert cross[0] > CUTOFF_B2 + 0.5 and not near_matrix(case.boxed(b), CUTOFF_B2)[0, 1]
                continue
            assert 2e-3 <= CUTOFF_B2 - cross[0] <= 1e-2 and cross[1] > CUTOFF_B2 + 1e-2   # exactly one pair, just inside
            assert dt[TS - 1, TS] == cross[0]                          # and it is the designed one
            assert near_matrix(case.boxed(b), CUTOFF_B2)[0, 1]
            lo, hi = tile_boxes(case.boxed(b))
            assert np.linalg.norm(0.5 * (lo[0] + hi[0]) - 0.5 * (lo[1] + hi[1])) > CUTOFF_B2 + 1.0    # centres: too far
            if variant == "diagonal":
                assert (gaps > 8.0).all() and np.abs(gaps).sum() > CUTOFF_B2 + 5.0       # the 1-norm of the gap: too far
                assert (gaps ** 2).sum() > CUTOFF_B2 ** 2 * 0.999      # a margin of the wrong sign culls the pair
            else:
                assert gaps[0] > 14.9 and (gaps[1:] < -0.5).all()      # nested along y and z: without max(0, .) too far
                assert (gaps ** 2).sum() > CUTOFF_B2 ** 2 * 1.001
            if variant == "nested":
                assert (lo[1, 1:] > lo[0, 1:]).all() and (hi[1, 1:] < hi[0, 1:]).all()
    return Case("box-cull", "truth", ("slddt", "lddt"), pred, true, seq, CUTOFF_B2, (128,) * 6, 6, facts, designed)


# ----------------------------------------------------------------------------- B3: rows of one strip that disagree
N_HAIRPIN = 13


def _hairpin_xyz(width, spacing, rng):
    """13 tiles of 64 atoms, uniform in cubes of `width`, centres `spacing` apart along x; the last beside tile 0 at -spacing."""
    centres = np.arange(N_HAIRPIN, dtype=np.float64) * spacing
    centres[-1] = -spacing
    xyz = rng.uniform(-0.5 * width, 0.5 * width, (N_HAIRPIN, TS, 3))
    xyz[:, :, 0] += centres[:, None]
    return xyz.reshape(-1, 3).astype(np.float32)


def _hairpin_facts(case):
    near = near_matrix(case.boxed(0), case.reach() * np.sqrt(1.001))   # (the kernel's 0.1 % on the squares)
    strict = near_matrix(case.boxed(0), case.reach() * np.sqrt(0.999))
    assert np.array_equal(near, strict)                                # no tile pair sits on the margin
    k = np.arange(N_HAIRPIN)
    want = np.abs(k[:, None] - k[None]) <= 1
    want[N_HAIRPIN - 1, N_HAIRPIN - 2] = want[N_HAIRPIN - 2, N_HAIRPIN - 1] = False
    want[0, N_HAIRPIN - 1] = want[N_HAIRPIN - 1, 0] = True
    assert np.array_equal(near, want)
    kept = kept_matrix(near)
    assert kept.shape == (4, N_HAIRPIN) and -(-N_HAIRPIN // CHUNK_TILES) == 2
    assert list(near[:4, 12]) == [True, False, False, False]          # the rows of strip 0 disagree about column tile 12
    assert list(kept[:, 12]) == [True, False, False, True]
    ref = reference(case, case.kernels[0])[0]
    tile = np.searchsorted(case.present(0), ref["slots_i"]) // TS, np.searchsorted(case.present(0), ref["slots_j"]) // TS
    assert ((tile[0] == 0) & (tile[1] == 12)).any() and ((tile[0] == 4) & (tile[1] == 5)).any()      # pairs do cross


def _hairpin_truth(seed):
    rng = np.random.default_rng(seed)
    xyz = _hairpin_xyz(3.0, 12.0, rng)
    pred = xyz + rng.normal(0, 1.0, xyz.shape).astype(np.float32)
    pred, true, seq = stack([place(dense_slots(len(xyz)), xyz, pred, len(xyz) // PER_RES, rng)])
    cutoff = CUTOFF
    settle_truth(pred, true, seq, cutoff, rng)
    settle(pred, true, seq, cutoff, rng)
    return Case("hairpin", "truth", ("slddt", "lddt"), pred, true, seq, cutoff, (832,), 1, _hairpin_facts)


def _hairpin_clash(seed):
    rng = np.random.default_rng(seed)
    xyz = _hairpin_xyz(6.0, 6.5, rng)
    L = len(xyz) // PER_RES
    pred = np.zeros((1, L * SLOTS, 3), np.float32)
    pred[0, dense_slots(len(xyz))] = xyz
    seq = rng.choice(EIGHT_ATOM_TYPES, (1, L)).astype(np.int64)
    settle_clash(pred, seq, rng)
    return Case("hairpin-clash", "clash", ("clash",), pred, None, seq, None, (832,), 1, _hairpin_facts)


# ----------------------------------------------------------------------------- B4: the shares of the compaction
def share_width(L):
    return -(-(-(-L * SLOTS // NWAVE)) // 64) * 64


def fape_prediction(xyz, slots, rng):
    """A prediction whose FAPE deviations stay clear of the 10 A clamp, so that `well_posed_clamp` finds its gap among 300 000
    pairs: 0.1 A off the truth (deviations of an A or two, through the rotation of the frames), and every tenth side-chain atom
    20 A away (clamped by every frame)."""
    pred = xyz + rng.normal(0, 0.1, xyz.shape)
    far = np.nonzero(slots % SLOTS >= 3)[0][::10]
    shift = rng.normal(0, 1, (len(far), 3))
    pred[far] += 20.0 * shift / np.linalg.norm(shift, axis=1, keepdims=True)
    return pred.astype(np.float32)


def _shares(L, empty, single, seed, compact=False):
    """Every slot present but: at each share start s0 the slots s0 - 1, s0, s0 + 63, s0 + 64; share `empty` whole; share `single`
    but one slot.  Residues strung along x - or `compact`, for FAPE alone: on a 6 x 6 x n lattice 3.8 A apart, so that no
    frame-to-atom distance exceeds the 64 A that the value bar of tests/test_gpu_fape.py assumes."""
    rng = np.random.default_rng(seed)
    nslot, per = L * SLOTS, share_width(L)
    ok = np.ones(nslot, bool)
    for s0 in range(per, nslot, per):
        for s in (s0 - 1, s0, s0 + 63, s0 + 64):
            if s < nslot:
                ok[s] = False
    ok[empty * per:(empty + 1) * per] = False
    ok[single * per:(single + 1) * per] = False
    ok[single * per + 37] = True
    slots = np.nonzero(ok)[0]
    xyz = rng.normal(0, 1.5, (len(slots), 3))
    r = slots // SLOTS
    xyz += 3.8 * (np.stack([r % 6, r // 6 % 6, r // 36], 1) if compact else np.stack([r, 0 * r, 0 * r], 1))
    xyz = xyz.astype(np.float32)
    pred = fape_prediction(xyz, slots, rng) if compact else xyz + rng.normal(0, 1.5, xyz.shape).astype(np.float32)
    pred, true, seq = stack([place(slots, xyz, pred, L, rng)])
    cutoff = CUTOFF
    if not compact:
        settle_truth(pred, true, seq, cutoff, rng)
        settle(pred, true, seq, cutoff, rng)

    def facts(c):
        assert per == {74: 128, 147: 192}[L] and nslot == {74: 1036, 147: 2058}[L]
        have = np.zeros(nslot, bool)
        have[c.present(0)] = True
        shares = [have[w * per:(w + 1) * per] for w in range(-(-nslot // per))]
        assert shares[empty].sum() == 0 and shares[single].sum() == 1
        for w in range(1, len(shares)):
            assert not have[w * per - 1] and not have[w * per]
            assert all(not have[s] for s in (w * per + 63, w * per + 64) if s < nslot)
        assert sum(s.sum() > 1 for s in shares) == len(shares) - 2
        if compact:
            ref = reference(c, "fape")[0]
            assert 0 < ref["nclamped"] < ref["npairs"] == len(ref["res"]) * len(slots) and L // 2 < len(ref["res"]) < L
    if compact:
        return Case(f"shares-{L}-fape", "truth", ("fape",), pred, true, seq, None, (len(slots),), 1, facts)
    return Case(f"shares-{L}", "truth", ("slddt", "lddt"), pred, true, seq, cutoff, (len(slots),), 1, facts)


# ----------------------------------------------------------------------------- B2 and B4 for clash: built from residue types
REACH = 2 * 1.8 - clash_ref.TOLERANCE                                  # 2.1 A: two sulfurs; what csrc/clash.hip culls with
MET, SD = clash_ref.AA.index("M"), 6                                   # N CA C O CB CG SD CE: 8 atoms, the sulfur in slot 6


def _box_cull_clash(seed):
    """The two-tile geometry of `_two_tiles` in the PREDICTED coordinates, scaled to the reach of the clash term: 16 MET, a tile
    is 8 of them; the designed pair is the SD of the last residue of tile A and the SD of the first of tile B, REACH - INSIDE
    apart - two sulfurs, the only pair of elements that violates that far out - every other cross pair beyond REACH + 1e-2."""
    rng = np.random.default_rng(seed)
    names = [(v, c) for c in (False, True) for v in ("axis", "diagonal", "nested")]
    L, ia, ib = 2 * TS // PER_RES, TS - PER_RES + SD, TS + SD
    pred = np.zeros((len(names), L * SLOTS, 3), np.float32)
    seq = np.full((len(names), L), MET, np.int64)
    slots = dense_slots(2 * TS)
    for b, (variant, control) in enumerate(names):
        axes = np.array([1.0, 1.0, 1.0]) if variant == "diagonal" else np.array([1.0, 0.0, 0.0])
        g = (REACH - INSIDE) / np.sqrt(axes.sum())
        A = rng.uniform(0, 2, (TS, 3))
        if variant == "nested":
            A[:, 1:] = rng.uniform(0, 3, (TS, 2))
        a_star = np.array([3.0, 3.0, 3.0]) if variant == "diagonal" else np.array([3.0, 1.5, 1.5])
        A[ia] = a_star
        Bt = a_star + axes * (g + 1.0) + rng.uniform(0, 2, (TS, 3)) * axes + (1 - axes) * rng.uniform(-1.5, 1.5, (TS, 3))
        if variant == "nested":
            Bt[:, 1:] = a_star[1:] + rng.uniform(-0.5, 0.5, (TS, 2))
        Bt[ib - TS] = a_star + axes * g
        pred[b, slots] = np.concatenate([A, Bt + axes * control])
    keep = [int(slots[ia]), int(slots[ib])]
    settle_clash(pred, seq, rng, keep=keep)

    def facts(case):
        for b, (variant, control) in enumerate(names):
            x = case.boxed(b)
            d = np.sqrt(((x[:TS, None] - x[None, TS:]) ** 2).sum(-1))
            cross = np.sort(d.ravel())
            gaps = box_gaps(*tile_boxes(x))[0, 1]
            ref = reference(case, "clash")[b]
            hits = np.searchsorted(case.present(b), ref["slots_i"]) // TS != np.searchsorted(case.present(b), ref["slots_j"]) // TS
            if control:
                assert cross[0] > REACH + 0.5 and not near_matrix(x, REACH)[0, 1] and not hits.any()
                continue
            assert 2e-3 <= REACH - cross[0] <= 1e-2 and cross[1] > REACH + 1e-2 and d[ia, ib - TS] == cross[0]
            assert hits.sum() == 1 and (ref["slots_i"][hits][0], ref["slots_j"][hits][0]) == tuple(keep)    # it does violate
            assert near_matrix(x, REACH)[0, 1]
            lo, hi = tile_boxes(x)
            assert np.linalg.norm(0.5 * (lo[0] + hi[0]) - 0.5 * (lo[1] + hi[1])) > REACH + 1.0        # centres: too far
            if variant == "diagonal":
                assert (gaps > 0.5 * REACH).all() and np.abs(gaps).sum() > 1.5 * REACH              # the 1-norm: too far
                assert REACH ** 2 * 0.99 < (gaps ** 2).sum() < REACH ** 2      # (2e-3 A of 2.1 A is more than the kernel's 0.1 %)
            else:
                assert gaps[0] > REACH - 0.1 and (gaps[1:] < -0.5).all() and (gaps ** 2).sum() > REACH ** 2 * 1.001
            if variant == "nested":
                assert (lo[1, 1:] > lo[0, 1:]).all() and (hi[1, 1:] < hi[0, 1:]).all()
    designed = [None if c else tuple(keep) for v, c in names]
    return Case("box-cull-clash", "clash", ("clash",), pred, None, seq, None, (128,) * 6, 6, facts, designed)


ATOMS_OF_TYPE = {int((~np.isnan(clash_ref.radius_table()[r])).sum()): r for r in range(20)}    # atoms -> a residue type with them


def _shares_clash(L, empty, single, seed):
    """The share edges by residue type.  A residue's atoms are its slots 0 .. k - 1, so a slot is empty when its residue has k
    atoms or fewer than the slot's index in it, or is no residue at all (a pad id inside the chain: the kernel and the
    reference skip it).  Every residue gets the largest type that leaves the slots s0 - 1, s0, s0 + 63, s0 + 64 of every share
    start s0 empty; share `empty` holds pad ids only.  One atom alone in a share can only be the last atom of a residue that
    straddles the share's start, so share `single` has its atom AT s0 (and s0 - 1 occupied): the residue across its start has
    s0 % 14 + 1 atoms, pad ids fill the rest of the share."""
    rng = np.random.default_rng(seed)
    nslot, per = L * SLOTS, share_width(L)
    limit = np.full(L, SLOTS)                                          # atoms a residue may have
    for s0 in range(per, nslot, per):
        for s in ((s0 + 63, s0 + 64) if s0 // per == single else (s0 - 1, s0, s0 + 63, s0 + 64)):
            if s < nslot:
                limit[s // SLOTS] = min(limit[s // SLOTS], s % SLOTS)
    for w, keep_first in ((empty, 0), (single, 1)):
        lo, hi = w * per, min((w + 1) * per, nslot)
        for r in range(lo // SLOTS, -(-hi // SLOTS)):
            limit[r] = min(limit[r], max(lo + keep_first - r * SLOTS, 0))
    sizes = sorted(ATOMS_OF_TYPE)
    seq = np.array([ATOMS_OF_TYPE[max(k for k in sizes if k <= lim)] if lim >= sizes[0] else PAD for lim in limit], np.int64)[None]
    slots = clash_ref.atoms_of(seq[0])[0]
    xyz = rng.normal(0, 1.5, (len(slots), 3))
    xyz[:, 0] += 3.8 * (slots // SLOTS)
    pred = np.zeros((1, nslot, 3), np.float32)
    pred[0, slots] = xyz
    settle_clash(pred, seq, rng)

    def facts(c):
        have = np.zeros(nslot, bool)
        have[c.present(0)] = True
        shares = [have[w * per:(w + 1) * per] for w in range(-(-nslot // per))]
        assert shares[empty].sum() == 0 and shares[single].sum() == 1 and have[single * per] and have[single * per - 1]
        for w in range(1, len(shares)):
            assert w == single or (not have[w * per - 1] and not have[w * per])
            assert all(not have[s] for s in (w * per + 63, w * per + 64) if s < nslot)
        last = int(shares[-1].sum() == 0)                             # (L = 74: the 12 slots of the last share belong to a residue
        assert sum(s.sum() > 1 for s in shares) == len(shares) - 2 - last      # whose slots 1 and 2 must be empty: no residue)
        assert reference(c, "clash")[0]["npairs"] > 100
    return Case(f"shares-{L}-clash", "clash", ("clash",), pred, None, seq, None, (len(slots),), 1, facts)


# ----------------------------------------------------------------------------- FAPE: frames by atoms
Z_FAPE = 10.0
FAPE_GRID = [(f, a) for f in (63, 64, 65) for a in (511, 512, 513)]


def frameless_residues(L, frames):
    """The L - frames residues of a row of L residues that lose their CA: 0, 64, 63 and L - 1 first, then from the end backwards."""
    first = list(dict.fromkeys(r for r in (0, 64, 63, L - 1) if r < L))
    return sorted((first + [r for r in range(L - 1, -1, -1) if r not in first])[:L - frames])


def _fape_grid(L, seed):
    """Nine proteins of L residues, none of them padding: 63, 64, 65 frames by 511, 512, 513 atoms.  A residue with a frame has
    N, CA, C (slots 0, 1, 2), a frameless one N and C; the remaining atoms go to the slots from 3 on, spread evenly.  The 64-residue
    loop of fape_frames_kernel ends after (L = 65), on (128) and after (129) a boundary; frames are tiles of 64 (63, 64, 65),
    atoms chunks of 8 tiles (511, 512, 513).  Residue centres N(0, 6 A), atoms 1.5 A around them, the prediction of `fape_prediction`."""
    rng = np.random.default_rng(seed)
    rows = []
    for frames, atoms in FAPE_GRID:
        lost = frameless_residues(L, frames)
        extra = atoms - 3 * frames - 2 * len(lost)
        slots = []
        for r in range(L):
            own = [0, 2] if r in lost else [0, 1, 2]
            slots += [r * SLOTS + s for s in own + list(range(3, 3 + extra // L + (r < extra % L)))]
        slots = np.sort(np.array(slots))
        xyz = (rng.normal(0, 6.0, (L, 3))[slots // SLOTS] + rng.normal(0, 1.5, (len(slots), 3))).astype(np.float32)
        rows.append(place(slots, xyz, fape_prediction(xyz, slots, rng), L, rng))
    pred, true, seq = stack(rows)

    def facts(c):
        from test_gpu_fape import frame_residues
        assert -(-L // TS) == {65: 2, 128: 2, 129: 3}[L] and (c.seq != PAD).all()
        for b, (frames, atoms) in enumerate(FAPE_GRID):
            res = frame_residues(c.true[b], c.seq[b])
            lost = np.setdiff1d(np.arange(L), res)
            assert len(res) == frames and list(lost) == frameless_residues(L, frames)
            assert all(r in lost for r in (0, 64, 63, L - 1)[:min(L - frames, 4 - (L == 65))])
            ref = reference(c, "fape")[b]
            assert ref["npairs"] == frames * atoms and 0 < ref["nclamped"] < ref["npairs"]        # both branches of the clamp
        assert [-(-f // TS) for f, a in FAPE_GRID[::3]] == [1, 1, 2] and [-(-a // (TS * CHUNK_TILES)) for f, a in FAPE_GRID[:3]] == [1, 1, 2]
    return Case(f"fape-grid-{L}", "truth", ("fape",), pred, true, seq, None, tuple(a for f, a in FAPE_GRID), 9, facts)


@functools.lru_cache(maxsize=None)
def fape_clamp(name):
    """The clamp of a FAPE case, placed by `well_posed_clamp` in a gap of the unclamped reference's d; the lever arm is checked."""
    from test_gpu_fape import fape_reference, well_posed_clamp
    c = case(name)
    free = [fape_reference(c.pred[b], c.true[b], c.seq[b], float("inf")) for b in range(c.B)]
    assert max(r["lever"] for r in free) <= 64.0, name
    return well_posed_clamp([r["d"] for r in free])


def fape_table(pred, true, seq, clamp):
    """What every (frame, atom) pair adds: ga [F,A,3] to the atom's slot, gf [F,A,3,3] to the N, CA, C slots of the frame's
    residue (the frame-side terms, through algorithm 21 by autograd), and a bound of the fp32 error of one frame-side term."""
    import torch
    from test_gpu_fape import frame_residues, frames_from_points
    idx, res = present_atoms(true, seq), frame_residues(true, seq)
    L, F, A = len(seq), len(res), len(idx)
    unit = 1.0 / (Z_FAPE * max(F * A, 1))
    t64, p64 = torch.tensor(np.asarray(true, np.float64)), torch.tensor(np.asarray(pred, np.float64))
    bb = lambda x: [x.reshape(L, SLOTS, 3)[torch.tensor(res), k] for k in range(3)]      # noqa: E731
    Rt, tt, _, _ = frames_from_points(*bb(t64))
    P = torch.stack(bb(p64), 1).clone().requires_grad_()             # [F,3,3]: N, CA, C of the frames, apart from their role as atoms
    ga, gf, lever = np.zeros((F, A, 3)), np.zeros((F, A, 3, 3)), np.zeros((F, A))
    is_open = np.zeros((F, A), bool)
    for a0 in range(0, A, TS):
        ai = torch.tensor(idx[a0:a0 + TS])
        n = len(ai)
        Rp, tp, q1, q2 = frames_from_points(P[:, 0], P[:, 1], P[:, 2])
        rp = p64[ai][None] - tp[:, None]
        delta = torch.einsum("fmk,fam->fak", Rp, rp) - torch.einsum("fmk,fam->fak", Rt, t64[ai][None] - tt[:, None])
        d = ((delta ** 2).sum(-1) + 1e-4).sqrt()
        op = d.detach() < clamp
        val = torch.where(op, d, torch.zeros_like(d)) * unit
        (g,) = torch.autograd.grad(val.sum(0), P, torch.eye(n, dtype=torch.float64), is_grads_batched=True)
        gf[:, a0:a0 + n] = g.permute(1, 0, 2, 3).numpy()
        ga[:, a0:a0 + n] = (torch.einsum("fmk,fak->fam", Rp, delta / d[..., None]) * op[..., None] * unit).detach().numpy()
        lever[:, a0:a0 + n] = (rp.norm(dim=-1) / torch.minimum(q1, q2).sqrt()[:, None]).detach().numpy()
        is_open[:, a0:a0 + n] = op.numpy()
    return idx, res, ga, gf, lever, is_open, unit


def fape_scatter(nslot, idx, res, ga, gf):
    g = np.zeros((nslot, 3))
    np.add.at(g, idx, ga.sum(0))
    for k in range(3):
        np.add.at(g, res * SLOTS + k, gf[:, :, k].sum(1))
    return g


def _finish_fape(ref, nslot, idx, res, ga, gf, lever, is_open, unit):
    """scale_i with the frame-side terms; floor_i = 2^-24 * unit per pair for an atom (|g_ij| <= 1), and per pair times
    1 + 2 |r_ij| / min(|v1|, |u2|) for a frame's N, CA, C (g_ij (x) r_ij goes through the backward of algorithm 21)."""
    scale, floor = np.zeros(nslot), np.zeros(nslot)
    np.add.at(scale, idx, np.linalg.norm(ga, axis=-1).sum(0))
    np.add.at(floor, idx, EPS32 * unit * is_open.sum(0))
    for k in range(3):
        np.add.at(scale, res * SLOTS + k, np.linalg.norm(gf[:, :, k], axis=-1).sum(1))
        np.add.at(floor, res * SLOTS + k, EPS32 * unit * ((1 + 2 * lever) * is_open).sum(1))
    ref.update(idx=idx, res=res, ga=ga, gf=gf, open=is_open, scale=scale, floor=floor)
    assert (np.abs(fape_scatter(nslot, idx, res, ga, gf) - ref["grad"]).max(1) <= 1e-9 * scale + 1e-300).all()
    return ref


def fape_mutations(c, b, ref):
    """The mutations of `mutations` for FAPE: the open pair of median weight dropped, its sign flipped, the work item of the last
    frame tile and the first chunk of atom tiles dropped (FAPE has no cull), a gradient moved to the next slot."""
    idx, res, ga, gf, nslot = ref["idx"], ref["res"], ref["ga"], ref["gf"], len(ref["grad"])
    w = np.where(ref["open"], np.linalg.norm(ga, axis=-1), np.nan).ravel()
    k = int(np.argsort(w)[np.isfinite(w).sum() // 2])
    f, a = divmod(k, len(idx))
    one = fape_scatter(nslot, idx[a:a + 1], res[f:f + 1], ga[f:f + 1, a:a + 1], gf[f:f + 1, a:a + 1])
    out = {"pair dropped": ref["grad"] - one, "sign flipped": ref["grad"] - 2 * one}
    f0, a1 = (len(res) - 1) // TS * TS, CHUNK_TILES * TS
    out["work item dropped"] = ref["grad"] - fape_scatter(nslot, idx[:a1], res[f0:], ga[f0:, :a1], gf[f0:, :a1])
    moved = ref["grad"].copy()
    live = np.nonzero(ref["scale"][idx] > 0)[0]                       # (a clamped atom has no gradient to move)
    first = live[live >= (-(-len(idx) // TS) - 1) * TS]
    s = int(idx[first[0] if len(first) else live[-1]])                # the first such atom of the last tile, else the last before it
    moved[s + 1] += moved[s]
    moved[s] = 0.0
    out["gradient moved one slot"] = moved
    return out


BUILDERS = {
    "fape-grid-65": lambda: _fape_grid(65, 61),
    "fape-grid-128": lambda: _fape_grid(128, 62),
    "fape-grid-129": lambda: _fape_grid(129, 63),
    "shares-74-fape": lambda: _shares(74, 3, 5, 64, compact=True),
    "shares-147-fape": lambda: _shares(147, 4, 7, 65, compact=True),
    "box-cull-clash": lambda: _box_cull_clash(53),
    "shares-74-clash": lambda: _shares_clash(74, 4, 2, 54),
    "shares-147-clash": lambda: _shares_clash(147, 5, 1, 55),
    "counts": lambda: _counts_truth("counts", (255, 256, 257, 511, 512, 513), ("slddt", "lddt"), 11),
    "counts-lddt": lambda: _counts_truth("counts-lddt", (2047, 2048, 2049), ("lddt",), 12),
    "box-cull": lambda: _box_cull(21),
    "hairpin": lambda: _hairpin_truth(31),
    "shares-74": lambda: _shares(74, 3, 5, 41),
    "shares-147": lambda: _shares(147, 4, 7, 42),
    "counts-clash": lambda: _counts_clash(51),
    "hairpin-clash": lambda: _hairpin_clash(52),
}
RUNS = [(name, kernel) for name, kernels in (
    ("counts", ("slddt", "lddt")), ("counts-lddt", ("lddt",)), ("box-cull", ("slddt", "lddt")), ("hairpin", ("slddt", "lddt")),
    ("shares-74", ("slddt", "lddt")), ("shares-147", ("slddt", "lddt")), ("counts-clash", ("clash",)),
    ("hairpin-clash", ("clash",)), ("box-cull-clash", ("clash",)), ("shares-74-clash", ("clash",)),
    ("shares-147-clash", ("clash",)), ("fape-grid-65", ("fape",)), ("fape-grid-128", ("fape",)), ("fape-grid-129", ("fape",)),
    ("shares-74-fape", ("fape",)), ("shares-147-fape", ("fape",))) for kernel in kernels]


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


# ----------------------------------------------------------------------------- pair tables and references
def slddt_pairs(pred, true, seq, cutoff, tau=TAU):
    """(slots_i, slots_j, c [pairs, 3]): pair (i, j), i before j in slot order, adds +c to d loss / d pred of i and -c to j."""
    idx, dt, other = true_distances(true, seq)
    ii, jj = np.nonzero(np.triu(other & (dt < cutoff), 1))
    p = np.asarray(pred, np.float64)[idx]
    diff = p[ii] - p[jj]
    dp = np.sqrt((diff ** 2).sum(-1) + 1e-30)
    sd = dp - dt[ii, jj]
    sig = [1.0 / (1.0 + np.exp(np.minimum((np.abs(sd) - t) / tau, 700.0))) for t in THRESHOLDS]
    w = sum(s * (1 - s) for s in sig) / (4.0 * tau * max(len(ii), 1))
    return idx[ii], idx[jj], (w * np.sign(sd) / dp)[:, None] * diff


def clash_pairs(crd, seq):
    idx, ii, jj, over = clash_margins(crd, seq)
    hit = over > 0
    x = np.asarray(crd, np.float64)[idx]
    diff = x[ii[hit]] - x[jj[hit]]
    d = np.sqrt((diff ** 2).sum(-1) + 1e-30)
    return idx[ii[hit]], idx[jj[hit]], -diff / d[:, None] / len(idx)


def scatter(nslot, si, sj, c):
    g = np.zeros((nslot, 3))
    np.add.at(g, si, c)
    np.add.at(g, sj, -c)
    return g


def _finish(ref, nslot, si, sj, c, unit):
    """Adds the pair table, scale_i and floor_i = 2^-24 * unit per contributing pair (`unit` bounds one pair term: a pair's
    weight is computed in fp32 with an absolute error of that order however small the weight itself is - a saturated logistic
    is exactly 0 on the device and 1e-18 in fp64)."""
    mag = np.linalg.norm(c, axis=1)
    scale, cnt = np.zeros(nslot), np.zeros(nslot)
    for s in (si, sj):
        np.add.at(scale, s, mag)
        np.add.at(cnt, s, 1.0)
    ref.update(slots_i=si, slots_j=sj, c=c, scale=scale, floor=EPS32 * unit * cnt)
    assert (np.abs(scatter(nslot, si, sj, c) - ref["grad"]).max(1) <= 1e-9 * scale + 1e-300).all()      # the table IS the reference
    return ref


@functools.lru_cache(maxsize=None)
def _reference(name, kernel):
    c = case(name)
    nslot = c.L * SLOTS
    out = []
    for b in range(c.B):
        if kernel == "slddt":
            loss, n, grad, delta = slddt_reference(c.pred[b], c.true[b], c.seq[b], c.cutoff, TAU)
            assert n == 0 or delta.min() >= 1e-5
            ref = dict(loss=loss, npairs=n, grad=grad)
            out.append(_finish(ref, nslot, *slddt_pairs(c.pred[b], c.true[b], c.seq[b], c.cutoff), 1.0 / (4 * TAU * max(n, 1))))
        elif kernel == "fape":
            from test_gpu_fape import fape_reference
            r = fape_reference(c.pred[b], c.true[b], c.seq[b], fape_clamp(name))
            ref = dict(loss=r["loss"], npairs=r["npairs"], nclamped=r["nclamped"], grad=r["grad"])
            out.append(_finish_fape(ref, nslot, *fape_table(c.pred[b], c.true[b], c.seq[b], fape_clamp(name))))
        elif kernel == "clash":
            loss, n, atoms, grad, margin = clash_ref.clash_reference(c.pred[b], c.seq[b])
            ref = dict(loss=loss, npairs=n, grad=grad, atoms=atoms)
            out.append(_finish(ref, nslot, *clash_pairs(c.pred[b], c.seq[b]), 1.0 / max(atoms, 1)))
        else:
            lo, hi = lddt_reference(c.pred[b], c.true[b], c.seq[b], c.cutoff, eps=LDDT_EPS)
            assert np.array_equal(lo, hi), (name, b)                   # the counts are one number
            out.append(dict(counts=lo, npairs=int(lo[:, 0, 0].sum())))
    return out


def reference(c, kernel):
    """Per protein, computed once and shared: slddt and clash dict(loss, npairs, grad [L*14,3], scale [L*14], floor [L*14],
    slots_i, slots_j, c); lddt dict(counts [L,2,5], npairs); fape dict(loss, npairs, nclamped, grad, scale, floor and the table
    of `fape_table`)."""
    return _reference(c.name, kernel)


# ----------------------------------------------------------------------------- the per-atom bar and what it must reject
def atom_errors(got, ref):
    """err_i = max over x, y, z of |got - ref| per slot."""
    return np.abs(np.asarray(got, np.float64) - ref["grad"]).max(1)


def worst_ratio(got, ref):
    """max over the atoms of (err_i - floor_i) / scale_i: what K is 8 times of."""
    err, live = atom_errors(got, ref), ref["scale"] > 0
    return float((np.maximum(err - ref["floor"], 0)[live] / ref["scale"][live]).max()) if live.any() else 0.0


def excess(got, ref, kernel):
    """max over the slots of err_i / (K scale_i + floor_i); <= 1 passes.  A slot without a pair has scale = floor = 0: anything
    but an exact zero there is an infinite excess."""
    err = atom_errors(got, ref)
    bar = K[kernel] * ref["scale"] + ref["floor"]
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(err > 0, err / bar, 0.0).max())


def mutations(c, b, ref):
    """name -> the fp64 gradient of protein b with one defect: a pair dropped (the designed pair where the case has one, else
    the pair of median weight), the tile pair with the fewest pairs culled, the gradient of the first atom of the last tile that
    has a pair moved to the next slot, the sign of that one pair's coefficient flipped."""
    if "ga" in ref:
        return fape_mutations(c, b, ref)
    si, sj, cc, nslot = ref["slots_i"], ref["slots_j"], ref["c"], len(ref["grad"])
    if c.designed[b] is not None:
        k = int(np.nonzero((si == c.designed[b][0]) & (sj == c.designed[b][1]))[0][0])
    else:
        k = int(np.argsort(np.linalg.norm(cc, axis=1))[len(cc) // 2])
    one = scatter(nslot, si[k:k + 1], sj[k:k + 1], cc[k:k + 1])
    out = {"pair dropped": ref["grad"] - one, "sign flipped": ref["grad"] - 2 * one}
    present = c.present(b)
    ti, tj = np.searchsorted(present, si) // TS, np.searchsorted(present, sj) // TS
    tiles = -(-len(present) // TS)
    code = ti * tiles + tj
    codes, n = np.unique(code, return_counts=True)
    cull = code == codes[np.argmin(n)]
    out["tile pair culled"] = ref["grad"] - scatter(nslot, si[cull], sj[cull], cc[cull])
    moved = ref["grad"].copy()
    live = np.nonzero(ref["scale"][present] > 0)[0]                   # (positions of the atoms that have a pair)
    first = live[live >= (tiles - 1) * TS]
    a = int(present[first[0] if len(first) else live[-1]])            # the first such atom of the last tile, else the last before it
    moved[a + 1] += moved[a]
    moved[a] = 0.0
    out["gradient moved one slot"] = moved
    return out
