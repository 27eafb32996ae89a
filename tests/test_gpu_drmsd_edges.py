"""MI355X tests of csrc/drmsd.hip alone, PER ATOM against the fp64 restatement tests/drmsd_ref.py, with the atom counts on the
edges of its tiles (64 atoms), strips (256), 4- and 8-tile chunks (256 / 512) and of the backbone / other boundary inside a tile.

The coordinates are written here (truth N(0, 8 A); prediction independent of it - "far" - or truth + N(0, 0.5 A) - "near"), rounded
to fp32 before the reference sees them: no NeRF, no model, no conditioning of a chain in the bars.  `losses.drmsd_forward_backward`
is called directly, with and without `backbone_only` and `partial_budget_bytes`.

Bars:
  * n, n_bb and entries 6, 7 of the statistics exact; gradient slots of absent atoms, padded residues and proteins without a pair
    exact zeros; statistics of an empty pair set NaN exactly where the reference's are.
  * D, D/n, D_bb, D_bb/n_bb: inside the project's rel 1e-4 / abs 1e-6, and relative error <= C_STAT stat_unit, the reference's
    own figure for one fp32 rounding of every d and tau carried through D plus the final roundings (tests/drmsd_ref.py).  A flat
    relative bar below 1e-6 does not exist: the measured worst is 2.4e-6, at n = 2 in the "near" regime, where d - tau cancels
    (from 63 atoms on the measured worst is 3e-7, 7e-8 in the "far" regime).  The loss partials are fp64.
  * per atom |g_i - g_ref,i| <= C_ATOM unit_i, with unit_i = 2^-24 scale sum_j (d_ij + tau_ij) from the REFERENCE: the fp32 rounding
    of every d and tau of the atom, carried through cf (x_i - x_j).  C_ATOM = 4 x the worst measured ratio, rounded up to a power of two.
  * sensitivity, from the reference alone: in every "far" case with n >= 3, for every atom at least 90 % of its pairs have
    pairmove_ij = scale |d_ij - tau_ij| > 2 C_ATOM unit_i - losing or doubling almost any single pair of any atom breaks the bar.
    ("near" cases assert the bar only: their |d - tau| is a fraction of an Angstrom and at n = 1025 the condition does not hold.)
  * bits: a permutation of the batch permutes the results, other proteins' contents do not reach a protein, forward-only and
    gradient calls agree on the statistics, two runs agree, a sweep in passes gives the bits of one launch.
"""
import numpy as np
import pytest
import torch

import drmsd_ref

pytestmark = pytest.mark.gpu

# Measured on the MI355X over every case of this file (printed per case by the tests):
#   worst |g_i - g_ref,i| / unit_i: 2.62 (n = 512 in the 8-tile layout, "far"; 0.45 in the "near" regime); C_ATOM = 4 x that,
#   rounded up to a power of two
#   worst relative error of a statistic / stat_unit: 0.86 (n = 2, backbone call); C_STAT = 4 x that, rounded up to a power of two
C_ATOM = 16.0
C_STAT = 4.0
PROJECT_REL, PROJECT_ABS = 1e-4, 1e-6          # per-protein drmsd / lndrmsd

SIGMA, NEAR_SIGMA = 8.0, 0.5
DEGENERATE = [(0, 0), (1, 1), (0, 1), (2, 2), (1, 2), (2, 3)]
N_EDGES = [63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025]
NBB_EDGES = [63, 64, 65, 128, 255, 256, 257]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


# --------------------------------------------------------------------------- inputs
def make_protein(rng, L_pad, n_res, n_bb, n, regime, spr=14):
    """One protein with exactly n present atoms of the call's slot space (spr = 14: every slot, n_bb of them backbone; spr = 3: the
    backbone slots alone, n == n_bb), reached by writing NaN into chosen truth slots.  Where the counts leave room the absent set
    holds the first and the last slot of the protein and a whole row of 64 slots (64..127 of the call's slot space); an absent slot
    has NaN in all three coordinates, or in x, y or z alone.  Padded residues hold finite garbage in both structures.
    -> (pred [L_pad*14, 3], true [L_pad*14, 3], seq [L_pad]) fp32 / int64, and the set of patterns that were written."""
    true = rng.normal(0, SIGMA, (L_pad * 14, 3))
    pred = rng.normal(0, SIGMA, (L_pad * 14, 3)) if regime == "far" else true + rng.normal(0, NEAR_SIGMA, (L_pad * 14, 3))
    true, pred = true.astype(np.float32), pred.astype(np.float32)
    seq = np.full(L_pad, 20, np.int64)
    seq[:n_res] = rng.integers(0, 20, n_res)
    slots = np.arange(n_res * 14)
    if spr == 3:
        n_bb = n
        space = slots[slots % 14 < 3]                            # the call's slot space, as truth slots, in compact order
    else:
        space = slots
    forced = np.zeros(len(space), bool)
    if len(space):
        forced[[0, -1]] = True
    if len(space) >= 192:
        forced[64:128] = True
    is_bb = space % 14 < 3
    present = np.zeros(len(space), bool)
    patterns = set()
    for cls, want in ((is_bb, n_bb), (~is_bb, n - n_bb)):
        free = np.nonzero(cls & ~forced)[0]
        if len(free) < want:                                     # no room for the patterns in this class
            free = np.nonzero(cls)[0]
        assert len(free) >= want, (n_res, n_bb, n, spr)
        if want:
            present[rng.choice(free, want, replace=False)] = True
    if len(space) and not present[0] and not present[-1]:
        patterns.add("first and last")
    if len(space) >= 192 and not present[64:128].any():
        patterns.add("row of 64")
    for s in space[~present]:
        style = int(rng.integers(0, 4))
        if style == 0:
            true[s] = np.nan
        else:
            true[s, style - 1] = np.nan
            patterns.add("xyz"[style - 1] + " only")
    if spr == 3:                                                 # side-chain slots of the truth: the backbone call must not look
        other = slots[slots % 14 >= 3]
        true[other[rng.random(len(other)) < 0.3], 1] = np.nan
    return pred, true, seq, patterns


def make_batch(cases, L_pad, regime, seed, spr=14):
    """cases: [(n_res, n_bb, n)] -> dict of numpy arrays pred [B, L*14, 3], true, seq, and the cases."""
    rng = np.random.default_rng(seed)
    out = [make_protein(rng, L_pad, n_res, n_bb, n, regime, spr) for n_res, n_bb, n in cases]
    return dict(pred=np.stack([o[0] for o in out]), true=np.stack([o[1] for o in out]), seq=np.stack([o[2] for o in out]),
                cases=list(cases), patterns=set().union(*[o[3] for o in out]), regime=regime, L=L_pad)


def bb_of(pred):
    """the compact [B, L*3, 3] backbone of a [B, L*14, 3] array"""
    B = pred.shape[0]
    return np.ascontiguousarray(pred.reshape(B, -1, 14, 3)[:, :, :3].reshape(B, -1, 3))


def natural_bb(n):
    return round(3 * n / 14)


def res_for(slots_needed, per_res, L_pad):
    """residues that hold `slots_needed` slots of a class with `per_res` per residue, plus room for the absent patterns"""
    return min(L_pad, -(-(slots_needed + 80) // per_res) + 2)


L14, L3 = 96, 448                                               # 1344 atom slots = 21 tiles = 6 strips in either call


def full_atom_cases():
    cases = [(2 + k % 4, nb, n) for k, (nb, n) in enumerate(DEGENERATE)]
    cases += [(res_for(n - natural_bb(n), 11, L14), natural_bb(n), n) for n in N_EDGES]
    cases += [(L14, nb, 700 + k) for k, nb in enumerate(NBB_EDGES)]               # n_bb on an edge inside a larger protein
    cases += [(50, 130, 130), (30, 0, 130), (0, 0, 0)]                             # backbone only; no backbone; no residue at all
    return cases


def backbone_cases():
    cases = [(2 + k, n, n) for k, n in enumerate((0, 1, 2, 3))]
    cases += [(res_for(n, 3, L3), n, n) for n in N_EDGES]
    cases += [(90, 130, 130), (0, 0, 0)]
    return cases


def references(batch, spr):
    pred = batch["pred"] if spr == 14 else bb_of(batch["pred"])
    return [drmsd_ref.drmsd_reference(pred[b], batch["true"][b], batch["seq"][b], spr=spr) for b in range(len(pred))]


@pytest.fixture(scope="module")
def edge_batches():
    """The two edge batches per regime with their fp64 references, computed once and left unchanged."""
    out = {}
    for regime, seed in (("far", 1), ("near", 2)):
        b14 = make_batch(full_atom_cases(), L14, regime, seed)
        b3 = make_batch(backbone_cases(), L3, regime, seed + 10, spr=3)
        for b in (b14, b3):
            assert {"first and last", "row of 64", "y only", "z only"} <= b["patterns"], b["patterns"]
        b14["ref14"], b14["ref3"], b3["ref3"] = references(b14, 14), references(b14, 3), references(b3, 3)
        for b, key in ((b14, "ref14"), (b3, "ref3")):            # the counts are the targets, exactly
            for (n_res, nb, n), r in zip(b["cases"], b[key]):
                assert (r["n_bb"], r["n"]) == (nb, n), (n_res, nb, n, r["n_bb"], r["n"])
        out[regime] = (b14, b3)
    return out


def run(dev, batch, backbone_only=False, need_grad=True, budget=0, idx=None):
    """-> (stats [B, 8], grad [B, L*spr, 3] or None) as numpy, from one call on the device"""
    from protein_transformer_amd.losses import drmsd_forward_backward
    pred = bb_of(batch["pred"]) if backbone_only else batch["pred"]
    true, seq = batch["true"], batch["seq"]
    if idx is not None:
        pred, true, seq = pred[idx], true[idx], seq[idx]
    s, g = drmsd_forward_backward(torch.from_numpy(np.ascontiguousarray(pred)).to(dev), torch.from_numpy(np.ascontiguousarray(true)).to(dev),
                                  torch.from_numpy(np.ascontiguousarray(seq)).to(dev), need_grad=need_grad, partial_budget_bytes=budget,
                                  backbone_only=backbone_only)
    torch.cuda.synchronize()
    return s.cpu().numpy(), None if g is None else g.cpu().numpy()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# --------------------------------------------------------------------------- the bars
def check_protein(what, stats, grad, ref, regime, bb_call):
    """Every per-protein assertion of this file; -> (worst per-atom ratio, worst relative error of the four statistics)."""
    n, n_bb = ref["n"], ref["n_bb"]
    rs = ref["stats"].copy()
    if bb_call:
        rs[[0, 1, 4]] = rs[[2, 3, 5]]                           # the backbone call mirrors its numbers
    assert stats[4] == rs[4] and stats[5] == rs[5] and stats[6] == 0 and stats[7] == 0, (what, stats)
    stat_err = stat_ratio = 0.0
    for k in range(4):
        if np.isnan(rs[k]):
            assert np.isnan(stats[k]), (what, k, stats[k])      # the mean over an empty pair set
            continue
        err = abs(float(stats[k]) - rs[k]) / rs[k]
        unit = ref["stat_unit"][k if not bb_call else 2 + k % 2]
        stat_err, stat_ratio = max(stat_err, err), max(stat_ratio, err / unit)
        print(f"{what}: statistic {k}: {float(stats[k]):.9g} (fp64 {rs[k]:.9g}), relative error {err:.2e} = {err / unit:.3f} stat_unit")
        assert err <= C_STAT * unit and err <= PROJECT_REL, (what, k, float(stats[k]), rs[k], err, unit)
        if k in (1, 3):
            assert abs(float(stats[k]) - rs[k]) <= PROJECT_ABS
    absent = np.ones(len(grad), bool)
    absent[ref["slots"]] = False
    assert np.all(grad[absent] == 0), what                       # (NaN == 0 is False: a NaN fails here)
    if n < 2:
        assert np.all(grad == 0), what
        print(f"{what}: (n_bb, n) = ({n_bb}, {n}): no pair, zero gradient, statistics {stats[:4]}")
        return 0.0, stat_err, stat_ratio
    assert np.isfinite(grad).all(), what
    err = np.linalg.norm(grad[ref["slots"]].astype(np.float64) - ref["grad"][ref["slots"]], axis=1)
    ratio = err / ref["unit"]
    worst = float(ratio.max())
    line = f"{what}: (n_bb, n) = ({n_bb}, {n}) {regime}: worst |g_i - ref| / unit_i {worst:.3f} (atom {int(ratio.argmax())}), statistics rel {stat_err:.2e} = {stat_ratio:.3f} stat_unit"
    if regime == "far" and n >= 3:
        room = ref["pairmove_p10"] / (2.0 * ref["unit"])        # the condition holds for every c below min_i of this
        line += f", sensitivity holds up to c = {float(room.min()):.1f}"
        print(line)
        assert np.all(ref["pairmove_p10"] > 2.0 * C_ATOM * ref["unit"]), (what, float(room.min()))
    else:
        print(line)
    assert worst <= C_ATOM, (what, worst, int(ratio.argmax()))
    return worst, stat_err, stat_ratio


def check_batch(what, stats, grad, refs, regime, bb_call, only=None):
    worst = (0.0, 0.0, 0.0)
    for b, ref in enumerate(refs):
        if only is not None and b not in only:
            continue
        w = check_protein(f"{what}[{b}]", stats[b], grad[b], ref, regime, bb_call)
        worst = tuple(max(a, b) for a, b in zip(worst, w))
    print(f"{what} {regime}: WORST per-atom ratio {worst[0]:.3f}, WORST statistics relative error {worst[1]:.2e} = {worst[2]:.3f} stat_unit")
    return worst


# --------------------------------------------------------------------------- 1. tile, strip and n_bb edges, degenerate proteins
@pytest.mark.parametrize("regime", ["far", "near"])
def test_full_atom_call_at_its_edges(dev, edge_batches, regime):
    b14, _ = edge_batches[regime]
    stats, grad = run(dev, b14)
    check_batch("full-atom", stats, grad, b14["ref14"], regime, False)
    again = run(dev, b14)
    assert same_bits(stats, again[0]) and same_bits(grad, again[1])                  # two runs
    assert same_bits(stats, run(dev, b14, need_grad=False)[0])                       # forward-only


@pytest.mark.parametrize("regime", ["far", "near"])
def test_backbone_call_at_its_edges(dev, edge_batches, regime):
    b14, b3 = edge_batches[regime]
    stats, grad = run(dev, b3, backbone_only=True)
    check_batch("backbone", stats, grad, b3["ref3"], regime, True)
    again = run(dev, b3, backbone_only=True)
    assert same_bits(stats, again[0]) and same_bits(grad, again[1])
    assert same_bits(stats, run(dev, b3, backbone_only=True, need_grad=False)[0])
    # the backbone of the full-atom batch: n_bb on the edges again, now as the call's n, beside truth rows with side chains
    stats, grad = run(dev, b14, backbone_only=True)
    check_batch("backbone of the full-atom batch", stats, grad, b14["ref3"], regime, True)


# --------------------------------------------------------------------------- 2. the 8-tile chunk layout
CHUNK_L = 512
BIG = {14: [(512, natural_bb(n), n) for n in (2100, 512, 513, 1025)], 3: [(512, n, n) for n in (1500, 512, 513, 1025)]}
CHUNK_B = {14: (13, 12), 3: (214, 213)}                         # (8-tile chunks, 4-tile chunks) at L = 512


@pytest.fixture(scope="module")
def chunk_batches():
    """Per call: the small proteins (2 to 5 residues) of the batch, and the variants of the one long protein with references."""
    out = {}
    for spr in (14, 3):
        B = CHUNK_B[spr][0]
        rng = np.random.default_rng(40 + spr)
        small = []
        for k in range(B - 1):
            n_res = 2 + k % 4
            cap = n_res * 3 if spr == 3 else n_res * 14
            n = int(rng.integers(2, cap - 1))
            nb = n if spr == 3 else int(rng.integers(max(0, n - n_res * 11), min(n, n_res * 3) + 1))
            small.append((n_res, nb, n))
        tiny = make_batch(small, CHUNK_L, "far", 50 + spr, spr)
        tiny["ref"] = references(tiny, spr)
        big = []
        for k, case in enumerate(BIG[spr]):
            for regime in (("far", "near") if case[2] == 1025 else ("far",)):
                one = make_batch([case], CHUNK_L, regime, 60 + spr + k, spr)
                one["ref"] = references(one, spr)
                assert (one["ref"][0]["n_bb"], one["ref"][0]["n"]) == case[1:]
                big.append(one)
        out[spr] = (tiny, big)
    return out


@pytest.mark.parametrize("spr", [14, 3])
def test_both_chunk_widths_against_fp64(dev, chunk_batches, spr):
    from protein_transformer_amd import _lib
    lib = _lib.lib()
    tiny, big = chunk_batches[spr]
    B8, B4 = CHUNK_B[spr]
    size = lib.ptamd_drmsd_workspace_bytes if spr == 14 else lib.ptamd_drmsd_bb_workspace_bytes
    assert size(B8, CHUNK_L) * B4 != size(B4, CHUNK_L) * B8                          # the two batches are cut differently
    assert drmsd_ref.tri_layout(CHUNK_L * spr, B8)["chunk_tiles"] == 8 and drmsd_ref.tri_layout(CHUNK_L * spr, B4)["chunk_tiles"] == 4
    for one in big:
        results = {}
        for B in (B8, B4):
            # the long protein last but one: not at either end of the batch
            batch = {k: np.concatenate([tiny[k][:B - 2], one[k], tiny[k][B - 2:B - 1]]) for k in ("pred", "true", "seq")}
            refs = tiny["ref"][:B - 2] + one["ref"] + tiny["ref"][B - 2:B - 1]
            stats, grad = run(dev, batch, backbone_only=spr == 3)
            what = f"spr {spr}, B = {B} ({8 if B == B8 else 4}-tile chunks)"
            check_batch(what, stats, grad, refs, one["regime"], spr == 3, only={B - 2})
            check_batch(what + " small", stats, grad, refs, "far", spr == 3, only=set(range(0, B - 2, 7)) | {B - 1})
            assert same_bits(stats, run(dev, batch, backbone_only=spr == 3, need_grad=False)[0])
            results[B] = (stats[B - 2], grad[B - 2])
        # the same protein through both layouts: the same numbers to rounding (each was just held against fp64)
        assert np.allclose(results[B8][0], results[B4][0], rtol=2 * C_STAT * float(one["ref"][0]["stat_unit"].max()), atol=0)


# --------------------------------------------------------------------------- 3. the sweep in passes
@pytest.mark.parametrize("backbone_only", [False, True])
def test_passes_give_the_bits_of_one_launch(dev, edge_batches, backbone_only):
    from protein_transformer_amd import _lib
    lib = _lib.lib()
    b14, b3 = edge_batches["far"]
    batch, spr, refs = (b3, 3, b3["ref3"]) if backbone_only else (b14, 14, b14["ref14"])
    want = [(nb, n) for nb, n in ((3, 3), (65, 65), (257, 257), (513, 513), (1025, 1025))] if backbone_only else \
        [(2, 3), (natural_bb(65), 65), (natural_bb(257), 257), (256, 705), (natural_bb(1025), 1025)]
    idx = [[(c[1], c[2]) for c in batch["cases"]].index(w) for w in want]
    B, L = len(idx), batch["L"]
    size = lib.ptamd_drmsd_bb_workspace_bytes_budget if backbone_only else lib.ptamd_drmsd_workspace_bytes_budget
    one = drmsd_ref.layout(B, L, 0, spr)
    assert one["strips"] >= 5 and one["spp"] == one["strips"] and size(B, L, 0) == one["total"]
    s1, g1 = run(dev, batch, backbone_only, idx=idx)
    check_batch("one launch", s1, g1, [refs[i] for i in idx], "far", backbone_only)
    # layout() in csrc/drmsd.hip: per_strip = B (chunks RS + tiles TS) sizeof(float4) bytes of partials per strip, spp = budget / per_strip
    per_strip = B * (one["chunks"] * drmsd_ref.RS + one["tiles"] * drmsd_ref.TS) * 16
    assert per_strip == one["per_strip"]
    for budget, spp in ((per_strip, 1), (4 * per_strip + per_strip // 2, 4)):
        cut = drmsd_ref.layout(B, L, budget, spr)
        assert cut["spp"] == spp and (spp == 1 or one["strips"] % spp != 0)
        assert size(B, L, budget) == cut["total"] < one["total"]                     # really in passes
        for need_grad in (True, False):
            s2, g2 = run(dev, batch, backbone_only, need_grad=need_grad, budget=budget, idx=idx)
            assert same_bits(s1, s2), (budget, need_grad)
            assert g2 is None if not need_grad else same_bits(g1, g2), (budget, need_grad)


# --------------------------------------------------------------------------- 4. bits across the batch
@pytest.mark.parametrize("backbone_only", [False, True])
def test_a_protein_does_not_see_its_batch(dev, edge_batches, backbone_only):
    b14, b3 = edge_batches["far"]
    batch = b3 if backbone_only else b14
    B = len(batch["cases"])
    s1, g1 = run(dev, batch, backbone_only)
    # a permutation of the proteins permutes the results
    perm = np.random.default_rng(5).permutation(B)
    s2, g2 = run(dev, batch, backbone_only, idx=perm)
    assert same_bits(s1[perm], s2) and same_bits(g1[perm], g2)
    # other contents in every other slot of the batch: proteins without a pair where there were long ones and the other way round
    keep = np.arange(B) % 3 == 0
    other = make_batch(batch["cases"][::-1], batch["L"], "far", 99, 3 if backbone_only else 14)
    mixed = {k: np.where(keep.reshape(-1, *[1] * (batch[k].ndim - 1)), batch[k], other[k]) for k in ("pred", "true", "seq")}
    kinds = {(c[2] < 2) for c, kp in zip(batch["cases"], keep) if kp}
    assert kinds == {True, False}                                # proteins with and without a pair among the kept
    assert any((a[2] < 2) != (b[2] < 2) for a, b, kp in zip(batch["cases"], other["cases"], keep) if not kp)
    s3, g3 = run(dev, mixed, backbone_only)
    assert same_bits(s1[keep], s3[keep]) and same_bits(g1[keep], g3[keep])
    assert not same_bits(s1[~keep], s3[~keep])


# --------------------------------------------------------------------------- 5. the contract for proteins without a pair
@pytest.mark.parametrize("backbone_only", [False, True])
def test_proteins_without_a_pair(dev, edge_batches, backbone_only):
    """include/ptamd.h: fewer than two present atoms = a zero gradient and NaN statistics, in both calls, next to proteins that
    keep their bits.  (Before this test the full-atom call wrote scale * 0 = NaN into the slot of a single present atom.)"""
    b14, b3 = edge_batches["far"]
    batch, refs = (b3, b3["ref3"]) if backbone_only else (b14, b14["ref14"])
    stats, grad = run(dev, batch, backbone_only)
    lone = [b for b, r in enumerate(refs) if r["n"] < 2]
    assert sorted(refs[b]["n"] for b in lone) == ([0, 0, 1] if backbone_only else [0, 0, 1, 1])
    for b in lone:
        assert np.all(grad[b] == 0) and np.isnan(stats[b, :4]).all(), (b, stats[b])
        assert stats[b, 4] == refs[b]["n"] and stats[b, 5] == refs[b]["n_bb"] and stats[b, 6] == 0 and stats[b, 7] == 0
    if not backbone_only:                                        # a backbone without a pair inside a protein with pairs
        for b, r in enumerate(refs):
            if r["n"] >= 2 and r["n_bb"] < 2:
                assert np.isnan(stats[b, 2:4]).all() and np.isfinite(stats[b, :2]).all() and np.isfinite(grad[b]).all(), b
        assert any(r["n"] >= 130 and r["n_bb"] == 0 for r in refs)
    # the same batch without them: the others keep their bits
    rest = [b for b in range(len(refs)) if b not in lone]
    fill = make_batch([(20, 30, 100 if not backbone_only else 30)] * len(lone), batch["L"], "far", 77, 3 if backbone_only else 14)
    swapped = {k: batch[k].copy() for k in ("pred", "true", "seq")}
    for k in swapped:
        swapped[k][lone] = fill[k]
    s2, g2 = run(dev, swapped, backbone_only)
    assert same_bits(stats[rest], s2[rest]) and same_bits(grad[rest], g2[rest])
    assert np.isfinite(s2[lone][:, :2]).all() and np.isfinite(g2[lone]).all() and np.abs(g2[lone]).max() > 0


@pytest.mark.parametrize("backbone_only", [False, True])
def test_prediction_equal_to_truth(dev, backbone_only):
    """D = 0: statistics exactly 0 (e = d - tau is formed from two identically rounded numbers).  With a gradient requested the
    scale 1 / (n P D) is infinite, as sqrt'(0) is in the reference's autograd, and every sum it multiplies is exactly 0: the
    present atoms' gradient is NaN in the kernel as in the reference.  Recorded here (printed and held to `NaN or 0`), not changed."""
    spr = 3 if backbone_only else 14
    batch = make_batch([(24, 20, 20 if backbone_only else 100), (20, 40, 40 if backbone_only else 180), (9, 9, 9 if backbone_only else 30)],
                       24, "far", 31, spr)
    same = {k: batch[k].copy() for k in ("pred", "true", "seq")}
    present = ~np.isnan(batch["true"][1]).any(-1)
    same["pred"][1][present] = batch["true"][1][present]
    refs = references(batch, spr)
    s0, g0 = run(dev, batch, backbone_only)
    s1, g1 = run(dev, same, backbone_only)
    assert same_bits(s1[1, :4], np.zeros(4, np.float32)), s1[1]
    assert s1[1, 4] == refs[1]["n"] and s1[1, 5] == refs[1]["n_bb"]
    assert same_bits(s1[1], run(dev, same, backbone_only, need_grad=False)[0][1])
    slots = refs[1]["slots"]
    absent = np.ones(len(g1[1]), bool)
    absent[slots] = False
    assert np.all(g1[1][absent] == 0)
    got = g1[1][slots]
    print(f"prediction == truth (backbone_only {backbone_only}): gradient of the present atoms: "
          f"{'all NaN' if np.isnan(got).all() else 'all zero' if np.all(got == 0) else 'mixed'}")
    assert np.isnan(got).all() or np.all(got == 0)
    for b in (0, 2):                                             # the neighbours keep their bits
        assert same_bits(s0[b], s1[b]) and same_bits(g0[b], g1[b])
