"""lDDT on the device (csrc/lddt.hip, eval_metrics.lddt_batch, `train.py --eval_lddt`) against an fp64 numpy restatement of the
definition in include/ptamd.h.

Tolerance (derived, not measured).  With |x| <= 64 A and distances formed from coordinate differences, one fp32 distance is off
by less than 4e-5 A and |dp - dt| by less than 8e-5 A.  The reference therefore evaluates every comparison twice, with each
threshold and the cutoff moved by EPS = 2.5e-4 A either way, and yields a lower and an upper count per residue, set and counter;
the kernel's count must lie in [lo, hi].  The brackets may cover at most 0.1 % of the included pairs of a case
(sum(hi - lo) <= 1e-3 sum(total)): tests/test_lddt_cli.py holds every random case to that without a GPU, the seeds in `CASES`
were chosen for it.  A kernel that miscounts a tile edge is off by dozens of pairs in a residue.  Scores must equal the ratio of
the kernel's own counts to 1e-6.  The known-answer cases have no bracket at all.

Sizes are atoms present, around the kernel's 64-atom tile, its 256-atom strip (4 wavefronts) and, at ~2500 atoms (L = 300),
its chunk of 32 column tiles (2048 atoms: the protein spans two chunks and 10 strips).
"""
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PAD, SLOTS, CA = 20, 14, 1
EPS = 2.5e-4
CUTOFF = 15.0
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
SIGMAS = (0.3, 1.5, 5.0)
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 2500)
VARIANTS = ("base", "straddle", "allnan", "noca")


# ----------------------------------------------------------------------------- the fp64 reference
def lddt_reference(pred, true, seq, cutoff=CUTOFF, eps=0.0):
    """One protein: pred, true [L*14, 3], seq [L] -> (lo, hi) int64 [L, 2, 5] = {total, p0.5, p1, p2, p4} per residue and set
    (0: every atom, 1: C-alpha with C-alphas), every comparison made with its bound moved down (lo) and up (hi) by eps."""
    pred, true, seq = np.asarray(pred, np.float64), np.asarray(true, np.float64), np.asarray(seq)
    L = seq.shape[0]
    slot = np.arange(L * SLOTS)
    present = (seq[slot // SLOTS] != PAD) & ~np.isnan(true).any(1)
    idx = slot[present]
    res, ca = idx // SLOTS, (idx % SLOTS) == CA
    out = [np.zeros((L, 2, 5), np.int64) for _ in range(2)]
    if idx.size == 0:
        return out[0], out[1]
    with np.errstate(invalid="ignore", over="ignore"):
        t, p = true[idx], pred[idx]
        dt = np.sqrt(sum((t[:, None, k] - t[None, :, k]) ** 2 for k in range(3)))
        dp = np.sqrt(sum((p[:, None, k] - p[None, :, k]) ** 2 for k in range(3)))
        diff = np.abs(dp - dt)
        other = res[:, None] != res[None, :]
        for o, e in zip(out, (-eps, eps)):
            for s, pair_ok in enumerate((other, other & ca[:, None] & ca[None, :])):
                incl = pair_ok & (dt < cutoff + e)
                rows = [incl.sum(1)] + [(incl & (diff < th + e)).sum(1) for th in THRESHOLDS]
                for k, r in enumerate(rows):
                    np.add.at(o[:, s, k], res, r)
    return out[0], out[1]


def scores_of(counts):
    """counts [..., 5] -> (p0.5 + p1 + p2 + p4) / (4 total), NaN where total == 0 (fp64)."""
    counts = np.asarray(counts, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(counts[..., 0] > 0, counts[..., 1:].sum(-1) / (4 * counts[..., 0]), np.nan)


# ----------------------------------------------------------------------------- random cases
def residue_atoms(n_atoms, rng, variant):
    """Present slots per residue, n_atoms in all.  Residues of 4..14 atoms (slots 0..k-1, so with a C-alpha); `straddle` starts
    with residues cut so that one lies across atom 64 (atoms 60..69) and one across atom 256 (atoms 250..261); fewer than 3
    atoms: residues of one atom, the C-alpha."""
    if n_atoms < 3:
        counts = [1] * n_atoms
    else:
        counts = []
        for c in ([14, 14, 14, 14, 4, 10] + [14] * 12 + [12, 12]) if variant == "straddle" else []:
            if sum(counts) < n_atoms:
                counts.append(min(c, n_atoms - sum(counts)))
        while sum(counts) < n_atoms:
            counts.append(min(int(rng.integers(4, SLOTS + 1)), n_atoms - sum(counts)))
    atoms = [[CA] if c == 1 else list(range(c)) for c in counts]
    mid = len(atoms) // 2
    if variant == "allnan":                    # a residue without any present atom, in the middle of the chain
        atoms.insert(mid, [])
    if variant == "noca":                      # its C-alpha absent, the same number of other atoms present (slots 0, 2, 3, ...)
        mid = next(r for r in list(range(mid, len(atoms))) + list(range(mid)) if len(atoms[r]) < SLOTS)
        c = len(atoms[mid])
        atoms[mid] = [0] + list(range(2, c + 1))
    assert sum(len(a) for a in atoms) == n_atoms
    return atoms


def make_case(n_atoms, sigma, seed, variant="base"):
    """(pred, true, seq) of one protein, fp32 / int64 numpy: residue centres on a 3.8 A random walk reflected at the walls of a
    +-60 A box, each atom its centre plus an offset of at most 3 A, predicted = true + N(0, sigma) clipped to +-64 A (the bound
    the tolerance assumes).  Absent atoms: NaN truth, a finite prediction."""
    rng = np.random.default_rng(seed)
    atoms = residue_atoms(n_atoms, rng, variant)
    L = len(atoms)
    step = rng.normal(size=(L, 3))
    step *= 3.8 / np.linalg.norm(step, axis=1, keepdims=True)
    centre = np.zeros((L, 3))
    pos = rng.uniform(-40, 40, size=3)
    for r in range(L):
        pos = pos + step[r]
        pos = np.where(pos > 60, 120 - pos, pos)
        pos = np.where(pos < -60, -120 - pos, pos)
        centre[r] = pos
    off = rng.normal(size=(L * SLOTS, 3))
    off *= (3.0 * rng.uniform(size=(L * SLOTS, 1)) ** (1 / 3)) / np.linalg.norm(off, axis=1, keepdims=True)
    ideal = np.repeat(centre, SLOTS, axis=0) + off
    pred = np.clip(ideal + rng.normal(scale=sigma, size=ideal.shape), -64, 64).astype(np.float32)
    true = np.full((L * SLOTS, 3), np.nan, np.float32)
    for r, sl in enumerate(atoms):
        for s in sl:
            true[r * SLOTS + s] = ideal[r * SLOTS + s].astype(np.float32)
    seq = rng.integers(0, 20, size=L).astype(np.int64)
    assert int((~np.isnan(true).any(1)).sum()) == n_atoms
    return pred, true, seq


def _cases():
    out = []
    for vi, variant in enumerate(VARIANTS):
        for si, n in enumerate(SIZES):
            if variant == "straddle" and n < 65:
                continue                        # nothing to straddle: the case would repeat `base`
            out.append((n, SIGMAS[(si + vi) % 3], variant))
    out += [(n, sigma, "base") for n in (257, 2500) for sigma in SIGMAS]           # every sigma at two sizes
    return sorted(set(out), key=lambda c: (VARIANTS.index(c[2]), c[0], c[1]))


# seeds for which the brackets of the reference cover at most 0.1 % of the included pairs (tests/test_lddt_cli.py asserts it);
# a case without an entry uses DEFAULT_SEED
DEFAULT_SEED = 1
SEEDS = {(63, 5.0, "base"): 2, (256, 0.3, "base"): 2, (257, 0.3, "base"): 2, (65, 0.3, "allnan"): 2, (63, 5.0, "noca"): 2,
         (256, 0.3, "noca"): 2, (257, 1.5, "noca"): 2}
CASES = _cases()


def case_id(c):
    return f"{c[2]}-{c[0]}-s{c[1]}"


@functools.lru_cache(maxsize=None)
def case_with_reference(case):
    """(pred, true, seq, lo, hi) of a random case: built and bracketed once, shared by the tests, never modified."""
    n, sigma, variant = case
    pred, true, seq = make_case(n, sigma, SEEDS.get(case, DEFAULT_SEED), variant)
    lo, hi = lddt_reference(pred, true, seq, eps=EPS)
    for a in (pred, true, seq, lo, hi):
        a.setflags(write=False)
    return pred, true, seq, lo, hi


# ----------------------------------------------------------------------------- known answers
def lattice_case():
    """17 x 17 x 2 points of the integer lattice, 1 A apart: residue (x, y) has its C-alpha (slot 1) at z = 0 and its N (slot 0)
    at z = 1.  Expected counts by INTEGER arithmetic on the squared lattice distances: a pair is included iff dx^2 + dy^2 + dz^2
    < 225, which leaves out the ties at exactly 15 A - (15, 0, 0), (9, 12, 0) and their kin - as the strict comparison must."""
    nx = ny = 17
    L = nx * ny
    xy = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), indexing="ij"), -1).reshape(L, 2)
    true = np.full((L * SLOTS, 3), np.nan, np.float32)
    true[np.arange(L) * SLOTS + CA] = np.concatenate([xy, np.zeros((L, 1))], 1)
    true[np.arange(L) * SLOTS + 0] = np.concatenate([xy, np.ones((L, 1))], 1)
    d2 = ((xy[:, None, :] - xy[None, :, :]) ** 2).sum(-1)                      # in-plane, integers
    other = ~np.eye(L, dtype=bool)
    same_plane, cross_plane = (other & (d2 < 225)).sum(1), (other & (d2 + 1 < 225)).sum(1)
    want = np.zeros((L, 2, 5), np.int64)
    want[:, 0, :] = (2 * same_plane + 2 * cross_plane)[:, None]                 # both atoms of the residue, both planes
    want[:, 1, :] = same_plane[:, None]                                         # C-alphas: the plane z = 0
    return true, np.zeros(L, np.int64), want


def line_case():
    """Four residues of one atom each on the x axis at 0, 3, 7, 20 A; the atom at 7 is an N (slot 0), the others C-alphas.
    True distances: 0-3 3, 0-7 7, 0-20 20, 3-7 4, 3-20 17, 7-20 13; included (< 15): 3, 7, 4, 13.

    Predicted = 2 x truth (exact in fp32): |dp - dt| = dt = 3, 7, 4, 13; only the 3 is below a threshold (< 4; the 4 ties and
    fails the strict test).  {total, p0.5, p1, p2, p4} per residue, set 0:
        x=0: pairs 3, 7      -> 2 0 0 0 1        x=3: pairs 3, 4       -> 2 0 0 0 1
        x=7: pairs 7, 4, 13  -> 3 0 0 0 0        x=20: pair 13         -> 1 0 0 0 0
    set 1 (C-alphas 0, 3, 20: only 0-3 is included):  x=0: 1 0 0 0 1   x=3: 1 0 0 0 1   x=7, x=20: zeros (score NaN).
    Scores: set 0 per residue 1/8, 1/8, 0, 0, protein 2/32; set 1 per residue 1/4, 1/4, NaN, NaN, protein 2/8.

    Predicted = 1.1 x truth: |dp - dt| = 0.3, 0.7, 0.4, 1.3 (to rounding, far from every threshold): 0.3 and 0.4 pass all four
    thresholds, 0.7 passes 1, 2, 4, 1.3 passes 2, 4.  Set 0:
        x=0: 3 (0.3), 7 (0.7)            -> 2 1 2 2 2        x=3: 3 (0.3), 4 (0.4)  -> 2 2 2 2 2
        x=7: 7 (0.7), 4 (0.4), 13 (1.3)  -> 3 1 2 3 3        x=20: 13 (1.3)         -> 1 0 0 1 1
    set 1:  x=0: 1 1 1 1 1   x=3: 1 1 1 1 1   others zeros.
    """
    xs, slots = (0.0, 3.0, 7.0, 20.0), (CA, CA, 0, CA)
    true = np.full((4 * SLOTS, 3), np.nan, np.float32)
    for r, (x, s) in enumerate(zip(xs, slots)):
        true[r * SLOTS + s] = (x, 0.0, 0.0)
    want2 = np.array([[[2, 0, 0, 0, 1], [1, 0, 0, 0, 1]], [[2, 0, 0, 0, 1], [1, 0, 0, 0, 1]],
                      [[3, 0, 0, 0, 0], [0, 0, 0, 0, 0]], [[1, 0, 0, 0, 0], [0, 0, 0, 0, 0]]], np.int64)
    want11 = np.array([[[2, 1, 2, 2, 2], [1, 1, 1, 1, 1]], [[2, 2, 2, 2, 2], [1, 1, 1, 1, 1]],
                       [[3, 1, 2, 3, 3], [0, 0, 0, 0, 0]], [[1, 0, 0, 1, 1], [0, 0, 0, 0, 0]]], np.int64)
    return true, np.zeros(4, np.int64), {2.0: want2, 1.1: want11}


def two_atom_case(dist):
    """Two residues of one C-alpha each, `dist` A apart."""
    true = np.full((2 * SLOTS, 3), np.nan, np.float32)
    true[CA], true[SLOTS + CA] = (1.0, 2.0, 3.0), (1.0 + dist, 2.0, 3.0)
    return true, np.zeros(2, np.int64)


def finite_pred(true, scale=1.0):
    """truth x scale with zeros where the truth is absent (a prediction is finite everywhere)."""
    return (np.nan_to_num(true, nan=0.0) * np.float32(scale)).astype(np.float32)


# ----------------------------------------------------------------------------- device side
def run(pred, true, seq, cutoff=CUTOFF):
    """One protein or a batch through eval_metrics.lddt_batch -> (score, per_res, counts) as numpy."""
    from protein_transformer_amd.eval_metrics import lddt_batch
    dev = torch.device("cuda:0")
    p, t, s = (torch.tensor(np.asarray(a)) for a in (pred, true, seq))          # (copies: the shared cases are read-only)
    if s.dim() == 1:
        p, t, s = p[None], t[None], s[None]
    out = lddt_batch(p.to(dev), t.to(dev), s.to(dev), cutoff)
    return tuple(o.cpu().numpy() for o in out)


def check_scores(score, per_res, counts):
    """Per-residue and per-protein scores are the ratios of the kernel's own counts, NaN exactly where total == 0."""
    c = counts.astype(np.int64)
    want_res, want_prot = scores_of(c), scores_of(c.sum(1))
    assert np.array_equal(np.isnan(per_res), np.isnan(want_res)) and np.array_equal(np.isnan(score), np.isnan(want_prot))
    assert np.allclose(per_res, want_res, rtol=0, atol=1e-6, equal_nan=True)
    assert np.allclose(score, want_prot, rtol=0, atol=1e-6, equal_nan=True)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_random_case_within_the_reference_brackets(case):
    pred, true, seq, lo, hi = case_with_reference(case)
    score, per_res, counts = run(pred, true, seq)
    got = counts[0].astype(np.int64)
    print(f"{case_id(case)}: included pairs {int(got[:, 0, 0].sum())}, bracket width {int((hi - lo).sum())}, "
          f"outside {int(((got < lo) | (got > hi)).sum())}, lddt {score[0]}")
    assert np.all(got >= lo) and np.all(got <= hi), np.argwhere((got < lo) | (got > hi))[:8]
    check_scores(score, per_res, counts)
    n, _, variant = case
    atoms_of = (~np.isnan(true).any(1)).reshape(-1, SLOTS)
    empty = ~atoms_of.any(1)
    assert np.all(got[empty] == 0) and np.all(np.isnan(per_res[0][empty]))         # a residue without atoms: zeros, NaN
    no_ca = ~atoms_of[:, CA]
    assert np.all(got[no_ca, 1] == 0) and np.all(np.isnan(per_res[0][no_ca, 1]))   # no C-alpha: NaN for set 1 ...
    if variant == "allnan":
        assert empty.sum() == 1
    if variant == "noca":
        assert (no_ca & ~empty).sum() == 1
        if n > 2:
            assert np.all(np.isfinite(per_res[0][no_ca & ~empty, 0]))              # ... and for set 1 only
    if variant == "straddle":
        first = np.cumsum(atoms_of.sum(1)) - atoms_of.sum(1)                         # index of a residue's first atom
        for edge in (64, 256):
            if n > edge:
                assert np.any((first < edge) & (first + atoms_of.sum(1) > edge))
    if n < 2:
        assert np.all(got == 0) and np.all(np.isnan(score))


def test_lattice_identity_scores_one():
    true, seq, want = lattice_case()
    score, per_res, counts = run(finite_pred(true), true, seq)
    assert np.array_equal(counts[0], want)
    assert np.all(per_res == 1.0) and np.all(score == 1.0)


@pytest.mark.parametrize("scale", [1.1, 2.0])
def test_scaled_line_counts_by_hand(scale):
    true, seq, want = line_case()
    score, per_res, counts = run(finite_pred(true, scale), true, seq)
    assert np.array_equal(counts[0], want[scale])
    check_scores(score, per_res, counts)
    if scale == 2.0:
        assert np.allclose(per_res[0], [[1 / 8, 1 / 4], [1 / 8, 1 / 4], [0, np.nan], [0, np.nan]], atol=1e-7, equal_nan=True)
        assert np.allclose(score[0], [2 / 32, 2 / 8], atol=1e-7)


def test_cutoff_is_strict_on_either_side():
    for dist, total in ((14.9, 1), (15.1, 0)):
        true, seq = two_atom_case(dist)
        score, per_res, counts = run(finite_pred(true), true, seq)
        assert np.array_equal(counts[0], np.full((2, 2, 5), total)), dist
        assert np.all(score == 1.0) if total else np.all(np.isnan(score))


def test_nonfinite_prediction_fails_the_comparisons():
    true, seq, _ = line_case()
    pred = finite_pred(true)
    pred[CA] = (np.nan, np.inf, 0.0)                 # the atom at x = 0
    _, _, counts = run(pred, true, seq)
    assert np.array_equal(counts[0][:, 0, 0], [2, 2, 3, 1])           # still included ...
    assert np.array_equal(counts[0][0, 0, 1:], [0, 0, 0, 0])          # ... never preserved
    assert np.array_equal(counts[0][2, 0, 1:], [2, 2, 2, 2])          # x = 7: its pairs with 3 and 20 are, the one with 0 is not


def _ragged_batch():
    """B = 3, lengths L, 1 and L / 2 padded to L: residues PAD_ID, truth zeros (what collate writes), prediction zeros."""
    big = case_with_reference((2500, SIGMAS[(SIZES.index(2500)) % 3], "base"))[:3]
    one = make_case(1, 0.3, 3)
    half_full = make_case(2500, 1.5, 7)
    L = big[2].shape[0]
    h = L // 2
    half = (half_full[0][:h * SLOTS], half_full[1][:h * SLOTS], half_full[2][:h])
    P, T, S = np.zeros((3, L * SLOTS, 3), np.float32), np.zeros((3, L * SLOTS, 3), np.float32), np.full((3, L), PAD, np.int64)
    for b, (p, t, s) in enumerate((big, one, half)):
        P[b, :p.shape[0]], T[b, :t.shape[0]], S[b, :s.shape[0]] = p, t, s
    return (P, T, S), (big, one, half)


def test_ragged_batch_equals_each_protein_alone():
    (P, T, S), solo = _ragged_batch()
    score, per_res, counts = run(P, T, S)
    check_scores(score, per_res, counts)
    for b, (p, t, s) in enumerate(solo):
        n = s.shape[0]
        s1, r1, c1 = run(p, t, s)
        assert np.array_equal(counts[b, :n], c1[0])                                 # bit for bit
        assert np.array_equal(score[b], s1[0], equal_nan=True) and np.array_equal(per_res[b, :n], r1[0], equal_nan=True)
        assert np.all(counts[b, n:] == 0) and np.all(np.isnan(per_res[b, n:]))      # the padded tail
    assert counts[0].sum() > 0 and counts[2].sum() > 0
    assert np.all(np.isnan(score[1])) and np.all(counts[1] == 0)                    # one residue: no pair


def test_two_runs_give_identical_counts():
    (P, T, S), _ = _ragged_batch()
    a, b = run(P, T, S), run(P, T, S)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)


def test_refusals_leave_counts_untouched():
    from protein_transformer_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    B, L = 2, 5
    crd = torch.zeros(B, L * SLOTS, 3, device=dev)
    seq = torch.zeros(B, L, dtype=torch.int64, device=dev)
    counts = torch.full((B, L, 2, 5), 77, dtype=torch.int32, device=dev)
    per_res, score = torch.zeros(B, L, 2, device=dev), torch.zeros(B, 2, device=dev)
    need = lib.ptamd_lddt_workspace_bytes(B, L)
    assert need > 0 and lib.ptamd_lddt_workspace_bytes(0, L) == 0 and lib.ptamd_lddt_workspace_bytes(B, -1) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    P = _lib.ptr

    def call(pred=crd, true=crd, s=seq, b=B, l=L, cutoff=15.0, c=counts, r=per_res, sc=score, w=ws, wb=None):
        rc = lib.ptamd_lddt(P(pred), P(true), P(s), b, l, cutoff, P(c), P(r), P(sc), P(w), need if wb is None else wb, _lib.stream())
        torch.cuda.synchronize()
        return rc
    bad_shape = [dict(b=0), dict(b=-1), dict(l=0), dict(l=-3), dict(pred=None), dict(true=None), dict(s=None), dict(r=None),
                 dict(sc=None), dict(cutoff=0.0), dict(cutoff=-1.0), dict(cutoff=float("inf")), dict(cutoff=float("nan"))]
    for kw in bad_shape:
        assert call(**kw) == -1, kw                          # PTAMD_ERR_BAD_SHAPE
        assert bool((counts == 77).all()), kw
    assert call(c=None) == -1
    for kw in (dict(w=None), dict(wb=need - 1), dict(wb=0)):
        assert call(**kw) == -3, kw                          # PTAMD_ERR_WORKSPACE
        assert bool((counts == 77).all()), kw
    assert call() == 0       # the good call: every atom at the origin, so each of a residue's 14 atoms pairs with the 14 (L - 1)
    c = counts.cpu().numpy()     # atoms of the other residues and every pair is preserved - no stale 77 survives
    assert np.all(c[:, :, 0, :] == SLOTS * SLOTS * (L - 1)) and np.all(c[:, :, 1, :] == L - 1)


# ----------------------------------------------------------------------------- the flag, end to end
def _model_and_batch(dev, eval_lddt):
    from test_gpu_dp import _make
    model, opt, args, batch, lens = _make(dev, "combined", "ragged")
    args.eval_lddt = eval_lddt
    return model.eval(), args, batch, lens          # (the batch on the host, as a loader hands it over)


TODAY_KEYS = {"loss", "drmsd-full", "lndrmsd-full", "drmsd-bb", "lndrmsd-bb", "combined-full", "mse-full", "mse-bb", "mse-sc",
              "rmsd-full"}


def test_get_losses_reports_lddt_only_under_the_flag():
    from protein_transformer_amd.eval_metrics import batch_lddt
    from protein_transformer_amd.train import get_losses
    dev = torch.device("cuda:0")
    model, args, batch, _ = _model_and_batch(dev, True)
    seq, ang, crd = (t.to(dev) for t in batch)
    with torch.no_grad():
        pred = model(seq, ang)
        on = get_losses(args, pred, ang, crd, seq, do_backwards=False, eval_mode=True, return_rmsd=True)
        full, ca = batch_lddt(pred, crd, seq)
        assert set(on) == TODAY_KEYS | {"lddt-full", "lddt-ca"}
        assert 0.0 < full <= 1.0 and 0.0 < ca <= 1.0
        assert abs(float(on["lddt-full"]) - full) <= 1e-6 and abs(float(on["lddt-ca"]) - ca) <= 1e-6
        args.eval_lddt = False
        off = get_losses(args, pred, ang, crd, seq, do_backwards=False, eval_mode=True, return_rmsd=True)
        assert set(off) == TODAY_KEYS
        for k in TODAY_KEYS:
            assert float(on[k]) == float(off[k]), k
        del args.eval_lddt                                    # callers that never heard of the flag
        assert set(get_losses(args, pred, ang, crd, seq, do_backwards=False, eval_mode=True, return_rmsd=True)) == TODAY_KEYS
        args.eval_lddt = True                                 # a training step never computes it
    pred = model.train()(seq, ang)
    assert set(get_losses(args, pred, ang, crd, seq)) == TODAY_KEYS


def _dp_worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      PTAMD_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from test_gpu_dp import _shard
    from protein_transformer_amd import dp
    from protein_transformer_amd.log import init_metrics
    from protein_transformer_amd.train import eval_epoch
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dp.init_from_env()
    model, args, batch, lens = _model_and_batch(dev, True)
    dp.attach(model)
    (seq, ang, crd), _ = _shard(batch, lens, world, rank)
    m = eval_epoch(model, [(seq, ang, crd)], dev, args, init_metrics(args), mode="valid-70")["valid-70"]
    np.save(os.path.join(out_dir, f"lddt{rank}.npy"), np.array([m["epoch-lddt-full"], m["epoch-lddt-ca"], m["epoch-rmsd-full"]]))
    dp.barrier()
    dp.shutdown()


def test_two_ranks_report_the_lddt_of_the_whole_batch(tmp_path):
    """Two ranks on one GPU over gloo (3 + 2 ragged proteins), as tests/test_gpu_dp.py does: sums and counts of the proteins with
    a score travel in LossReport's vector, so every rank reports the mean over the GLOBAL batch."""
    import torch.multiprocessing as mp
    from test_gpu_dp import _free_port
    from protein_transformer_amd.log import init_metrics
    from protein_transformer_amd.train import eval_epoch
    mp.spawn(_dp_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    dev = torch.device("cuda:0")
    model, args, batch, _ = _model_and_batch(dev, True)
    m = eval_epoch(model, [batch], dev, args, init_metrics(args), mode="valid-70")["valid-70"]
    e0, e1 = np.load(tmp_path / "lddt0.npy"), np.load(tmp_path / "lddt1.npy")
    assert np.array_equal(e0, e1)
    assert 0.0 < m["epoch-lddt-full"] <= 1.0
    assert abs(e0[0] - m["epoch-lddt-full"]) <= 1e-6 and abs(e0[1] - m["epoch-lddt-ca"]) <= 1e-6
