"""Side-chain accuracy on the device (csrc/sidechain.hip) against tests/sidechain_ref.py on the same fp32 inputs, through the C
ABI on a workspace this file owns: the method of tests/test_gpu_atom_tiles_edges.py (a workspace filled with 0x00, with 0xFF and
with what a call on other proteins left there; guard bands round the workspace and every output).

Bars.  `counts`, chi1 and chi12 are integers and ratios of integers rounded once: compared EXACTLY, under the condition that
sidechain_ref.well_posed asserts on the CPU for every protein used here.  per_res, chi_mae and sc_rmsd: 8 x the largest error
measured against the fp64 reference over these cases on an MI355X - 2.470e-5 degrees (single-129) and 4.427e-7 A
(nonfinite-1-of-3, protein 2); the table is in profiles/sidechain/NOTES.md - which is 1.98e-4 degrees and 3.5e-6 A, inside the
derived bounds sidechain_ref.EPS_CHI (5.5e-4 degrees) and EPS_RMS (3.6e-5 A).  Every test prints its largest error."""
import numpy as np
import pytest
import torch

import sidechain_ref as R
from test_gpu_atom_tiles_edges import Guarded, POISON, same_bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORST_CHI, WORST_RMS = 2.470e-5, 4.427e-7        # measured on an MI355X over the cases below (single-129; nonfinite-1-of-3[2])
BAR_CHI, BAR_RMS = 8 * WORST_CHI, 8 * WORST_RMS  # degrees, Angstrom: the project's habit, and inside the derived bounds
assert BAR_CHI <= R.EPS_CHI and BAR_RMS <= R.EPS_RMS
SPEC = [("score", lambda B, L: (B, 4), torch.float32), ("counts", lambda B, L: (B, 12), torch.int32),
        ("per_res", lambda B, L: (B, L, 5), torch.float32)]
STATES = ("zeros", "ones", "stale")


def dev(batch):
    return tuple(torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in batch)


def call_abi(batch, threshold, ws, nbytes, outs, per_res=True):
    from protein_transformer_amd import _lib
    pred, truth, seq = batch
    B, L = seq.shape
    P = _lib.ptr
    rc = _lib.lib().ptamd_sidechain(P(pred), P(truth), P(seq), B, L, float(threshold), P(outs["score"]), P(outs["counts"]),
                                    P(outs["per_res"]) if per_res else None, P(ws), nbytes, _lib.stream())
    torch.cuda.synchronize()
    return rc


def run_state(batch, state, threshold=40.0, per_res=True):
    """One call on a workspace in `state` -> name -> numpy array of every output, after the guard and poison checks."""
    from protein_transformer_amd import _lib
    B, L = batch[2].shape
    nbytes = _lib.lib().ptamd_sidechain_workspace_bytes(B, L)
    assert nbytes > 0
    whole = torch.full((nbytes + 512,), POISON, dtype=torch.uint8, device=DEV)
    ws = whole[256:256 + nbytes]
    assert ws.data_ptr() % 16 == 0
    ws.fill_(0xFF if state == "ones" else 0x00)
    if state == "stale":                          # the same shapes, other proteins: the rows in reverse order, truth and prediction exchanged
        other = (batch[1].flip(0).nan_to_num(1.0), batch[0].flip(0).nan_to_num(2.0), batch[2].flip(0))
        scrap = {name: torch.empty(shape(B, L), dtype=dtype, device=DEV) for name, shape, dtype in SPEC}
        assert call_abi(other, threshold, ws, nbytes, scrap) == 0
    outs = {name: Guarded(shape(B, L), dtype, DEV) for name, shape, dtype in SPEC}
    assert call_abi(batch, threshold, ws, nbytes, {k: g.t for k, g in outs.items()}, per_res=per_res) == 0
    assert bool((whole[:256] == POISON).all()) and bool((whole[256 + nbytes:] == POISON).all()), "workspace guard band"
    for name, g in outs.items():
        assert g.guards_intact(), name
        if name == "per_res" and not per_res:
            assert g.poisoned().all()
        else:
            assert not g.poisoned().any(), (name, state)
    return {name: g.t.cpu().numpy().copy() for name, g in outs.items()}


def run_wrapper(batch, threshold=40.0):
    """The Python wrapper, right after a batch one row and three residues larger went through its cached workspace."""
    from protein_transformer_amd.eval_metrics import sidechain_batch
    B, L = batch[2].shape
    rng = np.random.default_rng(9)
    big = torch.from_numpy(rng.normal(0, 9.0, (B + 1, (L + 3) * R.SLOTS, 3)).astype(np.float32)).to(DEV)
    sidechain_batch(big + 1.0, big, torch.from_numpy(rng.integers(0, 20, (B + 1, L + 3))).to(DEV), threshold)
    score, counts, per_res = sidechain_batch(*batch, threshold=threshold, per_residue=True)
    torch.cuda.synchronize()
    return {"score": score.cpu().numpy(), "counts": counts.cpu().numpy(), "per_res": per_res.cpu().numpy()}


def exact_ratio(n, d):
    return np.float32(n / d) if d else np.float32(np.nan)


def check_protein(name, got, b, item, threshold=40.0):
    """Protein b of `got` against the reference of item = (pred, truth, seq); -> (worst chi error, worst RMSD error)."""
    pred, truth, seq = item
    n = len(seq)
    ref = R.reference(pred, truth, seq, threshold)
    score, counts, per_res = got["score"][b], got["counts"][b], got["per_res"][b]
    assert np.array_equal(counts, ref["counts"]), (name, counts, ref["counts"])
    assert np.isnan(per_res[n:]).all(), name                                      # nothing in the padding
    want = ref["per_res"]
    assert np.array_equal(np.isnan(per_res[:n]), np.isnan(want)), (name, np.argwhere(np.isnan(per_res[:n]) != np.isnan(want))[:8])
    err = np.abs(per_res[:n].astype(np.float64) - want)
    e_chi, e_rms = np.nanmax(err[:, :4], initial=0.0), np.nanmax(err[:, 4], initial=0.0)
    assert np.array_equal(np.isnan(score), np.isnan(ref["score"])), (name, score, ref["score"])
    if not ref["bad"]:
        c = ref["counts"]
        assert same_bits({"a": np.nan_to_num(score[:2], nan=-1.0)},
                         {"a": np.nan_to_num(np.array([exact_ratio(c[1], c[0]), exact_ratio(c[9], c[8])]), nan=-1.0)}), (name, score)
        if not np.isnan(ref["score"][2]):
            e_chi = max(e_chi, abs(float(score[2]) - ref["score"][2]))
        if not np.isnan(ref["score"][3]):
            e_rms = max(e_rms, abs(float(score[3]) - ref["score"][3]))
    print(f"{name}: counts {counts.tolist()}, worst chi error {e_chi:.3e} deg ({e_chi / R.EPS_CHI:.3f} eps), "
          f"worst rmsd error {e_rms:.3e} A ({e_rms / R.EPS_RMS:.3f} eps)")
    assert e_chi <= BAR_CHI and e_rms <= BAR_RMS, (name, e_chi, e_rms)
    return e_chi, e_rms


@pytest.mark.parametrize("name", list(R.gpu_cases()))
def test_poisoned_workspaces_at_the_tile_edges(name):
    items, L_pad = R.gpu_cases()[name]
    batch = dev(R.batch_of(items, L_pad))
    runs = {state: run_state(batch, state) for state in STATES}
    for state in STATES[1:]:
        assert same_bits(runs["zeros"], runs[state]), state
    assert same_bits(runs["zeros"], run_wrapper(batch))
    lean = run_state(batch, "ones", per_res=False)
    assert same_bits({k: runs["zeros"][k] for k in ("score", "counts")}, {k: lean[k] for k in ("score", "counts")})
    worst = [check_protein(f"{name}[{b}]", runs["zeros"], b, item) for b, item in enumerate(items)]
    print(f"{name}: worst of the case {max(w[0] for w in worst):.3e} deg, {max(w[1] for w in worst):.3e} A")


def test_the_cases_cover_what_they_claim():
    """All twenty types; the gaps of `with_gaps` do what they are for; the only scored chi of a protein in tile 0 and in tile 1."""
    cases = R.gpu_cases()
    item, notes = R.with_gaps(R.pair_case(129, 229))
    assert item[2].tolist() == cases["single-129"][0][0][2].tolist() and set(np.arange(20)) <= set(item[2].tolist())
    full, gaps = R.reference(*R.pair_case(129, 229)), R.reference(*item)
    for j in range(4):
        r = notes[f"chi2-atom{j}"]
        assert full["scored"][r, 1] and not gaps["scored"][r, 1]
        assert gaps["scored"][r, 0] == (j == 3)                                   # the last atom of chi2 is not on chi1
    r = notes["lys-nz"]
    assert gaps["scored"][r].tolist() == [True, True, True, False] and full["counted"][r] and not gaps["counted"][r]
    r = notes["no-c"]
    assert gaps["scored"][r, 0] and full["counted"][r] and not gaps["counted"][r]
    r = notes["id21"]
    assert not gaps["scored"][r].any() and not gaps["counted"][r] and np.isnan(gaps["per_res"][r]).all()
    # every protein of 63 residues or more carries every gap; the half-length rows of the batches from 31 residues on
    every = {"chi2-atom0", "chi2-atom1", "chi2-atom2", "chi2-atom3", "lys-nz", "no-c", "id21"}
    for L in R.SIZES:
        for row, (n, seed) in enumerate(((L, 100 + L), (max(1, L // 2), 200 + L))):
            item, notes = R.with_gaps(R.pair_case(n, seed))
            assert (set(notes) == every) == (n >= 31), (n, seed, sorted(notes))
            assert cases[f"batch-{L}"][0][row][2].tolist() == item[2].tolist()
        assert cases[f"single-{L}"][0][0][2].tolist() == cases[f"batch-{L}"][0][0][2].tolist()
    for b, at in enumerate((3, 100, 128)):
        ref = R.reference(*cases["only-chi"][0][b])
        assert ref["counts"][:10].tolist() == [1] * 10 and np.nonzero(ref["scored"].any(1))[0].tolist() == [at]


def test_a_protein_alone_in_a_batch_and_in_a_longer_row():
    """The bits of a protein do not depend on the batch around it or on how far its row is padded."""
    cases = R.gpu_cases()
    for name, b in (("batch-129", 0), ("batch-65", 1), ("nonfinite-1-of-3", 1), ("only-chi", 2)):
        items, L_pad = cases[name]
        item = items[b]
        n = len(item[2])
        inside = run_state(dev(R.batch_of(items, L_pad)), "zeros")
        alone = run_state(dev(R.batch_of([item])), "ones")
        far = run_state(dev(R.batch_of([R.empty_row(), item], L_pad=n + 70)), "zeros")
        for other, at in ((alone, 0), (far, 1)):
            assert same_bits({"s": inside["score"][b], "c": inside["counts"][b], "p": inside["per_res"][b, :n]},
                             {"s": other["score"][at], "c": other["counts"][at], "p": other["per_res"][at, :n]}), (name, at)


def test_every_refusal_returns_its_code_and_writes_nothing():
    from protein_transformer_amd import _lib
    lib, P = _lib.lib(), _lib.ptr
    items, L_pad = R.gpu_cases()["batch-63"]
    pred, truth, seq = dev(R.batch_of(items, L_pad))
    B, L = seq.shape
    nbytes = lib.ptamd_sidechain_workspace_bytes(B, L)
    assert nbytes == (B * 80 + 255) // 256 * 256
    l_max = (2 ** 31 - 1) // 28
    assert lib.ptamd_sidechain_workspace_bytes(0, 8) == 0 and lib.ptamd_sidechain_workspace_bytes(2, 0) == 0
    assert lib.ptamd_sidechain_workspace_bytes(1, l_max + 1) == 0 and lib.ptamd_sidechain_workspace_bytes(1, l_max) > 0
    whole = torch.full((nbytes + 512,), POISON, dtype=torch.uint8, device=DEV)
    ws = whole[256:256 + nbytes]
    outs = {name: Guarded(shape(B, L), dtype, DEV) for name, shape, dtype in SPEC}
    s, c, p = (P(outs[k].t) for k in ("score", "counts", "per_res"))
    st = _lib.stream()
    BAD, WS, ALIGN = -1, -3, -5
    odd_pred, odd_truth = (torch.cat([x.new_zeros(1), x.reshape(-1)])[1:] for x in (pred, truth))
    assert odd_pred.data_ptr() % 8 == 4 and odd_truth.data_ptr() % 8 == 4
    calls = [
        (BAD, (None, P(truth), P(seq), B, L, 40.0, s, c, p, P(ws), nbytes, st)),
        (BAD, (P(pred), None, P(seq), B, L, 40.0, s, c, p, P(ws), nbytes, st)),
        (BAD, (P(pred), P(truth), None, B, L, 40.0, s, c, p, P(ws), nbytes, st)),
        (BAD, (P(pred), P(truth), P(seq), B, L, 40.0, None, c, p, P(ws), nbytes, st)),
        (BAD, (P(pred), P(truth), P(seq), B, L, 40.0, s, None, p, P(ws), nbytes, st)),
        (BAD, (P(pred), P(truth), P(seq), 0, L, 40.0, s, c, p, P(ws), nbytes, st)),
        (BAD, (P(pred), P(truth), P(seq), B, -1, 40.0, s, c, p, P(ws), nbytes, st)),
        (BAD, (P(pred), P(truth), P(seq), 1, l_max + 1, 40.0, s, c, p, P(ws), nbytes, st)),
        (BAD, (P(pred), P(truth), P(seq), B, L, -1.0, s, c, p, P(ws), nbytes, st)),
        (BAD, (P(pred), P(truth), P(seq), B, L, float("nan"), s, c, p, P(ws), nbytes, st)),
        (BAD, (P(pred), P(truth), P(seq), B, L, float("inf"), s, c, p, P(ws), nbytes, st)),
        (WS, (P(pred), P(truth), P(seq), B, L, 40.0, s, c, p, None, nbytes, st)),
        (WS, (P(pred), P(truth), P(seq), B, L, 40.0, s, c, p, P(ws), nbytes - 1, st)),
        (ALIGN, (P(pred), P(truth), P(seq), B, L, 40.0, s, c, p, P(whole[260:]), nbytes, st)),
        # the coordinates are read as pairs of floats: a pointer that is only 4-byte aligned is refused (the same values, one float on)
        (ALIGN, (P(odd_pred), P(truth), P(seq), B, L, 40.0, s, c, p, P(ws), nbytes, st)),
        (ALIGN, (P(pred), P(odd_truth), P(seq), B, L, 40.0, s, c, p, P(ws), nbytes, st)),
    ]
    for want, args in calls:
        assert lib.ptamd_sidechain(*args) == want, (want, args[3:6])
    torch.cuda.synchronize()
    assert bool((whole == POISON).all())
    for name, g in outs.items():
        assert g.guards_intact() and g.poisoned().all(), name
    assert lib.ptamd_sidechain(P(pred), P(truth), P(seq), B, L, 0.0, s, c, p, P(ws), nbytes, st) == 0   # a threshold of 0 is one
    torch.cuda.synchronize()


def test_counts_do_not_depend_on_the_naming_of_the_truth():
    """losses.rename_symmetric applied to the truth first: the same counts (Delta and d2 are already the smaller of the two)."""
    from protein_transformer_amd.eval_metrics import sidechain_batch
    from protein_transformer_amd.losses import rename_symmetric
    for name in ("batch-129", "batch-64"):
        items, L_pad = R.gpu_cases()[name]
        batch = list(R.batch_of(items, L_pad))
        batch[1] = R.batch_of([(p, R.swap_symmetric(t, s), s) if b == 0 else (p, t, s) for b, (p, t, s) in enumerate(items)], L_pad)[1]
        pred, truth, seq = dev(batch)                                             # (row 0: every symmetric residue named the other way)
        renamed, _, swapped, _ = rename_symmetric(pred, truth, seq)
        plain, other = sidechain_batch(pred, truth, seq), sidechain_batch(pred, renamed, seq)
        torch.cuda.synchronize()
        assert int(swapped.sum()) > 0
        assert torch.equal(plain[1], other[1]), name
        assert np.array_equal(plain[1].cpu().numpy()[0], R.reference(*items[0])["counts"])


def test_two_shifted_chi_columns_miss_and_nothing_else():
    """Truth and prediction from the library's own NeRF; the prediction's angle columns 8 and 9 (chi2, chi3) turned by 60 degrees:
    every scored chi2 and chi3 misses, every scored chi1 and chi4 hits."""
    from protein_transformer_amd.eval_metrics import sidechain_batch
    from protein_transformer_amd.protein.Structure import nerf_forward
    L = 70
    seq = torch.from_numpy((np.arange(2 * L) % 20).reshape(2, L)).to(DEV)
    ang = torch.from_numpy(np.stack([R.angles(L, 31), R.angles(L, 32)]).astype(np.float32)).to(DEV)
    shifted = ang.clone()
    shifted[:, :, 8:10] += np.pi / 3
    truth, _ = nerf_forward(ang, seq)
    pred, _ = nerf_forward(shifted, seq)
    score, counts, per_res = sidechain_batch(pred, truth, seq, per_residue=True)
    torch.cuda.synchronize()
    counts, per_res = counts.cpu().numpy(), per_res.cpu().numpy()
    nchi = np.array(R.NCHI)[seq.cpu().numpy()]
    for b in range(2):
        want = [(nchi[b] >= k).sum() for k in (1, 2, 3, 4)]
        assert counts[b, 0:8:2].tolist() == want, (b, counts[b])
        assert counts[b, 1:8:2].tolist() == [want[0], 0, 0, want[3]], (b, counts[b])
        assert counts[b, 8] == want[1] and counts[b, 9] == 0
        d = per_res[b]
        assert np.nanmax(d[:, 0]) < 0.05 and np.nanmax(d[:, 3]) < 0.05 and np.nanmax(np.abs(d[:, 1:3] - 60.0)) < 0.05
    assert score.cpu().numpy()[:, 0].tolist() == [1.0, 1.0] and score.cpu().numpy()[:, 1].tolist() == [0.0, 0.0]
