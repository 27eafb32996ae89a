"""The three kernels that call tm_rotation::solve (csrc/tm_rotation.h) - csrc/kabsch_loss.hip, csrc/ensemble.hip, csrc/tmscore.hip -
on the degenerate geometry of tests/rotation_cases.py: planar, collinear, one-point, three-atom and equal-singular-value sets,
where the eigenvalues of Horn's matrix are close or equal and no other test of these kernels goes.  tests/test_rotation_cases.py
shows on the CPU that what is compared here does not depend on which optimal rotation a kernel returns; tests/test_rotation_host.py
runs the header itself against an SVD.

Bars are the kernels' own: VALUE_BAR and GRAD_BAR of tests/test_gpu_kabsch_loss.py, ensemble_ref.tol_sq, check_protein of
tests/test_gpu_tm.py.  Per class (rotation_cases.py):
  unique      everything is compared.
  free        the optimum (loss, rmsd) and, where every residual is invariant, the C-alpha rmsf column and the TM scores; of the
              gradient only what holds under ANY rotation: finite, +0.0 on absent slots, |sum g| <= 1e-6 max |g|, sum |g|^2 = 1 / n
              to 1e-6 (g = R^T r / (n loss): the norm needs R orthogonal, the sum needs sum r = 0).
  value-only  as free.
An exact motion has a reference loss that is the rounding of its fp32 coordinates: loss <= VALUE_BAR rg, the form in which
test_gpu_kabsch_loss.py holds `rigid`.  That form cannot be met by a correct implementation where the coordinates are large
against rg: the fp64 REFERENCE itself has 2.70e-7 rg on `collinear` (coordinates to 125 A, rg 7.8 A) and 5.3e-5 rg on
`offset-1e4-opposite`, against VALUE_BAR = 2.57e-7.  So the bar is the larger of VALUE_BAR rg and RIGID_MULT = 8 times the
reference's own loss of that case (the project's factor), and in class unique also |loss - reference| <= VALUE_BAR rg: the rotation
is determined to 2e-9 there, which moves a residual by at most 2e-9 x extent ~ 1e-8 rg.  Nothing is asserted of a gradient made
of rounding but that it is finite and zero on absent slots.  Outputs and workspaces are poisoned;
every call is made twice and must give the same bits.  The printed figures are in profiles/rotation/NOTES.md."""
import numpy as np
import pytest
import torch

import ensemble_ref as ER
import rotation_cases as C
import test_gpu_ensemble as TE
import test_gpu_kabsch_loss as TK
import test_gpu_tm as TT

pytestmark = pytest.mark.gpu

RIGID_MULT = 8.0
CHUNK = 12                                                      # proteins per call
bits = TK.bits


def run_loss(inputs):
    """[(pred, true, seq)] of one row length -> (stats [B,2], dcrd [B,L*14,3]), in calls of at most CHUNK proteins, each made twice"""
    stats, dcrd = [], []
    for at in range(0, len(inputs), CHUNK):
        pred, true, seq = (np.stack([x[k] for x in inputs[at:at + CHUNK]]) for k in range(3))
        s, d = TK.run(pred, true, seq)
        s2, d2 = TK.run(pred, true, seq, poison=-3.5)
        assert np.array_equal(bits(s), bits(s2)) and np.array_equal(bits(d), bits(d2))
        assert not (d == TK.POISON).any() and not (s == TK.POISON).any()
        stats.append(s)
        dcrd.append(d)
    return np.concatenate(stats), np.concatenate(dcrd)


@pytest.fixture(scope="module")
def loss_results():
    """layout -> (names, stats, dcrd) of every case"""
    names = list(C.cases())
    return {layout: (names, *run_loss([C.loss_inputs(n, layout) for n in names])) for layout in ("dense", "straddle")}


def test_kabsch_loss_on_every_geometry(loss_results):
    worst = {}
    for layout, (names, stats, dcrd) in loss_results.items():
        for i, name in enumerate(names):
            c, ref = C.cases()[name], C.loss_reference(name, layout)
            pred, true, seq = C.loss_inputs(name, layout)
            n, loss, g = ref["n"], float(stats[i, 0]), dcrd[i].astype(np.float64)
            assert stats[i, 1] == n, (layout, name)
            absent = np.ones(len(g), bool)
            absent[ref["slots"]] = False
            assert np.isfinite(loss) and np.isfinite(g).all() and absent.any() and not bits(dcrd[i][absent]).any(), (layout, name)
            if c["rigid"]:
                print(f"{layout:8s} {name:28s} {c['cls']:10s} exact motion: loss {loss:.3e} A = {loss / ref['rg']:.2e} rg "
                      f"(reference {ref['loss']:.3e} A)")
                assert 0 <= loss <= max(TK.VALUE_BAR * ref["rg"], RIGID_MULT * ref["loss"]), (layout, name, loss, ref["loss"])
                if c["cls"] == "unique":
                    assert abs(loss - ref["loss"]) <= TK.VALUE_BAR * ref["rg"], (layout, name, loss, ref["loss"])
                err = abs(loss - ref["loss"]) / ref["rg"]
                worst[(c["cls"], "exact")] = max(worst.get((c["cls"], "exact"), 0.0), err)
                continue
            ev = abs(loss - ref["loss"]) / ref["loss"]
            key = (c["cls"], "value")
            worst[key] = max(worst.get(key, 0.0), ev)
            assert ev <= TK.VALUE_BAR, (layout, name, loss, ref["loss"])
            if c["cls"] == "unique":
                eg = np.abs(g - ref["grad"]).max() / np.abs(ref["grad"]).max()
                worst[("unique", "grad")] = max(worst.get(("unique", "grad"), 0.0), eg)
                print(f"{layout:8s} {name:28s} unique     gap {c['gap']:.1e}  value error {ev:.2e}  gradient error {eg:.2e}")
                assert eg <= TK.GRAD_BAR, (layout, name, eg)
            else:
                esum = np.abs(g.sum(0)).max() / np.abs(g).max()
                enorm = abs((g * g).sum() * n - 1.0)
                for k, v in (("sum", esum), ("norm", enorm)):
                    worst[(c["cls"], k)] = max(worst.get((c["cls"], k), 0.0), v)
                print(f"{layout:8s} {name:28s} {c['cls']:10s} gap {c['gap']:.1e}  value error {ev:.2e}  |sum g| / max |g| {esum:.2e}  "
                      f"|n sum |g|^2 - 1| {enorm:.2e}  max |g - g_svd| / max |g_svd| "
                      f"{np.abs(g - ref['grad']).max() / np.abs(ref['grad']).max():.2e} (not compared)")
                assert esum <= 1e-6 and enorm <= 1e-6, (layout, name, esum, enorm)
    for key, v in sorted(worst.items()):
        print(f"worst {key[0]:10s} {key[1]:5s} {v:.2e}")


def test_kabsch_loss_of_a_structure_against_itself_is_zero_to_the_bit():
    """prediction == truth for every geometry, lines, planes and the single point included: loss 0.0 and all-zero gradient bits"""
    for layout in ("dense", "straddle"):
        inputs = []
        for name in C.cases():
            pred, true, seq = C.loss_inputs(name, layout)
            same = np.where(np.isnan(true), pred, true)           # the truth where it is present, garbage elsewhere
            inputs.append((same, true, seq))
        # ... and the prediction on ONE point, a present one, against the truth on that one point
        pred, true, seq = C.loss_inputs("one-point", layout)
        point = np.where(np.isnan(true), true, pred[C.loss_reference("one-point", layout)["slots"][0]])
        inputs.append((np.where(np.isnan(true), pred, point), point, seq))
        stats, dcrd = run_loss(inputs)
        for i, name in enumerate(list(C.cases()) + ["both on one point"]):
            assert stats[i, 0] == 0.0 and not np.signbit(stats[i, 0]) and not bits(dcrd[i]).any(), (layout, name, stats[i])
            assert stats[i, 1] == len(C.cases()[name]["a"] if i < len(C.cases()) else C.cases()["one-point"]["a"])


def test_kabsch_loss_of_a_line_against_itself_is_zero_to_the_bit():
    """rotation_cases.grid_lines: the identity ties with the half turn about the line, and must win"""
    lines = C.grid_lines()
    inputs = [C.M.embed(x, x, L=2) for _, x in lines]
    stats, dcrd = run_loss(inputs)
    bad = [d for (d, _), s, g in zip(lines, stats, dcrd) if not (s[0] == 0.0 and s[1] == 20 and not bits(g).any())]
    assert not bad, (len(bad), bad[:10])


def test_kabsch_loss_one_point_is_the_reference():
    for name in ("one-point", "one-point+noise", "axis-one-point"):
        for layout in ("dense", "straddle"):
            ref = C.loss_reference(name, layout)
            stats, dcrd = run_loss([C.loss_inputs(name, layout)])
            assert np.isfinite(stats[0, 0]) and abs(float(stats[0, 0]) - ref["loss"]) <= TK.VALUE_BAR * ref["loss"], (name, layout)
            assert abs(ref["loss"] - ref["rg"]) <= 1e-12 * ref["rg"]          # the prediction is its own centroid: loss = rg of the truth


def test_kabsch_loss_origin_search():
    """The first present slot in every round and wavefront of the origin search that rows of L = 37 and 74 have
    (rotation_cases.origin_cases says which first slot reaches which): value and gradient at the existing bars, and the same
    bits alone as inside a batch."""
    oc = C.origin_cases()
    for L in (37, 74):
        keys = [k for k in oc if k[0] == L]
        stats, dcrd = run_loss([oc[k] for k in keys])
        for i, k in enumerate(keys):
            pred, true, seq = oc[k]
            ref = C.KR.kabsch_loss_reference(pred, true, seq)
            first = int(ref["slots"][0])
            assert stats[i, 1] == ref["n"], k
            absent = np.ones(len(pred), bool)
            absent[ref["slots"]] = False
            assert not bits(dcrd[i][absent]).any(), k
            one = run_loss([oc[k]])
            assert np.array_equal(bits(one[0][0]), bits(stats[i])) and np.array_equal(bits(one[1][0]), bits(dcrd[i])), k
            if ref["n"] < 3:
                assert np.isnan(stats[i, 0]) and not bits(dcrd[i]).any(), k
                print(f"L {L} first slot {first:4d} (round {first // 256}, wavefront {first % 256 // 64}): n {ref['n']}, NaN")
                continue
            ev = abs(float(stats[i, 0]) - ref["loss"]) / ref["loss"]
            eg = np.abs(dcrd[i].astype(np.float64) - ref["grad"]).max() / np.abs(ref["grad"]).max()
            print(f"L {L} first slot {first:4d} (round {first // 256}, wavefront {first % 256 // 64}): n {ref['n']}  "
                  f"value error {ev:.2e}  gradient error {eg:.2e}")
            assert ev <= TK.VALUE_BAR and eg <= TK.GRAD_BAR, (k, ev, eg)


# ----------------------------------------------------------------------------- ensemble
@pytest.mark.parametrize("L", C.ENSEMBLE_LS)
def test_ensemble_spread_on_every_geometry(L):
    dev = torch.device("cuda:0")
    bases, ref, samples, seq, extent = C.ensemble_inputs(L)
    want_rmsd, want_rmsf, want_usable = C.ensemble_reference(L)
    got = {k: [] for k in ("rmsd", "rmsf", "usable")}
    for at in range(0, len(bases), CHUNK):
        d = [torch.from_numpy(np.ascontiguousarray(a[at:at + CHUNK])).to(dev) for a in (ref, samples, seq)]
        a, b = TE.call_abi(*d, 0xFF, dev), TE.call_abi(*d, 0x00, dev)
        for k in a:
            assert a[k].tobytes() == b[k].tobytes(), k
            got[k].append(a[k])
    got = {k: np.concatenate(v) for k, v in got.items()}
    assert np.array_equal(got["usable"], want_usable) and (want_usable == 3).all()
    worst = {}
    for i, base in enumerate(bases):
        kinds, per_atom, all_atom = C.ensemble_compared(base)
        pres = ER.present_of(seq[i])
        x = extent[i]
        ratio = lambda g, w: float((np.abs(g.astype(np.float64) ** 2 - w ** 2) / ER.tol_sq(w, x)).max())    # noqa: E731
        assert np.isfinite(want_rmsd[i]).all() and np.isfinite(got["rmsd"][i]).all(), base
        r_rmsd = ratio(got["rmsd"][i], want_rmsd[i])              # the optimum: compared in every class
        for col in (0, 1):                                         # the NaN pattern is exact, whatever is compared
            assert np.array_equal(np.isnan(got["rmsf"][i, :, col]), np.isnan(want_rmsf[i, :, col])), (base, col)
            assert np.array_equal(np.isfinite(want_rmsf[i, :, col]), pres), (base, col)
        r_ca = ratio(got["rmsf"][i, pres, 0], want_rmsf[i, pres, 0])
        r_all = ratio(got["rmsf"][i, pres, 1], want_rmsf[i, pres, 1])
        cls = "unique" if all_atom else ("free, residuals invariant" if per_atom else "free / value-only, optimum only")
        print(f"L {L} {base:24s} {'/'.join(kinds):32s} extent {x:8.1f} A  |gpu^2 - ref^2| / tol_sq: rmsd {r_rmsd:.3f}  C-alpha rmsf "
              f"{r_ca:.3f}{'' if per_atom else ' (not compared)'}  all-atom rmsf {r_all:.3f}{'' if all_atom else ' (not compared)'}")
        assert r_rmsd <= 1.0, (base, r_rmsd)
        assert not per_atom or r_ca <= 1.0, (base, r_ca)
        assert not all_atom or r_all <= 1.0, (base, r_all)
        for k, v, used in (("rmsd", r_rmsd, True), ("ca", r_ca, per_atom), ("all", r_all, all_atom)):
            if used:
                worst[(cls, k)] = max(worst.get((cls, k), 0.0), v)
    for key, v in sorted(worst.items()):
        print(f"L {L} worst ratio to tol_sq, {key[0]}, {key[1]}: {v:.3f}")


# ----------------------------------------------------------------------------- TM-score
@pytest.mark.parametrize("name", list(C.TM_CASES))
def test_tm_score_on_rank_deficient_chains(name):
    pred, true, seq, ref = C.tm_case_with_reference(name)
    score, counts, xform = TT.run(pred[None], true[None], seq[None])
    TT.check_protein(name, score[0], counts[0], xform[0], pred, true, seq, ref)
    again = TT.run(pred[None], true[None], seq[None])
    for a, b in zip((score, counts, xform), again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), name


def test_tm_score_in_a_batch_is_the_score_alone():
    names = ("line-line20", "line-3d65", "zigzag5", "three-collinear")
    pred, true, seq = C.T.stack([C.tm_case_with_reference(n)[:3] for n in names])
    score, counts, xform = TT.run(pred, true, seq)
    for b, n in enumerate(names):
        TT.check_protein(f"batch/{n}", score[b], counts[b], xform[b], pred[b], true[b], seq[b], C.tm_case_with_reference(n)[3])
        alone = TT.run(*(a[None] for a in C.tm_case_with_reference(n)[:3]))
        assert np.array_equal(score[b].view(np.int32), alone[0][0].view(np.int32)) and np.array_equal(counts[b], alone[1][0])
        assert np.array_equal(xform[b].view(np.int32), alone[2][0].view(np.int32))
