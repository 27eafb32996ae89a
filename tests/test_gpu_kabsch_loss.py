"""The superposition loss on the device (csrc/kabsch_loss.hip, `ptamd_kabsch_loss_fwd_bwd`, losses.kabsch_forward_backward) against
tests/kabsch_loss_ref.py - numpy fp64, the rotation from an SVD - on the same fp32 inputs.

Four batches, rows of L = 1, 5, 19 and 37 residues: 14 slots (under one wavefront), 70 (one wavefront plus 6), 266 (one round of the
256 threads plus 10) and 518 (two rounds plus a tail).  Each mixes the edges of kabsch_loss_ref.proteins: NaN truth at the first
slot, the last one and scattered between; proteins shorter than the row; no, 2 and 3 present atoms; the mirror image; a rigid
motion of the truth; the truth itself; a prediction 1e3 A from the origin; NaN and inf on a present predicted atom.

Bars.  Kernel and reference read the same fp32 inputs, so what separates them is the kernel's fp64 arithmetic and ONE rounding to
fp32 on output (2^-24 = 6.0e-8 relative).  Per protein, with ref the reference:
    value      |loss - ref| / ref                       measured 3.21e-8 (L 37 `short`),  VALUE_BAR  = 8 x that = 2.57e-7
    gradient   max |g - g_ref| / max |g_ref|            measured 4.71e-8 (L 37 `short`),  GRAD_BAR   = 8 x that = 3.77e-7
    metric     |loss - ptamd_kabsch_rmsd| / rg          measured 5.10e-8 (L 19 `three`),  METRIC_BAR = 8 x that = 4.08e-7
the largest figure over every usable protein of the four batches, on an MI355X (`rigid` and `copy` leave the first two: their
reference loss is rounding itself).  rg is the RMS distance of the present true atoms from their mean: the metric takes the
RMSD from a trace formula, sqrt of a difference of sums of squares, whose error is absolute in the protein's size - 1e-16 rg^2
under the root, 1e-8 rg where the RMSD itself is zero - and two eigen-solvers meet there, hence its own bar.  The factor 8 leaves
room for box-to-box differences in nothing but the final rounding.  All three are far below what tests/test_gpu_fape.py holds
`fape` to (value 1e-5 of a loss of order 1, gradient rel-L2 1e-4).  `rigid` - the truth rotated and shifted in fp64, rounded to
fp32 - has a loss below VALUE_BAR x rg (measured 3.1e-8 ... 4.0e-8 rg, the rounding of its coordinates) and a finite gradient;
`copy` has loss 0 and an all-zero gradient, to the bit.  The figures every test prints are in profiles/kabsch/NOTES.md."""
import ctypes

import numpy as np
import pytest
import torch

import kabsch_loss_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MEASURED_VALUE, MEASURED_GRAD, MEASURED_METRIC = 3.21e-8, 4.71e-8, 5.10e-8
VALUE_BAR, GRAD_BAR, METRIC_BAR = 8 * MEASURED_VALUE, 8 * MEASURED_GRAD, 8 * MEASURED_METRIC
POISON = 7.25


def run(pred, true, seq, need_grad=True, poison=POISON):
    """One call of the entry point on host arrays -> (stats [B,2] fp32, dcrd [B,L*14,3] fp32 or None) as numpy.  dcrd is
    poisoned beforehand: whatever the call does not write shows."""
    from protein_transformer_amd import _lib
    p, t, s = (torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (pred, true, seq))
    B, L = s.shape
    stats = torch.full((B, 2), poison, dtype=torch.float32, device=DEV)
    dcrd = torch.full_like(p, poison) if need_grad else None
    rc = _lib.lib().ptamd_kabsch_loss_fwd_bwd(_lib.ptr(p), _lib.ptr(t), _lib.ptr(s), B, L, _lib.ptr(stats), _lib.ptr(dcrd),
                                              _lib.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return stats.cpu().numpy(), None if dcrd is None else dcrd.cpu().numpy()


@pytest.fixture(scope="module")
def results():
    """L -> (names, pred, true, seq, stats, dcrd): every batch once, shared by the tests below and left unchanged."""
    out = {}
    for L in R.LENGTHS:
        names, pred, true, seq = R.batch(L)
        out[L] = (names, pred, true, seq, *run(pred, true, seq))
    return out


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def test_values_and_gradients_against_the_reference(results):
    worst = {"value": 0.0, "grad": 0.0}
    for L, (names, pred, true, seq, stats, dcrd) in results.items():
        for i, name in enumerate(names):
            ref = R.reference(L, name)
            assert stats[i, 1] == ref["n"], (L, name)
            if not np.isfinite(ref["loss"]):                       # n < 3, or a NaN / inf on a present predicted atom
                assert np.isnan(stats[i, 0]) and not bits(dcrd[i]).any(), (L, name)
                continue
            assert np.isfinite(dcrd[i]).all(), (L, name)
            if name == "copy":
                assert stats[i, 0] == 0.0 and not bits(dcrd[i]).any(), (L, name, stats[i, 0])
                continue
            if name == "rigid":
                print(f"L {L:2d} rigid: loss {stats[i, 0]:.3e} A = {stats[i, 0] / ref['rg']:.2e} rg (reference {ref['loss']:.3e} A)")
                assert 0 <= stats[i, 0] <= VALUE_BAR * ref["rg"], (L, name)
                continue
            ev = abs(float(stats[i, 0]) - ref["loss"]) / ref["loss"]
            eg = np.abs(dcrd[i].astype(np.float64) - ref["grad"]).max() / np.abs(ref["grad"]).max()
            print(f"L {L:2d} {name:18s} n {ref['n']:4d}  loss {stats[i, 0]:10.6f} A  value error {ev:.2e}  gradient error {eg:.2e}")
            worst = {"value": max(worst["value"], ev), "grad": max(worst["grad"], eg)}
    print(f"largest value error {worst['value']:.2e} (bar {VALUE_BAR:.1e}), largest gradient error {worst['grad']:.2e} "
          f"(bar {GRAD_BAR:.1e})")
    assert worst["value"] <= VALUE_BAR and worst["grad"] <= GRAD_BAR


def test_exact_zeros_outside_the_present_atoms(results):
    for L, (names, pred, true, seq, stats, dcrd) in results.items():
        for i, name in enumerate(names):
            absent = ~R.present_slots(true[i], seq[i])
            assert absent.any() and not bits(dcrd[i][absent]).any(), (L, name)          # +0.0, not the poison, not -0.0
        assert not (dcrd == POISON).any() and not (stats == POISON).any()


def test_a_mirror_image_is_told_from_the_structure(results):
    for L in (5, 19, 37):
        names, _, _, _, stats, _ = results[L]
        ref = R.reference(L, "mirror")
        assert stats[names.index("mirror"), 0] > 0.1 * ref["rg"] and stats[names.index("mirror"), 0] > 1.0


def test_an_unusable_prediction_touches_nobody_else(results):
    names, pred, true, seq, stats, dcrd = results[37]
    for name in R.UNUSABLE:
        i = names.index(name)
        assert np.isnan(stats[i, 0]) and not bits(dcrd[i]).any()
    # the same atom made absent in the truth: its NaN is never read, the bits are those of any finite value there
    a, b = names.index("nan-pred-absent"), names.index("finite-pred-absent")
    assert np.isfinite(stats[a, 0]) and np.array_equal(bits(stats[a]), bits(stats[b])) and np.array_equal(bits(dcrd[a]), bits(dcrd[b]))
    assert stats[a, 1] == stats[names.index("noisy"), 1] - 1
    # the neighbours, in a batch without the unusable proteins
    keep = [n for n in names if n not in R.UNUSABLE]
    _, p2, t2, s2 = R.batch(37, keep)
    stats2, dcrd2 = run(p2, t2, s2)
    at = [names.index(n) for n in keep]
    assert np.array_equal(bits(stats2), bits(stats[at])) and np.array_equal(bits(dcrd2), bits(dcrd[at]))


def test_forward_only_and_reproducibility(results):
    for L, (names, pred, true, seq, stats, dcrd) in results.items():
        fwd, none = run(pred, true, seq, need_grad=False)
        assert none is None and np.array_equal(bits(fwd), bits(stats)), L
        again = run(pred, true, seq, poison=-3.5)
        assert np.array_equal(bits(again[0]), bits(stats)) and np.array_equal(bits(again[1]), bits(dcrd)), L
    names, pred, true, seq, stats, dcrd = results[37]
    for name in ("noisy", "short", "far", "three"):               # alone in a batch: the bits it has inside the larger one
        i = names.index(name)
        one = run(pred[i:i + 1], true[i:i + 1], seq[i:i + 1])
        assert np.array_equal(bits(one[0][0]), bits(stats[i])) and np.array_equal(bits(one[1][0]), bits(dcrd[i])), name


def test_agreement_with_the_metric(results):
    from protein_transformer_amd.eval_metrics import kabsch_rmsd_batch
    worst = 0.0
    for L, (names, pred, true, seq, stats, _) in results.items():
        rmsd = kabsch_rmsd_batch(*(torch.from_numpy(x).to(DEV) for x in (pred, true, seq))).cpu().numpy()
        for i, name in enumerate(names):
            ref = R.reference(L, name)
            if ref["n"] < 3:
                continue
            if not np.isfinite(ref["loss"]):
                assert np.isnan(rmsd[i]) and np.isnan(stats[i, 0]), (L, name)
                continue
            err = abs(float(stats[i, 0]) - float(rmsd[i])) / ref["rg"]
            print(f"L {L:2d} {name:18s} loss {stats[i, 0]:.6e} A  rmsd-full {rmsd[i]:.6e} A  difference {err:.2e} rg")
            worst = max(worst, err)
    print(f"largest difference to ptamd_kabsch_rmsd {worst:.2e} rg (bar {METRIC_BAR:.1e})")
    assert worst <= METRIC_BAR


def test_host_mirror(results):
    from protein_transformer_amd.losses import kabsch_forward_backward
    names, pred, true, seq, stats, dcrd = results[19]
    p, t, s = (torch.from_numpy(x).to(DEV) for x in (pred, true, seq))
    st, g = kabsch_forward_backward(p, t, s)
    assert np.array_equal(bits(st.cpu().numpy()), bits(stats)) and np.array_equal(bits(g.cpu().numpy()), bits(dcrd))
    st, g = kabsch_forward_backward(p, t, s, need_grad=False)
    assert g is None and np.array_equal(bits(st.cpu().numpy()), bits(stats))


def test_refusals():
    from protein_transformer_amd import _lib
    lib = _lib.lib()
    buf = torch.full((64,), POISON, dtype=torch.float32, device=DEV)
    seq = torch.zeros(2, dtype=torch.int64, device=DEV)
    ok = dict(crd=_lib.ptr(buf), true=_lib.ptr(buf), seq=_lib.ptr(seq), B=1, L=1, stats=_lib.ptr(buf), dcrd=_lib.ptr(buf))

    def call(**kw):
        a = {**ok, **kw}
        return lib.ptamd_kabsch_loss_fwd_bwd(a["crd"], a["true"], a["seq"], a["B"], a["L"], a["stats"], a["dcrd"], _lib.stream())
    for kw in (dict(B=0), dict(L=0), dict(B=-1), dict(L=-4), dict(crd=None), dict(true=None), dict(seq=None), dict(stats=None),
               dict(L=(2 ** 31 - 1) // 28 + 1)):
        assert call(**kw) == -1, kw                                # PTAMD_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert (buf == POISON).all()                                   # nothing was written
    assert isinstance(lib.ptamd_kabsch_loss_fwd_bwd, ctypes._CFuncPtr)
