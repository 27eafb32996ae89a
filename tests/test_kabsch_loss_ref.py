"""tests/kabsch_loss_ref.py held against what does not depend on it: central finite differences, the oracle's Kabsch RMSD, the
dRMSD reference on a mirror image, and Horn's rotation (the arithmetic of csrc/tm_rotation.h, which the kernel calls) on the
inputs of tests/test_gpu_kabsch_loss.py.  CPU only."""
import numpy as np
import pytest

import kabsch_loss_ref as R
from drmsd_ref import drmsd_reference
from oracle.losses import kabsch_rmsd

USABLE = [(L, name) for L in R.LENGTHS for name in R.proteins(L) if np.isfinite(R.reference(L, name)["loss"])]


def test_the_cases_hold_every_edge():
    n = {(L, name): R.reference(L, name)["n"] for L in R.LENGTHS for name in R.proteins(L)}
    assert n[(1, "noisy")] == 12 and n[(5, "noisy")] > 50 and n[(19, "noisy")] > 200 and n[(37, "noisy")] > 400
    for L in R.LENGTHS:
        assert (n[(L, "none")], n[(L, "two")], n[(L, "three")]) == (0, 2, 3)
        assert all(np.isnan(R.reference(L, k)["loss"]) for k in ("none", "two")) and np.isfinite(R.reference(L, "three")["loss"])
        pred, true, seq = R.proteins(L)["noisy"]
        present = R.present_slots(true, seq)
        assert not present[0] and not present[-1] and (seq != R.PAD).all()             # NaN truth at the first and the last slot
    pred, true, seq = R.proteins(37)["short"]
    assert (seq == R.PAD).sum() == 2 and (true[-2 * R.SLOTS:] == 0).all()              # pad residues: zeros, not NaN
    for name in R.UNUSABLE:
        ref = R.reference(37, name)
        assert np.isnan(ref["loss"]) and not ref["grad"].any() and ref["n"] == n[(37, "noisy")]
    a, b = R.reference(37, "nan-pred-absent"), R.reference(37, "finite-pred-absent")
    assert a["n"] == n[(37, "noisy")] - 1 and a["loss"] == b["loss"] and np.array_equal(a["grad"], b["grad"])
    pred, true, seq = R.proteins(37)["copy"]
    m = R.present_slots(true, seq)
    assert np.array_equal(pred[m], true[m]) and not np.array_equal(pred[:len(m) - 2 * R.SLOTS], true[:len(m) - 2 * R.SLOTS])
    assert R.reference(37, "copy")["loss"] < 1e-12 and R.reference(37, "rigid")["loss"] < 1e-5 * R.reference(37, "rigid")["rg"]
    far = R.proteins(37)["far"]
    assert np.abs(far[0][R.present_slots(far[1], far[2])]).min() > 900


def test_gradient_against_central_differences():
    for L, name in ((5, "noisy"), (5, "short"), (1, "three"), (5, "mirror"), (5, "far")):
        pred, true, seq = R.proteins(L)[name]
        ref = R.reference(L, name)
        p = pred.astype(np.float64)
        h, worst = 1e-5, 0.0
        for s in list(ref["slots"][:6]) + [int(np.nonzero(~R.present_slots(true, seq))[0][0])]:
            for k in range(3):
                up, down = p.copy(), p.copy()
                up[s, k] += h
                down[s, k] -= h
                fd = (R.kabsch_loss_reference(up, true, seq)["loss"] - R.kabsch_loss_reference(down, true, seq)["loss"]) / (2 * h)
                worst = max(worst, abs(fd - ref["grad"][s, k]))
        # the truncation term h^2 f''' / 6 and the rounding 1e-16 loss / h, both far below 1e-7 of a gradient of size 1 / sqrt(n)
        assert worst < 1e-7 * np.abs(ref["grad"]).max(), (L, name, worst)
        assert not ref["grad"][~R.present_slots(true, seq)].any()
        assert abs(ref["grad"].sum(0)).max() < 1e-12                                   # sum r_k = 0


@pytest.mark.parametrize("L", R.LENGTHS)
def test_value_against_the_oracle(L):
    for name, (pred, true, seq) in R.proteins(L).items():
        ref = R.reference(L, name)
        if not np.isfinite(ref["loss"]):
            continue
        m = R.present_slots(true, seq)
        want = kabsch_rmsd(pred[m], true[m])                      # the trace formula: sqrt of a difference, 1e-16 e0 / n absolute
        assert abs(ref["loss"] ** 2 - want ** 2) < 1e-11 * ref["rg"] ** 2, (L, name)


def test_a_mirror_image_has_no_drmsd_and_a_large_loss():
    for L in (5, 19, 37):
        pred, true, seq = R.proteins(L)["mirror"]
        ref = R.reference(L, "mirror")
        d = drmsd_reference(pred, true, seq)["stats"][0]
        print(f"L {L}: mirror image, loss {ref['loss']:.3f} A (rg {ref['rg']:.3f} A), dRMSD {d:.2e} A")
        assert d < 1e-5 and ref["loss"] > 0.1 * ref["rg"] and ref["loss"] > 1.0
        assert abs(np.linalg.det(ref["R"]) - 1.0) < 1e-12                              # never the reflection that would score 0


def test_horn_and_the_svd_agree_on_the_rotation():
    worst = 0.0
    for L, name in USABLE:
        pred, true, seq = R.proteins(L)[name]
        m = R.present_slots(true, seq)
        a, b = pred[m].astype(np.float64), true[m].astype(np.float64)
        a, b = a - a.mean(0), b - b.mean(0)
        H = R.horn_rotation(a, b)
        assert abs(np.linalg.det(H) - 1.0) < 1e-12
        if name == "three" or R.reference(L, name)["n"] == 3:
            # three atoms span a plane: a proper rotation and its product with the reflection in that plane fit equally, both
            # routes must return the proper one
            assert abs(np.linalg.det(R.reference(L, name)["R"]) - 1.0) < 1e-12
        worst = max(worst, np.abs(H - R.reference(L, name)["R"]).max())
        assert np.abs(H - R.reference(L, name)["R"]).max() < 1e-9, (L, name)
    print(f"Horn against SVD over {len(USABLE)} proteins: largest entry difference {worst:.2e}")
    pred, true, seq = R.proteins(37)["copy"]                       # the truth itself: Horn's matrix has a zero first row, R = 1 exactly
    m = R.present_slots(true, seq)
    a = true[m].astype(np.float64) - true[m].astype(np.float64).mean(0)
    assert np.array_equal(R.horn_rotation(a, a), np.eye(3))
