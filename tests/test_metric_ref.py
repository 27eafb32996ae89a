"""Pins tests/metric_ref.py, the fp64 references and case builders that tests/test_gpu_angle_mse_edges.py and
tests/test_gpu_kabsch_edges.py hold csrc/angle_mse.hip and csrc/kabsch.hip against.  CPU only.

  * `mse_sums_ref` reproduces the g8_mse golden and `oracle.losses.mse_over_angles` on cases that hold every row class;
    `mse_grad_ref` is the fp64 autograd gradient of the oracle;
  * `superposed_rmsd_ref` (explicit superposition) agrees with `oracle.losses.kabsch_rmsd` (trace identity) in general position,
    gives 0 for an exact rigid motion, > 0 and rotation-invariant for a mirror image, is symmetric and translation-invariant,
    and gives the hand value of a two-point stretch;
  * the case builders are what they claim: row classes, present-atom counts, the rank of H of every geometry;
  * a numpy transcription of the kernel's fp64 arithmetic (moments, trace identity, Jacobi on H^T H) stays inside `kabsch_bar` on
    every geometry - the bar is not derived from it, this only shows that the bar can be met.
"""
import numpy as np
import pytest
import torch

import metric_ref as R
from oracle import losses as olosses


# --------------------------------------------------------------------------- angle MSE
def test_mse_sums_ref_reproduces_the_golden(golden):
    g = golden("g8_mse")
    sums, counts = R.mse_sums_ref(g["pred"], g["true"])
    for k, key in enumerate(("full", "bb", "sc")):
        assert sums[2 * k] / sums[2 * k + 1] == pytest.approx(float(g[key]), rel=1e-6)
        assert counts[k] == sums[2 * k + 1] and isinstance(counts[k], int)


@pytest.mark.parametrize("T,heavy", [(27, None), (255, 0), (257, 256), (600, 599)])
def test_mse_refs_against_the_oracle_on_every_row_class(T, heavy):
    pred, true, classes = R.make_mse_case(T, heavy, seed=T)
    R.check_row_classes(true, classes)
    assert set(classes) == set(R.ROW_CLASSES)
    sums, counts = R.mse_sums_ref(pred, true)
    p = torch.from_numpy(pred).double()[None].requires_grad_()
    t = torch.from_numpy(true).double()[None]
    for k, kw in enumerate(({}, {"bb_only": True}, {"sc_only": True})):
        want = olosses.mse_over_angles(p, t, **kw)
        assert sums[2 * k] / counts[k] == pytest.approx(want.item(), rel=1e-12)
    # the counts, by hand from the class table
    tab = np.array([R.ROW_CLASSES[c] for c in classes], dtype=np.int64)
    assert counts == (int((tab[:, 0] * (tab[:, 3] + tab[:, 4])).sum()), int((tab[:, 1] * tab[:, 3]).sum()),
                      int((tab[:, 2] * tab[:, 4]).sum()))
    olosses.mse_over_angles(p, t).backward()
    g = R.mse_grad_ref(pred[None], true[None], 1.0, counts[0])
    assert np.abs(g - p.grad.numpy()).max() <= 1e-15
    assert np.all(g[0][~R.mse_masks(true)["full"]] == 0)
    if heavy is not None:                                         # the heavy row is >= 1e-3 of every sum it is in
        assert 24 * R.HEAVY ** 2 * 0.999 >= 1e-3 * sums[0] and 12 * R.HEAVY ** 2 * 0.999 >= 1e-3 * max(sums[2], sums[4])


def test_heavy_row_outweighs_the_bar_at_the_largest_case():
    """T = 32768 + 257 rows with |p - t| <= 0.5: the sum is at most T 24 / 4 = 1.98e5, mean uniform 1/12 per element = 6.6e4, and
    the heavy row adds 24 * 64 = 1536: more than 1e-3 of the sum, a hundred times the rel 1e-5 bar."""
    T = 32768 + 257
    assert 24 * R.HEAVY ** 2 >= 1e-3 * T * 24 * R.LIGHT ** 2 / 3 * 1.2   # E (u^2) = LIGHT^2 / 3, rows outside the slice only lower it


def test_row_selection_rules_one_by_one():
    t = np.zeros((6, 24))
    t[1, 3] = np.nan                       # NaN selects full and bb; nothing of it is counted
    t[2, 20] = 1e-40                       # a denormal selects full and sc
    t[3, :] = -0.0                         # -0.0 selects nothing
    t[4, 0], t[4, 23] = 1.0, np.nan
    t[5, 12] = -2.0
    _, counts = R.mse_sums_ref(np.ones((6, 24)), t)
    # full: rows 1 (23), 2 (24), 4 (23), 5 (24); bb: rows 1 (11), 4 (12); sc: rows 2 (12), 4 (11), 5 (12)
    assert counts == (94, 23, 35)
    sums, _ = R.mse_sums_ref(np.ones((6, 24)), t)
    assert sums[2] == pytest.approx(11 + 11)                      # row 1: eleven (1 - 0)^2; row 4: (1 - 1)^2 + eleven


# --------------------------------------------------------------------------- superposed RMSD
def test_rmsd_ref_agrees_with_the_oracle_in_general_position():
    rng = np.random.default_rng(0)
    for n in (3, 4, 17, 200):
        a, b = rng.normal(0, 9, (n, 3)), rng.normal(0, 9, (n, 3))
        got, sig, m, M = R.superposed_rmsd_ref(a, b)
        assert got == pytest.approx(olosses.kabsch_rmsd(a, b), rel=1e-12) and m == n
        assert sig[0] >= sig[1] >= sig[2] >= 0 and M == pytest.approx((a ** 2).sum() + (b ** 2).sum(), rel=1e-15)
        near = b @ R.rotation(rng).T + rng.normal(0, 0.5, (n, 3))
        assert R.superposed_rmsd_ref(near, b)[0] == pytest.approx(olosses.kabsch_rmsd(near, b), rel=1e-10)


def test_rmsd_ref_known_answers():
    rng = np.random.default_rng(1)
    b = rng.normal(0, 8, (30, 3))
    q, q2 = R.rotation(rng), R.rotation(rng)
    moved = b @ q.T + [3.0, -40.0, 7.0]
    assert R.superposed_rmsd_ref(moved, b)[0] <= 1e-12                          # an exact rigid motion
    mirrored = b * [1.0, 1.0, -1.0]
    m0 = R.superposed_rmsd_ref(mirrored, b)[0]
    assert m0 > 1.0
    assert R.superposed_rmsd_ref(mirrored @ q2.T + [1.0, 2.0, 3.0], b)[0] == pytest.approx(m0, rel=1e-12)
    noisy = moved + rng.normal(0, 0.5, b.shape)
    r = R.superposed_rmsd_ref(noisy, b)[0]
    assert R.superposed_rmsd_ref(b, noisy)[0] == pytest.approx(r, rel=1e-12)     # symmetric
    assert R.superposed_rmsd_ref(noisy + 1e4, b + 1e4)[0] == pytest.approx(r, rel=1e-9)   # 1e4 / 8 * 2^-52 per coordinate
    # two points 2 apart against two points 4 apart: centred +-1 against +-2, residual 1 each: rmsd 1 (= sqrt(2) * sqrt(1/2), the
    # hand value per point pair); and a stretch by s of a unit pair: |s - 1| / 2 * sqrt(2) / sqrt(2)
    two = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    far = np.array([[5.0, 5.0, 5.0], [5.0, 9.0, 5.0]])
    got, sig, n, _ = R.superposed_rmsd_ref(two, far)
    assert got == pytest.approx(np.sqrt(2.0) * np.sqrt(0.5), rel=1e-14) and n == 2
    assert sig[0] == pytest.approx(4.0) and sig[1] <= 1e-15
    assert np.isnan(R.superposed_rmsd_ref(np.zeros((0, 3)), np.zeros((0, 3)))[0])
    assert R.superposed_rmsd_ref([[1.0, 2.0, 3.0]], [[-4.0, 0.0, 9.0]])[0] == 0.0
    for bad in (np.nan, np.inf, -np.inf):
        x = b.copy()
        x[4, 1] = bad
        assert np.isnan(R.superposed_rmsd_ref(x, b)[0]) and np.isnan(olosses.kabsch_rmsd(x, b))
    big = b.copy()
    big[4, 1] = 1e30
    assert np.isfinite(R.superposed_rmsd_ref(big, b)[0]) and R.superposed_rmsd_ref(big, b)[0] > 1e28


def test_present_atoms_rule():
    rng = np.random.default_rng(2)
    L = 4
    pred, true = rng.normal(size=(L * 14, 3)), rng.normal(size=(L * 14, 3))
    seq = np.array([3, R.PAD_ID, 7, 0])
    true[0, 0], true[1, 1], true[2, 2], true[50] = np.nan, np.nan, np.nan, np.nan
    pred[5] = np.nan                                              # the prediction does not decide presence
    m = R.present_atoms(pred, true, seq)
    assert m.sum() == 3 * 14 - 4 and not m[:3].any() and not m[14:28].any() and not m[50] and m[5] and m[3]


# --------------------------------------------------------------------------- the Kabsch cases are what they claim
def kernel_arithmetic(a, b):
    """csrc/kabsch.hip after its sweep, in numpy fp64: the 18 uncentred moments, H and e0 centred from them, cyclic Jacobi on
    H^T H, s1 + s2 + sign(det) s3, the clamp - and the rounding of the result to fp32"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = float(len(a))
    sa, sb, H0 = a.sum(0), b.sum(0), a.T @ b
    H = H0 - np.outer(sa, sb) / n
    e0 = ((a * a).sum() - (sa * sa).sum() / n) + ((b * b).sum() - (sb * sb).sum() / n)
    m = H.T @ H
    for _ in range(12):
        if abs(m[0, 1]) + abs(m[0, 2]) + abs(m[1, 2]) <= 1e-300:
            break
        for p in range(2):
            for q in range(p + 1, 3):
                apq = m[p, q]
                if apq == 0.0:
                    continue
                theta = (m[q, q] - m[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                r = 3 - p - q
                m[p, p], m[q, q] = m[p, p] - t * apq, m[q, q] + t * apq
                m[p, q] = m[q, p] = 0.0
                arp, arq = m[r, p], m[r, q]
                m[r, p] = m[p, r] = c * arp - s * arq
                m[r, q] = m[q, r] = s * arp + c * arq
    sv = np.sqrt(np.maximum(np.diag(m), 0.0))
    trace = sv.sum() - (2.0 * sv.min() if np.linalg.det(H) < 0 else 0.0)
    return float(np.float32(np.sqrt(max(e0 - 2.0 * trace, 0.0) / n)))


def test_geometry_cases_are_what_they_claim_and_the_bar_can_be_met():
    cases = R.geometry_cases()
    assert len(cases) == 2 * len(R.GEOMETRY_RANK)
    worst = 0.0
    for name, (a, b, rigid) in cases.items():
        assert a.dtype == b.dtype == np.float32 and a.shape == b.shape and len(a) in (8, R.N_GEO)
        want, sig, n, M = R.superposed_rmsd_ref(a, b)
        rank = R.GEOMETRY_RANK[name.replace("+noise", "")]
        # rank by the singular values: a lost direction is at fp32 rounding level (coordinates up to 1e4: 1e-3 A on 40 atoms)
        small = 1e-4 * sig[0] if sig[0] > 0 else 0.0
        assert int((sig > small).sum()) == rank, (name, sig)
        if rank == 1:
            assert sig[1] <= R.RANK1_TOL * sig[0], (name, sig)
        elif rank >= 2:
            assert sig[1] > 100 * R.RANK1_TOL * sig[0], (name, sig)
        if rigid:                                                 # zero up to the fp32 rounding of coordinates of size c: 1e-7 c
            assert want <= 2e-7 * np.sqrt(M / n), (name, want)
        if name.startswith("mirror"):
            assert want > 1.0
        if name.startswith("mirror-cube") and not name.endswith("noise"):
            assert sig[2] == pytest.approx(sig[0], rel=1e-6)      # equal singular values ...
            ac, bc = a.astype(np.float64) - a.mean(0), b.astype(np.float64) - b.mean(0)
            assert np.linalg.det(ac.T @ bc) < 0                   # ... under a reflection
        if name.endswith("+noise") and rank == 3 and "mirror" not in name:
            assert 0.4 < want < 1.0                               # sqrt(3) * 0.5 less the fitted part
        with np.errstate(over="ignore"):                         # theta^2 may overflow: t = 1 / inf = 0, as on the device
            got = kernel_arithmetic(a, b)
        ratio = abs(got * got - want * want) / R.kabsch_bar(want, sig, n, M)
        worst = max(worst, ratio)
        assert ratio <= 1.0, (name, got, want, ratio)
    print(f"worst ratio of the numpy transcription: {worst:.3f}")
    m = R.superposed_rmsd_ref(*cases["mirror"][:2])[0]
    assert R.superposed_rmsd_ref(*cases["mirror-rotated"][:2])[0] == pytest.approx(m, rel=1e-5)   # fp32 inputs


def test_slot_sets_and_embedding():
    seen = set()
    for L in R.SLOT_LS:
        last = L * 14 - 1
        sets = R.sparse_slot_sets(L)
        for s in sets:
            assert 4 <= len(s) <= 6 and len(set(s)) == len(s) and max(s) <= last and last in s, (L, s)
        covered = set().union(*sets)
        assert {e for e in R.SLOT_EDGES if e <= last} <= covered and last in covered, (L, sets)
        seen |= covered
        a = np.arange(len(sets[0]) * 3, dtype=np.float32).reshape(-1, 3)
        pred, true, seq = R.embed(a, a + 1, L=L, slots=sets[0])
        m = R.present_atoms(pred, true, seq)
        assert sorted(np.nonzero(m)[0].tolist()) == sets[0] and np.isfinite(pred).all()
        assert np.array_equal(pred[m], a) and np.array_equal(true[m], a + 1)
    assert set(R.SLOT_EDGES) <= seen
    assert [L * 14 for L in R.SLOT_LS] == [14, 252, 266, 518, 1036]
