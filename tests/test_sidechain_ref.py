"""The numpy restatement of the side-chain accuracy metric (tests/sidechain_ref.py) against known answers, and its two forms
against each other - without a GPU.  Also what the GPU test rests on: every case it uses is `well_posed`."""
import math

import numpy as np
import pytest

import nerf_ref
import sidechain_ref as R


def agree(item, threshold=40.0):
    """reference == reference_loops on one protein; returns the reference."""
    ref = R.reference(*item, threshold)
    score, counts, per_res = R.reference_loops(*item, threshold)
    assert np.array_equal(counts, ref["counts"]), (counts, ref["counts"])
    assert np.allclose(score, ref["score"], rtol=0, atol=1e-9, equal_nan=True), (score, ref["score"])
    assert np.allclose(per_res, ref["per_res"], rtol=0, atol=1e-9, equal_nan=True)
    return ref


def all_types(seed, n=40):
    seq = np.arange(n) % 20
    a = R.angles(n, seed)
    return seq, a, R.centred(R.build(seq, a))


def test_the_tables_agree_with_the_atom_names():
    """chi_k ends on side-chain atom k + 1; the symmetric chi is the one the renaming negates; the chi atoms carry the IUPAC names."""
    from protein_transformer_amd.protein.PDB_Creator import ATOM_MAP_14
    assert R.SYM_CHI == {2: 2, 3: 3, 4: 2, 19: 2}
    for r, one in enumerate(R.AA):
        names = ATOM_MAP_14[one]
        assert sum(n != "PAD" for n in names) == 4 + R.NSC[r]
        assert R.NCHI[r] == 0 or R.NSC[r] >= R.NCHI[r] + 1
    chain = {"R": ["CB", "CG", "CD", "NE", "CZ"], "K": ["CB", "CG", "CD", "CE", "NZ"], "M": ["CB", "CG", "SD", "CE"],
             "E": ["CB", "CG", "CD", "OE1"], "Q": ["CB", "CG", "CD", "OE1"], "I": ["CB", "CG1", "CD1"], "L": ["CB", "CG", "CD1"],
             "T": ["CB", "OG1"], "V": ["CB", "CG1"], "S": ["CB", "OG"], "C": ["CB", "SG"], "D": ["CB", "CG", "OD1"],
             "N": ["CB", "CG", "OD1"], "H": ["CB", "CG", "ND1"], "F": ["CB", "CG", "CD1"], "Y": ["CB", "CG", "CD1"],
             "W": ["CB", "CG", "CD1"], "P": ["CB", "CG", "CD"]}
    for one, want in chain.items():
        assert ATOM_MAP_14[one][4:4 + len(want)] == want and R.NCHI[R.AA.index(one)] == len(want) - 1, one


def test_chosen_chi_are_recovered():
    """A chain built by the fp64 NeRF with chosen chi: the reference reads them back - chi_k is angle column 6 + k."""
    seq, a, crd = all_types(7)
    ref = R.reference(crd, crd, seq)
    for r, s in enumerate(seq):
        k = R.NCHI[s]
        assert ref["scored"][r].tolist() == [j < k for j in range(4)]
        assert np.abs(nerf_ref.circ(ref["chi_true"][r, :k] - a[r, 7:7 + k])).max(initial=0.0) < 1e-9, R.AA[s]
    assert not ref["delta"][ref["scored"]].any() and ref["score"].tolist() == [1.0, 1.0, 0.0, 0.0]
    # and a prediction with chi1 of every residue turned by 50 degrees, chi2 by 10: chi1 misses, chi2 hits
    b = a.copy()
    b[:, 7] += math.radians(50)
    b[:, 8] += math.radians(10)
    ref = agree((R.build(seq, b), crd, seq))
    has1, has2 = np.array(R.NCHI)[seq] >= 1, np.array(R.NCHI)[seq] >= 2
    assert np.allclose(ref["delta"][has1, 0], 50.0, atol=1e-9) and np.allclose(ref["delta"][has2, 1], 10.0, atol=1e-9)
    assert ref["score"][0] == 0.0 and ref["score"][1] == 0.0 and ref["counts"][3] == has2.sum()
    assert agree((R.build(seq, b), crd, seq), threshold=50.0 + 1e-6)["score"][0] == 1.0


def test_a_rigid_motion_changes_nothing():
    seq, a, crd = all_types(8)
    ref = agree((R.rigid(crd, 3), crd, seq))
    assert np.nanmax(ref["delta"]) < 1e-9 and ref["score"][2] < 1e-9 and ref["score"][3] < 1e-9
    assert ref["score"][0] == 1.0 and ref["score"][1] == 1.0


def test_a_mirror_image_negates_every_chi():
    seq, a, crd = all_types(9)
    mirror = crd * np.array([1.0, 1.0, -1.0])
    ref, back = R.reference(crd, crd, seq), R.reference(mirror, mirror, seq)
    ok = ref["scored"]
    assert ok.sum() > 40 and np.array_equal(ok, back["scored"])
    assert np.abs(nerf_ref.circ(ref["chi_true"][ok] + back["chi_true"][ok])).max() < 1e-9


def test_exchanging_symmetric_atoms_changes_nothing_and_others_something():
    seq, a, crd = all_types(10)
    b = a.copy()
    b[:, 7:] += np.random.default_rng(1).normal(0, 0.4, (len(seq), 5))
    pred = R.rigid(R.centred(R.build(seq, b)), 5)
    plain, other = agree((pred, crd, seq)), agree((pred, R.swap_symmetric(crd, seq), seq))
    assert np.allclose(plain["delta"], other["delta"], atol=1e-7, equal_nan=True)
    assert np.allclose(plain["d2"], other["d2"], atol=1e-9, equal_nan=True) and np.array_equal(plain["counts"], other["counts"])
    # the same on the prediction
    other = agree((R.swap_symmetric(pred, seq), crd, seq))
    assert np.allclose(plain["delta"], other["delta"], atol=1e-7, equal_nan=True) and np.allclose(plain["d2"], other["d2"], atol=1e-9, equal_nan=True)
    # LEU CD1 / CD2 and VAL CG1 / CG2 are NOT interchangeable
    leu_val = (R.AA.index("L"), R.AA.index("V"))
    other = agree((pred, R.swap_symmetric(crd, seq, types=leu_val), seq))
    rows = np.isin(seq, leu_val)
    col = np.where(seq[rows] == leu_val[0], 1, 0)                # the chi that ends on the exchanged atom: LEU chi2, VAL chi1
    assert (np.abs(plain["delta"][rows, col] - other["delta"][rows, col]) > 1.0).all()
    assert (np.abs(plain["d2"][rows] - other["d2"][rows]) > 1e-3).all()
    assert np.allclose(plain["d2"][~rows], other["d2"][~rows], equal_nan=True)


def test_glycine_and_alanine():
    for one, finite in (("G", False), ("A", True)):
        seq = np.full(12, R.AA.index(one))
        crd = R.centred(R.build(seq, R.angles(12, 11)))
        ref = agree((R.rigid(crd, 2), crd, seq))
        assert np.isnan(ref["score"][:3]).all() and not ref["counts"][:10].any()
        assert np.isfinite(ref["score"][3]) == finite and ref["counts"][10] == (12 if finite else 0)


def test_degenerate_truth_is_not_scored_and_a_degenerate_prediction_is_unusable():
    seq, a, crd = all_types(12, n=20)
    t = crd.reshape(20, R.SLOTS, 3).copy()
    k = R.AA.index("K")
    t[k, 5] = t[k, 4] + (t[k, 4] - t[k, 1])                      # CA, CB, CG on a line: no normal, chi1 and chi2 go
    ref = agree((crd, t.reshape(-1, 3), seq))
    assert ref["scored"][k].tolist() == [False, False, True, True] and not ref["bad"]
    p = crd.reshape(20, R.SLOTS, 3).copy()
    p[k, 2] = p[k, 1]
    ref = agree((p.reshape(-1, 3), crd, seq))
    assert ref["bad"] and np.isnan(ref["score"]).all() and not ref["counts"][[1, 3, 5, 7, 9]].any() and ref["counts"][0] == 18   # (every type but GLY and ALA)


def test_the_bounds_are_what_the_docstring_derives():
    assert R.EPS_CHI == pytest.approx(5.48e-4, rel=1e-2) and R.EPS_RMS == pytest.approx(3.5e-5, rel=2e-2)
    # fp32 arithmetic of the same formulas stays inside them (numpy float32, no fused operations)
    worst = 0.0
    for seed in (1, 2, 3):
        pred, truth, seq = R.pair_case(60, seed)
        ref = R.reference(pred, truth, seq)
        n = len(seq)
        x32 = [v.reshape(n, R.SLOTS, 3) for v in (pred, truth)]
        for k, sl in enumerate(R.CHI_SLOTS):
            chi = []
            for x in x32:
                b1, b2, b3 = x[:, sl[1]] - x[:, sl[0]], x[:, sl[2]] - x[:, sl[1]], x[:, sl[3]] - x[:, sl[2]]
                n1, n2 = np.cross(b1, b2), np.cross(b2, b3)
                with np.errstate(invalid="ignore"):
                    chi.append(np.arctan2(np.sqrt((b2 * b2).sum(-1)) * (b1 * n2).sum(-1), (n1 * n2).sum(-1)))
            assert chi[0].dtype == np.float32
            d = np.abs(chi[0] - chi[1])
            d = np.where(d > np.float32(math.pi), np.float32(2 * math.pi) - d, d) * np.float32(180 / math.pi)
            sym = np.array([R.SYM_CHI.get(int(s)) == k + 1 for s in seq])
            d = np.where(sym, np.minimum(d, np.float32(180) - d), d)
            ok = ref["scored"][:, k]
            worst = max(worst, np.abs(d[ok].astype(np.float64) - ref["delta"][ok, k]).max(initial=0.0))
    assert 0 < worst <= R.EPS_CHI, worst


def test_every_gpu_case_is_well_posed_and_both_forms_agree_on_it():
    cases = R.gpu_cases()                                          # (asserts well_posed protein by protein)
    assert sorted({len(items) for items, _ in cases.values()}) == [1, 3]
    assert {L for _, L in cases.values()} >= set(R.SIZES)
    for name, (items, L_pad) in cases.items():
        for item in items:
            agree(item)
        assert max(len(s) for _, _, s in items) <= L_pad
    with pytest.raises(AssertionError, match="within EPS_CHI"):
        pred, truth, seq = R.pair_case(65, 401)                    # a Delta 4.2e-4 degrees under 40
        R.well_posed(pred, truth, seq)
