"""The fp64 reference of the steric clash term (tests/clash_ref.py) against values worked out by hand and against the chain
geometry, without a GPU."""
import numpy as np
import pytest
import torch

import clash_ref as R

SLOTS = R.SLOTS


def far_apart(seq):
    """Every slot on a 10 A grid (residue along x, slot along y): nothing is near anything."""
    L = len(seq)
    crd = np.zeros((L * SLOTS, 3), np.float32)
    crd[:, 0] = 10.0 * np.repeat(np.arange(L), SLOTS) + 5.0
    crd[:, 1] = 10.0 * np.tile(np.arange(SLOTS), L)
    return crd


def test_radii_and_atoms_from_the_atom_names():
    tab = R.radius_table()
    assert tab.shape == (20, 14)
    assert (~np.isnan(tab)).sum(1).tolist() == [5, 6, 8, 9, 11, 4, 10, 8, 9, 8, 8, 8, 7, 9, 11, 6, 7, 7, 14, 12]
    assert tab[:, :4].tolist() == [[1.55, 1.7, 1.7, 1.52]] * 20                    # N, CA, C, O
    assert tab[R.CYS, 5] == 1.8 and tab[R.AA.index("M"), 6] == 1.8                 # SG, SD
    assert tab[R.AA.index("S"), 5] == 1.52 and tab[R.AA.index("K"), 8] == 1.55     # OG, NZ
    assert set(np.unique(tab[~np.isnan(tab)])) == {1.52, 1.55, 1.7, 1.8}
    idx, rad, res, ls, sg = R.atoms_of([5, 20, 1, 21, -1])                         # GLY, pad, CYS, unknown, negative
    assert idx.tolist() == [0, 1, 2, 3] + [28 + s for s in range(6)] and sg.tolist() == [False] * 9 + [True]


@pytest.mark.parametrize("d", [0.5, 1.0, 1.6, 1.89, 1.91, 3.0])
def test_two_atoms_by_hand(d):
    """CA of residue 0 and CA of residue 1 (both C: 1.7 + 1.7 - 1.5 = 1.9) at distance d along x, two GLY: 8 atoms."""
    seq = np.array([5, 5])
    crd = far_apart(seq)
    crd[1] = (0, 50, 7)
    crd[SLOTS + 1] = (d, 50, 7)
    loss, nclash, n, grad, margin = R.clash_reference(crd, seq)
    v = max(0.0, 1.9 - d)
    assert n == 8 and nclash == (1 if v > 0 else 0)
    assert loss == pytest.approx(v / 8, abs=1e-7)                                   # (d is an fp32 number)
    want = np.zeros_like(grad)
    if v > 0:
        want[1, 0], want[SLOTS + 1, 0] = 1 / 8, -1 / 8                              # pushed apart by descent
    assert np.abs(grad - want).max() < 1e-12
    assert margin == pytest.approx(abs(1.9 - d), abs=1e-6)
    # another tolerance moves the kink
    assert R.clash_reference(crd, seq, tau=0.0)[0] == pytest.approx((3.4 - d) / 8, abs=1e-6)


def test_elements_set_the_threshold():
    seq = np.array([R.CYS, R.AA.index("S")])                                        # SG (1.8) against OG (1.52): 1.82
    crd = far_apart(seq)
    crd[5], crd[SLOTS + 5] = (0, 0, 90), (0, 1.0, 90)
    loss, nclash, n, grad, _ = R.clash_reference(crd, seq)
    assert n == 12 and nclash == 1 and loss == pytest.approx(0.82 / 12, abs=1e-7)
    assert grad[5, 1] == pytest.approx(1 / 12) and grad[SLOTS + 5, 1] == pytest.approx(-1 / 12)


def test_special_cases():
    assert np.isnan(R.clash_reference(np.zeros((28, 3)), [20, 20])[0])              # no atom
    assert R.clash_reference(np.zeros((28, 3)), [20, 20])[1:3] == (0, 0)
    seq = np.array([5, 5])
    crd = far_apart(seq)
    assert R.clash_reference(crd, seq)[:3] == (0.0, 0, 8)                           # atoms, no violation: 0, not NaN
    for poison in (np.nan, np.inf, 2e18):
        bad = crd.copy().astype(np.float64)
        bad[2, 1] = poison
        loss, nclash, n, grad, _ = R.clash_reference(bad, seq)
        assert np.isnan(loss) and nclash == 0 and n == 8 and not grad.any()
    crd[4:SLOTS] = np.nan                                                           # slots GLY does not have: never read
    assert R.clash_reference(crd, seq)[:3] == (0.0, 0, 8)
    same = far_apart(seq)
    same[1], same[SLOTS + 1] = (1, 2, 3), (1, 2, 3)                                 # coinciding atoms: finite, zero gradient
    loss, nclash, _, grad, _ = R.clash_reference(same, seq)
    assert loss == pytest.approx(1.9 / 8) and nclash == 1 and not grad.any()


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_the_peptide_exclusion_is_worth_one_pair_per_bond(seed):
    """A chain built by the oracle, without CYS: every C(i)-N(i+1) bond has the one length the NeRF build gives it, below 1.4 A,
    against a threshold of 1.7 + 1.55 - 1.5 = 1.75 A, so switching the exclusion off raises nclash by exactly L - 1, and the loss
    by their overlap."""
    from oracle import geometry
    from protein_transformer_amd import synthetic
    rng = np.random.default_rng(seed)
    L = 40
    seq = rng.choice([r for r in range(20) if r != R.CYS], L)
    crd = geometry.generate_coords(torch.from_numpy(synthetic.sample_angles(rng, L)), torch.from_numpy(seq)).numpy()
    on = R.clash_reference(crd, seq)
    off = R.clash_reference(crd, seq, peptide_exclusion=False)
    bond = np.linalg.norm(crd[np.arange(L - 1) * SLOTS + 2].astype(np.float64) - crd[np.arange(1, L) * SLOTS], axis=1)
    assert np.abs(bond - bond[0]).max() < 1e-4 and 1.3 < bond[0] < 1.4
    assert off[1] - on[1] == L - 1 and off[2] == on[2]
    assert off[0] - on[0] == pytest.approx((1.75 - bond).sum() / on[2], abs=1e-9)
    assert R.clash_reference(crd, seq, disulfide_exclusion=False)[:2] == on[:2]     # no CYS: nothing to exclude
    assert on[4] >= R.MARGIN


def test_the_disulfide_exclusion():
    seq = np.array([R.CYS, 0, R.CYS])
    crd = far_apart(seq)
    crd[5], crd[2 * SLOTS + 5] = (0, 0, 90), (2.0, 0, 90)                           # SG-SG at 2.0 A: 1.8 + 1.8 - 1.5 = 2.1
    assert R.clash_reference(crd, seq)[:2] == (0.0, 0)
    loss, nclash = R.clash_reference(crd, seq, disulfide_exclusion=False)[:2]
    assert nclash == 1 and loss == pytest.approx(0.1 / 17, abs=1e-7)
    crd[SLOTS + 4] = (0, 1.5, 90)                                                   # CB of ALA 1.5 A from the first SG: counted
    loss, nclash = R.clash_reference(crd, seq)[:2]
    assert nclash == 1 and loss == pytest.approx(0.5 / 17, abs=1e-7)


def test_the_margin_is_enforced():
    seq = np.array([5, 5])
    crd = far_apart(seq).astype(np.float64)
    crd[1], crd[SLOTS + 1] = (0, 0, 90), (1.9 - 2e-5, 0, 90)
    with pytest.raises(AssertionError, match="from the kink"):
        R.clash_reference(crd, seq)
    assert R.clash_reference(crd, seq, check_margin=False)[1] == 1


def test_sequences_of_a_given_atom_count():
    rng = np.random.default_rng(0)
    for n in (63, 64, 65, 129):
        assert len(R.atoms_of(R.sequence_with_atoms(n, rng))[0]) == n
