"""CPU checks of tests/ensemble_ref.py, the fp64 restatement of `ptamd_ensemble_spread` (include/ptamd.h): its two forms against
each other and the known answers of the definition.  The GPU tests hold the kernel against the same module."""
import numpy as np
import pytest

import ensemble_ref as er


def make_case(seed, lens, K, sigma=1.0):
    """B proteins of `lens` residues in rows of max(lens): (ref [B, L*14, 3], samples [B, K, L*14, 3], seq [B, L]); a sample is
    the reference under a rigid motion plus Gaussian displacements of `sigma` A."""
    rng = np.random.default_rng(seed)
    B, L = len(lens), max(lens)
    seq = np.full((B, L), er.PAD_ID, np.int64)
    ref = np.zeros((B, L * er.SLOTS, 3), np.float32)
    samples = np.zeros((B, K, L * er.SLOTS, 3), np.float32)
    for b, n in enumerate(lens):
        seq[b, :n] = rng.integers(0, 20, n)
        ref[b] = er.random_chain(rng, seq[b])
        for k in range(K):
            R, t = er.random_rigid(rng)
            samples[b, k] = (ref[b].astype(np.float64) @ R.T + t + rng.normal(0, sigma, ref[b].shape)).astype(np.float32)
    return ref, samples, seq


def same(a, b, tol=1e-12):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool((np.isnan(a) == np.isnan(b)).all()) and bool(np.nanmax(np.abs(a - b), initial=0.0) <= tol)


@pytest.mark.parametrize("lens,K", [([9, 4, 6], 3), ([17], 1), ([2, 12], 4), ([1], 2)])
def test_two_forms_agree(lens, K):
    ref, samples, seq = make_case(3, lens, K)
    samples[0, 0, 5] = np.nan                                         # a side-chain or backbone atom of residue 0
    if len(lens) > 1:
        samples[1, K - 1, 1 * er.SLOTS + er.CA] = np.inf                  # a C-alpha: the sample is unusable
    a, b = er.reference(ref, samples, seq), er.reference_loops(ref, samples, seq)
    for x, y in zip(a, b):
        assert same(x, y), (x, y)
    assert (a[2] == b[2]).all()


def test_rigid_motions_give_zero():
    ref, samples, seq = make_case(5, [23, 11], 4, sigma=0.0)
    rmsd, rmsf, usable = er.reference(ref, samples, seq)
    x = er.extent_of(ref, samples)
    assert (usable == 4).all()
    # (the samples were ROUNDED to fp32 after the motion: what is left is that rounding, u X per coordinate)
    assert np.nanmax(rmsd) < 4 * 2.0 ** -24 * x and np.nanmax(rmsf) < 4 * 2.0 ** -24 * x
    assert np.isnan(rmsf[1, 11:]).all() and not np.isnan(rmsf[0]).any() and not np.isnan(rmsf[1, :11]).any()


def test_mirror_image_is_not_fitted_by_a_reflection():
    rng = np.random.default_rng(11)
    seq = rng.integers(0, 20, (1, 14))
    ref = er.random_chain(rng, seq[0])[None]
    mirrored = (ref * np.array([1.0, 1.0, -1.0], np.float32))[:, None]
    rmsd, rmsf, usable = er.reference(ref, mirrored, seq)
    assert usable[0] == 1 and rmsd[0, 0] > 1.0
    ca = ref[0].reshape(-1, er.SLOTS, 3)[:, er.CA].astype(np.float64)
    brute = er.brute_force_rmsd(ca * np.array([1.0, 1.0, -1.0]), ca, rng)
    assert rmsd[0, 0] <= brute + 1e-9                                  # no proper rotation does better ...
    assert brute - rmsd[0, 0] < 1e-3 * rmsd[0, 0]                        # ... and the search comes down to it
    # a reflection would have fitted it exactly
    improper = np.sqrt((((ca * [1, 1, -1]) * [1, 1, -1] - ca) ** 2).sum(1).mean())
    assert improper == 0.0


def test_one_displaced_residue():
    K, d, at = 5, 2.5, 7
    ref, samples, seq = make_case(7, [20], K, sigma=0.0)
    samples = np.repeat(ref[:, None], K, axis=1).copy()               # identical samples: no rounding of a motion
    samples[0, 2, at * er.SLOTS:(at + 1) * er.SLOTS, 0] += np.float32(d)   # the whole residue, along x, in sample 2
    rmsd, rmsf, usable = er.reference(ref, samples, seq)
    loops = er.reference_loops(ref, samples, seq)
    assert usable[0] == K
    assert rmsf[0, at, 0] ** 2 == pytest.approx(loops[1][0, at, 0] ** 2, abs=1e-12)    # the exact value, from the loop form
    # the fit answers the displacement of 1 C-alpha in 20 by moving the others 1/20 of the way (and turning a little)
    assert 0.85 * d * d / K < rmsf[0, at, 0] ** 2 < d * d / K
    assert 0.85 * d * d / K < rmsf[0, at, 1] ** 2 < d * d / K
    others = np.delete(rmsf[0, :, 0], at)
    assert 0 < others.max() < 0.2 * d / np.sqrt(K)
    assert rmsd[0, 2] > 0 and np.abs(np.delete(rmsd[0], 2)).max() < 1e-12      # (the SVD's rotation of an identical copy)


def test_nan_calpha_makes_the_sample_unusable_and_changes_nothing_else():
    ref, samples, seq = make_case(9, [15, 8], 4)
    base = er.reference(ref, samples, seq)
    broken = samples.copy()
    broken[0, 1, 3 * er.SLOTS + er.CA, 2] = np.nan
    rmsd, rmsf, usable = er.reference(ref, broken, seq)
    assert list(usable) == [3, 4] and np.isnan(rmsd[0, 1])
    keep = [0, 2, 3]
    assert same(rmsd[0, keep], base[0][0, keep]) and same(rmsd[1], base[0][1]) and same(rmsf[1], base[1][1])
    alone = er.reference(ref[:1], samples[:1, keep], seq[:1])          # the spread of the three that are left
    assert same(rmsf[0], alone[1][0])
    # a NaN in the reference's C-alpha: no sample of that protein is usable
    ref2 = ref.copy()
    ref2[1, 2 * er.SLOTS + er.CA, 0] = np.nan
    rmsd, rmsf, usable = er.reference(ref2, samples, seq)
    assert list(usable) == [4, 0] and np.isnan(rmsd[1]).all() and np.isnan(rmsf[1]).all()


def test_side_chain_nan_is_left_out_of_its_own_term():
    ref, samples, seq = make_case(13, [10], 3)
    seq[0, 4] = er.AA.index("W")                                      # ten side-chain atoms
    ref[0] = er.random_chain(np.random.default_rng(1), seq[0])
    base = er.reference(ref, samples, seq)
    broken = samples.copy()
    broken[0, 0, 4 * er.SLOTS + 9] = np.nan
    rmsd, rmsf, usable = er.reference(ref, broken, seq)
    assert usable[0] == 3 and same(rmsd, base[0]) and same(rmsf[:, :, 0], base[1][:, :, 0])
    assert same(np.delete(rmsf[0, :, 1], 4), np.delete(base[1][0, :, 1], 4))
    assert np.isfinite(rmsf[0, 4, 1]) and rmsf[0, 4, 1] != base[1][0, 4, 1]
    assert same(rmsf, er.reference_loops(ref, broken, seq)[1])
    # what a slot the type does not have holds is never looked at (GLY: slots 4..13)
    seq[0, 2] = er.AA.index("G")
    a = er.reference(ref, samples, seq)
    junk = samples.copy()
    junk[0, :, 2 * er.SLOTS + 4:3 * er.SLOTS] = np.nan
    assert all(same(x, y) for x, y in zip(a, er.reference(ref, junk, seq)))


def test_fewer_than_three_residues_is_all_nan():
    ref, samples, seq = make_case(17, [2, 5], 3)
    seq[1, 1] = 21                                                    # an unknown id is absent too
    rmsd, rmsf, usable = er.reference(ref, samples, seq)
    assert list(usable) == [0, 3] and np.isnan(rmsd[0]).all() and np.isnan(rmsf[0]).all()
    assert np.isnan(rmsf[1, 1]).all() and np.isfinite(rmsf[1, [0, 2, 3, 4]]).all()
    seq[1, 2:4] = er.PAD_ID                                           # two present residues left
    rmsd, rmsf, usable = er.reference(ref, samples, seq)
    assert list(usable) == [0, 0] and np.isnan(rmsd).all() and np.isnan(rmsf).all()


def test_bound_is_what_the_module_states():
    assert er.EPS32 == np.finfo(np.float32).eps
    assert er.tol(0.0, 100.0) == pytest.approx(32 * 1.1920929e-07 * 100.0)
    assert er.tol_sq(0.0, 100.0) == pytest.approx(er.tol(0.0, 100.0) ** 2)
    assert er.tol_sq(2.0, 100.0) == pytest.approx(er.tol(2.0, 100.0) * (4.0 + er.tol(2.0, 100.0)))
    # fp32 arithmetic on the definition stays inside it: apply an fp32 (R, t) in fp32, sum squares in fp32
    ref, samples, seq = make_case(19, [40], 2, sigma=1.5)
    want = er.reference(ref, samples, seq)
    x = er.extent_of(ref, samples)
    pres = er.present_of(seq[0])
    r = ref[0].reshape(-1, er.SLOTS, 3)
    for k in range(2):
        s = samples[0, k].reshape(-1, er.SLOTS, 3)
        R, t = er.kabsch(s[pres, er.CA].astype(np.float64), r[pres, er.CA].astype(np.float64))
        R, t = R.astype(np.float32), t.astype(np.float32)
        e = (s[:, er.CA] @ R.T + t - r[:, er.CA]).astype(np.float32)
        got = np.sqrt(np.float32((e * e).sum(1, dtype=np.float32).mean(dtype=np.float32)))
        assert abs(float(got) ** 2 - want[0][0, k] ** 2) <= er.tol_sq(want[0][0, k], x)
