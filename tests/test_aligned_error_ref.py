"""CPU checks of tests/aligned_error_ref.py, the fp64 restatement of `ptamd_aligned_error` (include/ptamd.h): the two forms agree,
the definition does what it is for - a hinge shows as two blocks where the global fit of `ptamd_ensemble_spread` smears it -, and
the stated fp32 bound `tol` holds for a numpy float32 restatement of the kernel's arithmetic on every case of
tests/test_gpu_aligned_error.py, before anything runs on a device."""
import numpy as np
import pytest

import aligned_error_ref as ar
import ensemble_ref as er


def small_case(rng, n=9, L=11, K=2, B=2):
    seq = np.full((B, L), ar.PAD_ID, np.int64)
    ref = np.zeros((B, L * 14, 3), np.float32)
    samples = np.zeros((B, K, L * 14, 3), np.float32)
    for b in range(B):
        m = n - 2 * b
        seq[b, :m] = rng.integers(0, 20, m)
        ref[b, :m * 14] = ar.random_chain(rng, seq[b, :m])
        for k in range(K):
            R, t = ar.random_rigid(rng)
            samples[b, k] = (ref[b].astype(np.float64) @ R.T + t + rng.normal(0, 1.5, ref[b].shape)).astype(np.float32)
    return ref, samples, seq


def same(a, b, atol=1e-9):
    assert (np.isnan(a) == np.isnan(b)).all()
    ok = ~np.isnan(a)
    assert np.abs(a[ok] - b[ok]).max(initial=0.0) <= atol


def test_loops_and_vectorised_form_agree():
    rng = np.random.default_rng(1)
    ref, samples, seq = small_case(rng)
    ref[0, 2 * 14 + ar.N_SLOT, 0] = np.nan              # residue 2: no frame, still a point
    ref[0, 4 * 14 + ar.CA, 1] = np.nan                  # residue 4: neither
    ref[1, 3 * 14 + ar.C_SLOT] = ref[1, 3 * 14 + ar.CA]   # residue 3 of protein 1: a degenerate frame
    samples[1, 0, 1 * 14 + ar.CA, 2] = np.nan           # sample 0 of protein 1 is unusable
    samples[0, 1, 0 * 14 + 7, 0] = np.nan               # a side-chain atom: nothing
    a, b = ar.reference(ref, samples, seq), ar.reference_loops(ref, samples, seq)
    for x, y in zip(a, b):
        same(np.asarray(x, np.float64), np.asarray(y, np.float64))
    ae, stats, usable = a
    assert list(usable) == [2, 1]
    assert np.isnan(ae[0, 2]).all() and np.isfinite(ae[0, 0, 2])            # a row without its column
    assert np.isnan(ae[0, 4]).all() and np.isnan(ae[0, :, 4]).all()         # a row and its column
    assert np.isnan(ae[1, 3]).all() and np.isfinite(ae[1, 0, 3])
    assert np.isnan(ae[0, 9:]).all() and np.isnan(ae[0, :, 9:]).all()       # padding
    assert np.isfinite(stats).all()
    n0 = 9 - 1
    assert np.isfinite(ae[0]).sum() == (9 - 2) * n0
    assert abs(stats[0, 0] - np.nanmean(ae[0])) < 1e-12
    assert (np.diagonal(ae[0])[np.isfinite(np.diagonal(ae[0]))] == 0.0).all()
    assert np.abs(ae[0] - ae[0].T)[np.isfinite(ae[0] + ae[0].T)].max() > 0.1   # not symmetric


def test_every_sample_spoiled_gives_nan():
    rng = np.random.default_rng(2)
    ref, samples, seq = small_case(rng)
    samples[0, :, 0 * 14 + ar.CA, 0] = 1.0e19           # finite, beyond 1e18
    for f in (ar.reference, ar.reference_loops):
        ae, stats, usable = f(ref, samples, seq)
        assert usable[0] == 0 and np.isnan(ae[0]).all() and np.isnan(stats[0]).all()
        assert usable[1] == 2 and np.isfinite(stats[1]).all()


def test_identical_sample_is_exactly_zero_and_rigid_motion_is_within_tol():
    for L in (3, 65):
        c = ar.make_case(L, 3, "identical")
        ae, stats, usable = c["want"]
        assert (ae[np.isfinite(ae)] == 0.0).all() and (stats[:, 0] == 0.0).all() and (stats[:, 1] == 1.0).all()
        assert list(usable) == [3, 3, 3]
        c = ar.make_case(L, 3, "rigid")
        ae = c["want"][0]
        got = ar.emulate32(c["ref"], c["samples"], c["seq"])
        for b, n in enumerate(c["lens"]):
            # a moved copy ROUNDED TO FP32 is no rigid image: fp64 itself gives up to `moved_copy_slack` for it
            slack = ar.moved_copy_slack(c["ref"][b], n, c["extent"])
            assert np.nanmax(ae[b]) <= slack and np.nanmax(got[b]) <= ar.tol(c["extent"]) + slack


def test_hinge_shows_as_two_blocks_where_the_global_fit_smears_it():
    c = ar.make_case(65, 1, "hinge")
    ae, stats, usable = c["want"]
    x = c["extent"]
    for b, n in enumerate(c["lens"]):
        h, dist = c["hinge"][b]
        a = ae[b, :n, :n]
        assert np.isfinite(a).all()
        lo, hi = np.arange(n) < h, np.arange(n) >= h
        # (the rotated side was rounded to fp32: `moved_copy_slack` bounds what that alone does to the fp64 value)
        slack = ar.moved_copy_slack(c["ref"][b], n, x)
        assert (a[np.ix_(lo, lo)] == 0.0).all() and a[np.ix_(hi, hi)].max(initial=0.0) <= slack
        # across the hinge an entry is how far the POINT moved: its distance from the axis at 60 degrees, whatever the frame
        assert np.abs(a[np.ix_(lo, hi)] - dist[None, :n][:, hi]).max(initial=0.0) <= slack
        assert np.abs(a[np.ix_(hi, lo)] - dist[None, :n][:, lo]).max(initial=0.0) <= slack
    n, (h, dist) = c["lens"][0], c["hinge"][0]
    a = ae[0]
    assert np.abs(a - a.T).max() > 5.0                                      # visibly asymmetric
    # the global fit of ptamd_ensemble_spread moves BOTH sides: no residue shows where the hinge is
    rmsf = er.reference(np.nan_to_num(c["ref"]), np.nan_to_num(c["samples"]), c["seq"])[1][0, :n, 0]
    assert rmsf[:h].min() > 0.05 and rmsf[h:].min() > 0.05
    assert np.median(rmsf[:h]) > 1.0 and np.median(rmsf[h:]) > 1.0


def test_mirror_image_is_far_although_every_distance_is_kept():
    c = ar.make_case(65, 1, "mirror")
    ae, stats, usable = c["want"]
    ca_r = c["ref"].reshape(3, 65, 14, 3)[0, :, ar.CA].astype(np.float64)
    ca_s = c["samples"].reshape(3, 1, 65, 14, 3)[0, 0, :, ar.CA].astype(np.float64)
    d = lambda p: np.linalg.norm(p[:, None] - p[None], axis=-1)            # noqa: E731
    assert np.abs(d(ca_r) - d(ca_s)).max() < 1e-4
    assert stats[0, 0] > 1000 * ar.tol(c["extent"]) and stats[0, 0] > 1.0 and stats[0, 1] < 0.9


def test_stats_follow_the_ptm_formula():
    assert abs(ar.d0_of(19) - (1.24 * 4 ** (1 / 3) - 1.8)) < 1e-12 and ar.d0_of(3) == ar.d0_of(19)
    assert abs(ar.d0_of(100) - (1.24 * 85 ** (1 / 3) - 1.8)) < 1e-12
    ae = np.full((4, 4), np.nan)
    frame, point = np.array([True, True, False, False]), np.array([True, True, True, False])
    ae[0, :3], ae[1, :3] = (0.0, 1.0, 2.0), (0.5, 0.0, 0.1)
    mean, tm = ar.stats_of(ae, frame, point)
    d0 = ar.d0_of(3)
    assert abs(mean - 3.6 / 6) < 1e-12
    assert abs(tm - sum(1 / (1 + (v / d0) ** 2) for v in (0.5, 0.0, 0.1)) / 3) < 1e-12
    # the Lipschitz constant behind tol_tm
    x = np.linspace(0, 5, 200001)
    assert np.abs(np.gradient(1 / (1 + x * x), x)).max() <= 3 * np.sqrt(3) / 8 + 1e-6 < 0.65


@pytest.mark.parametrize("K", ar.KS)
@pytest.mark.parametrize("L", ar.LENGTHS)
def test_float32_arithmetic_stays_inside_tol_on_every_gpu_case(L, K):
    """`tol` comes from the arithmetic (module docstring of aligned_error_ref), not from a device: the float32 restatement of
    that arithmetic is held against fp64 here, on the cases tests/test_gpu_aligned_error.py runs."""
    worst = 0.0
    for kind in ar.KINDS:
        c = ar.make_case(L, K, kind)
        inputs = [(c["ref"], c["samples"], c["seq"], c["want"][0])]
        if kind == "noise" and L >= 3:
            for what in ar.SPOILS:
                r, s, q = ar.spoiled(c, what)
                inputs.append((r, s, q, ar.reference(r, s, q)[0]))
        for r, s, q, want in inputs:
            got = ar.emulate32(r, s, q).astype(np.float64)
            assert (np.isnan(got) == np.isnan(want)).all()
            ok = ~np.isnan(want)
            if ok.any():
                err = float(np.abs(got[ok] - want[ok]).max())
                worst = max(worst, err / ar.tol(c["extent"], K))
                assert err <= ar.tol(c["extent"], K), (kind, err, ar.tol(c["extent"], K))
    print(f"L {L} K {K}: worst |float32 - fp64| / tol {worst:.3f}")
    assert worst < 1.0
