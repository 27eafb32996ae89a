"""The yardstick of tests/test_gpu_tm.py pinned by known answers, without a GPU: tests/tm_ref.py restates the TM-score / GDT
definition of include/ptamd.h in numpy fp64, and no TM-score binary is at hand to compare it with - so it is held to answers
that follow from the definition by hand, and every GPU case is shown to sit where a correct fp64 kernel must make the same
decisions (min_margin >= 1e-9 A, min_rank >= 1e-3)."""
import numpy as np
import pytest

import tm_ref as T


def _chains(ref_in):
    return T.ca_pairs(*ref_in)


def test_an_exact_rigid_motion_scores_one():
    rng = np.random.default_rng(11)
    for n in (3, 4, 12, 50):
        q = T.random_walk(n, rng)
        p = q @ T.rotation(rng).T + np.array([3.0, -7.0, 11.0])
        p64, q64 = np.zeros((n, T.NUM_SLOTS, 3)), np.full((n, T.NUM_SLOTS, 3), np.nan)
        p64[:, T.CA_SLOT], q64[:, T.CA_SLOT] = p, q                    # fp64 inputs: the motion is exact to rounding
        r = T.tm_ref(p64.reshape(-1, 3), q64.reshape(-1, 3), np.zeros(n, np.int64))
        assert np.allclose(r["score"], 1.0, atol=1e-12, rtol=0) and r["counts"].tolist() == [n] * 6, n
        R, t = r["xform"][:, :3], r["xform"][:, 3]
        assert np.abs(p @ R.T + t - q).max() < 1e-9 and np.linalg.det(R) > 0


def test_three_and_four_residues_by_hand():
    # N = 3: one seed (the whole chain), d0 = 0.5, d_search = 4.5.  Truth on a line, the middle residue predicted 2.4 A off it:
    # the least-squares fit of the symmetric triple makes the centroids coincide - the prediction moves 0.8 A towards the line.
    q = np.array([[-4.0, 0, 0], [0.0, 0, 0], [4.0, 0, 0]])
    p = q.copy()
    p[1, 1] = 2.4
    r = T.tm_ref(*T.embed(p, q))
    assert r["counts"][0] == 3 and T.seed_list(3) == [(3, 0)]
    d = np.array([0.8, 1.6, 0.8])
    assert r["score"][0] == pytest.approx(np.mean(1 / (1 + (d / 0.5) ** 2)), abs=1e-6)      # (2.4 is not an fp32 number)
    assert r["counts"].tolist() == [3, 0, 2, 3, 3, 3]
    assert r["score"][1] == pytest.approx((2 + 3 + 3 + 3) / 12) and r["score"][2] == pytest.approx((0 + 2 + 3 + 3) / 12)
    assert r["visited"] == 2 and r["min_margin"] == pytest.approx(0.2, abs=1e-6)     # all three are selected: the refit changes nothing
    # N = 4: one seed again (every length is raised to 4).  A square whose fourth corner is predicted 20 A away: the first fit
    # leaves fewer than 3 residues within d_search - 1 = 3.5 A, the cutoff widens until three are in, and the refit of those
    # three is exact - tm = (3 + 1 / (1 + (20 / 0.5)^2)) / 4.
    q = np.array([[0.0, 0, 0], [4.0, 0, 0], [4.0, 4, 0], [0.0, 4, 0]])
    p = q.copy()
    p[3] = [0.0, 4.0, 20.0]
    r = T.tm_ref(*T.embed(p, q))
    assert T.seed_list(4) == [(4, 0)]
    assert r["score"][0] == pytest.approx((3 + 1 / (1 + (20 / 0.5) ** 2)) / 4, abs=1e-12)
    assert r["counts"].tolist() == [4, 3, 3, 3, 3, 3] and r["score"][1] == pytest.approx(12 / 16)
    # fewer than three present C-alphas, or a non-finite prediction on one
    for bad in (T.embed(p[:2], q[:2]), T.embed(np.where(np.arange(4)[:, None] == 1, np.nan, p), q)):
        r = T.tm_ref(*bad)
        assert np.isnan(r["score"]).all() and r["counts"][1:].tolist() == [0] * 5 and np.isnan(r["xform"]).all()


def test_scales():
    assert T.d0_of(21) == 0.5 and T.d0_of(3) == 0.5
    assert T.d0_of(22) == pytest.approx(1.24 * 7 ** (1 / 3) - 1.8) and 0.57 < T.d0_of(22) < 0.58
    assert T.d0_of(100) == pytest.approx(1.24 * 85 ** (1 / 3) - 1.8) and 3.65 < T.d0_of(100) < 3.66
    assert T.d0_of(16) == 0.5 and T.d0_of(19) == 0.5                   # the floor
    assert T.d_search_of(22) == 4.5 and T.d_search_of(100) == 4.5 and T.d_search_of(400) == pytest.approx(T.d0_of(400))
    assert T.d_search_of(2000) == 8.0


def test_seed_lists():
    def lengths(n):
        return sorted({ell for ell, _ in T.seed_list(n)}, reverse=True)
    want = {3: [3], 7: [7, 4], 8: [8, 4], 9: [9, 4], 64: [64, 32, 16, 8, 4], 65: [65, 32, 16, 8, 4], 130: [130, 65, 32, 16, 8, 4]}
    for n, ells in want.items():
        seeds = T.seed_list(n)
        assert lengths(n) == ells, n
        assert len(seeds) == sum(n - ell + 1 for ell in ells) and len(set(seeds)) == len(seeds)
        assert seeds == sorted(seeds, key=lambda x: (-x[0], x[1])) and seeds[0] == (n, 0)       # (l descending, s ascending)
        assert all(0 <= s and s + ell <= n for ell, s in seeds)
    assert len(T.seed_list(3)) == 1 and len(T.seed_list(7)) == 5 and len(T.seed_list(512)) == 2082


def test_the_hinge_is_found():
    """Two rigid domains, the second turned by 90 degrees: the search finds the superposition of the first domain; the single
    least-squares superposition of all 80 - what `rmsd-full` looks at - does not."""
    p, q = T.hinge_chains()
    r = T.tm_ref(*T.hinge_case())
    d0 = T.d0_of(80)
    assert np.abs(p[:50] - q[:50]).max() == 0.0                        # the first domain is already superposed: (R, t) = (I, 0)
    d_rest = np.sqrt(((p[50:] - q[50:]) ** 2).sum(1))
    floor = (50 + (1 / (1 + (d_rest / d0) ** 2)).sum()) / 80
    R, t, _, _ = T.kabsch(*T.ca_pairs(*T.hinge_case()))
    single = T.tm_of(T.distances(R, t, *T.ca_pairs(*T.hinge_case())), d0)
    print(f"hinge: tm {r['score'][0]:.4f}, first domain superposed {floor:.4f}, one least-squares fit of all 80 {single:.4f}")
    assert r["score"][0] >= floor - 1e-6                               # (fp32 storage of the chains: ~1e-6 A on the first domain)
    assert r["score"][0] > single and floor > single
    assert r["counts"][2] >= 50


def test_a_mirror_image_scores_below_a_noised_copy():
    mirror, control = T.tm_ref(*T.mirror_case()), T.tm_ref(*T.mirror_control_case())
    assert mirror["score"][0] < control["score"][0] and mirror["score"][0] < 0.5 < control["score"][0]
    assert np.linalg.det(mirror["xform"][:, :3]) == pytest.approx(1.0)   # a proper rotation, also there


@pytest.mark.parametrize("name", list(T.GPU_CASES))
def test_gpu_cases_sit_away_from_every_decision(name):
    """The condition under which a correct fp64 kernel must make the reference's decisions: route noise between Jacobi and SVD in
    fp64 at coordinates of order 100 A is of order 1e-13."""
    pred, true, seq, r = T.case_with_reference(name)
    assert pred.dtype == np.float32 and true.dtype == np.float32
    assert r["min_margin"] >= 1e-9 and r["min_rank"] >= 1e-3, (name, r["min_margin"], r["min_rank"])
    assert r["min_gap"] >= 1e-3, (name, r["min_gap"])                  # the proper rotation is unique, the mirror case included
    assert r["counts"][0] >= 3 and np.isfinite(r["score"]).all()


def test_gpu_cases_cover_the_edges():
    n_of = {name: int(T.case_with_reference(name)[3]["counts"][0]) for name in T.GPU_CASES}
    assert {n_of[f"walk{n}"] for n in T.LENGTHS} == {3, 4, 5, 7, 8, 9, 63, 64, 65}
    pred, true, seq, r = T.case_with_reference("walk129_missing")
    assert n_of["walk129_missing"] == 129 and len(seq) == 134          # five true C-alphas are NaN, garbage predicted there
    gone = np.isnan(true.reshape(-1, T.NUM_SLOTS, 3)[:, T.CA_SLOT]).any(1)
    assert gone.sum() == 5 and np.abs(pred.reshape(-1, T.NUM_SLOTS, 3)[gone, T.CA_SLOT]).max() >= 1e30
    # noise of 0.5 - 4 A spreads the distances across all five GDT thresholds
    c = T.case_with_reference("walk65")[3]["counts"]
    assert 0 < c[1] < c[2] < c[3] < c[4] <= c[5] == c[0]
    assert np.nanmax(np.abs(T.case_with_reference("rigid1e3")[1])) > 900
