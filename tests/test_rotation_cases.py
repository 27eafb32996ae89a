"""tests/rotation_cases.py pinned without a GPU: every case is in exactly one class by the reference's own gap, what the GPU test
compares on the `free` cases is the same for every optimal rotation (in the reference itself), and the new TM chains sit away from
every decision.  The classes, the families and what is invariant under each are described in rotation_cases.py."""
import numpy as np
import pytest

import kabsch_loss_ref as KR
import metric_ref as M
import rotation_cases as C
import tm_ref as T

SPREAD_BAR = 1e-12


def test_every_case_is_in_exactly_one_class():
    cs = C.cases()
    assert set(M.geometry_cases()) < set(cs) and len(cs) == 24 + 12
    for name, c in cs.items():
        assert c["a"].dtype == np.float32 and c["b"].dtype == np.float32 and c["a"].shape == c["b"].shape
        g = c["gap"]
        print(f"{name:28s} {c['cls']:10s} gap {g:.3e}  family {c['kind']}")
        assert (c["cls"] == "unique") == (g >= C.GAP_UNIQUE) and (c["cls"] == "free") == (g == 0.0)
        assert (c["cls"] == "value-only") == (name in C.VALUE_ONLY) == (0.0 < g < C.GAP_UNIQUE), name
        assert (c["kind"] is not None) == (c["cls"] == "free"), name
        if c["cls"] == "free":
            assert C.free_kind(c["a"], c["b"]) == c["kind"], name
    free = {n for n, c in cs.items() if c["cls"] == "free"}
    assert free == {"one-point", "one-point+noise", "mirror-cube", "axis-line", "axis-line-stretched", "axis-line-vs-3d",
                    "3d-vs-axis-line", "axis-mirror-cube-moved", "axis-one-point"}
    for name in ("planar-axis", "planar-rotated", "planar-vs-3d", "mirror", "mirror-cube+noise", "three", "three-exact",
                 "near-line-1e-2", "near-line-1e-2-exact", "near-line-1e-1", "near-line-1e-1-exact"):
        assert cs[name]["cls"] == "unique", name
    # the exact motions really are: the reference loss is rounding
    for name, c in cs.items():
        if c["rigid"]:
            ref = C.loss_reference(name, "dense")
            assert ref["loss"] <= 2.0 ** -21 * max(np.abs(c["a"]).max(), np.abs(c["b"]).max()), (name, ref["loss"])


def free_pairs():
    """(tag, a, b, kind): every free case, and every free (sample, truth) pair of the ensemble cases"""
    out = [(n, c["a"], c["b"], c["kind"]) for n, c in C.cases().items() if c["cls"] == "free"]
    for base in C.ENSEMBLE_BASES:
        kinds, _, _ = C.ensemble_compared(base)
        for k, (s, kind) in enumerate(zip(C.ensemble_samples(base), kinds)):
            if kind in C.FREE_KINDS:
                out.append((f"ensemble/{base}/{k}", s, C.cases()[base]["b"], kind))
    return out


def test_what_is_compared_on_free_cases_is_the_same_for_every_optimal_rotation():
    pairs = free_pairs()
    assert {p[3] for p in pairs} == set(C.FREE_KINDS)
    worst = 0.0
    for tag, a, b, kind in pairs:
        fam = C.free_family(a, b, kind)
        assert len(fam) == 8 and max(np.abs(R - fam[0]).max() for R in fam[1:]) > 0.1, tag      # really other rotations
        n = len(a)
        res = np.array([C.residuals(R, a, b) for R in fam])       # [8, n, 3]
        b64 = np.asarray(b, np.float64)
        rg = np.sqrt(((b64 - b64.mean(0)) ** 2).sum() / n)
        loss = np.sqrt((res ** 2).sum((1, 2)) / n)
        spread = (loss.max() - loss.min()) / rg
        per_atom = np.sqrt((res ** 2).sum(2))                     # what rmsd, the C-alpha rmsf column and TM distances are made of
        spread_atom = (per_atom.max(0) - per_atom.min(0)).max() / rg
        print(f"{tag:36s} {kind:6s} loss {loss[0]:.6f} A  spread of the loss {spread:.1e} rg, of single residuals {spread_atom:.1e} rg")
        assert spread <= SPREAD_BAR, tag
        if "per-atom" in C.FREE_KINDS[kind]:
            assert spread_atom <= SPREAD_BAR, tag
            worst = max(worst, spread_atom)
        else:
            assert spread_atom > 1e-3, tag                         # the cube: single residuals DO depend on the member
        worst = max(worst, spread)
        if loss[0] <= 1e-9 * rg:                                   # an exact motion: the residuals are rounding, nothing to divide by
            continue
        for R, r in zip(fam, res):                                 # the identities the GPU test asserts of the gradient
            g = (r @ R) / (n * np.sqrt((r * r).sum() / n))
            assert np.abs(g.sum(0)).max() <= 1e-12 * np.abs(g).max() and abs((g * g).sum() * n - 1.0) <= 1e-12, tag
    print(f"largest spread of a compared quantity {worst:.1e} (bar {SPREAD_BAR:.0e})")


def test_the_reference_loss_of_a_free_case_is_the_optimum():
    """kabsch_loss_reference on a free case returns the loss of the family, and no member does better"""
    for name, c in C.cases().items():
        if c["cls"] != "free":
            continue
        ref = C.loss_reference(name, "dense")
        for R in C.free_family(c["a"], c["b"], c["kind"]):
            r = C.residuals(R, c["a"], c["b"])
            assert abs(np.sqrt((r * r).sum() / len(r)) - ref["loss"]) <= SPREAD_BAR * ref["rg"], name
        assert np.isfinite(ref["loss"]) and ref["n"] == len(c["a"])


def test_layouts_of_the_loss_cases():
    for n in (3, 8, 12, 40):
        s = C.straddling_slots(n)
        assert len(s) == n and min(s) < 256 and any(256 <= x < 512 for x in s) and 512 <= max(s) < 518     # rounds 0, 1 and 2
    for name in C.cases():
        for layout, L in (("dense", 3), ("straddle", 37)):
            pred, true, seq = C.loss_inputs(name, layout)
            assert len(seq) == L and C.loss_reference(name, layout)["n"] == len(C.cases()[name]["a"])
    oc = C.origin_cases()
    assert len(oc) == 2 * len(C.ORIGIN_FIRST)
    for (L, first), (pred, true, seq) in oc.items():
        present = np.nonzero(KR.present_slots(true, seq))[0]
        want = L * 14 - 1 if first == "last" else first
        assert present[0] == want and (len(present) >= 4 or want >= L * 14 - 3), (L, first, present)
    assert {(int(np.nonzero(KR.present_slots(t, s))[0][0]) // 256) for (_, _), (_, t, s) in oc.items()} >= {0, 1, 2, 4}
    assert {(int(np.nonzero(KR.present_slots(t, s))[0][0]) % 256) // 64 for (_, _), (_, t, s) in oc.items()} == {0, 1, 2, 3}


@pytest.mark.parametrize("name", list(C.TM_CASES))
def test_tm_cases_sit_away_from_every_decision(name):
    pred, true, seq, r = C.tm_case_with_reference(name)
    assert pred.dtype == np.float32 and true.dtype == np.float32
    print(f"{name:16s} N {r['counts'][0]:3d}  margin {r['min_margin']:.2e} A  min_rank {r['min_rank']:.1e}  min_gap {r['min_gap']:.1e}  "
          f"visited {r['visited']}  tm {r['score'][0]:.4f}  counts {r['counts'][1:].tolist()}")
    assert r["min_margin"] >= C.TM_MARGIN, (name, r["min_margin"])
    assert np.isfinite(r["score"]).all() and r["counts"][0] >= 3
    if name in C.TM_RANK1:
        assert r["min_rank"] == 0.0 and r["min_gap"] == 0.0, name      # exactly rank 1 in every superposed subset
    else:
        assert r["min_gap"] > 0.0, name


def test_tm_case_table():
    ns = {name: int(C.tm_case_with_reference(name)[3]["counts"][0]) for name in C.TM_CASES}
    for stem in ("line-line", "line-3d", "zigzag"):
        assert [ns[f"{stem}{n}"] for n in C.TM_NS] == list(C.TM_NS)
    assert ns["three-collinear"] == 3 and len(ns) == 13 and not set(C.TM_CASES) & set(T.GPU_CASES)
    # the noise spreads the distances over the GDT cutoffs: the counts are not all N
    for name in ("line-line65", "line-3d65", "zigzag65"):
        c = C.tm_case_with_reference(name)[3]["counts"]
        assert 0 < c[1] < c[2] < c[3] <= c[5] == c[0], (name, c)


def test_tm_distances_of_a_rank_one_set_do_not_depend_on_the_free_rotation():
    """whole chain and seed fragments of the rank-1 chains: every distance after superposing a subset - what the scores and the
    counts are made of - is the same under every optimal rotation of that subset"""
    worst = 0.0
    for name in C.TM_RANK1:
        pred, true, seq, _ = C.tm_case_with_reference(name)
        p, q = T.ca_pairs(pred, true, seq)
        n = len(p)
        for ell, s in [(n, 0), (min(4, n), 0), (min(4, n), n - min(4, n)), (max(n // 2, 3), n // 4)]:
            sel = slice(s, s + ell)
            d = np.array([T.distances(R, q[sel].mean(0) - R @ p[sel].mean(0), p, q) for R in C.free_family(p[sel], q[sel], "line")])
            spread = (d.max(0) - d.min(0)).max()
            worst = max(worst, spread)
            assert spread <= SPREAD_BAR * max(np.abs(q - q[0]).max(), 1.0), (name, ell, s, spread)
    print(f"largest change of a distance over the free rotations {worst:.1e} A")
