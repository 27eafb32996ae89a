"""The cases of tests/atom_tiles_cases.py are what they claim to be, and the per-atom bar of
tests/test_gpu_atom_tiles_edges.py rejects a wrong gradient: no GPU needed.

Per case: the atom counts and what they mean in tiles, the conditions on the inputs (cutoff, delta, clash margin), the facts
the case was built for (box gaps of the two-tile cases, the near masks of the hairpin, the shares of the compaction), how many
proteins have a pair, that the pair table sums to the imported fp64 reference (asserted inside `reference`), and that each of
four mutations of the fp64 gradient exceeds the bar K scale_i + floor_i at some atom by a factor of at least ten."""
import numpy as np
import pytest

import atom_tiles_cases as atc


@pytest.mark.parametrize("name", list(atc.BUILDERS))
def test_the_case_is_what_it_claims(name):
    c = atc.case(name)
    c.check()
    assert set(k for n, k in atc.RUNS if n == name) == set(c.kernels)
    for kernel in c.kernels:
        refs = atc.reference(c, kernel)
        have = [r["npairs"] > 0 or (kernel == "clash" and r["atoms"] > 0) for r in refs]
        assert sum(have) == c.with_pairs and len(have) - sum(have) == c.B - c.with_pairs


@pytest.mark.parametrize("name,kernel", [r for r in atc.RUNS if r[1] != "lddt"])
def test_the_bar_rejects_every_mutation_tenfold(name, kernel):
    c = atc.case(name)
    for b, ref in enumerate(atc.reference(c, kernel)):
        if ref["npairs"] == 0:
            continue
        assert atc.excess(ref["grad"], ref, kernel) == 0.0 and atc.worst_ratio(ref["grad"], ref) == 0.0
        for what, grad in atc.mutations(c, b, ref).items():
            x = atc.excess(grad, ref, kernel)
            print(f"{name}[{b}] {kernel}: {what}: {x:.3g} x the bar")
            assert x >= 10.0, (what, b)


def test_the_stale_batch_has_the_layout_of_the_case():
    c = atc.case("counts")
    pred, true, seq = c.stale_batch(np.random.default_rng(0))
    assert pred.shape == c.pred.shape and seq.shape == c.seq.shape
    counts = [int((~np.isnan(true[b]).any(1) & np.repeat(seq[b] != atc.PAD, atc.SLOTS)).sum()) for b in range(c.B)]
    want = list(c.atoms)[::-1]
    want[want.index(max(c.atoms))] = c.L * atc.SLOTS                  # the longest row fills every slot
    assert counts == want
