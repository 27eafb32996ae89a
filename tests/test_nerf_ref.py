"""Pins tests/nerf_ref.py, the fp64 helpers that tests/test_gpu_nerf_edges.py holds csrc/geometry.hip against.  CPU only.

  * `internal_coordinates` on the fp64 oracle's coordinates gives back the bond lengths, bond angles and torsions the build was
    asked for to better than 1e-10 (torsions on the circle; a negative bond angle shows as |theta| and chi + pi), for every
    placement of a ragged batch that holds every residue type at residue 0, at residue 1 and as the last residue;
  * it notices a build that differs from `SC_PROGRAM` in ONE place: a swapped parent slot, a bond or an angle moved by 1e-3 -
    at exactly the atoms of that residue type that the change reaches, and nowhere else;
  * `expected_support` (autograd of the fp64 oracle, entries with a non-zero derivative) against a rule written by hand, for
    every atom of a protein that holds every residue type, and against the literal sets of four named atoms.
"""
import copy
import math

import numpy as np
import pytest
import torch

import nerf_ref
from oracle import batched
from oracle.geometry import SC_PROGRAM
from protein_transformer_amd import synthetic

TIGHT = 1e-10
LENS = [2, 3, 23, 40]


@pytest.fixture(scope="module")
def built():
    """a ragged batch, every residue type at residue 0, 1 and len - 1 of some protein, and its fp64 coordinates"""
    lens = LENS + [24] * 20
    batch = synthetic.make_batch(lens, L_pad=40, seed=3)
    seq, ang = batch["seq"], batch["start_ang_rad"]
    for b in range(len(LENS), len(lens)):
        seq[b, 0], seq[b, 1], seq[b, lens[b] - 1] = b % 20, (b + 7) % 20, (b + 13) % 20
    ang[5, 3, 4] = -ang[5, 3, 4]                      # negative bond angles: N of residue 4, and C of residue 6
    ang[5, 6, 3] = -ang[5, 6, 3]
    crd = batched.generate_coords_batched(ang.double(), seq, torch.float64)
    return lens, seq.numpy(), ang.numpy(), crd.numpy()


def test_recovers_the_inputs_from_the_fp64_build(built):
    lens, seq, ang, crd = built
    for pos in (0, 1, -1):
        assert {int(seq[b, pos if pos >= 0 else n - 1]) for b, n in enumerate(lens) if n == 24} == set(range(20))
    worst = np.zeros(3)
    count = 0
    for b, n in enumerate(lens):
        ic = nerf_ref.internal_coordinates(crd[b], seq[b], ang[b])
        owned = sum(4 + len(SC_PROGRAM[int(r)]) for r in seq[b, :n])
        assert len(ic["atom"]) == owned - 3 and len(set(ic["atom"].tolist())) == owned - 3    # every placed atom, once
        assert np.all(ic["exp_angle"] >= 0)
        worst = np.maximum(worst, [e.max() for e in nerf_ref.internal_errors(ic)])
        count += len(ic["atom"])
    print(f"{count} placements, worst |recovered - asked for|: bond {worst[0]:.1e} A, angle {worst[1]:.1e}, torsion {worst[2]:.1e}")
    assert np.all(worst < TIGHT), worst


def test_fp32_build_is_at_the_storage_floor(built):
    """what the GPU test measures against: the fp32 oracle's internal coordinates, and the fp64 coordinates rounded to fp32"""
    lens, seq, ang, crd = built
    crd32 = batched.generate_coords_batched(torch.from_numpy(ang), torch.from_numpy(seq), torch.float32).numpy()
    for b in (3, 10):
        e32 = [e.max() for e in nerf_ref.internal_errors(nerf_ref.internal_coordinates(crd32[b], seq[b], ang[b]))]
        est = [e.max() for e in nerf_ref.internal_errors(
            nerf_ref.internal_coordinates(crd[b].astype(np.float32), seq[b], ang[b]))]
        assert max(e32) < 1e-4 and max(est) < 1e-4 and min(est) > 0, (e32, est)


def mutated(change):
    prog = copy.deepcopy(SC_PROGRAM)
    change(prog)
    return prog


def swap_parents(prog):              # TRP atom 5 (slot 9): (6, 7, 8) -> (7, 6, 8)
    b, a, t, _ = prog[18][5]
    prog[18][5] = (b, a, t, (7, 6, 8))


def move_bond(prog):                 # MET atom 2 (slot 6): 1.81 -> 1.811
    b, a, t, p = prog[10][2]
    prog[10][2] = (b + 1e-3, a, t, p)


def move_angle(prog):                # HIS atom 3 (slot 7): + 1e-3 rad
    b, a, t, p = prog[6][3]
    prog[6][3] = (b, a + 1e-3, t, p)


@pytest.mark.parametrize("change, rtype, slot, which, least", [
    (swap_parents, 18, 9, 2, 1e-2), (move_bond, 10, 6, 0, 0.99e-3), (move_angle, 6, 7, 1, 0.99e-3)])
def test_one_changed_table_entry_is_detected(built, monkeypatch, change, rtype, slot, which, least):
    """coordinates built with a table that is wrong in one place, read with the right table: the changed atom of every residue
    of that type stands out by the size of the change, every other residue type still reads back its inputs"""
    lens, seq, ang, _ = built
    monkeypatch.setattr(batched, "SC_PROGRAM", mutated(change))
    crd = batched.generate_coords_batched(torch.from_numpy(ang).double(), torch.from_numpy(seq), torch.float64).numpy()
    monkeypatch.undo()
    seen = 0
    for b in range(len(lens)):
        ic = nerf_ref.internal_coordinates(crd[b], seq[b], ang[b])
        err = nerf_ref.internal_errors(ic)
        hit = (seq[b][ic["res"]] == rtype) & (ic["slot"] == slot)
        seen += int(hit.sum())
        assert np.all(err[which][hit] > least), (b, err[which][hit])
        other = seq[b][ic["res"]] != rtype
        assert all(e[other].max() < TIGHT for e in err)
    assert seen >= 3


def test_the_helper_with_a_wrong_table_disagrees_with_the_right_build(built):
    """the other way round: the right coordinates read through a table with a swapped parent slot or a moved constant"""
    lens, seq, ang, crd = built
    for change, which, least in ((swap_parents, 2, 1e-2), (move_bond, 0, 0.99e-3), (move_angle, 1, 0.99e-3)):
        prog = mutated(change)
        worst = max(nerf_ref.internal_errors(nerf_ref.internal_coordinates(crd[b], seq[b], ang[b], prog))[which].max()
                    for b in range(len(lens)))
        assert worst > least, (change.__name__, worst)


# ----------------------------------------------------------------------------------------------- expected_support
def chain_rule(j):
    """angle entries of the backbone placements 3 .. j (chain atom j = 3 i + slot)"""
    out = set()
    for k in range(3, j + 1):
        i, a = divmod(k, 3)
        out |= {(i - 1, 4), (i - 1, 1)} if a == 0 else {(i - 1, 5), (i - 1, 2)} if a == 1 else {(i, 3), (i, 0)}
    return out


def rule_support(seq, i, slot):
    """written by hand from StructureBuilder.py: the chain up to the atom (or up to what it hangs off), psi for O, and the
    predicted torsions of the side-chain atom itself and of the side-chain atoms it is built from"""
    if slot < 3:
        return chain_rule(3 * i + slot)
    if slot == 3:
        return chain_rule(3 * i + 2) | {(i, 1)}
    prog = SC_PROGRAM[int(seq[i])]

    def chis(k):
        _, _, tors, parents = prog[k]
        own = {(i, 6 + min(k, 5))} if tors == "p" else chis_of_torsion(k - 1) if tors == "i" else set()
        for p in (parents or ()):
            if p >= 4:
                own |= chis(p - 4)
        return own

    def chis_of_torsion(k):
        tors = prog[k][2]
        return {(i, 6 + min(k, 5))} if tors == "p" else chis_of_torsion(k - 1) if tors == "i" else set()

    base = chain_rule(3) if i == 0 else chain_rule(3 * i + 1)          # CB hangs off N_1 (residue 0) or C_{i-1}, N_i, CA_i
    return base | chis(slot - 4)


def test_expected_support_against_the_rule():
    n, L = 24, 26
    seq = np.full(L, 20, np.int64)
    seq[:n] = [18, 14] + list(range(20)) + [19, 4]
    probes = [(i, s) for i in range(n) for s in range(4 + len(SC_PROGRAM[int(seq[i])]))]
    got = nerf_ref.support_sets(seq, n, probes)
    for (i, s), g in zip(probes, got):
        assert g == rule_support(seq, i, s), (i, s, sorted(g ^ rule_support(seq, i, s)))
    by = dict(zip(probes, got))
    assert by[(0, 0)] == by[(0, 1)] == by[(0, 2)] == set()                       # constants of the build
    assert by[(0, 4)] == {(0, 4), (0, 1), (0, 6)}                                # CB of residue 0 hangs off N_1
    assert by[(0, 3)] == {(0, 1)}                                                # O_0: psi alone
    ca = nerf_ref.expected_support(seq, n, 7, 1)                                 # CA_7: nothing of residue 7
    assert ca == by[(7, 1)] and not any(r >= 7 for r, _ in ca) and (6, 2) in ca and (6, 5) in ca and (0, 0) not in ca
    o = by[(7, 3)]                                                               # O_7: C_7's chain and psi_7
    assert o == by[(7, 2)] | {(7, 1)} and (7, 1) not in by[(7, 2)] and (7, 0) in o and (7, 3) in o
    w = by[(20, 13)]                                                             # last atom of the TRP at residue 20
    assert int(seq[20]) == 18 and w == by[(20, 1)] | {(20, 6), (20, 7), (20, 8)}
    assert int(seq[16]) == 14 and by[(16, 10)] == by[(16, 1)] | {(16, c) for c in range(6, 12)}          # ARG: the planar partner of chi 6
    last = by[(n - 1, 2)]
    assert not any((n - 1, c) in last for c in (1, 2, 4, 5)) and (n - 1, 0) in last and (n - 1, 3) in last


def test_jacobian_rows_are_the_rows_of_the_dense_gradient():
    """replicas with one-hot upstream gradients give the rows whose sum is the gradient of the dense upstream gradient"""
    batch = synthetic.make_batch([9], L_pad=11, seed=1)
    seq, ang = batch["seq"][0], batch["start_ang_rad"][0]
    probes = [(i, s) for i in range(9) for s in range(4 + len(SC_PROGRAM[int(seq[i])]))]
    w = torch.from_numpy(np.random.default_rng(0).normal(size=(len(probes), 3)))
    rows, crd = nerf_ref.jacobian_rows(ang, seq, probes, w)
    a = ang.double()[None].clone().requires_grad_()
    full = batched.generate_coords_batched(a, seq[None], torch.float64)[0]
    dense = torch.zeros_like(full)
    dense[[i * 14 + s for i, s in probes]] = w
    (full * dense).sum().backward()
    assert torch.equal(crd, full.detach())
    assert (rows.sum(0) - a.grad[0]).abs().max() < 1e-12 * a.grad.abs().max()
    assert math.isfinite(float(rows.abs().max()))
