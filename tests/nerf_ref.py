"""fp64 CPU helpers for the NeRF build (csrc/geometry.hip), for tests/test_nerf_ref.py and tests/test_gpu_nerf_edges.py.
TEST INFRASTRUCTURE ONLY: the product never imports it.

Two things that a comparison of coordinates with the oracle's coordinates cannot give:

  * `internal_coordinates`: every placement d = nerf(a, b, c; l, theta, chi) read BACK from a set of coordinates - the bond length
    |d - c|, the bond angle (b, c, d) and the dihedral (a, b, c, d) - next to the values the build was asked for.  The error of a
    placement does not travel down the chain: an atom 100 A from the origin is judged by its own three parents.  The parents come
    from the backbone rules and from `oracle.geometry.SC_PROGRAM`, written from the definition (Structure.py:44-59), numpy fp64.
  * `jacobian_rows` / `support_sets` / `expected_support`: one atom's derivative with respect to every angle, and the set of
    angle entries it depends on at all, from autograd of `oracle.batched.generate_coords_batched` on a batch of replicas of one
    protein (replica p carries the upstream gradient of probe p alone, so one backward pass gives every row).

Layout as everywhere: residue i owns atom slots 14 i .. 14 i + 13 (0 N, 1 CA, 2 C, 3 O, 4.. side chain), angle columns
0 phi, 1 psi, 2 omega, 3 N-CA-C, 4 CA-C-N, 5 C-N-CA, 6.. chi.
"""
import math

import numpy as np
import torch

from oracle import batched
from oracle.geometry import BA_CA_C_O, BL_C_N, BL_C_O, BL_CA_C, BL_N_CA, PAD_ID, SC_ANGLE0, SC_PROGRAM

SLOTS, ANGLES = 14, 12
BACKBONE, OXYGEN, SIDECHAIN = 0, 1, 2                 # `kind` of a placement


def protein_len(seq):
    """`len` of a protein: the count of its non-pad ids (its residues are the first `len`)."""
    return int((np.asarray(seq) != PAD_ID).sum())


def circ(d):
    """a difference of two angles, on the circle: in [-pi, pi)"""
    return (np.asarray(d, np.float64) + math.pi) % (2 * math.pi) - math.pi


def placements(seq, program=SC_PROGRAM):
    """Every placed atom of one protein, in build order per residue: a list of
        (kind, residue, slot, (a, b, c) as flat atom indices 14 i + slot, bond, angle, torsion)
    where angle and torsion are either a float (a constant of the build) or a tuple (residue, column, offset) meaning
    ang[residue, column] + offset.  N, CA, C of residue 0 are constants of the build, not placements, and are not listed."""
    seq = np.asarray(seq)
    n = protein_len(seq)
    at = lambda i, s: i * SLOTS + s                                             # noqa: E731
    out = []
    for i in range(n):
        if i >= 1:                                                              # build_bb, StructureBuilder.py:147-179
            out.append((BACKBONE, i, 0, (at(i - 1, 0), at(i - 1, 1), at(i - 1, 2)), BL_C_N, (i - 1, 4, 0.0), (i - 1, 1, 0.0)))
            out.append((BACKBONE, i, 1, (at(i - 1, 1), at(i - 1, 2), at(i, 0)), BL_N_CA, (i - 1, 5, 0.0), (i - 1, 2, 0.0)))
            out.append((BACKBONE, i, 2, (at(i - 1, 2), at(i, 0), at(i, 1)), BL_CA_C, (i, 3, 0.0), (i, 0, 0.0)))
        out.append((OXYGEN, i, 3, (at(i, 0), at(i, 1), at(i, 2)), BL_C_O, BA_CA_C_O, (i, 1, -math.pi)))
        last = None
        for k, (bond, angle, tors, parents) in enumerate(program[int(seq[i])]):  # build_sc, StructureBuilder.py:193-231
            if k == 0:
                abc = (at(1, 0), at(0, 2), at(0, 1)) if i == 0 else (at(i - 1, 2), at(i, 0), at(i, 1))
            else:
                abc = tuple(at(i, p) for p in parents)
            if tors == "p":
                t = (i, SC_ANGLE0 + min(k, 5), 0.0)
            elif tors == "i":
                t = (last[0], last[1], last[2] - math.pi) if isinstance(last, tuple) else last - math.pi
            else:
                t = float(tors)
            out.append((SIDECHAIN, i, 4 + k, abc, float(bond), float(angle), t))
            last = t
    return out


def recover(a, b, c, d):
    """(bond, angle, torsion) of d over (a, b, c), [n, 3] fp64 each: the inverse of Structure.py:44-65 in the frame of the
    definition, x = unit(c - b), z = unit(unit(b - a) x x), y = z x x, d - c = l (-cos th, sin th cos chi, sin th sin chi);
    theta in [0, pi] (a negative theta of the build shows as |theta| and chi + pi)."""
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)              # noqa: E731
    x = unit(c - b)
    z = unit(np.cross(unit(b - a), x))
    y = np.cross(z, x)
    v = d - c
    vx, vy, vz = (v * x).sum(-1), (v * y).sum(-1), (v * z).sum(-1)
    return np.linalg.norm(v, axis=-1), np.arctan2(np.hypot(vy, vz), -vx), np.arctan2(vz, vy)


def internal_coordinates(crd, seq, ang=None, program=SC_PROGRAM):
    """crd [len*14 or more, 3], seq [L] of ONE protein -> dict of arrays over its placements (see `placements`):
        kind, res, slot, atom (flat index of d), bond, angle, torsion          recovered from crd, fp64
        exp_bond, exp_angle, exp_torsion                                         what the build was asked for (needs ang [L, 12])
    Compare torsions with `circ`."""
    crd = np.asarray(crd, np.float64).reshape(-1, 3)
    pl = placements(seq, program)
    kind = np.array([p[0] for p in pl], np.int64)
    res = np.array([p[1] for p in pl], np.int64)
    slot = np.array([p[2] for p in pl], np.int64)
    abc = np.array([p[3] for p in pl], np.int64).reshape(-1, 3)
    atom = res * SLOTS + slot
    bond, angle, torsion = recover(crd[abc[:, 0]], crd[abc[:, 1]], crd[abc[:, 2]], crd[atom])
    out = dict(kind=kind, res=res, slot=slot, atom=atom, bond=bond, angle=angle, torsion=torsion)
    if ang is not None:
        ang = np.asarray(ang, np.float64)
        val = lambda s: s if isinstance(s, float) else ang[s[0], s[1]] + s[2]   # noqa: E731
        th = np.array([val(p[5]) for p in pl], np.float64)
        chi = np.array([val(p[6]) for p in pl], np.float64)
        out["exp_bond"] = np.array([p[4] for p in pl], np.float64)
        out["exp_angle"] = np.abs(th)
        out["exp_torsion"] = np.where(th < 0, chi + math.pi, chi)
    return out


def internal_errors(ic):
    """|recovered - expected| per placement: (bond, angle, torsion on the circle)"""
    return (np.abs(ic["bond"] - ic["exp_bond"]), np.abs(ic["angle"] - ic["exp_angle"]),
            np.abs(circ(ic["torsion"] - ic["exp_torsion"])))


# ----------------------------------------------------------------------------------------------- one atom at a time
def jacobian_rows(ang, seq, probes, w, dtype=torch.float64):
    """ang [L, 12], seq [L] of one protein, probes [(residue, slot)] * P, w [P, 3] ->
    (d (w_p . x_probe_p) / d ang  [P, L, 12], coordinates [L*14, 3]) by autograd of the oracle in `dtype`."""
    ang, seq = torch.as_tensor(ang), torch.as_tensor(seq)
    P, L = len(probes), seq.shape[0]
    a = ang.to(dtype)[None].repeat(P, 1, 1).requires_grad_()
    crd = batched.generate_coords_batched(a, seq[None].repeat(P, 1), dtype)
    flat = torch.tensor([i * SLOTS + s for i, s in probes])
    (crd[torch.arange(P), flat] * torch.as_tensor(w).to(dtype)).sum().backward()
    return a.grad.detach(), crd[0].detach()


def generic_angles(L, seed=0):
    """angles with nothing special about them (no torsion at 0 or pi, bond angles 2.0 +- 0.1): for `support_sets`"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-3.0, 3.0, (L, ANGLES))
    a[:, 3:6] = rng.normal(2.0, 0.1, (L, 3))
    return torch.from_numpy(a)


def support_sets(seq, n, probes):
    """for every probe atom (residue, slot) of the protein seq[:n]: the set of (residue, column) angle entries it depends on in
    the reference's graph - where the fp64 autograd of the oracle is non-zero for any of the atom's three coordinates."""
    seq = torch.as_tensor(seq).clone()
    assert protein_len(seq) == n
    P = len(probes)
    w = torch.eye(3, dtype=torch.float64).repeat_interleave(P, dim=0)           # x for every probe, then y, then z
    rows, _ = jacobian_rows(generic_angles(seq.shape[0]), seq, list(probes) * 3, w)
    hit = (rows.reshape(3, P, -1, ANGLES) != 0).any(0).numpy()
    return [set(zip(*(int_list(v) for v in np.nonzero(hit[p])))) for p in range(P)]


def int_list(v):
    return [int(x) for x in v]


def expected_support(seq, n, i, slot):
    """the (residue, column) angle entries on which atom (i, slot) of the protein seq[:n] depends"""
    return support_sets(seq, n, [(i, slot)])[0]
