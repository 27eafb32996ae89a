"""The steric clash term (include/ptamd.h, ptamd_clash_fwd_bwd) restated in fp64 with numpy and torch autograd: the reference of
tests/test_clash_ref.py (CPU) and tests/test_gpu_clash.py.

Which slots are atoms and which element an atom is come from protein/PDB_Creator.py's ATOM_MAP_14 - a slot exists when its name
is not "PAD", the element is the first letter of the name - and not from the kernel's table or from csrc/nerf_tables.h.

The pair term has a kink: v = max(0, r_a + r_b - tau - d).  A pair whose exact r_a + r_b - tau - d is below the fp32 error of d
(a few ulps of a distance <= 3.6 A, ~1e-6 A) is a violation or not by rounding, in any fp32 implementation, and its whole
gradient term - a unit vector over n - comes or goes with it.  `clash_reference` therefore asserts a condition on the INPUT: no
candidate pair within `MARGIN` = 1e-4 A of the kink.  Under it `nclash` is exact.  Cases pick seeds that satisfy it."""
import numpy as np
import torch

from protein_transformer_amd.protein.PDB_Creator import ATOM_MAP_14

SLOTS, PAD = 14, 20
AA = "ACDEFGHIKLMNPQRSTVWY"                       # residue ids 0..19 (include/ptamd.h)
RADII = {"C": 1.7, "N": 1.55, "O": 1.52, "S": 1.8}          # van der Waals, Angstrom (Bondi 1964)
TOLERANCE = 1.5                                   # AlphaFold 2
MARGIN = 1e-4
PRED_MAX = 1e18
CYS, SG_SLOT = AA.index("C"), 5


def radius_table():
    """[20,14] fp64: the radius of slot s of residue type r, NaN where the type has no such atom."""
    tab = np.full((len(AA), SLOTS), np.nan)
    for r, one in enumerate(AA):
        for s, name in enumerate(ATOM_MAP_14[one]):
            if name != "PAD":
                tab[r, s] = RADII[name[0]]
    return tab


def atoms_of(seq):
    """One protein: (idx [n] slot indices in slot order, radius [n], residue [n], local slot [n], is_sg [n])."""
    seq = np.asarray(seq, np.int64)
    tab = radius_table()
    known = (seq >= 0) & (seq < len(AA))
    rad = np.where(known[:, None], tab[np.where(known, seq, 0)], np.nan).reshape(-1)
    idx = np.nonzero(~np.isnan(rad))[0]
    res, ls = idx // SLOTS, idx % SLOTS
    return idx, rad[idx], res, ls, (ls == SG_SLOT) & (seq[res] == CYS)


def candidate_pairs(seq, peptide_exclusion=True, disulfide_exclusion=True):
    """(idx, radius, ii, jj): the unordered pairs (ii < jj, positions in idx) of atoms in different residues, without the peptide
    bond C(i)-N(i+1) and without SG-SG of two CYS unless the exclusion is switched off."""
    idx, rad, res, ls, sg = atoms_of(seq)
    ok = res[:, None] != res[None]
    if peptide_exclusion:
        bond = (ls[:, None] == 2) & (ls[None] == 0) & (res[None] == res[:, None] + 1)
        ok &= ~(bond | bond.T)
    if disulfide_exclusion:
        ok &= ~(sg[:, None] & sg[None])
    ii, jj = np.nonzero(np.triu(ok, 1))
    return idx, rad, ii, jj


def clash_reference(crd, seq, tau=TOLERANCE, peptide_exclusion=True, disulfide_exclusion=True, check_margin=True):
    """One protein in fp64: (loss, nclash, n_atoms, d loss / d crd [L*14,3], margin) - margin the smallest |r_a + r_b - tau - d|
    over the candidate pairs (inf without one).  `crd`: an array, or an fp64 torch tensor inside an autograd graph (then the
    gradient slot is None and the loss is a tensor).  Asserts margin >= MARGIN unless `check_margin` is off."""
    idx, rad, ii, jj = candidate_pairs(seq, peptide_exclusion, disulfide_exclusion)
    n = len(idx)
    graph = torch.is_tensor(crd) and crd.requires_grad
    x_all = crd if graph else torch.tensor(np.asarray(crd, np.float64), requires_grad=True)
    nan = lambda: (x_all.sum() * 0 + float("nan")) if graph else float("nan")      # noqa: E731
    zeros = None if graph else np.zeros(tuple(x_all.shape))
    if n == 0:
        return nan(), 0, 0, zeros, np.inf
    x = x_all[torch.tensor(idx)]
    xv = x.detach().numpy()
    if not (np.abs(xv) <= PRED_MAX).all():                             # (NaN fails): the whole protein is unusable
        return nan(), 0, n, zeros, np.inf
    if len(ii) == 0:
        return (x.sum() * 0 if graph else 0.0), 0, n, zeros, np.inf
    diff = x[torch.tensor(ii)] - x[torch.tensor(jj)]
    d = torch.sqrt((diff ** 2).sum(-1) + 1e-30)
    over = torch.tensor(rad[ii] + rad[jj] - tau) - d
    margin = float(over.detach().abs().min())
    if check_margin:
        assert margin >= MARGIN, f"pick another seed: a pair sits {margin:.1e} A from the kink"
    loss = torch.clamp(over, min=0).sum() / n
    nclash = int((over.detach() > 0).sum())
    if graph:
        return loss, nclash, n, None, margin
    loss.backward()
    return float(loss.detach()), nclash, n, x_all.grad.numpy(), margin


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def sequence_with_atoms(n_atoms, rng, letters=AA):
    """Residue ids of a protein with exactly `n_atoms` atoms, drawn from `letters`."""
    size = {AA.index(c): int((~np.isnan(radius_table()[AA.index(c)])).sum()) for c in letters}
    for _ in range(1000):
        seq, left = [], n_atoms
        while left > 0:
            fits = [r for r, a in size.items() if a == left or left - a >= min(size.values())]
            if not fits:
                break
            seq.append(int(rng.choice(fits)))
            left -= size[seq[-1]]
        if left == 0 and len(seq) >= 2:
            return np.array(seq, np.int64)
    raise AssertionError(f"no sequence of {n_atoms} atoms from {letters}")


def build_chain(seq, rng, L_pad=None):
    """A NeRF-built all-atom chain (oracle, fp64, rounded to fp32) of random backbone and uniform side-chain torsions - side
    chains run into each other freely: ([L_pad*14,3] fp32 with zeros in the slots a residue does not have, [L_pad] ids)."""
    from oracle import batched
    from protein_transformer_amd import synthetic
    seq = np.asarray(seq, np.int64)
    L = len(seq)
    L_pad = L_pad or L
    ids = np.full((1, L_pad), PAD, np.int64)
    ids[0, :L] = seq
    ang = np.zeros((1, L_pad, 12), np.float32)
    ang[0, :L] = synthetic.sample_angles(rng, L)
    crd = batched.generate_coords_batched(torch.from_numpy(ang), torch.from_numpy(ids), torch.float64).float().numpy()[0]
    return crd, ids[0]
