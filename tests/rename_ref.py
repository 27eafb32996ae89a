"""fp64 numpy restatement of the symmetric side-chain renaming (include/ptamd.h, `ptamd_rename_symmetric`), for
tests/test_rename_cli.py and tests/test_gpu_rename.py.  TEST INFRASTRUCTURE ONLY: the product never imports it.

Two forms of the same definition: `rename_reference` (vectorised per residue) and `rename_loops` (a plain triple loop over
residue, ambiguous atom and partner), which the CPU test holds against each other."""
import numpy as np

AA = "ACDEFGHIKLMNPQRSTVWY"
PAD_ID, SLOTS = 20, 14
PRED_MAX = 1.0e18
# residue id -> (swap pairs as slots, chi column); written out here independently of losses.SYMMETRIC_SWAPS
SWAPS = {2: (((6, 7),), 8), 3: (((7, 8),), 9), 4: (((6, 10), (7, 9)), 8), 19: (((6, 11), (7, 10)), 8)}


def swaps_from_atom_names(atom_map_14):
    """The table derived from atom names alone ({one letter: 14 names}, protein/PDB_Creator.ATOM_MAP_14): two atoms of a residue
    are a swap pair when their names differ only in a final 1 / 2 and both hang off the same kind of symmetric group - the
    carboxylate oxygens of ASP / GLU and the ring carbons CD, CE of PHE / TYR.  The chi column is 6 + (side-chain index of the first
    atom of the first pair): side-chain atom k is placed with angle column 6 + k."""
    groups = {"D": ("OD",), "E": ("OE",), "F": ("CD", "CE"), "Y": ("CD", "CE")}
    out = {}
    for one, stems in groups.items():
        names = atom_map_14[one]
        pairs = tuple((names.index(stem + "1"), names.index(stem + "2")) for stem in stems)
        out[AA.index(one)] = (pairs, 6 + pairs[0][0] - 4)
    return out


def _dist(a, q):
    d = a[:, None, :].astype(np.float64) - q[None, :, :].astype(np.float64)
    return np.sqrt((d * d).sum(-1))


def masks(truth, seq):
    """present [L,14] (non-pad residue, true coordinate without NaN) and ambiguous [L,14] (member of a swap pair)."""
    L = len(seq)
    t = truth.reshape(L, SLOTS, 3)
    present = (np.asarray(seq) != PAD_ID)[:, None] & ~np.isnan(t).any(-1)
    amb = np.zeros((L, SLOTS), bool)
    for r, s in enumerate(seq):
        for pair in SWAPS.get(int(s), ((), 0))[0]:
            amb[r, list(pair)] = True
    return present, amb


def candidates(truth, seq):
    present, amb = masks(truth, seq)
    return [r for r, s in enumerate(seq) if int(s) in SWAPS and present[r][amb[r]].all()]


def unusable(pred, truth, seq):
    present, _ = masks(truth, seq)
    p = pred.reshape(-1, SLOTS, 3)[present]
    return bool((~(np.abs(p) <= PRED_MAX)).any())


def rename_reference(pred, truth, seq, ang=None):
    """One protein: pred, truth [L*14,3] fp32, seq [L], ang [L,24] fp32 or None -> (truth', ang' or None, swapped [L] int32,
    cost [L,2] fp64)."""
    L = len(seq)
    present, amb = masks(truth, seq)
    p, t = pred.reshape(L, SLOTS, 3), truth.reshape(L, SLOTS, 3)
    q_mask = present & ~amb
    pq, tq = p[q_mask], t[q_mask]
    cost = np.zeros((L, 2))
    swapped = np.zeros(L, np.int32)
    bad = unusable(pred, truth, seq)
    for r in candidates(truth, seq):
        if bad:
            cost[r] = np.nan
            continue
        pairs = SWAPS[int(seq[r])][0]
        a = [s for pair in pairs for s in pair]
        partner = [s for pair in pairs for s in pair[::-1]]
        dp, dt, dt_alt = _dist(p[r, a], pq), _dist(t[r, a], tq), _dist(t[r, partner], tq)
        cost[r] = np.abs(dp - dt).sum(), np.abs(dp - dt_alt).sum()
        swapped[r] = cost[r, 1] < cost[r, 0]
    return apply(truth, ang, seq, swapped) + (swapped, cost)


def rename_loops(pred, truth, seq):
    """The same costs by a plain triple loop; (swapped, cost)."""
    L = len(seq)
    p, t = pred.reshape(L, SLOTS, 3).astype(np.float64), truth.reshape(L, SLOTS, 3).astype(np.float64)
    present, amb = masks(truth, seq)
    cost, swapped = np.zeros((L, 2)), np.zeros(L, np.int32)
    for r in range(L):
        pairs = SWAPS.get(int(seq[r]), ((), 0))[0]
        if seq[r] == PAD_ID or not pairs or not all(present[r, s] for pair in pairs for s in pair):
            continue
        for pair in pairs:
            for a, a2 in (pair, pair[::-1]):
                for r2 in range(L):
                    for s2 in range(SLOTS):
                        if not present[r2, s2] or amb[r2, s2]:
                            continue
                        dp = np.sqrt(((p[r, a] - p[r2, s2]) ** 2).sum())
                        cost[r, 0] += abs(dp - np.sqrt(((t[r, a] - t[r2, s2]) ** 2).sum()))
                        cost[r, 1] += abs(dp - np.sqrt(((t[r, a2] - t[r2, s2]) ** 2).sum()))
        swapped[r] = cost[r, 1] < cost[r, 0]
    return swapped, cost


def apply(truth, ang, seq, swapped):
    """The permutation and the negation: (truth', ang' or None); every other value keeps its bits."""
    L = len(seq)
    out = truth.reshape(L, SLOTS, 3).copy()
    ang_out = None if ang is None else ang.reshape(L, 12, 2).copy()
    for r in np.nonzero(swapped)[0]:
        pairs, col = SWAPS[int(seq[r])]
        for a, b in pairs:
            out[r, [a, b]] = out[r, [b, a]]
        if ang_out is not None:
            ang_out[r, col] = -ang_out[r, col]
    return out.reshape(truth.shape), None if ang is None else ang_out.reshape(ang.shape)


def well_posed(cost, rows):
    """The smallest |alt - orig| / (alt + orig) over the residues `rows` (inf without any)."""
    c = cost[rows]
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.min(np.abs(c[:, 1] - c[:, 0]) / (c[:, 1] + c[:, 0]))) if len(rows) else float("inf")
