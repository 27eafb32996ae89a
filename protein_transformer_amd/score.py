"""Score a model structure against the native one, from two PDB files, with the device metrics of this package.

    python -m protein_transformer_amd.score PRED.pdb TRUE.pdb [--threshold 40] [--per_residue OUT.csv]
                                            [--aligned_error OUT.json]

prints one JSON line: the superposed RMSD, lDDT (all-atom and C-alpha), TM-score and GDT, the secondary-structure agreement, the
clash term and the side-chain accuracy (chi1 / chi1+2 within `--threshold` degrees, mean chi error, local-frame side-chain RMSD) -
the kernels behind `train.py --eval_*` and `eval_metrics.sidechain_batch`, on a batch of one.  The reference (protein_transformer)
has no counterpart.  One upload, one read back; there is no CPU path.

`--aligned_error OUT.json` also writes the TRUE frame-aligned error matrix (`eval_metrics.aligned_error_batch`,
csrc/aligned_error.hip: TRUE.pdb is the reference, PRED.pdb its one sample) in the layout `predict --pae` writes - row = the residue
whose backbone frame aligns the two structures, column = the residue whose C-alpha error is measured, `null` in the rows of
residues the truth has no N, CA, C for and in the columns of residues it has no CA for - and appends `ae-mean` and `ae-tm` to the
JSON line.  One further read back.

`read_pdb` understands what `protein.PDB_Creator` writes and the ATOM records of an ordinary single-chain PDB entry: the first
MODEL and the first chain only, no mmCIF.
"""
import argparse
import csv
import json
import sys

import numpy as np
import torch

from .protein.PDB_Creator import ATOM_MAP_14, NUM_PREDICTED_COORDS
from .protein.Sequence import AA_MAP, AA_MAP_INV, ONE_TO_THREE_LETTER_MAP, THREE_TO_ONE_LETTER_MAP

KEYS = ("rmsd-full", "lddt-full", "lddt-ca", "tm-ca", "gdt-ts", "gdt-ha", "ss-q3", "ss-h", "ss-e", "clash-full", "sc-chi1", "sc-chi12",
        "sc-chi-mae", "sc-rmsd", "n-res")
AE_KEYS = ("ae-mean", "ae-tm")                                    # appended to KEYS by --aligned_error
PER_RESIDUE_HEADER = ("resnum", "resname", "lddt", "chi1_err", "chi2_err", "chi3_err", "chi4_err", "sc_rmsd")
_SLOT = {one: {name: s for s, name in enumerate(names) if name != "PAD"} for one, names in ATOM_MAP_14.items()}


def _is_hydrogen(line, name):
    element = line[76:78].strip().upper()
    if element:
        return element in ("H", "D")
    return name.lstrip("0123456789")[:1] in ("H", "D")


def read_pdb(path, with_numbers=False):
    """ATOM records of the first MODEL and first chain of a PDB file -> (seq_ids [L] int64, crd [L*14, 3] float32): residues in
    the order of their residue numbers, atoms in the slots of `PDB_Creator.ATOM_MAP_14`, NaN where the file has no atom.
    Hydrogens, HETATM records, alternate locations other than blank or 'A', residue names outside the twenty and atom names the
    residue type does not have are skipped.  `with_numbers`: also the residue numbers [L]."""
    residues = {}                                  # (number, insertion code) -> (one-letter type, {slot: xyz})
    chain = None
    with open(path) as f:
        for number, line in enumerate(f, 1):
            record = line[:6]
            if record == "ENDMDL":
                break
            if record != "ATOM  ":
                continue
            one = THREE_TO_ONE_LETTER_MAP.get(line[17:20].strip().upper())
            name = line[12:16].strip().upper()
            if one is None or line[16:17] not in " A" or _is_hydrogen(line, name):
                continue
            if chain is None:
                chain = line[21:22]
            if line[21:22] != chain:
                continue
            slot = _SLOT[one].get(name)
            if slot is None:
                continue
            try:
                key = (int(line[22:26]), line[26:27] or " ")
                xyz = (float(line[30:38]), float(line[38:46]), float(line[46:54]))
            except ValueError:
                raise ValueError(f"{path}, line {number}: an ATOM record without a residue number in columns 23-26 or without "
                                 f"coordinates in columns 31-54: {line.rstrip()!r}") from None
            kind, atoms = residues.setdefault(key, (one, {}))
            if kind == one and slot not in atoms:
                atoms[slot] = xyz
    keys = sorted(residues)
    seq = np.array([AA_MAP[residues[k][0]] for k in keys], np.int64)
    crd = np.full((len(keys), NUM_PREDICTED_COORDS, 3), np.nan, np.float32)
    for r, k in enumerate(keys):
        for slot, xyz in residues[k][1].items():
            crd[r, slot] = xyz
    crd = crd.reshape(-1, 3)
    return (seq, crd, np.array([k[0] for k in keys], np.int64)) if with_numbers else (seq, crd)


def _aligned(pred, true):
    (pseq, pcrd), (tseq, tcrd) = pred, true
    pseq, tseq = np.asarray(pseq, np.int64), np.asarray(tseq, np.int64)
    if pseq.shape != tseq.shape or (pseq != tseq).any():
        show = lambda s: "".join(AA_MAP_INV.get(int(i), "?") for i in s)                 # noqa: E731
        raise ValueError(f"the two structures are aligned by position and must have the same sequence: the prediction has "
                         f"{len(pseq)} residues ({show(pseq[:30])}...), the truth {len(tseq)} ({show(tseq[:30])}...)")
    if len(tseq) == 0:
        raise ValueError("no residue of the twenty standard types was read")
    return tseq, np.asarray(pcrd, np.float32).reshape(-1, 3), np.asarray(tcrd, np.float32).reshape(-1, 3)


def score_structures(pred, true, threshold=40.0, per_residue=False, device=None, aligned_error=False):
    """pred, true: each (seq [L], crd [L*14, 3]) as `read_pdb` returns them -> {key of KEYS: float} (n-res: int).  An atom the
    truth lacks is left out of every metric (NaN = absent); an atom only the PREDICTION lacks is a non-finite prediction: the
    metrics that use it are NaN.  `per_residue`: also an array [L, 6] = {lDDT, chi error 1..4 in degrees, side-chain RMSD}.
    `aligned_error`: the result also has the keys of AE_KEYS, and the matrix [L, L] is returned last (one further read back)."""
    from . import eval_metrics as E
    seq, pcrd, tcrd = _aligned(pred, true)
    L = len(seq)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    # one upload: the two coordinate arrays and the sequence as the bytes of one buffer
    host = np.concatenate([pcrd.reshape(-1).view(np.uint8), tcrd.reshape(-1).view(np.uint8), seq.view(np.uint8)])
    buf = torch.from_numpy(host).to(dev)
    n = L * NUM_PREDICTED_COORDS * 3 * 4
    p = buf[:n].view(torch.float32).view(1, L * NUM_PREDICTED_COORDS, 3)
    t = buf[n:2 * n].view(torch.float32).view(1, L * NUM_PREDICTED_COORDS, 3)
    s = buf[2 * n:].view(torch.int64).view(1, L)
    lddt, lddt_res, _ = E.lddt_batch(p, t, s)
    sc = E.sidechain_batch(p, t, s, threshold, per_residue=True)
    # (the clash term looks at the prediction alone and has no "absent": an atom the prediction lacks makes it NaN)
    values = torch.cat([E.kabsch_rmsd_batch(p, t, s), lddt[0], E.tm_batch(p, t, s)[0][0], E.ss_batch(p, t, s)[0][0],
                        E.clash_batch(p, s)[0], sc[0][0]])
    rows = torch.cat([lddt_res[0, :, :1], sc[2][0]], dim=1)
    out = torch.cat([values, rows.reshape(-1)]).cpu().numpy()                            # one read back
    result = {k: float(v) for k, v in zip(KEYS[:-1], out[:len(KEYS) - 1])}
    result["n-res"] = int(L)
    ret = (result, out[len(KEYS) - 1:].reshape(L, 6)) if per_residue else (result,)
    if aligned_error:
        ae, stats = E.aligned_error_batch(p, t, s)
        host = torch.cat([ae.reshape(-1), stats.reshape(-1)]).cpu().numpy()
        result.update({k: float(v) for k, v in zip(AE_KEYS, host[L * L:])})
        ret += (host[:L * L].reshape(L, L),)
    return ret if len(ret) > 1 else result


def write_per_residue(path, seq, numbers, rows):
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(PER_RESIDUE_HEADER)
        for s, n, row in zip(seq, numbers, rows):
            w.writerow([int(n), ONE_TO_THREE_LETTER_MAP[AA_MAP_INV[int(s)]]] + [f"{x:.4f}" for x in row])


def parser():
    ap = argparse.ArgumentParser(prog="python -m protein_transformer_amd.score", description=__doc__.split("\n\n")[0])
    ap.add_argument("pred", metavar="PRED.pdb", help="the model structure")
    ap.add_argument("true", metavar="TRUE.pdb", help="the native structure: what it lacks is left out of every metric")
    ap.add_argument("--threshold", type=float, default=40.0, help="degrees within which a chi angle counts as correct (default 40)")
    ap.add_argument("--per_residue", metavar="OUT.csv", default=None,
                    help="also write residue number, name, lDDT, the four chi errors and the side-chain RMSD of every residue")
    ap.add_argument("--aligned_error", metavar="OUT.json", default=None,
                    help="also write the true frame-aligned error matrix (the layout of predict --pae; null where the truth lacks "
                         "the residue) and add ae-mean and ae-tm to the JSON line")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    try:
        pseq, pcrd = read_pdb(args.pred)
        tseq, tcrd, numbers = read_pdb(args.true, with_numbers=True)
        result, rows, *matrix = score_structures((pseq, pcrd), (tseq, tcrd), args.threshold, per_residue=True,
                                                 aligned_error=args.aligned_error is not None)
    except ValueError as e:
        print(f"score: {e}", file=sys.stderr)
        return 2
    if args.per_residue:
        write_per_residue(args.per_residue, tseq, numbers, rows)
    if args.aligned_error:
        from .predict import write_pae
        write_pae(args.aligned_error, matrix[0])
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
