"""Predict all-atom structures from amino-acid sequences with a trained checkpoint, with a dropout-ensemble confidence.

    python -m protein_transformer_amd.predict CHECKPOINT SEQS.fasta --out DIR [--samples 8] [--seed 0] [--batch_residues 16384]
                                              [--per_residue] [--pae] [--plddt] [--ptm]

reads a checkpoint that `train.checkpoint_model` wrote and a multi-record FASTA file, and for every sequence writes
`DIR/<identifier>.pdb` - the structure of the deterministic (`model.eval()`) pass, built by the NeRF kernels - and prints one JSON
line: id, n-res, ens-lddt, ens-rmsd, ens-rmsf-ca, usable, samples.  `--samples K` passes in training mode (the encoder's dropout
masks, no backward pass) make an ensemble around that structure (`ensemble.predict_ensemble`, csrc/ensemble.hip); the temperature
factor of every atom is its residue's `conf`, and `--per_residue` also writes `DIR/<identifier>.csv`.  The reference
(protein_transformer) has no counterpart.  One upload and one read back per batch; there is no CPU path.

`--pae` (needs `--samples` >= 1) also writes `DIR/<identifier>.pae.json`, the frame-aligned error matrix of the samples around the
written structure (`ensemble.aligned_error`, csrc/aligned_error.hip) in the layout of AlphaFold DB's version-2 aligned-error files -
a list holding one object with `predicted_aligned_error` (n x n, row = the residue whose backbone frame aligns the two structures,
column = the residue whose C-alpha error is measured, two decimals, `null` where undefined) and `max_predicted_aligned_error` - and
appends `ens-pae` (its mean) and `ens-ptm` (the pTM formula applied to that mean error) to the JSON line; a protein without a usable
sample gets no file.  One further read back per batch.

`--plddt` (needs a checkpoint with a confidence head, written by `python -m protein_transformer_amd.confidence fit`; works with
`--samples 0`) runs the head on the last hidden state of the deterministic pass - no further pass of the encoder -: the temperature
factor of every atom is then its residue's pLDDT, `plddt` (the mean over the residues) is appended to the JSON line and
`--per_residue` gains a last column `plddt`.

`--ptm` (needs a checkpoint with a PAE head, written by `python -m protein_transformer_amd.confidence fit-pae`; works with
`--samples 0`; independent of `--pae` and `--plddt`) runs that head on the same hidden state: `DIR/<identifier>.head_pae.json` is
the head's expected aligned error in the same AlphaFold DB layout, and `pae` (its mean) and `ptm` (the pTM formula applied to the
head's predicted DISTRIBUTION of errors) are appended to the JSON line.  One further read back per batch.  A head is as good as its
fit: `confidence calibrate --pae` measures it, and nobody has measured it on a really trained model yet.

`ens-pae` and `ens-ptm`, like `ens-lddt`, measure the dropout ensemble's SELF-CONSISTENCY: they are NOT calibrated predictions of
the true aligned error or TM-score; how well they track them is what `confidence calibrate --pae --samples K` measures, and that
has not been done on any trained model.

`ens-lddt` (and, without `--plddt`, the temperature factors) is a dropout SELF-CONSISTENCY score on the lDDT scale - 100 x the mean
lDDT-C-alpha of the samples against the written structure - NOT a calibrated pLDDT.  How well it, or the head's `plddt`, tracks the
true lDDT of a given model is what `python -m protein_transformer_amd.confidence calibrate` measures.
"""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

from .protein.PDB_Creator import NUM_PREDICTED_COORDS, PDB_Creator
from .protein.Sequence import AA_MAP, ONE_TO_THREE_LETTER_MAP, VOCAB

KEYS = ("id", "n-res", "ens-lddt", "ens-rmsd", "ens-rmsf-ca", "usable", "samples")
PAE_KEYS = ("ens-pae", "ens-ptm")                                 # appended to KEYS by --pae
PLDDT_KEYS = ("plddt",)                                           # appended by --plddt, behind PAE_KEYS
PTM_KEYS = ("pae", "ptm")                                         # appended by --ptm, behind PLDDT_KEYS
PER_RESIDUE_HEADER = ("resnum", "resname", "conf", "rmsf_ca", "rmsf_all")
PLDDT_COLUMN = "plddt"                                            # last column of --per_residue under --plddt


def read_fasta(path):
    """A multi-record FASTA file -> [(identifier, sequence)] in file order.  A line that starts with '>' opens a record, its
    identifier is everything up to the first blank; the sequence lines of a record are joined and upper-cased, blanks inside them
    and one '*' at the end dropped.  ValueError, naming the record: an empty record, a letter outside the twenty amino acids, two
    records with one identifier, an identifier that cannot name a file, sequence lines in front of the first header."""
    records, seen = [], set()
    name, where, parts = None, 0, []

    def close():
        if name is None:
            return
        seq = "".join(parts).upper()
        if seq.endswith("*"):
            seq = seq[:-1]
        what = f"{path}, record '{name}' (line {where})"
        if not seq:
            raise ValueError(f"{what}: the record has no sequence")
        bad = sorted(set(seq) - set(AA_MAP))
        if bad:
            raise ValueError(f"{what}: {''.join(bad)!r} is outside the twenty amino acids ({''.join(sorted(AA_MAP))})")
        if name in seen:
            raise ValueError(f"{what}: a second record with this identifier")
        seen.add(name)
        records.append((name, seq))

    with open(path) as f:
        for number, line in enumerate(f, 1):
            line = line.strip()
            if line.startswith(">"):
                close()
                fields = line[1:].split()
                name, where, parts = (fields[0] if fields else ""), number, []
                if not name or os.sep in name or name in (".", ".."):
                    raise ValueError(f"{path}, line {number}: the identifier {name!r} cannot name a file")
            elif line:
                if name is None:
                    raise ValueError(f"{path}, line {number}: sequence letters in front of the first '>' header")
                parts.append("".join(line.split()))
    close()
    if not records:
        raise ValueError(f"{path}: no record")
    return records


def make_batches(lengths, batch_residues):
    """Indices of the sequences, sorted by length (ties in input order) and cut into batches of at most `batch_residues` PADDED
    residues - sequences x the longest of them - and at least one sequence."""
    order = sorted(range(len(lengths)), key=lambda i: lengths[i])
    batches, cur = [], []
    for i in order:
        if cur and (len(cur) + 1) * lengths[i] > batch_residues:
            batches.append(cur)
            cur = []
        cur.append(i)
    if cur:
        batches.append(cur)
    return batches


def load_checkpoint(path, device=None):
    """The model of a checkpoint written by `train.checkpoint_model`, on `device` (default: the current one): rebuilt from the
    stored settings by `train.make_model`; every weight, the angle-mean output bias among them, comes from the state dict."""
    from .train import make_model
    try:
        ck = torch.load(path, map_location="cpu", weights_only=False)
        settings, state = ck["settings"], ck["model_state_dict"]
    except Exception as e:                                          # (whatever the unpickler makes of a file that is none)
        what = " ".join(f"{type(e).__name__}: {e}".split())
        raise ValueError(f"{path}: not a checkpoint of train.checkpoint_model ({what})") from None
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    try:
        model = make_model(settings, device, np.zeros(24))
    except AttributeError as e:
        raise ValueError(f"{path}: the checkpoint's settings do not describe a model ({e})") from None
    model.load_state_dict(state)
    return model.to(device)


def predict_records(model, records, samples=8, seed=0, batch_residues=16384, device=None, pae=False, head=None, pae_head=None):
    """records [(identifier, sequence)] -> per record, in input order, dict(crd [n*14, 3], conf, rmsf_ca, rmsf_all [n], rmsd [K],
    usable) as host arrays (the ensemble fields None with samples = 0).  One upload and one read back per batch.  `pae` (needs
    samples >= 1): also ae [n, n] and ae_stats [2] = {mean, tm}, from one further read back per batch.  `head` (a
    `confidence.ConfidenceHead`): also plddt [n], the head on the last hidden state of the deterministic pass, in the same read
    back.  `pae_head` (a `confidence.PaeHead`): also head_pae [n, n] and head_pae_stats [2] = {mean, ptm}, from one further read
    back per batch."""
    from .confidence import mask_padding
    from .ensemble import predict_ensemble
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    K = int(samples)
    out = [None] * len(records)
    for batch in make_batches([len(s) for _, s in records], batch_residues):
        B, L = len(batch), max(len(records[i][1]) for i in batch)
        ids = np.full((B, L), VOCAB.pad_id, np.int64)
        for row, i in enumerate(batch):
            ids[row, :len(records[i][1])] = [AA_MAP[c] for c in records[i][1]]
        seq = torch.from_numpy(ids).to(dev)
        ens = predict_ensemble(model, seq, samples=K, seed=seed, aligned_error=bool(pae),
                               hidden=head is not None or pae_head is not None)
        fields = [ens.crd.reshape(B, -1)]
        if K:
            fields += [ens.conf, ens.rmsf.reshape(B, -1), ens.rmsd, ens.usable.float()[:, None]]
        if head is not None:
            fields.append(mask_padding(head.forward(ens.hidden)[0], seq))                # [B, L], behind everything else
        host = torch.cat(fields, dim=1).cpu().numpy()                                    # one read back
        if pae:
            matrix = torch.cat([ens.ae.reshape(B, -1), ens.ae_stats], dim=1).cpu().numpy()   # and the one of --pae
        if pae_head is not None:
            head_pae, head_stats, _ = pae_head.forward(ens.hidden, seq)
            head_matrix = torch.cat([head_pae.reshape(B, -1), head_stats], dim=1).cpu().numpy()   # and the one of --ptm
        n_crd = L * NUM_PREDICTED_COORDS * 3
        for row, i in enumerate(batch):
            n = len(records[i][1])
            r = dict(crd=host[row, :n_crd].reshape(-1, 3)[:n * NUM_PREDICTED_COORDS], conf=None, rmsf_ca=None, rmsf_all=None,
                     rmsd=None, usable=0)
            if K:
                rmsf = host[row, n_crd + L:n_crd + 3 * L].reshape(L, 2)[:n]
                r.update(conf=host[row, n_crd:n_crd + n], rmsf_ca=rmsf[:, 0], rmsf_all=rmsf[:, 1],
                         rmsd=host[row, n_crd + 3 * L:n_crd + 3 * L + K], usable=int(host[row, n_crd + 3 * L + K]))
            if head is not None:
                r.update(plddt=host[row, host.shape[1] - L:host.shape[1] - L + n])
            if pae:
                r.update(ae=matrix[row, :L * L].reshape(L, L)[:n, :n], ae_stats=matrix[row, L * L:])
            if pae_head is not None:
                r.update(head_pae=head_matrix[row, :L * L].reshape(L, L)[:n, :n], head_pae_stats=head_matrix[row, L * L:])
            out[i] = r
    return out


def _finite_mean(x):
    from .losses import finite_mean
    v = None if x is None else finite_mean(x)
    return None if v is None or not np.isfinite(v) else v


def summary(name, seq, r, samples):
    return {"id": name, "n-res": len(seq), "ens-lddt": _finite_mean(r["conf"]), "ens-rmsd": _finite_mean(r["rmsd"]),
            "ens-rmsf-ca": _finite_mean(r["rmsf_ca"]), "usable": r["usable"], "samples": int(samples)}


def pae_summary(r):
    mean, tm = (float(v) for v in r["ae_stats"])
    return {"ens-pae": mean if np.isfinite(mean) else None, "ens-ptm": tm if np.isfinite(tm) else None}


def ptm_summary(r):
    mean, ptm = (float(v) for v in r["head_pae_stats"])
    return {"pae": mean if np.isfinite(mean) else None, "ptm": ptm if np.isfinite(ptm) else None}


def pae_document(ae):
    """ae [n, n] -> what `json.dump` makes an AlphaFold DB version-2 aligned-error file of: a list holding one object, the matrix
    as a list of rows (row = frame residue, column = point) rounded to two decimals, None (JSON null, never NaN) where an entry
    is not finite, and the largest entry (None when there is none)."""
    ae = np.asarray(ae, np.float64)
    rows = [[round(float(v), 2) if np.isfinite(v) else None for v in row] for row in ae]
    finite = [v for row in rows for v in row if v is not None]
    return [{"predicted_aligned_error": rows, "max_predicted_aligned_error": max(finite) if finite else None}]


def write_pae(path, ae):
    with open(path, "w") as f:
        json.dump(pae_document(ae), f, allow_nan=False, separators=(",", ":"))
        f.write("\n")


def b_factors(r, n):
    """The temperature factor of every residue: its `plddt` where a head made one, else its `conf`; 0 where that is NaN or there
    is neither."""
    v = r.get("plddt") if r.get("plddt") is not None else r["conf"]
    return np.zeros(n) if v is None else np.nan_to_num(np.asarray(v, np.float64), nan=0.0)


def write_per_residue(path, seq, r):
    nan = np.full(len(seq), np.nan)
    cols = [nan if r[k] is None else r[k] for k in ("conf", "rmsf_ca", "rmsf_all")]
    header = PER_RESIDUE_HEADER
    if r.get("plddt") is not None:
        cols.append(r["plddt"])
        header += (PLDDT_COLUMN,)
    with open(path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(header)
        for i, c in enumerate(seq):
            w.writerow([i + 1, ONE_TO_THREE_LETTER_MAP[c]] + [f"{col[i]:.4f}" for col in cols])


def parser():
    ap = argparse.ArgumentParser(prog="python -m protein_transformer_amd.predict", description=__doc__.split("\n\n")[0])
    ap.add_argument("checkpoint", metavar="CHECKPOINT", help="a checkpoint written by train.py (<name>_best.chkpt)")
    ap.add_argument("fasta", metavar="SEQS.fasta", help="the sequences, one record each")
    ap.add_argument("--out", metavar="DIR", required=True, help="where <identifier>.pdb (and .csv) are written; created if missing")
    ap.add_argument("--samples", type=int, default=8, help="dropout passes of the ensemble; 0: the structure only (default 8)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the dropout masks of the ensemble (default 0)")
    ap.add_argument("--batch_residues", type=int, default=16384, help="padded residues per batch (default 16384)")
    ap.add_argument("--per_residue", action="store_true",
                    help="also write <identifier>.csv: residue number, name, conf, C-alpha RMSF and all-atom RMSF")
    ap.add_argument("--pae", action="store_true",
                    help="also write <identifier>.pae.json, the frame-aligned error matrix of the samples (AlphaFold DB layout), and "
                         "add ens-pae and ens-ptm to the JSON line: dropout self-consistency, not calibrated; needs --samples >= 1")
    ap.add_argument("--plddt", action="store_true",
                    help="run the checkpoint's confidence head (`confidence fit`) on the deterministic pass: temperature factors = "
                         "pLDDT, `plddt` on the JSON line, a last column `plddt` under --per_residue; works with --samples 0")
    ap.add_argument("--ptm", action="store_true",
                    help="run the checkpoint's PAE head (`confidence fit-pae`) on the deterministic pass: write "
                         "<identifier>.head_pae.json (AlphaFold DB layout) and add `pae` and `ptm` to the JSON line; works with "
                         "--samples 0")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    try:
        if args.samples < 0 or args.batch_residues < 1:
            raise ValueError("--samples must be >= 0 and --batch_residues >= 1")
        if args.pae and args.samples < 1:
            raise ValueError("--pae is made of the dropout samples and needs --samples >= 1")
        records = read_fasta(args.fasta)
        entry = pae_entry = None
        if args.plddt or args.ptm:                   # (decided on the host, before the model is built)
            from .confidence import head_from_entry, pae_head_from_entry, read_head_entries
            entry, pae_entry = read_head_entries(args.checkpoint)
            if args.ptm and pae_entry is None:
                raise ValueError(f"{args.checkpoint}: --ptm needs a checkpoint with a PAE head, and this one has none "
                                 "(`python -m protein_transformer_amd.confidence fit-pae` writes one)")
            if args.plddt and entry is None:
                raise ValueError(f"{args.checkpoint}: --plddt needs a checkpoint with a confidence head, and this one has none "
                                 "(`python -m protein_transformer_amd.confidence fit` writes one)")
        model = load_checkpoint(args.checkpoint)
        for name, seq in records:
            if len(seq) < 2:
                raise ValueError(f"{args.fasta}, record '{name}': one residue, and the NeRF build needs two")
            if len(seq) > model.max_seq_len:
                raise ValueError(f"{args.fasta}, record '{name}': {len(seq)} residues, and the checkpoint's max_seq_len is "
                                 f"{model.max_seq_len}")
    except (ValueError, OSError) as e:
        print(f"predict: {e}", file=sys.stderr)
        return 2
    os.makedirs(args.out, exist_ok=True)
    dev = next(model.parameters()).device
    head = head_from_entry(entry, dev) if args.plddt else None
    pae_head = pae_head_from_entry(pae_entry, dev) if args.ptm else None
    results = predict_records(model, records, args.samples, args.seed, args.batch_residues, pae=args.pae, head=head,
                              pae_head=pae_head)
    for (name, seq), r in zip(records, results):
        PDB_Creator(r["crd"], seq=seq, b_factors=b_factors(r, len(seq))).save_pdb(os.path.join(args.out, name + ".pdb"), title=name)
        if args.per_residue:
            write_per_residue(os.path.join(args.out, name + ".csv"), seq, r)
        line = summary(name, seq, r, args.samples)
        if args.pae:
            line.update(pae_summary(r))
            if r["usable"] > 0:
                write_pae(os.path.join(args.out, name + ".pae.json"), r["ae"])
        if args.plddt:
            line[PLDDT_KEYS[0]] = _finite_mean(r["plddt"])
        if args.ptm:
            line.update(ptm_summary(r))
            write_pae(os.path.join(args.out, name + ".head_pae.json"), r["head_pae"])
        print(json.dumps(line))
    return 0


if __name__ == "__main__":
    sys.exit(main())
