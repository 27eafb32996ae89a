"""Eval-only metrics: RMSD after optimal superposition (Kabsch), SURVEY.md section 8f row 1, and lDDT (below).

Reference: `rmsd` (/root/reference/protein_transformer/losses.py:281-286) calls ProDy's
calcTransformation / calcRMSD, reached only from `eval_epoch` (train.py:125-127) with
return_rmsd=True.  ProDy is not installable here, so this is the textbook Kabsch algorithm
(PARITY UNPINNED, same caveat as oracle/losses.py:kabsch_rmsd).  It runs as ONE kernel launch per batch
(csrc/kabsch.hip: fp64 moments per protein, Jacobi eigenvalues of H^T H on the device) - no per-protein host
round trip, no torch.linalg.

lDDT (`lddt_batch`, `batch_lddt`; `train.py --eval_lddt`) has no counterpart in the reference: Mariani et al., Bioinformatics
29(21):2722-2728 (2013), all-atom and C-alpha, per residue and per protein, counted on the device (csrc/lddt.hip; definition in
include/ptamd.h).

The steric clash term (`clash_batch`; `train.py --eval_clash`) has none either: the between-residue violation term of AlphaFold 2
(Jumper et al. 2021, supplementary 1.9.11) on the predicted structure alone (csrc/clash.hip).

TM-score and GDT_TS / GDT_HA (`tm_batch`, `batch_tm`; `train.py --eval_tm`) have none either: Zhang & Skolnick, Proteins
57:702-710 (2004), over the C-alphas, maximised by the seed-and-refine superposition search of the TMscore program on the device
(csrc/tmscore.hip; definition in include/ptamd.h; PARITY UNPINNED like the Kabsch RMSD above).

Secondary-structure agreement (`ss_batch`; `train.py --eval_ss`) has none either: Kabsch & Sander, Biopolymers 22:2577-2637
(1983), simplified - every hydrogen bond under the energy threshold counts, three states H / E / C - for both structures, and Q3
between them (csrc/dssp.hip; definition in include/ptamd.h; PARITY UNPINNED).

Side-chain accuracy (`sidechain_batch`, `batch_sidechain`; the scorer `python -m protein_transformer_amd.score`) has none either:
the IUPAC-IUB (1970) chi1 .. chi4 of both structures, the share within a threshold of the native ones with the ASP / GLU / PHE /
TYR ambiguity resolved, and the RMSD of the side-chain atoms in each residue's own backbone frame (csrc/sidechain.hip; definition
in include/ptamd.h; PARITY UNPINNED).  It is not a record of EVAL_METRICS yet: INTEGRATION.md, "Side-chain accuracy".
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib
from .protein.Structure import NUM_PREDICTED_COORDS, structure_pair


def kabsch_rmsd_batch(pred_crd, true_crd, seq):
    """pred_crd, true_crd [B, L*14, 3] device tensors (NaN truth = absent atom), seq [B, L] -> rmsd [B] (device, no sync)."""
    pred_crd, true_crd, seq, B, L = structure_pair(pred_crd, true_crd, seq)
    out = torch.empty(B, dtype=torch.float32, device=seq.device)
    rc = _lib.lib().ptamd_kabsch_rmsd(_lib.ptr(pred_crd), _lib.ptr(true_crd), _lib.ptr(seq), B, L, _lib.ptr(out), _lib.stream())
    _lib.check(rc, "kabsch_rmsd")
    return out


def lddt_batch(pred_crd, true_crd, seq, cutoff=15.0):
    """pred_crd, true_crd [B, L*14, 3] device tensors (NaN truth = absent atom), seq [B, L] ->
    (score [B,2], per_res [B,L,2], counts [B,L,2,5] int32), all on the device, no sync.  Last-but-one axis / `score` columns:
    0 = every atom, 1 = C-alpha only; counts = {total, p0.5, p1, p2, p4} per residue (include/ptamd.h); NaN = no included pair."""
    pred_crd, true_crd, seq, B, L = structure_pair(pred_crd, true_crd, seq)
    dev = seq.device
    counts = torch.empty(B, L, 2, 5, dtype=torch.int32, device=dev)       # zero-filled by the entry point
    per_res = torch.empty(B, L, 2, dtype=torch.float32, device=dev)
    score = torch.empty(B, 2, dtype=torch.float32, device=dev)
    ws = _lib.workspace("lddt", _lib.lib().ptamd_lddt_workspace_bytes(B, L), dev)
    rc = _lib.lib().ptamd_lddt(_lib.ptr(pred_crd), _lib.ptr(true_crd), _lib.ptr(seq), B, L, float(cutoff), _lib.ptr(counts),
                               _lib.ptr(per_res), _lib.ptr(score), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "lddt")
    return score, per_res, counts


def tm_batch(pred_crd, true_crd, seq):
    """pred_crd, true_crd [B, L*14, 3] device tensors (NaN truth = absent atom), seq [B, L] ->
    (score [B,3] = {tm, gdt_ts, gdt_ha}, counts [B,6] int32 = {N, c0.5, c1, c2, c4, c8}, xform [B,3,4] = (R | t) with
    R p + t on q), all on the device, no sync: TM-score and GDT over the C-alphas, maximised by the seed-and-refine search of
    csrc/tmscore.hip (definition in include/ptamd.h).  NaN = fewer than 3 present C-alphas or a non-finite prediction on one."""
    pred_crd, true_crd, seq, B, L = structure_pair(pred_crd, true_crd, seq)
    dev = seq.device
    score = torch.empty(B, 3, dtype=torch.float32, device=dev)
    counts = torch.empty(B, 6, dtype=torch.int32, device=dev)
    xform = torch.empty(B, 12, dtype=torch.float32, device=dev)
    ws = _lib.workspace("tm", _lib.lib().ptamd_tm_workspace_bytes(B, L), dev)
    rc = _lib.lib().ptamd_tm_score(_lib.ptr(pred_crd), _lib.ptr(true_crd), _lib.ptr(seq), B, L, _lib.ptr(score), _lib.ptr(counts),
                                   _lib.ptr(xform), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "tm_score")
    return score, counts, torch.cat([xform[:, :9].reshape(B, 3, 3), xform[:, 9:].reshape(B, 3, 1)], dim=2)


def ss_batch(crd, true_crds, seq, hbonds=False):
    """crd, true_crds [B, L*14, 3] device tensors (NaN truth = absent atom), seq [B, L] -> (score [B,3] = {q3, h, e},
    confusion [B,3,3] int32 = true state x predicted state in the order H, E, C, states [B,L,2] int8 = {pred, true}, -1 = absent),
    all on the device, no sync: the simplified DSSP of csrc/dssp.hip on both structures (definition in include/ptamd.h).  NaN = no
    residue in the denominator, or a non-finite predicted backbone atom on a present residue.  `hbonds`: also the bond bits
    [B, 2, L, ceil(L/64)] int64 ({pred, true}; bit j & 63 of word j >> 6 of row i = the C=O of i accepts from the N-H of j)."""
    crd, true_crds, seq, B, L = structure_pair(crd, true_crds, seq)
    dev = seq.device
    score = torch.empty(B, 3, dtype=torch.float32, device=dev)
    confusion = torch.empty(B, 3, 3, dtype=torch.int32, device=dev)
    states = torch.empty(B, L, 2, dtype=torch.int8, device=dev)
    bits = torch.empty(B, 2, L, (L + 63) // 64, dtype=torch.int64, device=dev) if hbonds else None
    ws = _lib.workspace("ss", _lib.lib().ptamd_ss_workspace_bytes(B, L), dev)
    rc = _lib.lib().ptamd_ss(_lib.ptr(crd), _lib.ptr(true_crds), _lib.ptr(seq), B, L, _lib.ptr(score), _lib.ptr(confusion),
                             _lib.ptr(states), _lib.ptr(bits), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "ss")
    return (score, confusion, states, bits) if hbonds else (score, confusion, states)


def sidechain_batch(pred_crd, true_crd, seq, threshold=40.0, per_residue=False):
    """pred_crd, true_crd [B, L*14, 3] device tensors (NaN truth = absent atom), seq [B, L] -> (score [B,4] = {chi1, chi12,
    chi_mae, sc_rmsd}, counts [B,12] int32 = {scored, hit of chi1 .. chi4, n12, hit12, residues, atoms}), all on the device, no
    sync: the side-chain accuracy of csrc/sidechain.hip (definition in include/ptamd.h); `threshold` in degrees.  NaN = nothing in
    the denominator, or an unusable prediction.  `per_residue`: also per_res [B,L,5] = {Delta_1 .. Delta_4 in degrees, local-frame
    RMSD of the residue's side chain}, NaN where not scored."""
    pred_crd, true_crd, seq, B, L = structure_pair(pred_crd, true_crd, seq)
    dev = seq.device
    score = torch.empty(B, 4, dtype=torch.float32, device=dev)
    counts = torch.empty(B, 12, dtype=torch.int32, device=dev)
    per_res = torch.empty(B, L, 5, dtype=torch.float32, device=dev) if per_residue else None
    ws = _lib.workspace("sidechain", _lib.lib().ptamd_sidechain_workspace_bytes(B, L), dev)
    rc = _lib.lib().ptamd_sidechain(_lib.ptr(pred_crd), _lib.ptr(true_crd), _lib.ptr(seq), B, L, float(threshold), _lib.ptr(score),
                                    _lib.ptr(counts), _lib.ptr(per_res), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "sidechain")
    return (score, counts, per_res) if per_residue else (score, counts)


def aligned_error_batch(pred_crd, true_crd, seq):
    """pred_crd, true_crd [B, L*14, 3] device tensors (NaN truth = absent atom), seq [B, L] -> (ae [B,L,L], stats [B,2] = {mean,
    tm}), all on the device, no sync: the TRUE frame-aligned error of csrc/aligned_error.hip (definition in include/ptamd.h) - the
    truth as the reference, the prediction as its one sample.  ae[b,i,j] = how far the predicted C-alpha of j lies from the true
    one when both structures are aligned on the backbone frame of i.  NaN = a residue the truth has no frame / no C-alpha for,
    padding, or a prediction that lacks a frame or a C-alpha the truth has."""
    from .ensemble import aligned_error
    pred_crd, true_crd, seq, B, L = structure_pair(pred_crd, true_crd, seq)
    ae, stats, _ = aligned_error(true_crd, pred_crd.view(B, 1, -1, 3), seq)
    return ae, stats


def clash_batch(crd, seq, tolerance=1.5):
    """crd [B, L*14, 3] predicted coordinates (device), seq [B, L] -> (loss [B], nclash [B] int64, n_atoms [B]), all on the
    device, no sync: the steric clash term of csrc/clash.hip (include/ptamd.h), forward only - Angstrom of overlap per atom
    between atoms of different residues, the number of clashing pairs, and the atom count; NaN loss = no atom or an unusable
    prediction.  The truth is not an argument (`train.py --eval_clash`)."""
    from .losses import clash_forward_backward
    stats, nclash, _ = clash_forward_backward(crd, seq, need_grad=False, tolerance=tolerance)
    return stats[:, 0], nclash, stats[:, 1]


def _clash_of(crd, true_crds, seq, args):
    from .losses import CLASH_TOLERANCE
    return clash_batch(crd, seq, float(getattr(args, "clash_tolerance", CLASH_TOLERANCE)))[0]


# All the host code knows about an optional evaluation metric (`train.py --eval_<x>`), in the order of their columns in the log.
# flag: the attribute of args that asks for it; field: its field in losses.REPORT_FIELDS - and the keyword of log.log_batch; columns:
# per column of that field (key of the get_losses dictionary and of a split's metrics, name in the CSV header); run(crd, true_crds,
# seq, args) -> the per-protein values [B] or [B,k] on the device; esm: higher is better, the keys keep an epoch-history and are
# targets of `-esm <split>-<key>`.
EvalMetric = namedtuple("EvalMetric", "flag field columns run esm")
EVAL_METRICS = (
    EvalMetric("eval_lddt", "lddt", (("lddt-full", "lddt"), ("lddt-ca", "lddt_ca")), lambda c, t, s, a: lddt_batch(c, t, s)[0], False),
    EvalMetric("eval_clash", "clash", (("clash-full", "clash"),), _clash_of, False),
    # (--rename_symmetric renames side-chain atoms: the C-alphas of `tm`, and N, CA, C, O of `ss`, are the same)
    EvalMetric("eval_tm", "tm", (("tm-ca", "tm"), ("gdt-ts", "gdt_ts"), ("gdt-ha", "gdt_ha")),
               lambda c, t, s, a: tm_batch(c, t, s)[0], False),
    EvalMetric("eval_ss", "ss", (("ss-q3", "ss_q3"), ("ss-h", "ss_h"), ("ss-e", "ss_e")), lambda c, t, s, a: ss_batch(c, t, s)[0], True),
)
METRIC_KEYS = tuple(key for m in EVAL_METRICS for key, _ in m.columns)
ESM_KEYS = tuple(key for m in EVAL_METRICS if m.esm for key, _ in m.columns)


def rmsd(a, b):
    """RMSD between two [n,3] coordinate sets after superposing `a` on `b` (losses.py:281-286); host float."""
    dev = a.device if torch.is_tensor(a) and a.is_cuda else torch.device("cuda", torch.cuda.current_device())
    a = torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).to(dev, torch.float32)
    b = torch.as_tensor(np.asarray(b) if not torch.is_tensor(b) else b).to(dev, torch.float32)
    n = a.shape[0]
    L = max(1, -(-n // NUM_PREDICTED_COORDS))
    pa = torch.zeros(1, L * NUM_PREDICTED_COORDS, 3, dtype=torch.float32, device=dev)
    pb = torch.full((1, L * NUM_PREDICTED_COORDS, 3), float("nan"), dtype=torch.float32, device=dev)
    pa[0, :n], pb[0, :n] = a, b
    return float(kabsch_rmsd_batch(pa, pb, torch.zeros(1, L, dtype=torch.int64, device=dev))[0])


def batch_rmsd(pred_sincos, true_crds, input_seqs):
    """np.mean over proteins of the superposed RMSD of the structures built from pred_sincos (one host read)."""
    from .losses import predicted_coords
    crd, _ = predicted_coords(pred_sincos, input_seqs)
    return float(kabsch_rmsd_batch(crd, true_crds, input_seqs).double().mean())


def _finite_means(scores):
    """scores [B,k] (device) -> k host floats: per column the mean over the proteins with a finite score, NaN when none has one;
    one host read."""
    from .losses import finite_sums
    k = scores.shape[1]
    s = finite_sums(scores).cpu().numpy()
    return tuple(float(s[j] / s[k + j]) if s[k + j] > 0 else float("nan") for j in range(k))


def batch_lddt(pred_sincos, true_crds, input_seqs, cutoff=15.0):
    """(lddt-full, lddt-ca): means over the proteins with a finite score of the lDDT of the structures built from
    pred_sincos (NaN when no protein has one); one host read."""
    from .losses import predicted_coords
    crd, _ = predicted_coords(pred_sincos, input_seqs)
    return _finite_means(lddt_batch(crd, true_crds, input_seqs, cutoff)[0])


def batch_tm(pred_sincos, true_crds, input_seqs):
    """(tm, gdt_ts, gdt_ha): means over the proteins with a finite score of the TM-score and GDT of the structures built from
    pred_sincos (NaN when no protein has one); one host read."""
    from .losses import predicted_coords
    crd, _ = predicted_coords(pred_sincos, input_seqs)
    return _finite_means(tm_batch(crd, true_crds, input_seqs)[0])


def batch_sidechain(pred_sincos, true_crds, input_seqs, threshold=40.0):
    """(chi1, chi12, chi_mae, sc_rmsd): means over the proteins with a finite score of the side-chain accuracy of the structures
    built from pred_sincos (NaN when no protein has one); one host read."""
    from .losses import predicted_coords
    crd, _ = predicted_coords(pred_sincos, input_seqs)
    return _finite_means(sidechain_batch(crd, true_crds, input_seqs, threshold)[0])
