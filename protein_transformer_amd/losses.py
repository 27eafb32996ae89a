"""Loss functions of the training hot path, on the device.

Same names, arguments and return conventions as
/root/reference/protein_transformer/losses.py (combine_drmsd_mse :15, inverse_trig_transform :26,
drmsd_work :49, angles_to_coords :101, compute_batch_drmsd :133, mse_over_angles :175, drmsd :256);
the arithmetic runs in csrc/geometry.hip and csrc/drmsd.hip through libptamd.  Nothing is moved
to the CPU and no worker pool is needed: `device` and `pool` are accepted and ignored.
"""
import functools
from collections import namedtuple

import numpy as np
import torch

from . import _lib, dp
from .protein.Sequence import VOCAB
from .protein.structure_utils import get_backbone_from_full_coords  # noqa: F401  (losses.py:12: importable from here too)
from .protein.Structure import (NUM_BB_ATOMS, NUM_PREDICTED_ANGLES, NUM_PREDICTED_COORDS, SC_ANGLES_START_POS, generate_coords,
                                nerf_backward, nerf_forward, raise_for_status, structure_pair)


def combine_drmsd_mse(d, mse, w=.5, lndrmsd_norm=0.02, mse_norm=0.01, log=True):
    """w * d / lndrmsd_norm + (1 - w) * mse / mse_norm   (losses.py:15-23; `log` only fed wandb)."""
    d = w * (d / lndrmsd_norm)
    mse = (1 - w) * (mse / mse_norm)
    return d + mse


# ----------------------------------------------------------------------------- atan2
def angles_forward(sincos):
    _lib.require_gpu(sincos)
    sincos = sincos.contiguous()
    ang = torch.empty(sincos.shape[:-1] + (sincos.shape[-1] // 2,), dtype=torch.float32, device=sincos.device)
    rc = _lib.lib().ptamd_angles_fwd(_lib.ptr(sincos), _lib.ptr(ang), ang.numel(), _lib.stream())
    _lib.check(rc, "angles_fwd")
    return ang


def angles_backward(sincos, dang):
    dsc = torch.empty_like(sincos)
    rc = _lib.lib().ptamd_angles_bwd(_lib.ptr(sincos.contiguous()), _lib.ptr(dang.contiguous()), _lib.ptr(dsc),
                                     dang.numel(), _lib.stream())
    _lib.check(rc, "angles_bwd")
    return dsc


class _AnglesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, sincos):
        ctx.save_for_backward(sincos)
        return angles_forward(sincos)

    @staticmethod
    def backward(ctx, dang):
        (sincos,) = ctx.saved_tensors
        return angles_backward(sincos, dang)


def inverse_trig_transform(t):
    """[B, L, 24] (cos, sin interleaved) -> [B, L, 12] radians via atan2 (losses.py:26-36)."""
    t = t.view(t.shape[0], -1, NUM_PREDICTED_ANGLES * 2)
    return _AnglesFn.apply(t.float())


# ----------------------------------------------------------------------------- dRMSD
def drmsd_forward_backward(pred_crd, true_crd, seq, need_grad=True, partial_budget_bytes=0, backbone_only=False):
    """Batched loss kernel. Returns stats [B,8] (device) and d(drmsd/n)/d(pred_crd) or None.  `partial_budget_bytes`: cap on the
    fixed-order partial sums of the pair sweep (0 = the library's 200 MB; smaller = the sweep runs in passes, same bits).
    `backbone_only`: the dRMSD over the present N, CA, C alone (losses.py:83-92) - pred_crd is the compact [B,L*3,3] array of
    nerf_forward(..., backbone_only=True), true_crd stays [B,L*14,3]; stats[:, 2], [:, 3], [:, 5] are what the full call reports
    there and [:, 0], [:, 1], [:, 4] mirror them; the gradient is d(bb_drmsd/n_bb)/d(pred_crd), [B,L*3,3]."""
    _lib.require_gpu(pred_crd, true_crd, seq)
    B, L = seq.shape
    pred_crd, true_crd, seq = pred_crd.contiguous(), true_crd.contiguous(), seq.contiguous()
    stats = torch.empty(B, 8, dtype=torch.float32, device=seq.device)
    dcrd = torch.empty_like(pred_crd) if need_grad else None
    budget = int(partial_budget_bytes)
    if backbone_only:
        assert pred_crd.shape == (B, L * NUM_BB_ATOMS, 3) and true_crd.shape == (B, L * NUM_PREDICTED_COORDS, 3)
        nbytes = _lib.lib().ptamd_drmsd_bb_workspace_bytes_budget(B, L, budget)
        ws = _lib.workspace("drmsd_bb", nbytes, seq.device)
        rc = _lib.lib().ptamd_drmsd_bb_fwd_bwd_budget(_lib.ptr(pred_crd), _lib.ptr(true_crd), _lib.ptr(seq), B, L, _lib.ptr(stats),
                                                      _lib.ptr(dcrd), _lib.ptr(ws), ws.numel(), budget, _lib.stream())
        _lib.check(rc, "drmsd_bb_fwd_bwd")
        return stats, dcrd
    nbytes = _lib.lib().ptamd_drmsd_workspace_bytes_budget(B, L, budget)
    ws = _lib.workspace("drmsd", nbytes, seq.device)
    rc = _lib.lib().ptamd_drmsd_fwd_bwd_budget(_lib.ptr(pred_crd), _lib.ptr(true_crd), _lib.ptr(seq), B, L, _lib.ptr(stats),
                                               _lib.ptr(dcrd), _lib.ptr(ws), ws.numel(), budget, _lib.stream())
    _lib.check(rc, "drmsd_fwd_bwd")
    return stats, dcrd


# ----------------------------------------------------------------------------- smooth lDDT
def slddt_forward_backward(crd, true_crds, seq, need_grad=True, cutoff=15.0, temperature=1.0):
    """Smooth lDDT loss of a batch (csrc/slddt.hip; definition in include/ptamd.h; no counterpart in the reference).
    crd, true_crds [B,L*14,3], seq [B,L].  Returns (stats [B,2] = {loss_i, score_i}, npairs [B] int64, d(loss_i)/d(crd) or None);
    a protein without an included pair has NaN statistics, npairs 0 and a zero gradient.  No host synchronisation."""
    crd, true_crds, seq, B, L = structure_pair(crd, true_crds, seq)
    stats = torch.empty(B, 2, dtype=torch.float32, device=seq.device)
    npairs = torch.empty(B, dtype=torch.int64, device=seq.device)
    dcrd = torch.empty_like(crd) if need_grad else None
    ws = _lib.workspace("slddt", _lib.lib().ptamd_slddt_workspace_bytes(B, L), seq.device)
    rc = _lib.lib().ptamd_slddt_fwd_bwd(_lib.ptr(crd), _lib.ptr(true_crds), _lib.ptr(seq), B, L, float(cutoff), float(temperature),
                                        _lib.ptr(stats), _lib.ptr(npairs), _lib.ptr(dcrd), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "slddt_fwd_bwd")
    return stats, npairs, dcrd


# ----------------------------------------------------------------------------- FAPE
def fape_forward_backward(crd, true_crds, seq, need_grad=True, clamp=10.0):
    """Frame aligned point error of a batch (csrc/fape.hip; definition in include/ptamd.h; no counterpart in the reference).
    crd, true_crds [B,L*14,3], seq [B,L]; `clamp` in Angstrom, float("inf") = unclamped.  Returns (stats [B,2] = {loss_i,
    nclamped_i / npairs_i}, npairs [B] int64, nclamped [B] int64, d(loss_i)/d(crd) or None); a protein without a frame or an atom,
    or with an unusable prediction, has a NaN loss and a zero gradient.  No host synchronisation."""
    crd, true_crds, seq, B, L = structure_pair(crd, true_crds, seq)
    stats = torch.empty(B, 2, dtype=torch.float32, device=seq.device)
    npairs = torch.empty(B, dtype=torch.int64, device=seq.device)
    nclamped = torch.empty(B, dtype=torch.int64, device=seq.device)
    dcrd = torch.empty_like(crd) if need_grad else None
    ws = _lib.workspace("fape", _lib.lib().ptamd_fape_workspace_bytes(B, L), seq.device)
    rc = _lib.lib().ptamd_fape_fwd_bwd(_lib.ptr(crd), _lib.ptr(true_crds), _lib.ptr(seq), B, L, float(clamp), _lib.ptr(stats),
                                       _lib.ptr(npairs), _lib.ptr(nclamped), _lib.ptr(dcrd), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "fape_fwd_bwd")
    return stats, npairs, nclamped, dcrd


# ----------------------------------------------------------------------------- superposed RMSD as a loss
def kabsch_forward_backward(crd, true_crds, seq, need_grad=True):
    """RMSD after optimal superposition (proper rotations) of a batch, as a loss (csrc/kabsch_loss.hip; definition in
    include/ptamd.h; the reference only evaluates it, losses.py:281-286).  crd, true_crds [B,L*14,3], seq [B,L].  Returns (stats
    [B,2] = {loss_i, n_i}, d(loss_i)/d(crd) or None); a protein with fewer than 3 present atoms, or with a NaN / infinite predicted
    coordinate on a present atom, has a NaN loss and a zero gradient.  One launch, no workspace, no host synchronisation."""
    crd, true_crds, seq, B, L = structure_pair(crd, true_crds, seq)
    stats = torch.empty(B, 2, dtype=torch.float32, device=seq.device)
    dcrd = torch.empty_like(crd) if need_grad else None
    rc = _lib.lib().ptamd_kabsch_loss_fwd_bwd(_lib.ptr(crd), _lib.ptr(true_crds), _lib.ptr(seq), B, L, _lib.ptr(stats),
                                              _lib.ptr(dcrd), _lib.stream())
    _lib.check(rc, "kabsch_loss_fwd_bwd")
    return stats, dcrd


# ----------------------------------------------------------------------------- steric clashes
CLASH_RADII = {"C": 1.7, "N": 1.55, "O": 1.52, "S": 1.8}       # van der Waals radius by element, in Angstrom (include/ptamd.h)
CLASH_TOLERANCE = 1.5                                           # AlphaFold 2's overlap tolerance, in Angstrom


def clash_forward_backward(crd, seq, need_grad=True, tolerance=CLASH_TOLERANCE, weight=1.0, accumulate_into=None):
    """Steric clash term of a batch of predicted structures (csrc/clash.hip; definition in include/ptamd.h; AlphaFold 2's
    between-residue violation term; no counterpart in the reference).  crd [B,L*14,3], seq [B,L]; the truth is not an argument.
    Returns (stats [B,2] = {loss_i, n_i}, nclash [B] int64, gradient or None).  The gradient is `weight` * d(loss_i)/d(crd) in a
    new tensor, or - `accumulate_into`: a contiguous fp32 [B,L*14,3] tensor - added to that tensor in place, which is returned.
    A protein without an atom or with an unusable prediction has a NaN loss and a zero gradient.  No host synchronisation."""
    _lib.require_gpu(crd, seq, accumulate_into)
    B, L = seq.shape
    crd, seq = crd.float().contiguous(), seq.contiguous()
    assert crd.shape == (B, L * NUM_PREDICTED_COORDS, 3)
    stats = torch.empty(B, 2, dtype=torch.float32, device=seq.device)
    nclash = torch.empty(B, dtype=torch.int64, device=seq.device)
    dcrd = None
    if accumulate_into is not None:
        assert need_grad and accumulate_into.shape == crd.shape and accumulate_into.dtype == torch.float32 \
            and accumulate_into.is_contiguous()
        dcrd = accumulate_into
    elif need_grad:
        dcrd = torch.empty_like(crd)
    ws = _lib.workspace("clash", _lib.lib().ptamd_clash_workspace_bytes(B, L), seq.device)
    rc = _lib.lib().ptamd_clash_fwd_bwd(_lib.ptr(crd), _lib.ptr(seq), B, L, float(tolerance), float(weight),
                                        int(accumulate_into is not None), _lib.ptr(stats), _lib.ptr(nclash), _lib.ptr(dcrd),
                                        _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "clash_fwd_bwd")
    return stats, nclash, dcrd


CLASH_BACKBONE_MESSAGE = ("--clash_weight penalises clashes between side-chain and backbone atoms: it cannot be combined with "
                          "--backbone_loss (no side chains are built there)")
CLASH_NO_STRUCTURE_MESSAGE = ("--clash_weight penalises the predicted structure: it cannot be combined with -l mse, whose "
                              "training steps build no structure")


def clash_check(weight, tolerance):
    """The parser's complaint about --clash_weight / --clash_tolerance, or None."""
    if not (0 <= weight < np.inf):                                                  # (NaN fails)
        return "--clash_weight must be finite and not negative"
    if not (0 <= tolerance < np.inf):
        return "--clash_tolerance must be finite and not negative"
    return None


# ----------------------------------------------------------------------------- symmetric side chains
# residue id -> (swap pairs as atom slots, the angle column whose torsion turns by pi when the names are exchanged); the table of
# include/ptamd.h.  The names behind the slots are protein/PDB_Creator.py's (tests/test_rename_cli.py derives the table from them).
SYMMETRIC_SWAPS = {2: (((6, 7),), 8), 3: (((7, 8),), 9), 4: (((6, 10), (7, 9)), 8), 19: (((6, 11), (7, 10)), 8)}


def rename_symmetric(crd, true_crds, seq, true_ang=None):
    """The truth of a batch under the naming of its symmetric side chains (ASP, GLU, PHE, TYR) that agrees better with the
    prediction `crd` (csrc/rename.hip; definition in include/ptamd.h; AlphaFold 2's algorithm 26; no counterpart in the reference).
    crd, true_crds [B,L*14,3], seq [B,L], true_ang [B,L,24] (cos, sin interleaved) or None.  Returns (true_crds', true_ang' or
    None, swapped [B,L] int32, cost [B,L,2] = {orig, alt}): new tensors, the inputs are untouched.  A constant for the gradient.
    No host synchronisation."""
    _lib.require_gpu(true_ang)
    crd, true_crds, seq, B, L = structure_pair(crd.detach(), true_crds, seq)
    crd_out = torch.empty_like(true_crds)
    ang_out = None
    if true_ang is not None:
        true_ang = true_ang.float().contiguous()
        assert true_ang.shape == (B, L, NUM_PREDICTED_ANGLES * 2)
        ang_out = torch.empty_like(true_ang)
    swapped = torch.empty(B, L, dtype=torch.int32, device=seq.device)
    cost = torch.empty(B, L, 2, dtype=torch.float32, device=seq.device)
    ws = _lib.workspace("rename_symmetric", _lib.lib().ptamd_rename_symmetric_workspace_bytes(B, L), seq.device)
    rc = _lib.lib().ptamd_rename_symmetric(_lib.ptr(crd), _lib.ptr(true_crds), _lib.ptr(true_ang), _lib.ptr(seq), B, L,
                                           _lib.ptr(crd_out), _lib.ptr(ang_out), _lib.ptr(swapped), _lib.ptr(cost), _lib.ptr(ws),
                                           ws.numel(), _lib.stream())
    _lib.check(rc, "rename_symmetric")
    return crd_out, ang_out, swapped, cost


# ----------------------------------------------------------------------------- the extra structural losses
# All the host code knows about a structural loss beside the dRMSD family (`train.py -l <name>`; the name is also its keyword in
# `batch_loss`, its field in REPORT_FIELDS and its key in `LossReport.wait()`).  run(crd, true_crds, seq, need_grad, params) -> (per-protein
# loss [B], its gradient d/d(crd) or None); params(args): as batch_loss takes them; check(params): the parser's complaint or None.
ExtraLoss = namedtuple("ExtraLoss", "name run params check backbone_message")


def _run_slddt(crd, true_crds, seq, need_grad, params):
    stats, _, dcrd = slddt_forward_backward(crd, true_crds, seq, need_grad=need_grad, cutoff=params[0], temperature=params[1])
    return stats[:, 0], dcrd


def _run_fape(crd, true_crds, seq, need_grad, params):
    stats, _, _, dcrd = fape_forward_backward(crd, true_crds, seq, need_grad=need_grad, clamp=params)
    return stats[:, 0], dcrd


def _run_kabsch(crd, true_crds, seq, need_grad, params):
    stats, dcrd = kabsch_forward_backward(crd, true_crds, seq, need_grad=need_grad)
    return stats[:, 0], dcrd


EXTRA_LOSSES = {e.name: e for e in (
    ExtraLoss("slddt", _run_slddt, lambda a: (float(getattr(a, "slddt_cutoff", 15.0)), float(getattr(a, "slddt_temperature", 1.0))),
              lambda p: None if all(0 < x < np.inf for x in p) else "--slddt_cutoff and --slddt_temperature must be finite and positive",
              "-l slddt is an all-atom loss: it cannot be combined with --backbone_loss "
              "(a backbone or C-alpha smooth lDDT does not exist here)"),
    ExtraLoss("fape", _run_fape, lambda a: float(getattr(a, "fape_clamp", 10.0)),
              lambda p: None if p > 0 else "--fape_clamp must be positive (inf = unclamped)",          # (NaN fails)
              "-l fape needs every atom: it cannot be combined with --backbone_loss "
              "(a backbone FAPE needs the compact backbone layout and does not exist here)"),
    ExtraLoss("kabsch", _run_kabsch, lambda a: True, lambda p: None,                                   # (no parameters)
              "-l kabsch is an all-atom loss: it cannot be combined with --backbone_loss "
              "(a backbone or C-alpha superposition loss does not exist here)"),
)}


RENAME_BACKBONE_MESSAGE = ("--rename_symmetric renames side-chain atoms: it cannot be combined with --backbone_loss "
                           "(no side chains are built there)")
RENAME_NO_STRUCTURE_MESSAGE = ("--rename_symmetric compares the truth with the predicted structure: it cannot be combined with "
                               "-l mse, whose training steps build no structure")


class _DrmsdFn(torch.autograd.Function):
    """drmsd(a, b) for two [n,3] point sets, differentiable in a."""

    @staticmethod
    def forward(ctx, a, b):
        n = a.shape[0]
        L = max(2, -(-n // NUM_PREDICTED_COORDS))
        dev = a.device
        pa = torch.zeros(1, L * NUM_PREDICTED_COORDS, 3, dtype=torch.float32, device=dev)
        pb = torch.full((1, L * NUM_PREDICTED_COORDS, 3), float("nan"), dtype=torch.float32, device=dev)
        pa[0, :n], pb[0, :n] = a.float(), b.float()
        seq = torch.zeros(1, L, dtype=torch.int64, device=dev)
        stats, dcrd = drmsd_forward_backward(pa, pb, seq, need_grad=True)
        ctx.save_for_backward(dcrd)
        ctx.n = n
        return stats[0, 0].clone()

    @staticmethod
    def backward(ctx, g):
        (dcrd,) = ctx.saved_tensors
        return g * ctx.n * dcrd[0, :ctx.n], None      # kernel differentiates drmsd / n


def drmsd(a, b):
    """Distance RMSD between coordinate tensors a and b, both [n,3] (losses.py:256-278)."""
    dev = a.device if a.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return _DrmsdFn.apply(a.to(dev), b.to(dev))


def pairwise_internal_dist(x):
    """All pairwise distances of an [n, d] coordinate tensor -> [n, n] (losses.py:233-253).  API parity only:
    the loss kernels never build this matrix."""
    assert len(x.shape) == 2, "Pairwise internal distance method is not implemented for batches."
    dev = x.device if x.is_cuda else torch.device("cuda", torch.cuda.current_device())
    x = x.to(dev, torch.float32).contiguous()
    out = torch.empty(x.shape[0], x.shape[0], dtype=torch.float32, device=dev)
    rc = _lib.lib().ptamd_pairwise_dist(_lib.ptr(x), x.shape[0], x.shape[1], _lib.ptr(out), _lib.stream())
    _lib.check(rc, "pairwise_dist")
    return out


def remove_sos_eos_from_input(input_seq):
    """A sequence of integers without a leading SOS / trailing EOS id (losses.py:39-46).  With the default vocabulary
    (no SOS / EOS characters) both ids are the unknown id 21 (protein/Sequence.py), as in the reference."""
    start_idx = 1 if input_seq[0] == VOCAB.sos_id else 0
    end_idx = -1 if input_seq[-1] == VOCAB.eos_id else None
    return input_seq[start_idx:end_idx]


def angles_to_coords(angles, seq, remove_batch_padding=False):
    """Torsional angles -> coordinates (losses.py:99-116)."""
    if remove_batch_padding:
        seq = seq[seq.ne(VOCAB.pad_id)]
    seq = remove_sos_eos_from_input(seq)
    angles = angles[:seq.shape[0]]
    return generate_coords(angles, seq)


def predicted_coords(pred_sincos, seqs, status=None, backbone_only=False):
    """Every atom ([B,L*14,3]; `backbone_only`: N, CA, C as the compact [B,L*3,3]) of the structures that the predictions
    pred_sincos [B,L,24] (cos, sin) stand for, as a constant: (crd, status word - `status` itself when one is passed).  No sync."""
    B, L = seqs.shape
    return nerf_forward(angles_forward(pred_sincos.detach().float().contiguous().view(B, L, -1)), seqs, status=status,
                        backbone_only=backbone_only)


BatchLoss = namedtuple("BatchLoss", "stats grad status crd per_protein true_crds true_ang clash", defaults=(None,) * 8)
_renamed_truth = rename_symmetric            # (batch_loss has a keyword of the function's name)


def batch_loss(pred_sincos, true_crds, input_seqs, do_backward=True, backbone_only=False, slddt=None, fape=None, kabsch=None,
               clash=None, rename_symmetric=False, true_ang=None):
    """Device-resident core of compute_batch_drmsd: angles -> NeRF forward -> the loss -> NeRF adjoint -> angles adjoint, no host
    synchronisation.  Returns a BatchLoss; a field nobody asked for is None:

    stats        [B,8], the dRMSD statistics.  `backbone_only` (losses.py:83-92, --backbone_loss; the backbone chain kernels and a
                 pair sweep over 3 L atoms, no side chains): [:, 2], [:, 3], [:, 5] of the full call, mirrored in [:, :2], [:, 4].
    grad         with `do_backward`, d(sum_i loss_i)/d(pred_sincos) [B,L,24]: loss_i is lndrmsd_i, lndrmsd-bb_i under `backbone_only`
                 (exactly zero in the side-chain channels), or the extra loss (`stats` is then forward-only, on the same build).
    status       int32[1], the status word of the build.
    crd          the coordinates that were built, [B,L*14,3]; the compact [B,L*3,3] backbone under `backbone_only`.
    per_protein  [B] (NaN: the protein has none), the extra loss that trains the structure instead of the dRMSD (EXTRA_LOSSES, at
                 most one): `slddt` = (cutoff, temperature), csrc/slddt.hip; `fape` = clamp in Angstrom, csrc/fape.hip;
                 `kabsch` = True (it has no parameters), csrc/kabsch_loss.hip.
    true_crds,   the truth every number above was taken against and every caller's RMSD, lDDT and MSE should be: the arguments as
    true_ang     passed, or with `rename_symmetric` the tensors renamed once against `crd` (`rename_symmetric` above; a constant for
                 the gradient; true_ang None when it was not given).
    clash        [B] (unweighted; NaN: none), with `clash` = (weight, tolerance): the clash term of csrc/clash.hip joins the loss.
                 Its kernel adds weight * d(sum_i clash_i) to the coordinate gradient in place, in front of the one NeRF adjoint.

    The extra losses, `rename_symmetric` and `clash` need side chains and are refused together with `backbone_only`; whatever is
    not asked for launches nothing.
    """
    asked = dict(slddt=slddt, fape=fape, kabsch=kabsch)
    given = [(extra, asked[name]) for name, extra in EXTRA_LOSSES.items() if asked[name] is not None]
    assert len(given) <= 1, "one structural loss at a time"
    extra, params = given[0] if given else (None, None)
    assert extra is None or not backbone_only, extra.backbone_message
    assert not (rename_symmetric and backbone_only), RENAME_BACKBONE_MESSAGE
    assert clash is None or not backbone_only, CLASH_BACKBONE_MESSAGE
    pred_sincos = pred_sincos.detach().float().contiguous()
    B, L = input_seqs.shape
    sc = pred_sincos.view(B, L, NUM_PREDICTED_ANGLES * 2)
    ang = angles_forward(sc)
    crd, status = nerf_forward(ang, input_seqs, backbone_only=backbone_only)
    if rename_symmetric:
        true_crds, true_ang = _renamed_truth(crd, true_crds, input_seqs, true_ang)[:2]
    stats, dcrd = drmsd_forward_backward(crd, true_crds.float(), input_seqs, need_grad=do_backward and extra is None,
                                         backbone_only=backbone_only)
    per_protein = clashes = grad = None
    if extra is not None:
        per_protein, dcrd = extra.run(crd, true_crds, input_seqs, do_backward, params)
    if clash is not None:
        clashes = clash_forward_backward(crd, input_seqs, need_grad=do_backward, tolerance=clash[1], weight=clash[0],
                                         accumulate_into=dcrd if do_backward else None)[0][:, 0]
    if do_backward:
        dang = nerf_backward(ang, input_seqs, crd, dcrd, backbone_only=backbone_only)
        grad = angles_backward(sc, dang)
    return BatchLoss(stats, grad, status, crd, per_protein, true_crds, true_ang, clashes)


# ----------------------------------------------------------------------------- statistics hand-over
_PINNED = {}


def _pinned(kind, n, dtype, device):
    """Pinned host buffer per (kind, size, device, STREAM): a stream's reports are consumed in order (`LossReport.wait`
    runs before the next one is built), two streams never share one."""
    key = (kind, n, dtype, device, torch.cuda.current_stream(device).cuda_stream)
    buf = _PINNED.get(key)
    if buf is None:
        buf = _PINNED[key] = torch.empty(n, dtype=dtype).pin_memory()
    return buf


# THE FIELDS of a report beside stats, mse, status and rmsd, in the order they travel in: per-protein fp32 values [B] or [B,k], every
# column reported as its mean over the proteins of the global batch that have a finite one.  name, the `wait()` keys of its columns,
# and where it lies - the one wire fact, which nothing outside this section needs to know: the FIXED fields are part of every
# report (their keys are always in `wait()`, their slots always in the reduced vector, where they have always been); whatever came
# later lies in the TAIL behind them - `kabsch` too, an extra loss like `slddt` and `fape` - and only in the reports of callers that
# ASK for it.  Asking is the field being a key of the mapping a caller passes, with None where it has no value; every rank of a job
# asks for the same fields, a rank with an empty shard included, so their vectors have one length.  A report nobody asked a tail
# field of has exactly the layout, the keys and the size it had before there was one.
ReportField = namedtuple("ReportField", "name keys fixed")
REPORT_FIELDS = (ReportField("lddt", ("lddt", "lddt-ca"), True), ReportField("slddt", ("slddt",), True),
                 ReportField("fape", ("fape",), True), ReportField("clash", ("clash",), False),
                 ReportField("tm", ("tm-ca", "gdt-ts", "gdt-ha"), False), ReportField("kabsch", ("kabsch",), False),
                 ReportField("ss", ("ss-q3", "ss-h", "ss-e"), False))
REPORT_KEYS = {f.name: f.keys for f in REPORT_FIELDS}
_MEANS = ("drmsd", "lndrmsd", "drmsd-bb", "lndrmsd-bb")        # stats[:, :4], reported as their means over the proteins
_NO_REPORT = {**dict.fromkeys(_MEANS, 0.0), "rmsd": None, "n_proteins": 0, "status": 0, "n_res": None, "mse": None,
              **{key: None for f in REPORT_FIELDS if f.fixed for key in f.keys}}


def _take(fields):
    """[(name, width), ...] -> ({name: slice}, total width): consecutive fields behind one running cursor (what atom_tiles::take
    does for the kernels' workspaces).  Every offset of a report comes from here."""
    at, cursor = {}, 0
    for name, width in fields:
        at[name] = slice(cursor, cursor + width)
        cursor += width
    return at, cursor


def finite_sums(x):
    """x [B] or [B,k] -> fp64 [2k] on x's device: per column the sum of the finite entries, then their counts.  No host sync."""
    ok = torch.isfinite(x)
    return torch.cat([torch.where(ok, x, torch.zeros_like(x)).double().sum(0).reshape(-1), ok.double().sum(0).reshape(-1)])


def finite_mean(x):
    """The mean, in fp64, of the finite entries of a host array; NaN when it has none."""
    x = np.asarray(x).astype(np.float64)
    return float(x[np.isfinite(x)].mean()) if np.isfinite(x).any() else float("nan")


@functools.lru_cache(maxsize=None)
def _local_layout(B, present, hollow):
    """({name of `present` or `hollow`: its slice}, size): stats, mse, status, rmsd keep their room when absent; a field of
    REPORT_FIELDS takes room where it is `present`, and an empty slice where it was asked for without a value (`hollow`)."""
    at, size = _take([("stats", 8 * B), ("mse", 6), ("status", 1), ("rmsd", B)]
                     + [(f.name, len(f.keys) * B if f.name in present else 0) for f in REPORT_FIELDS if f.name in present + hollow])
    return {name: s for name, s in at.items() if name in present + hollow}, size


def pack_local(stats=None, mse=None, status=None, rmsd=None, channels=None, alloc=torch.empty, tail=None):
    """What a single process reports, in one fp32 buffer: stats [B,8], the six MSE sums, the status word (int32[1], as raw bits),
    rmsd [B], each of them or None, and the fields of REPORT_FIELDS ({field: [B] or [B,k], or None}; `channels` and `tail` are one
    mapping, in two keywords for the callers that tell fixed fields from tail fields).  One (asynchronous) copy per field into
    `alloc(size)` (default: a host tensor); returns the buffer and its layout (B, {field that was passed: slice}) - a tail field
    that was asked for without a value has an empty slice, a fixed field without one is left out."""
    fields = {**(channels or {}), **(tail or {})}
    given = {k: t for k, t in dict(stats=stats, mse=mse, status=status, rmsd=rmsd).items() if t is not None}
    given.update({f.name: fields[f.name] for f in REPORT_FIELDS if fields.get(f.name) is not None})
    hollow = tuple(f.name for f in REPORT_FIELDS if not f.fixed and f.name in fields and fields[f.name] is None)
    B = next((t.shape[0] for name, t in given.items() if name not in ("mse", "status")), 0)
    at, size = _local_layout(B, tuple(given), hollow)
    buf = alloc(size)
    for name, t in given.items():
        dst = buf.view(torch.int32) if name == "status" else buf
        dst[at[name]].copy_(t if t.dim() == 1 else t.reshape(-1), non_blocking=True)
    return buf, (B, at)


def unpack_local(host, layout, n_res=None):
    """The `LossReport.wait()` dictionary of a single process, from the landed buffer (numpy fp32) and its layout: np.mean in fp64
    over the proteins of the per-protein values; a channel over the proteins with a finite value."""
    host, (B, at) = np.asarray(host), layout
    out = dict(_NO_REPORT, n_res=n_res)
    if "stats" in at and B:
        st = host[at["stats"]].reshape(B, 8).astype(np.float64)
        out.update({key: np.mean(st[:, k]) for k, key in enumerate(_MEANS)}, n_proteins=B)
    if "mse" in at:
        out["mse"] = host[at["mse"]].astype(np.float64)
    if "status" in at:
        out["status"] = int(host[at["status"]].view(np.int32)[0])
    if "rmsd" in at and B:
        out["rmsd"] = float(np.mean(host[at["rmsd"]].astype(np.float64)))
    for f in REPORT_FIELDS:
        if f.name in at:                              # passed or asked for: the keys exist, None when no value was passed
            values = host[at[f.name]].reshape(-1, len(f.keys))
            out.update({key: finite_mean(values[:, k]) if len(values) else None for k, key in enumerate(f.keys)})
    return out


@functools.lru_cache(maxsize=None)
def _vector_layout(asked=frozenset()):
    """({slot: slice}, size) of the fp64 vector a rank adds to the SUM reduction, in a job that asks for the fields `asked`.  sums: of
    stats[:, :4]; ranks_counted: the ranks that passed a residue count (0: n_res stays None like on one rank); a field of
    REPORT_FIELDS: its `finite_sums` (zeros on a rank without a value).  The fixed fields have their slots whoever asks, a tail
    field when it was ASKED for - the length depends on that alone, so an empty shard adds a vector as long as the others'."""
    return _take([("sums", 4), ("proteins", 1), ("rmsd_sum", 1), ("mse", 6), ("status_bits", 4), ("residues", 1),
                  ("rmsd_proteins", 1), ("ranks_counted", 1)]
                 + [(f.name, 2 * len(f.keys)) for f in REPORT_FIELDS if f.fixed or f.name in asked])


VECTOR_SLOTS, VECTOR_SIZE = _vector_layout()         # what every vector starts with: the tail's slots lie behind these


def reduce_vector(stats=None, mse=None, status=None, rmsd=None, n_res=None, channels=None, device=None, tail=None):
    """This rank's vector (arguments as `pack_local`; an empty shard passes None for everything - and None for every tail field
    the job asks for).  No host sync."""
    fields = {**(channels or {}), **(tail or {})}
    S, size = _vector_layout(frozenset(fields))
    v = torch.zeros(size, dtype=torch.float64, device=device)
    if stats is not None:
        v[S["sums"]], v[S["proteins"]] = stats[:, :4].double().sum(0), stats.shape[0]
    if rmsd is not None:
        v[S["rmsd_sum"]], v[S["rmsd_proteins"]] = rmsd.double().sum(), rmsd.shape[0]
    if mse is not None:
        v[S["mse"]] = mse.double()
    if status is not None:
        v[S["status_bits"]] = ((status.to(torch.int64) >> torch.arange(4, device=status.device)) & 1).double()
    v[S["residues"]], v[S["ranks_counted"]] = float(n_res or 0), 0.0 if n_res is None else 1.0
    for field, t in fields.items():
        if t is not None:
            v[S[field]] = finite_sums(t)
    return v


def unpack_global(v, passed=(), tail=()):
    """The `LossReport.wait()` dictionary from the REDUCED vector (numpy fp64), the same on every rank.  A column stays None unless
    a protein of the global batch has a value (a rank with an empty shard reads it too) or this rank `passed` its field (then NaN).
    `tail`: the fields the job asked for - the keys of the tail fields among them exist then, under the same rule."""
    S = _vector_layout(frozenset(tail))[0]
    one = {name: v[at][0] for name, at in VECTOR_SLOTS.items()}          # (the first entry of every slot: for the one-entry slots)
    out = dict(_NO_REPORT, n_proteins=int(one["proteins"]), mse=v[VECTOR_SLOTS["mse"]],
               status=sum(1 << k for k, n in enumerate(v[VECTOR_SLOTS["status_bits"]]) if n > 0),
               n_res=int(one["residues"]) if one["ranks_counted"] > 0 else None)
    out.update(zip(_MEANS, v[VECTOR_SLOTS["sums"]] / max(one["proteins"], 1.0)))
    if one["rmsd_proteins"] > 0:
        out["rmsd"] = one["rmsd_sum"] / one["rmsd_proteins"]
    for f in REPORT_FIELDS:
        if f.name in S:
            total, count = v[S[f.name]].reshape(2, -1)
            out.update({key: total[k] / count[k] if count[k] > 0 else float("nan") if f.name in passed else None
                        for k, key in enumerate(f.keys)})
    return out


class LossReport:
    """The loss statistics of one batch on their way to the host, without draining the stream.

    The reference returns host numbers every step (losses.py:169-172, train.py:64-66).  Here the kernels leave
    per-protein dRMSD statistics [B,8], the six MSE sums, the status word and (evaluation) per-protein RMSDs on the
    device; this object enqueues ONE set of asynchronous copies into a pinned buffer right behind them, records an event,
    and `wait()` - called after the backward pass has been enqueued - blocks on that event only.

    Data parallel: every reported loss is a statistic of the GLOBAL batch, so the ranks first
    SUM-reduce a small fp64 vector (sums over proteins, protein / residue counts, MSE numerators and denominators, status
    flags): every rank then sees the same numbers and takes the same NaN / early-stopping / scheduler decisions.
    `global_mse_sums` is the device tensor the MSE gradient must be normalised with (count of the whole global batch).
    A rank whose shard is empty passes None for everything and still takes part in the reduction.
    """

    def __init__(self, device, stats=None, status=None, mse_sums_local=None, rmsd=None, n_res=None, fields=None):
        """`fields`: {field of REPORT_FIELDS: its per-protein values [B] or [B,k], or None} - what the job reports beside the
        arguments in front.  A key is there on EVERY rank of the job, with None on one that has no value (an empty shard)."""
        fields = dict(fields or {})
        if not REPORT_KEYS.keys() >= fields.keys():
            raise ValueError(f"not a field of a loss report: {sorted(fields.keys() - REPORT_KEYS.keys())}")
        self.world, self.n_res = dp.world_size(), n_res
        if self.world == 1:
            buf, layout = pack_local(stats, mse_sums_local, status, rmsd, fields,
                                     alloc=lambda n: _pinned("report32", n, torch.float32, device))
            self.global_mse_sums = mse_sums_local
            self._unpack = lambda: unpack_local(buf.numpy(), layout, n_res)
        else:
            v = dp.all_reduce_sum_(reduce_vector(stats, mse_sums_local, status, rmsd, n_res, fields, device))
            self.global_mse_sums = v[VECTOR_SLOTS["mse"]].float()
            buf = _pinned("report64", v.numel(), torch.float64, device)
            buf.copy_(v, non_blocking=True)
            passed = {field for field, t in fields.items() if t is not None}
            self._unpack = lambda: unpack_global(buf.numpy().copy(), passed, tuple(fields))
        self._event = torch.cuda.Event()
        self._event.record()

    def wait(self):
        """Block until the copies have landed; returns a dict of host numbers (float64 / int)."""
        self._event.synchronize()
        return self._unpack()


def compute_batch_drmsd(pred_angs, true_crds, input_seqs, device=None, return_rmsd=False,
                        do_backward=False, retain_graph=False, pool=None, backbone_only=False):
    """DRMSD loss of a batch (losses.py:133-172), entirely on the GPU.

    pred_angs [B,L,24] (cos,sin) predictions attached to the model's graph, true_crds [B,L*14,3]
    (NaN = missing atom), input_seqs [B,L].  With do_backward the SUM over proteins of
    d(lndrmsd_i)/d(pred_angs) is back-propagated through pred_angs (losses.py:166-167).
    Returns np.mean over proteins of (drmsd, lndrmsd, bb drmsd, bb lndrmsd[, rmsd]); under data parallelism the means
    are those of the global batch (every rank calls this with its shard).

    `backbone_only` (what losses.py:83-92 means; the reference's own code throws there): loss and gradient are
    those of the backbone atoms N, CA, C alone; the tuple keeps its shape and its first two entries carry the backbone values
    too.  The RMSD of `return_rmsd` is still that of all atoms (one full build beside the backbone path).
    """
    dev = pred_angs.device
    true_crds, input_seqs = true_crds.to(dev), input_seqs.to(dev)
    stats, grad, status, crd = batch_loss(pred_angs, true_crds, input_seqs, do_backward, backbone_only=backbone_only)[:4]
    rmsd = None
    if return_rmsd:
        from .eval_metrics import kabsch_rmsd_batch
        if backbone_only:
            crd, _ = predicted_coords(pred_angs, input_seqs, status=status)
        rmsd = kabsch_rmsd_batch(crd, true_crds, input_seqs)
    # The copy to the host is enqueued right behind the loss kernels and the host waits for THAT copy only after the
    # whole backward pass has been enqueued: waiting on the stream instead would drain the queue at the end of every
    # step and leave the GPU idle while the next launches are being issued.
    report = LossReport(dev, stats=stats, status=status, rmsd=rmsd)
    if do_backward:
        pred_angs.backward(gradient=grad.view_as(pred_angs), retain_graph=retain_graph)
    host = report.wait()
    raise_for_status(host["status"], theta_is_error=False)
    out = (host["drmsd"], host["lndrmsd"], host["drmsd-bb"], host["lndrmsd-bb"])
    if return_rmsd:
        out = out + (host["rmsd"],)
    return out


def drmsd_work(pred_ang, true_crd, input_seq, return_rmsd=False, do_backward=True, backbone_only=False):
    """One protein (losses.py:49-98): returns (grad [L,12] or None, drmsd, lndrmsd, bb, bb_ln[, rmsd]).
    `backbone_only`: gradient and all four numbers are those of the backbone atoms alone (the first pair repeats the second);
    the RMSD is that of all atoms."""
    dev = torch.device("cuda", torch.cuda.current_device())
    ang = torch.as_tensor(np.asarray(pred_ang) if not torch.is_tensor(pred_ang) else pred_ang).to(dev, torch.float32)[None]
    crd_t = torch.as_tensor(np.asarray(true_crd) if not torch.is_tensor(true_crd) else true_crd).to(dev, torch.float32)[None]
    seq = torch.as_tensor(np.asarray(input_seq) if not torch.is_tensor(input_seq) else input_seq).to(dev, torch.int64)[None]
    crd, status = nerf_forward(ang.contiguous(), seq, backbone_only=backbone_only)
    stats, dcrd = drmsd_forward_backward(crd, crd_t, seq, need_grad=do_backward, backbone_only=backbone_only)
    grad = nerf_backward(ang.contiguous(), seq, crd, dcrd, backbone_only=backbone_only)[0].cpu() if do_backward else None
    raise_for_status(int(status.item()), theta_is_error=False)
    s = stats[0].cpu().numpy().astype(np.float64)
    out = (grad, float(s[0]), float(s[1]), float(s[2]), float(s[3]))
    if return_rmsd:
        from .eval_metrics import kabsch_rmsd_batch
        if backbone_only:
            crd, _ = nerf_forward(ang.contiguous(), seq)
        out = out + (float(kabsch_rmsd_batch(crd, crd_t, seq)[0]),)
    return out


# ----------------------------------------------------------------------------- angle MSE
def mse_sums(pred, true):
    """One pass over [B,L,24]: device tensor [6] = (sum, count) for full / backbone / side-chain columns, i.e. the three
    variants get_losses asks for back to back (train.py:64-66).  No host synchronisation."""
    _lib.require_gpu(pred, true)
    T = pred.shape[0] * pred.shape[1]
    out = torch.empty(6, dtype=torch.float32, device=pred.device)
    ws = _lib.workspace("mse_angles", _lib.lib().ptamd_mse_angles_workspace_bytes(), pred.device)
    rc = _lib.lib().ptamd_mse_angles_fwd(_lib.ptr(pred.detach().float().contiguous()),
                                         _lib.ptr(true.float().contiguous()), T, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                         _lib.stream())
    _lib.check(rc, "mse_angles_fwd")
    return out


def mse_grad(pred, true, sums, coef=1.0, accumulate_into=None):
    """d(coef * mse_full)/d(pred) = coef * 2 (pred - true) / count on the selected elements, where count = sums[1] is
    read ON THE DEVICE (under data parallelism it is the count of the global batch, so the SUM of the ranks' parameter
    gradients is the gradient of the global mean).  `accumulate_into`: add to that [B,L,24] tensor instead of a new one."""
    T = pred.shape[0] * pred.shape[1]
    acc = accumulate_into is not None
    dpred = accumulate_into if acc else torch.empty(pred.shape, dtype=torch.float32, device=pred.device)
    assert dpred.is_contiguous()
    rc = _lib.lib().ptamd_mse_angles_bwd(_lib.ptr(pred.detach().float().contiguous()), _lib.ptr(true.float().contiguous()),
                                         T, _lib.ptr(sums), float(coef), int(acc), _lib.ptr(dpred), _lib.stream())
    _lib.check(rc, "mse_angles_bwd")
    return dpred


class _MseFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, true, which):
        sums = mse_sums(pred, true)
        ctx.save_for_backward(pred, true, sums)
        ctx.which = which
        return sums[2 * which] / sums[2 * which + 1]

    @staticmethod
    def backward(ctx, g):
        pred, true, sums = ctx.saved_tensors
        if ctx.which != 0:
            raise NotImplementedError("only the full-angle MSE is ever differentiated (train.py:86,97)")
        # API-parity path (a host read of the incoming scalar); the training step uses mse_grad directly
        return mse_grad(pred, true, sums, coef=float(g)).view_as(pred), None, None


def mse_over_angles(pred, true, bb_only=False, sc_only=False):
    """Mean squared error over (cos, sin) values with batch padding (all-zero rows) and missing
    angles (NaN) removed (losses.py:175-214).  Returns a 0-d device tensor."""
    assert len(pred.shape) == 3, "This function must operate on a batch of angles."
    if pred.shape[-1] != NUM_PREDICTED_ANGLES * 2:
        raise Exception("Unknown angle tensor shape.")
    which = 1 if bb_only else (2 if sc_only else 0)
    return _MseFn.apply(pred, true.to(pred.device), which)
