"""A trained pLDDT head: per-residue confidence out of the one deterministic pass of a frozen encoder.

    python -m protein_transformer_amd.confidence fit CHECKPOINT (--data DATA.pt | --synthetic B,L,n) --out CHECKPOINT2
                                                 [--epochs 1] [--lr 1e-3] [--batch_size 32] [--seed 0] [--hidden 128] [--nbins 50]
                                                 [--split train]
    python -m protein_transformer_amd.confidence calibrate CHECKPOINT (--data DATA.pt | --synthetic B,L,n) [--samples 0] [--seed 0]
                                                 [--batch_size 32] [--split test] [--pae]
    python -m protein_transformer_amd.confidence fit-pae CHECKPOINT (--data DATA.pt | --synthetic B,L,n) --out CHECKPOINT2
                                                 [--epochs 1] [--lr 1e-3] [--batch_size 32] [--seed 0] [--hidden 32] [--nbins 64]
                                                 [--split train]

The head is the one of AlphaFold 2 (Jumper et al., Nature 596:583-589 (2021), supplementary 1.9.6): LayerNorm -> Linear(d -> hidden)
-> ReLU -> Linear(hidden -> nbins) on the encoder's last hidden state (`model.keep_hidden`, models/encoder_only.py), a softmax over
nbins equal bins of [0, 1], trained by cross-entropy against the bin of the per-residue lDDT-C-alpha (cutoff 15 A,
`eval_metrics.lddt_batch`) of the model's OWN prediction against the truth; the pLDDT of a residue is 100 x the expected bin centre.
The reference (protein_transformer) has no counterpart.  The encoder stays frozen: the head reads a detached hidden state of a
`model.eval()` pass under `no_grad`, nothing of the model is written, and `train.py` knows nothing of the head.

`fit` writes CHECKPOINT2 = the input checkpoint's dictionary, unchanged, plus one top-level key `confidence_head` = {"state_dict",
"settings"}; `python -m protein_transformer_amd.predict CHECKPOINT2 SEQS.fasta --out DIR --plddt` reads it.  Readers that do not know
the key (`predict.load_checkpoint`, `train.load_model`) behave as before.  RESUMING TRAINING FROM CHECKPOINT2 AND CHECKPOINTING AGAIN
DROPS THE HEAD (`train.checkpoint_model` writes its own dictionary): a head belongs to the weights it was fitted on, and is fitted
again after them.

`calibrate` measures how well a score tracks the true lDDT-C-alpha on data with known structures: the head's pLDDT and, with
`--samples K` >= 1, the dropout ensemble's `conf` (ensemble.py) - n, Pearson r, mean absolute error, bias and a ten-row reliability
table per score, as one JSON object.

`fit-pae` fits the PAIR head (`PaeHead`; AlphaFold 2's aligned-error head, supplementary 1.9.7, without relative-position
features): LayerNorm -> Linear(d -> 2 hidden) = a frame side u and a point side v per residue, per pair relu(u_i + v_j) ->
Linear(hidden -> nbins), a softmax over nbins bins of 0.5 A (the last one open), trained by cross-entropy against the bin of the
TRUE aligned error of the model's own prediction (`ensemble.aligned_error`, the truth as the reference).  The pair part is
csrc/pae_head.hip: no L x L x nbins tensor is ever stored.  The head is written under the top-level key `pae_head`, beside a
`confidence_head` if there is one (and `fit` keeps a `pae_head`); `predict --ptm` reads it: the expected error per pair, its mean
`pae`, and `ptm`, the pTM formula applied to the head's predicted distribution of errors.  `calibrate --pae` adds "pae" (per pair,
against the true aligned error), "ptm" (100 x, per protein, against 100 x the true matrix's tm) and, with `--samples K` >= 1,
"ens-pae" and "ens-ptm" of the dropout samples against the same truth.  HOW WELL `ptm` IS CALIBRATED ON A REALLY TRAINED MODEL HAS
NOT BEEN MEASURED BY ANYONE: this is only the tool that measures it.

Forward and backward of the head are written out on the library's kernels (kernels.py: LayerNorm, GEMM with its ReLU epilogue, the
ReLU backward, the weight- and input-gradient products; csrc/plddt.hip for the binned loss), the products in the three-term bf16
arithmetic (fp32-grade; the two-term f16 arithmetic needs scales nobody computes here), the step is `grad_sqnorm` + `adam_step` on
the head's flat buffers.  There is no CPU path.
"""
import argparse
import json
import math
import sys

import numpy as np
import torch

from . import _lib, kernels as K

LDDT_CUTOFF = 15.0
NAMES = ("ln.gamma", "ln.beta", "w1", "b1", "w2", "b2")


def plddt_fwd(logits, nbins, target=None, target_stride=1):
    """logits [T, ld >= nbins] device fp32 -> (plddt [T], ce [T] or None, sums [2] or None) (csrc/plddt.hip; include/ptamd.h).
    `target`: a 1-D view whose element t * target_stride is the true lDDT of row t (NaN: the row does not count); None: inference."""
    _lib.require_gpu(logits, target)
    T, ld = logits.shape[0], logits.stride(0)
    dev = logits.device
    plddt = torch.empty(T, dtype=torch.float32, device=dev)
    ce = sums = ws = None
    if target is not None:
        assert target.dtype == torch.float32 and target.dim() == 1 and target.stride(0) == 1
        assert target.numel() >= (T - 1) * target_stride + 1
        ce = torch.empty(T, dtype=torch.float32, device=dev)
        sums = torch.empty(2, dtype=torch.float32, device=dev)
        ws = _lib.workspace("plddt", _lib.lib().ptamd_plddt_workspace_bytes(T), dev)
    rc = _lib.lib().ptamd_plddt_fwd(_lib.ptr(logits), ld, _lib.ptr(target), int(target_stride), T, int(nbins), _lib.ptr(plddt),
                                    _lib.ptr(ce), _lib.ptr(sums), _lib.ptr(ws), ws.numel() if ws is not None else 0, _lib.stream())
    _lib.check(rc, "plddt_fwd")
    return plddt, ce, sums


def plddt_bwd(logits, nbins, target, target_stride, sums, coef=1.0, ldd=None):
    """d(coef x mean ce)/d(logits) as [T, ldd] (default: the stride of `logits`), exactly 0 in the spare columns and in rows that
    do not count; `sums` is read on the device."""
    T = logits.shape[0]
    ldd = logits.stride(0) if ldd is None else int(ldd)
    dlogits = torch.empty(T, ldd, dtype=torch.float32, device=logits.device)
    rc = _lib.lib().ptamd_plddt_bwd(_lib.ptr(logits), logits.stride(0), _lib.ptr(target), int(target_stride), T, int(nbins),
                                    _lib.ptr(sums), float(coef), _lib.ptr(dlogits), ldd, _lib.stream())
    _lib.check(rc, "plddt_bwd")
    return dlogits


class ConfidenceHead:
    """LayerNorm -> Linear(d_in -> hidden) -> ReLU -> Linear(hidden -> nbins).  Parameters and gradients each live in ONE flat fp32
    buffer (`flat`, `grad`); `params[name]` / `grads[name]` are the views ln.gamma, ln.beta, w1 [hidden, d_in], b1, w2 [nbins,
    hidden], b2.  The last layer is stored with pad4(nbins) rows - the products read K-contiguous rows 16 bytes at a time, so the
    logits and their gradient are [T, pad4(nbins)] -; the spare rows are zero, get a zero gradient (csrc/plddt.hip writes 0 into
    the spare gradient columns) and so stay zero under Adam without weight decay.  The last layer starts at zero: an unfitted head
    gives CE = ln(nbins) and pLDDT = 50 on every row."""

    def __init__(self, d_in, hidden=128, nbins=50, device=None, seed=0):
        d_in, hidden, nbins = int(d_in), int(hidden), int(nbins)
        if d_in < 4 or d_in % 4 or d_in > 2048 or hidden < 4 or hidden % 4 or not 2 <= nbins <= 64:
            raise ValueError("ConfidenceHead: d_in and hidden must be multiples of 4 (d_in <= 2048), nbins in 2 .. 64")
        self.d_in, self.hidden, self.nbins, self.nbp = d_in, hidden, nbins, K.pad4(nbins)
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        shapes = {"ln.gamma": (d_in,), "ln.beta": (d_in,), "w1": (hidden, d_in), "b1": (hidden,), "w2": (self.nbp, hidden),
                  "b2": (self.nbp,)}
        self._layout, off = {}, 0
        for name in NAMES:                                        # (every extent is a multiple of 4 floats: 16-byte offsets)
            self._layout[name] = (off, shapes[name])
            off += int(np.prod(shapes[name]))
        init = torch.zeros(off, dtype=torch.float32)
        g = torch.Generator().manual_seed(int(seed))
        bound = math.sqrt(6.0 / (d_in + hidden))                  # xavier_uniform, as the encoder's matrices
        o = self._layout["w1"][0]
        init[o:o + hidden * d_in] = (torch.rand(hidden * d_in, generator=g, dtype=torch.float64) * 2 - 1).float() * bound
        init[self._layout["ln.gamma"][0]:][:d_in] = 1.0
        self.flat = init.to(self.device)
        self.grad = torch.zeros_like(self.flat)
        self._m, self._v = torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self._sqnorm = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.steps = 0
        self.arith = K.GEMM_BF16X3
        self._padded = {n: self._views(self.flat, n, pad=True) for n in NAMES}
        self._gpadded = {n: self._views(self.grad, n, pad=True) for n in NAMES}
        self.params = {n: self._views(self.flat, n) for n in NAMES}
        self.grads = {n: self._views(self.grad, n) for n in NAMES}
        self._saved = None

    def _views(self, buf, name, pad=False):
        off, shape = self._layout[name]
        v = buf[off:off + int(np.prod(shape))].view(shape)
        return v if pad or name not in ("w2", "b2") else v[:self.nbins]

    def settings(self):
        return {"d_in": self.d_in, "hidden": self.hidden, "nbins": self.nbins, "lddt_cutoff": LDDT_CUTOFF, "steps": self.steps}

    def state_dict(self):
        return {n: v.detach().cpu().clone() for n, v in self.params.items()}

    def load_state_dict(self, state):
        if set(state) != set(NAMES):
            raise ValueError(f"confidence head: expected the parameters {NAMES}, got {tuple(state)}")
        for n, v in self.params.items():
            if tuple(state[n].shape) != tuple(v.shape):
                raise ValueError(f"confidence head: {n} is {tuple(state[n].shape)}, this head has {tuple(v.shape)}")
            v.copy_(state[n].to(self.device, torch.float32))

    # ------------------------------------------------------------------ forward / backward / step
    def forward(self, x, target=None, target_stride=1):
        """x [T, d_in] (a detached hidden state) -> (plddt [T], ce [T] or None, sums [2] or None); with a target the activations
        are kept for `backward`."""
        _lib.require_gpu(x)
        if x.dim() != 2 or x.shape[1] != self.d_in or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError(f"ConfidenceHead.forward: x must be a contiguous fp32 [T, {self.d_in}] tensor")
        P = self._padded
        y, mean, rstd = K.layernorm_fwd(x, P["ln.gamma"], P["ln.beta"])
        h = K.linear_fwd(y, P["w1"], P["b1"], flags=K.EPI_RELU, arith=self.arith)
        logits = K.linear_fwd(h, P["w2"], P["b2"], arith=self.arith)                  # [T, pad4(nbins)], the spare columns 0
        out = plddt_fwd(logits, self.nbins, target, target_stride)
        self._saved = (x, y, mean, rstd, h, logits, target, target_stride, out[2]) if target is not None else None
        self.logits = logits
        return out

    def backward(self, coef=1.0):
        """The gradient of coef x (mean CE over the counted rows) of the last `forward` with a target, into `grad` (overwritten)."""
        if self._saved is None:
            raise RuntimeError("ConfidenceHead.backward: no forward pass with a target to differentiate")
        x, y, mean, rstd, h, logits, target, stride, sums = self._saved
        self._saved = None
        P, G = self._padded, self._gpadded
        K.fill_u32([(self.grad, 0)])                                                    # the products below accumulate
        dlogits = plddt_bwd(logits, self.nbins, target, stride, sums, coef)
        K.linear_bwd_weight(dlogits, h, G["w2"], G["b2"], arith=self.arith)
        dh = K.linear_bwd_input(dlogits, P["w2"], arith=self.arith)
        dz = K.relu_dropout_bwd(dh, h, 0.0)
        K.linear_bwd_weight(dz, y, G["w1"], G["b1"], arith=self.arith)
        dy = K.linear_bwd_input(dz, P["w1"], arith=self.arith)
        K.layernorm_bwd(dy, x, P["ln.gamma"], mean, rstd, G["ln.gamma"], G["ln.beta"])   # (dx is dropped: the encoder is frozen)
        return self.grad

    def step(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, clip=1.0):
        """Clip the gradient to the norm `clip` (0: no clipping) and take one Adam step; no host synchronisation."""
        self.steps += 1
        K.grad_sqnorm(self.grad, self._sqnorm)
        K.adam_step(self.flat, self.grad, self._m, self._v, self._sqnorm, float(clip or 0.0), lr, betas[0], betas[1], eps, 0.0,
                    self.steps)


# ---------------------------------------------------------------------- the pair head
def pae_head_fwd(uv, w2, b2, seq, bins_per_angstrom, target=None):
    """uv [B*L, >= 2H] device fp32 (u | v per residue), w2 [nbins, H], b2 [nbins], seq [B, L] int64 -> (pae [B,L,L], stats [B,2] =
    {mean, ptm}, sums [2] or None) (csrc/pae_head.hip; include/ptamd.h).  `target` [B,L,L] contiguous fp32: the true aligned
    error (NaN: the pair does not count); None: inference, and then no workspace is used."""
    _lib.require_gpu(uv, w2, b2, seq, target)
    (B, L), (nbins, H), dev = seq.shape, w2.shape, uv.device
    assert uv.shape[0] == B * L and seq.dtype == torch.int64 and seq.is_contiguous() and w2.is_contiguous()
    pae = torch.empty(B, L, L, dtype=torch.float32, device=dev)
    stats = torch.empty(B, 2, dtype=torch.float32, device=dev)
    sums = ws = None
    if target is not None:
        assert target.dtype == torch.float32 and target.shape == (B, L, L) and target.is_contiguous()
        sums = torch.empty(2, dtype=torch.float32, device=dev)
        ws = _lib.workspace("pae_head", _lib.lib().ptamd_pae_head_workspace_bytes(B, L, H, nbins), dev)
    rc = _lib.lib().ptamd_pae_head_fwd(_lib.ptr(uv), uv.stride(0), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(seq), _lib.ptr(target), B, L,
                                       H, nbins, float(bins_per_angstrom), _lib.ptr(pae), _lib.ptr(stats), _lib.ptr(sums),
                                       _lib.ptr(ws), ws.numel() if ws is not None else 0, _lib.stream())
    _lib.check(rc, "pae_head_fwd")
    return pae, stats, sums


def pae_head_bwd(uv, w2, b2, seq, bins_per_angstrom, target, sums, dw2, db2, coef=1.0):
    """d(coef x mean CE)/d(uv) as [B*L, 2H]; d/d(w2) and d/d(b2) are written into `dw2` and `db2`; `sums` is read on the device."""
    (B, L), (nbins, H), dev = seq.shape, w2.shape, uv.device
    duv = torch.empty(B * L, 2 * H, dtype=torch.float32, device=dev)
    ws = _lib.workspace("pae_head", _lib.lib().ptamd_pae_head_workspace_bytes(B, L, H, nbins), dev)
    rc = _lib.lib().ptamd_pae_head_bwd(_lib.ptr(uv), uv.stride(0), _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(seq), _lib.ptr(target), B, L,
                                       H, nbins, float(bins_per_angstrom), _lib.ptr(sums), float(coef), _lib.ptr(duv), 2 * H,
                                       _lib.ptr(dw2), _lib.ptr(db2), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "pae_head_bwd")
    return duv


class PaeHead:
    """LayerNorm -> Linear(d_in -> 2 hidden) = (u | v) per residue, then per pair relu(u_i + v_j) -> Linear(hidden -> nbins) and a
    softmax over bins of 1 / bins_per_angstrom A (the last one open): the aligned-error head of AlphaFold 2 (supplementary 1.9.7)
    without relative-position features.  The same flat `flat` / `grad` / Adam buffers and parameter names as `ConfidenceHead`:
    ln.gamma, ln.beta, w1 [2 hidden, d_in], b1 [2 hidden], w2 [nbins, hidden], b2 [nbins] (no spare rows: the pair kernel reads
    w2, the products do not).  The last layer starts at zero: an unfitted head gives CE = ln(nbins) on every pair."""

    def __init__(self, d_in, hidden=32, nbins=64, bins_per_angstrom=2.0, device=None, seed=0):
        d_in, hidden, nbins, bpa = int(d_in), int(hidden), int(nbins), float(bins_per_angstrom)
        if d_in < 4 or d_in % 4 or d_in > 2048 or not 4 <= hidden <= 64 or hidden % 4 or not 2 <= nbins <= 64:
            raise ValueError("PaeHead: d_in a multiple of 4 (<= 2048), hidden a multiple of 4 in 4 .. 64, nbins in 2 .. 64")
        if not (math.isfinite(bpa) and bpa > 0):
            raise ValueError("PaeHead: bins_per_angstrom must be finite and positive")
        self.d_in, self.hidden, self.nbins, self.bins_per_angstrom = d_in, hidden, nbins, bpa
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        shapes = {"ln.gamma": (d_in,), "ln.beta": (d_in,), "w1": (2 * hidden, d_in), "b1": (2 * hidden,), "w2": (nbins, hidden),
                  "b2": (nbins,)}
        self._layout, off = {}, 0
        for name in NAMES:                                        # (b2 is the last one: every offset is a multiple of 4 floats)
            self._layout[name] = (off, shapes[name])
            off += int(np.prod(shapes[name]))
        init = torch.zeros(K.pad4(off), dtype=torch.float32)
        g = torch.Generator().manual_seed(int(seed))
        bound = math.sqrt(6.0 / (d_in + 2 * hidden))              # xavier_uniform, as the encoder's matrices
        o = self._layout["w1"][0]
        init[o:o + 2 * hidden * d_in] = (torch.rand(2 * hidden * d_in, generator=g, dtype=torch.float64) * 2 - 1).float() * bound
        init[self._layout["ln.gamma"][0]:][:d_in] = 1.0
        self.flat = init.to(self.device)
        self.grad = torch.zeros_like(self.flat)
        self._m, self._v = torch.zeros_like(self.flat), torch.zeros_like(self.flat)
        self._sqnorm = torch.zeros(1, dtype=torch.float32, device=self.device)
        self.steps = 0
        self.arith = K.GEMM_BF16X3
        self.params = {n: self._views(self.flat, n) for n in NAMES}
        self.grads = {n: self._views(self.grad, n) for n in NAMES}
        self._saved = None

    def _views(self, buf, name):
        off, shape = self._layout[name]
        return buf[off:off + int(np.prod(shape))].view(shape)

    def settings(self):
        return {"d_in": self.d_in, "hidden": self.hidden, "nbins": self.nbins, "bins_per_angstrom": self.bins_per_angstrom,
                "steps": self.steps}

    def top(self):
        """The upper end of the last bin if it were closed: no entry of `pae` is above it."""
        return self.nbins / self.bins_per_angstrom

    state_dict = ConfidenceHead.state_dict
    step = ConfidenceHead.step

    def load_state_dict(self, state):
        if set(state) != set(NAMES):
            raise ValueError(f"PAE head: expected the parameters {NAMES}, got {tuple(state)}")
        for n, v in self.params.items():
            if tuple(state[n].shape) != tuple(v.shape):
                raise ValueError(f"PAE head: {n} is {tuple(state[n].shape)}, this head has {tuple(v.shape)}")
            v.copy_(state[n].to(self.device, torch.float32))

    def forward(self, x, seq, target=None):
        """x [B*L, d_in] (a detached hidden state), seq [B, L] -> (pae [B,L,L], stats [B,2] = {mean, ptm}, sums [2] or None); with
        a target [B,L,L] (the true aligned error, NaN where a pair does not count) the activations are kept for `backward`."""
        _lib.require_gpu(x, seq)
        B, L = seq.shape
        if x.dim() != 2 or x.shape != (B * L, self.d_in) or x.dtype != torch.float32 or not x.is_contiguous():
            raise ValueError(f"PaeHead.forward: x must be a contiguous fp32 [B * L, {self.d_in}] tensor")
        seq = seq.to(torch.int64).contiguous()
        P = self.params
        y, mean, rstd = K.layernorm_fwd(x, P["ln.gamma"], P["ln.beta"])
        uv = K.linear_fwd(y, P["w1"], P["b1"], arith=self.arith)                      # [B*L, 2 hidden]: no ReLU here
        out = pae_head_fwd(uv, P["w2"], P["b2"], seq, self.bins_per_angstrom, target)
        self._saved = (x, y, mean, rstd, uv, seq, target, out[2]) if target is not None else None
        return out

    def backward(self, coef=1.0):
        """The gradient of coef x (mean CE over the counted pairs) of the last `forward` with a target, into `grad` (overwritten)."""
        if self._saved is None:
            raise RuntimeError("PaeHead.backward: no forward pass with a target to differentiate")
        x, y, mean, rstd, uv, seq, target, sums = self._saved
        self._saved = None
        P, G = self.params, self.grads
        K.fill_u32([(self.grad, 0)])                                                    # the products below accumulate
        duv = pae_head_bwd(uv, P["w2"], P["b2"], seq, self.bins_per_angstrom, target, sums, G["w2"], G["b2"], coef)
        K.linear_bwd_weight(duv, y, G["w1"], G["b1"], arith=self.arith)
        dy = K.linear_bwd_input(duv, P["w1"], arith=self.arith)
        K.layernorm_bwd(dy, x, P["ln.gamma"], mean, rstd, G["ln.gamma"], G["ln.beta"])   # (dx is dropped: the encoder is frozen)
        return self.grad


# ---------------------------------------------------------------------- the encoder's side
def hidden_state(model, seq):
    """One deterministic (`model.eval()`, `no_grad`) pass: (pred [B,L,24], last hidden state [B*L, d], seq on the device).  The
    model is handed back as it was found (`ensemble._Borrowed`), `keep_hidden` and the absence of `last_hidden` included."""
    from .ensemble import _Borrowed
    with _Borrowed(model) as m, torch.no_grad():
        m.eval()
        m.keep_hidden = True
        pred = m(seq)
        x = m.__dict__.pop("last_hidden")
    return pred, x, seq.to(pred.device, torch.int64).contiguous()


def hidden_and_target(model, seq, true_crd):
    """What a fitting step reads of a batch: (hidden [B*L, d], target) - target a 1-D view whose element 2 t is the lDDT-C-alpha of
    residue t of the model's own prediction against `true_crd`, read in place from the per-residue table of `lddt_batch` (stride
    2), NaN for absent residues and padding.  Everything stays on the device."""
    from .eval_metrics import lddt_batch
    from .losses import predicted_coords
    pred, x, seq = hidden_state(model, seq)
    with torch.no_grad():
        crd, _ = predicted_coords(pred, seq)
        per_res = lddt_batch(crd, true_crd.to(crd.device), seq, cutoff=LDDT_CUTOFF)[1]          # [B, L, 2] = {all-atom, C-alpha}
    return x, per_res.view(-1)[1:]


def mask_padding(plddt, seq):
    """[B*L] -> [B, L], NaN where `seq` holds no residue."""
    B, L = seq.shape
    return torch.where((seq >= 0) & (seq < 20), plddt.view(B, L), torch.full_like(plddt.view(B, L), float("nan")))


def predict_plddt(model, head, seq):
    """seq [B, L] residue ids with trailing padding -> pLDDT [B, L] on the device, NaN on padding: one deterministic pass of the
    encoder and the head on its last hidden state.  The model is left as it was found."""
    _, x, seq = hidden_state(model, seq)
    return mask_padding(head.forward(x)[0], seq)


def fit_head(model, batches, head=None, epochs=1, lr=1e-3, seed=0, hidden=128, nbins=50, clip=1.0, log=None):
    """Fit a head on a frozen model.  batches: a sequence of (seq [B,L], ..., true_crd [B,L*14,3]) tuples (first and last element
    are read; NaN truth = absent atom).  Per batch: the deterministic pass, its last hidden state, the lDDT-C-alpha of its own
    prediction as the target, then head forward, loss, backward and one Adam step.  `log` is called with one dict per epoch:
    {"epoch", "ce" (mean over the counted residues of the epoch), "residues", "steps"}.  Returns (head, [those dicts]).  Two calls
    with the same arguments give the same bits."""
    dev = next(model.parameters()).device
    if head is None:
        head = ConfidenceHead(model.dlayer, hidden, nbins, device=dev, seed=seed)
    history = []
    for epoch in range(int(epochs)):
        sums = []
        for batch in batches:
            x, target = hidden_and_target(model, batch[0].to(dev), batch[-1])
            sums.append(head.forward(x, target, 2)[2])
            head.backward()
            head.step(lr=lr, clip=clip)
        s = torch.stack(sums).double().cpu().numpy()                                        # one read back per epoch
        n = float(s[:, 1].sum())
        ce = float(np.nansum(s[:, 0] * s[:, 1]) / n) if n > 0 else float("nan")
        history.append({"epoch": epoch, "ce": ce, "residues": int(n), "steps": head.steps})
        if log is not None:
            log(history[-1])
    return head, history


def hidden_and_aligned_error(model, seq, true_crd):
    """What a fitting step of the pair head reads of a batch: (hidden [B*L, d], seq [B,L] int64, target [B,L,L]) - target the true
    aligned error of the model's own prediction, the call `score --aligned_error` makes (`ensemble.aligned_error` with the truth as
    the reference and the prediction as its one sample), read in place; NaN where it is undefined.  Everything stays on the
    device."""
    from .ensemble import aligned_error
    from .losses import predicted_coords
    pred, x, seq = hidden_state(model, seq)
    with torch.no_grad():
        crd, _ = predicted_coords(pred, seq)
        ae = aligned_error(true_crd.to(crd.device), crd[:, None], seq)[0]
    return x, seq, ae


def fit_pae_head(model, batches, head=None, epochs=1, lr=1e-3, seed=0, hidden=32, nbins=64, bins_per_angstrom=2.0, clip=1.0,
                 log=None):
    """`fit_head` for the pair head: per batch the deterministic pass, its last hidden state, the true aligned error of its own
    prediction as the target, then head forward, loss, backward and one Adam step.  `log` is called with one dict per epoch:
    {"epoch", "ce" (mean over the counted pairs of the epoch), "pairs", "steps"}.  Returns (head, [those dicts]); one read back
    per epoch.  Two calls with the same arguments give the same bits."""
    dev = next(model.parameters()).device
    if head is None:
        head = PaeHead(model.dlayer, hidden, nbins, bins_per_angstrom, device=dev, seed=seed)
    history = []
    for epoch in range(int(epochs)):
        sums = []
        for batch in batches:
            x, seq, target = hidden_and_aligned_error(model, batch[0].to(dev), batch[-1])
            sums.append(head.forward(x, seq, target)[2])
            head.backward()
            head.step(lr=lr, clip=clip)
        s = torch.stack(sums).double().cpu().numpy()                                        # one read back per epoch
        n = float(s[:, 1].sum())
        ce = float(np.nansum(s[:, 0] * s[:, 1]) / n) if n > 0 else float("nan")
        history.append({"epoch": epoch, "ce": ce, "pairs": int(n), "steps": head.steps})
        if log is not None:
            log(history[-1])
    return head, history


# ---------------------------------------------------------------------- checkpoints
HEAD_KEY, PAE_HEAD_KEY = "confidence_head", "pae_head"


def read_head_entries(path):
    """(`confidence_head`, `pae_head`) of a checkpoint, None for one it does not have - read on the CPU, no device needed."""
    try:
        ck = torch.load(path, map_location="cpu", weights_only=False)
        ck["model_state_dict"]
    except Exception as e:
        what = " ".join(f"{type(e).__name__}: {e}".split())
        raise ValueError(f"{path}: not a checkpoint of train.checkpoint_model ({what})") from None
    return ck.get(HEAD_KEY), ck.get(PAE_HEAD_KEY)


def pae_head_from_entry(entry, device=None):
    s = entry["settings"]
    head = PaeHead(s["d_in"], s["hidden"], s["nbins"], s["bins_per_angstrom"], device=device)
    head.load_state_dict(entry["state_dict"])
    head.steps = int(s.get("steps", 0))
    return head


def read_head_entry(path):
    """The `confidence_head` entry of a checkpoint, or None when it has none - read on the CPU, no device needed."""
    return read_head_entries(path)[0]


def head_from_entry(entry, device=None):
    s = entry["settings"]
    head = ConfidenceHead(s["d_in"], s["hidden"], s["nbins"], device=device)
    head.load_state_dict(entry["state_dict"])
    head.steps = int(s.get("steps", 0))
    return head


def load_head(path, device=None):
    """The head of a checkpoint written by `fit`, on `device`; None when the checkpoint has none."""
    entry = read_head_entry(path)
    return None if entry is None else head_from_entry(entry, device)


def save_with_head(src, dst, head, key=HEAD_KEY):
    """dst = the dictionary of checkpoint `src`, unchanged, plus the top-level key `confidence_head` (`pae_head` for the pair
    head); whatever other head `src` holds survives."""
    ck = torch.load(src, map_location="cpu", weights_only=False)
    ck[key] = {"state_dict": head.state_dict(), "settings": head.settings()}
    torch.save(ck, dst)


# ---------------------------------------------------------------------- calibration
def calibration(score, truth, top=100.0):
    """score, truth: arrays on the scale 0 .. `top` (100: lDDT, pLDDT, 100 x pTM; nbins / bins_per_angstrom A: aligned errors) ->
    dict(n, pearson, mae, bias, reliability) over the entries where both are finite.  bias = mean(score - truth), mae =
    mean |score - truth|; pearson is None where it is undefined (n < 2, a constant score or a constant truth).  reliability: ten
    rows, one per tenth [i top / 10, (i + 1) top / 10) of the SCORE's scale (the last one closed at `top`, scores outside
    0 .. top clamped into the end rows): {"lo", "hi", "n", "mean_truth" (None for an empty row)} - a calibrated score has
    mean_truth inside [lo, hi].  With top = 100 the edges are the integers 0, 10, .. 100, as they always were; any other top
    gives floats.  Pure numpy, fp64."""
    score, truth = np.asarray(score, np.float64).reshape(-1), np.asarray(truth, np.float64).reshape(-1)
    if score.shape != truth.shape:
        raise ValueError("calibration: score and truth differ in size")
    ok = np.isfinite(score) & np.isfinite(truth)
    s, t = score[ok], truth[ok]
    n = int(s.size)
    out = {"n": n, "pearson": None, "mae": None, "bias": None}
    if n:
        out["mae"], out["bias"] = float(np.abs(s - t).mean()), float((s - t).mean())
        ds, dt = s - s.mean(), t - t.mean()
        den = math.sqrt(float((ds * ds).sum()) * float((dt * dt).sum()))
        if n >= 2 and den > 0:
            out["pearson"] = float((ds * dt).sum() / den)
    step = float(top) / 10.0
    edge = (lambda i: 10 * i) if float(top) == 100.0 else (lambda i: step * i)
    row = np.clip(np.floor(s / step), 0, 9).astype(np.int64)
    out["reliability"] = [{"lo": edge(i), "hi": edge(i + 1), "n": int((row == i).sum()),
                           "mean_truth": float(t[row == i].mean()) if (row == i).any() else None} for i in range(10)]
    return out


def calibrate(model, head, batches, samples=0, seed=0, pae_head=None, pae=False):
    """For every residue with a finite true lDDT-C-alpha (x 100): the head's pLDDT (head not None) and, with samples >= 1, the
    ensemble's `conf`, through `calibration` -> {"plddt": {...}, "ens-lddt": {...}} (the scores that were asked for).  One read
    back per batch.  `pae`: also, against the TRUE aligned error of the written structure (`ensemble.aligned_error`, the truth as
    the reference) - "pae", the pair head's entries per pair on the scale 0 .. nbins / bins_per_angstrom, and "ptm", 100 x its pTM
    against 100 x the true matrix's tm per protein (pae_head not None); with samples >= 1 "ens-pae" (per pair, on the pair head's
    scale, 32 A without one) and "ens-ptm" of the dropout samples on the same truth.  One further read back per batch."""
    from .ensemble import aligned_error, predict_ensemble
    from .eval_metrics import lddt_batch
    K_ = int(samples)
    if head is None and K_ < 1 and not (pae and pae_head is not None):
        raise ValueError("calibrate: no head and no samples - there is no score to calibrate")
    dev = next(model.parameters()).device
    cols = {"truth": [], "plddt": [], "ens-lddt": []}
    pcols = {"truth": [], "pae": [], "ens-pae": [], "tm": [], "ptm": [], "ens-ptm": []}
    for batch in batches:
        seq = batch[0].to(dev)
        ens = predict_ensemble(model, seq, samples=K_, seed=seed, aligned_error=bool(pae) and K_ >= 1,
                               hidden=head is not None or (pae and pae_head is not None))
        seq = seq.to(torch.int64).contiguous()
        truth = 100.0 * lddt_batch(ens.crd, batch[-1].to(dev), seq, cutoff=LDDT_CUTOFF)[1][:, :, 1]
        fields = [("truth", truth)]
        if head is not None:
            fields.append(("plddt", mask_padding(head.forward(ens.hidden)[0], seq)))
        if K_ >= 1:
            fields.append(("ens-lddt", ens.conf))
        host = torch.stack([f for _, f in fields]).cpu().numpy()                            # one read back
        ok = np.isfinite(host[0])
        for (name, _), values in zip(fields, host):
            cols[name].append(values[ok])
        if not pae:
            continue
        B = seq.shape[0]
        true_ae, true_stats, _ = aligned_error(batch[-1].to(dev), ens.crd[:, None], seq)
        pairs, prots = [("truth", true_ae)], [("tm", true_stats[:, 1])]
        if pae_head is not None:
            head_pae, head_stats, _ = pae_head.forward(ens.hidden, seq)
            pairs.append(("pae", head_pae))
            prots.append(("ptm", head_stats[:, 1]))
        if K_ >= 1:
            pairs.append(("ens-pae", ens.ae))
            prots.append(("ens-ptm", ens.ae_stats[:, 1]))
        host = torch.cat([torch.stack([f for _, f in pairs]).reshape(len(pairs), -1),
                          torch.stack([f for _, f in prots]).reshape(len(prots), -1)], dim=1).cpu().numpy()   # and the one of pae
        ok = np.isfinite(host[0, :-B])
        for (name, _), values in zip(pairs, host[:len(pairs), :-B]):
            pcols[name].append(values[ok])
        for (name, _), values in zip(prots, host[:len(prots), -B:]):
            pcols[name].append(100.0 * values)
    truth = np.concatenate(cols["truth"]) if cols["truth"] else np.zeros(0)
    out = {name: calibration(np.concatenate(cols[name]), truth) for name in ("plddt", "ens-lddt") if cols[name]}
    if pae:
        top = pae_head.top() if pae_head is not None else 32.0
        cat = {k: np.concatenate(v) for k, v in pcols.items() if v}
        for name, ref, scale in (("pae", "truth", top), ("ptm", "tm", 100.0), ("ens-pae", "truth", top), ("ens-ptm", "tm", 100.0)):
            if name in cat:
                out[name] = calibration(cat[name], cat[ref], top=scale)
    return out


# ---------------------------------------------------------------------- command line
def data_batches(data, split, batch_size, max_seq_len):
    """The proteins of `data[split]` (the dictionary format of dataset.py) in file order, `batch_size` at a time, padded to the
    longest of the batch and cut at `max_seq_len`: [(seq [B,L] int64, true_crd [B,L*14,3])] on the host."""
    from .dataset import collate_fn
    from .protein.Sequence import VOCAB
    d = data[split]
    seqs = [VOCAB.str2ints(s, False) for s in d["seq"]]
    out = []
    for i in range(0, len(seqs), int(batch_size)):
        out.append((collate_fn(seqs[i:i + batch_size], sequences=True, max_seq_len=max_seq_len),
                    collate_fn(d["crd"][i:i + batch_size], coords=True, max_seq_len=max_seq_len)))
    return out


def parser():
    ap = argparse.ArgumentParser(prog="python -m protein_transformer_amd.confidence", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="command", required=True)

    def common(p, split):
        p.add_argument("checkpoint", metavar="CHECKPOINT", help="a checkpoint written by train.py (or by `fit`)")
        src = p.add_mutually_exclusive_group(required=True)
        src.add_argument("--data", metavar="DATA.pt", help="a dataset dictionary in the format train.py reads")
        src.add_argument("--synthetic", metavar="B,L,n", help="generated proteins, as train.py --synthetic")
        p.add_argument("--split", default=split, help=f"the split of the data that is read (default {split})")
        p.add_argument("--batch_size", type=int, default=32, help="proteins per batch (default 32)")
        p.add_argument("--seed", type=int, default=0)

    fit = sub.add_parser("fit", help="fit a pLDDT head on a frozen checkpoint and write CHECKPOINT2")
    common(fit, "train")
    fit.add_argument("--out", metavar="CHECKPOINT2", required=True, help="the checkpoint plus its `confidence_head`")
    fit.add_argument("--epochs", type=int, default=1)
    fit.add_argument("--lr", type=float, default=1e-3)
    fit.add_argument("--hidden", type=int, default=128)
    fit.add_argument("--nbins", type=int, default=50)
    fitp = sub.add_parser("fit-pae", help="fit a PAE head on a frozen checkpoint and write CHECKPOINT2")
    common(fitp, "train")
    fitp.add_argument("--out", metavar="CHECKPOINT2", required=True, help="the checkpoint plus its `pae_head`")
    fitp.add_argument("--epochs", type=int, default=1)
    fitp.add_argument("--lr", type=float, default=1e-3)
    fitp.add_argument("--hidden", type=int, default=32)
    fitp.add_argument("--nbins", type=int, default=64)
    cal = sub.add_parser("calibrate", help="measure how the pLDDT (and the ensemble's conf) track the true lDDT")
    common(cal, "test")
    cal.add_argument("--samples", type=int, default=0, help="dropout passes: also calibrate the ensemble's conf (default 0)")
    cal.add_argument("--pae", action="store_true",
                     help="also measure the PAE head's matrix and pTM (and, with --samples, ens-pae and ens-ptm) against the true "
                          "aligned error")
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    try:
        if args.batch_size < 1:
            raise ValueError("--batch_size must be >= 1")
        if args.command == "fit" and (args.epochs < 1 or args.hidden < 4 or args.hidden % 4 or not 2 <= args.nbins <= 64):
            raise ValueError("--epochs must be >= 1, --hidden a multiple of 4, --nbins in 2 .. 64")
        if args.command == "fit-pae" and (args.epochs < 1 or not 4 <= args.hidden <= 64 or args.hidden % 4 or not 2 <= args.nbins <= 64):
            raise ValueError("--epochs must be >= 1, --hidden a multiple of 4 in 4 .. 64, --nbins in 2 .. 64")
        entry, pae_entry = read_head_entries(args.checkpoint)
        want_pae = args.command == "calibrate" and args.pae
        if want_pae and (args.samples < 0 or (pae_entry is None and args.samples < 1)):
            raise ValueError(f"{args.checkpoint}: the checkpoint has no PAE head (`confidence fit-pae` writes one) and --samples "
                             "is 0: there is no pair score to calibrate")
        if args.command == "calibrate" and not want_pae and (args.samples < 0 or (entry is None and args.samples < 1)):
            raise ValueError(f"{args.checkpoint}: the checkpoint has no confidence head (`confidence fit` writes one) and "
                             "--samples is 0: there is no score to calibrate")
        from .predict import load_checkpoint
        model = load_checkpoint(args.checkpoint)
        dev = next(model.parameters()).device
        if args.synthetic:
            from .synthetic_data import make_synthetic_dataset
            data = make_synthetic_dataset(args.synthetic, args.seed, dev)
        else:
            data = torch.load(args.data, weights_only=False)
        if args.split not in data:
            raise ValueError(f"the data has no split '{args.split}'")
        batches = data_batches(data, args.split, args.batch_size, model.max_seq_len)
    except (ValueError, OSError) as e:
        print(f"confidence: {e}", file=sys.stderr)
        return 2
    if args.command == "fit":
        head, _ = fit_head(model, batches, epochs=args.epochs, lr=args.lr, seed=args.seed, hidden=args.hidden, nbins=args.nbins,
                           log=lambda line: print(json.dumps(line), flush=True))
        save_with_head(args.checkpoint, args.out, head)
        return 0
    if args.command == "fit-pae":
        head, _ = fit_pae_head(model, batches, epochs=args.epochs, lr=args.lr, seed=args.seed, hidden=args.hidden,
                               nbins=args.nbins, log=lambda line: print(json.dumps(line), flush=True))
        save_with_head(args.checkpoint, args.out, head, key=PAE_HEAD_KEY)
        return 0
    head = None if entry is None else head_from_entry(entry, dev)
    if not args.pae:
        print(json.dumps(calibrate(model, head, batches, samples=args.samples, seed=args.seed)))
        return 0
    pae_head = None if pae_entry is None else pae_head_from_entry(pae_entry, dev)
    print(json.dumps(calibrate(model, head, batches, samples=args.samples, seed=args.seed, pae_head=pae_head, pae=True)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
