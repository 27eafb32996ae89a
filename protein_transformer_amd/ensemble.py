"""Dropout ensembles: how far K stochastic passes of a model move around its deterministic prediction, per residue.

`ensemble_spread` is the device kernel (csrc/ensemble.hip; definition in include/ptamd.h): every sample is superposed on the
reference by least squares over the C-alphas, and what each residue does after the fit comes back as an RMSD per sample and an
RMSF per residue.  `predict_ensemble` makes the samples: one `model.eval()` pass is the reference, K passes in training mode under
`no_grad` - the dropout masks of the encoder, no backward pass - are the ensemble.  The reference (protein_transformer) has no
counterpart.  `python -m protein_transformer_amd.predict` is the command line on top.

`aligned_error` is the second kernel (csrc/aligned_error.hip): the L x L matrix of how far residue j lies from the reference's
once a sample and the reference are aligned on the backbone frame of residue i, averaged over the samples.  Like `conf`, the
matrix and its two summaries (mean, tm) measure the dropout ensemble's SELF-CONSISTENCY and are not calibrated predictions.

`conf` is a dropout SELF-CONSISTENCY score on the lDDT scale: 100 x the mean lDDT-C-alpha of the samples against the reference
pass.  It is NOT a calibrated pLDDT: how well it tracks the true lDDT of a given model is what
`python -m protein_transformer_amd.confidence calibrate` measures.
"""
from collections import namedtuple

import torch

from . import _lib
from .protein.Structure import NUM_PREDICTED_COORDS

Ensemble = namedtuple("Ensemble", "angles crd rmsd rmsf conf usable ae ae_stats hidden", defaults=(None, None, None))


def ensemble_spread(ref_crd, sample_crd, seq):
    """ref_crd [B, L*14, 3] and sample_crd [B, K, L*14, 3] device tensors, seq [B, L] -> (rmsd [B,K], rmsf [B,L,2] = {C-alpha,
    every atom of the residue}, usable [B] int32), all on the device, no sync: the spread of the K samples of every protein around
    its reference after a least-squares fit over the C-alphas (csrc/ensemble.hip; definition in include/ptamd.h).  NaN = an
    unusable sample (fewer than 3 residues, a non-finite C-alpha), an absent residue, or no usable sample."""
    _lib.require_gpu(ref_crd, sample_crd, seq)
    B, L = seq.shape
    assert ref_crd.shape == (B, L * NUM_PREDICTED_COORDS, 3)
    assert sample_crd.dim() == 4 and sample_crd.shape[0] == B and sample_crd.shape[1] >= 1 and sample_crd.shape[2:] == ref_crd.shape[1:]
    ref_crd, sample_crd, seq = ref_crd.float().contiguous(), sample_crd.float().contiguous(), seq.contiguous()
    K = sample_crd.shape[1]
    dev = seq.device
    rmsd = torch.empty(B, K, dtype=torch.float32, device=dev)
    rmsf = torch.empty(B, L, 2, dtype=torch.float32, device=dev)
    usable = torch.empty(B, dtype=torch.int32, device=dev)
    ws = _lib.workspace("ensemble", _lib.lib().ptamd_ensemble_workspace_bytes(B, K, L), dev)
    rc = _lib.lib().ptamd_ensemble_spread(_lib.ptr(ref_crd), _lib.ptr(sample_crd), _lib.ptr(seq), B, K, L, _lib.ptr(rmsd),
                                          _lib.ptr(rmsf), _lib.ptr(usable), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "ensemble_spread")
    return rmsd, rmsf, usable


def aligned_error(ref_crd, sample_crd, seq):
    """ref_crd [B, L*14, 3] and sample_crd [B, K, L*14, 3] device tensors, seq [B, L] -> (ae [B,L,L], stats [B,2] = {mean, tm},
    usable [B] int32), all on the device, no sync: ae[b,i,j] is the mean over the usable samples of how far the C-alpha of
    residue j lies from the reference's once both are seen from the backbone frame of residue i (csrc/aligned_error.hip;
    definition in include/ptamd.h).  Row = frame, column = point.  NaN = a residue that is no frame / no point of the reference,
    padding, or no usable sample."""
    _lib.require_gpu(ref_crd, sample_crd, seq)
    B, L = seq.shape
    assert ref_crd.shape == (B, L * NUM_PREDICTED_COORDS, 3)
    assert sample_crd.dim() == 4 and sample_crd.shape[0] == B and sample_crd.shape[1] >= 1 and sample_crd.shape[2:] == ref_crd.shape[1:]
    ref_crd, sample_crd, seq = ref_crd.float().contiguous(), sample_crd.float().contiguous(), seq.contiguous()
    K = sample_crd.shape[1]
    dev = seq.device
    ae = torch.empty(B, L, L, dtype=torch.float32, device=dev)
    stats = torch.empty(B, 2, dtype=torch.float32, device=dev)
    usable = torch.empty(B, dtype=torch.int32, device=dev)
    ws = _lib.workspace("aligned_error", _lib.lib().ptamd_aligned_error_workspace_bytes(B, K, L), dev)
    rc = _lib.lib().ptamd_aligned_error(_lib.ptr(ref_crd), _lib.ptr(sample_crd), _lib.ptr(seq), B, K, L, _lib.ptr(ae),
                                        _lib.ptr(stats), _lib.ptr(usable), _lib.ptr(ws), ws.numel(), _lib.stream())
    _lib.check(rc, "aligned_error")
    return ae, stats, usable


_aligned_error = aligned_error          # (`predict_ensemble` has an argument of that name)


def sample_seed(seed, k):
    """The dropout seed of sampling pass k: a function of (seed, k) only - not of the model's own seed, of how many steps it has
    taken, or of the batch."""
    return (int(seed) * 0x9E3779B1 + (int(k) + 1) * 0x632BE59BD9B4E019) & (2 ** 62 - 1)


class _Borrowed:
    """A model for the length of a prediction, handed back as it was found: `training`, `dropout_seed`, `_step_counter` - the
    forward pass advances the counter in training mode and derives the dropout seed from both - and the AutoGuard.  The guard
    counts passes, honours a pending measurement at a fixed later pass and measures on passes without a backward pass
    (`AutoGuard.poll`, `want_measure_forward`): K + 1 forward passes between two training steps would move the step at which the
    arithmetic of a site changes.  So the passes made here run under a guard of their own - as untrusting as any new one, the
    same for every call - and the model's guard, with whatever it has pending, is put back untouched."""

    def __init__(self, model):
        self.model = model

    def __enter__(self):
        m = self.model
        self.saved = {k: getattr(m, k) for k in ("training", "dropout_seed", "_step_counter", "auto_guard", "keep_hidden")
                      if hasattr(m, k)}
        guard = self.saved.get("auto_guard")
        if guard is not None:
            m.auto_guard = type(guard)(guard.nlayers, guard.interval, guard.max_slack, guard.max_spread)
            m.auto_guard.enabled = guard.enabled
        return m

    def __exit__(self, *exc):
        m = self.model
        m.train(self.saved.pop("training"))
        for k, v in self.saved.items():
            setattr(m, k, v)
        return False


def predict_ensemble(model, seq, samples=8, seed=0, aligned_error=False, hidden=False):
    """model: an encoder of this package on the device; seq [B, L] residue ids with trailing padding -> Ensemble(
      angles [B,L,12]   radians, of the deterministic (`model.eval()`) pass;
      crd    [B,L*14,3] its NeRF build (`losses.predicted_coords`): THE prediction - the structure a caller writes;
      rmsd   [B,K]      of each sample after its fit on `crd`,
      rmsf   [B,L,2]    per residue over the usable samples, {C-alpha, every atom}  (`ensemble_spread`);
      conf   [B,L]      100 x the mean over the usable samples of the per-residue lDDT-C-alpha (cutoff 15 A, `lddt_batch`) of the
                        sample against `crd`; NaN where that lDDT has no pair or no sample is usable;
      usable [B]        int32, the number of usable samples;
      ae     [B,L,L]    with `aligned_error=True`: the frame-aligned error matrix of the samples around `crd` (`aligned_error`:
                        row = frame, column = point), and
      ae_stats [B,2]    its {mean, tm}; both None otherwise, and then nothing further is launched;
      hidden [B*L,d]    with `hidden=True`: the last hidden state of the deterministic pass (`model.keep_hidden`), what the
                        confidence head reads (confidence.py); None otherwise).
    The K samples are passes in training mode under `no_grad`, pass k under the dropout seed `sample_seed(seed, k)`.  `samples=0`
    runs the reference pass only: the ensemble fields are None.  Everything stays on the device; the model is left as it was
    found (`_Borrowed`): a training run that calls this between two steps continues bit-identically."""
    from .eval_metrics import lddt_batch
    from .losses import angles_forward, predicted_coords
    K = int(samples)
    if K < 0:
        raise ValueError("samples must be >= 0")
    B, L = seq.shape
    with _Borrowed(model) as m, torch.no_grad():
        m.eval()
        m.keep_hidden = bool(hidden)             # (for the deterministic pass alone; `_Borrowed` puts the attribute back)
        pred = m(seq)
        hidden = m.__dict__.pop("last_hidden") if hidden else None
        m.keep_hidden = False
        seq = seq.to(pred.device, torch.int64).contiguous()
        angles = angles_forward(pred.detach().float().contiguous().view(B, L, -1))
        crd, _ = predicted_coords(pred, seq)
        if K == 0:
            return Ensemble(angles, crd, None, None, None, None, hidden=hidden)
        m.train()
        sample_crd = torch.empty(B, K, L * NUM_PREDICTED_COORDS, 3, dtype=torch.float32, device=crd.device)
        for k in range(K):
            m.dropout_seed, m._step_counter = sample_seed(seed, k), 0
            sample_crd[:, k] = predicted_coords(m(seq), seq)[0]
    rmsd, rmsf, usable = ensemble_spread(crd, sample_crd, seq)
    # the reference as the truth of every sample: B * K "proteins" through the one lDDT kernel.  Only its C-alpha column is read
    # here, and that column counts pairs of C-alphas alone: a truth with every other slot absent (NaN) gives the same counts and
    # spares the sweep the all-atom pairs (14 x the atoms, ~200 x the pairs: 9.5 ms of a 43 ms call at 32 x 512, K = 8)
    flat = sample_crd.view(B * K, L * NUM_PREDICTED_COORDS, 3)
    truth = torch.full((B, L, NUM_PREDICTED_COORDS, 3), float("nan"), dtype=torch.float32, device=crd.device)
    truth[:, :, 1] = crd.view(B, L, NUM_PREDICTED_COORDS, 3)[:, :, 1]
    truth = truth.view(B, 1, L * NUM_PREDICTED_COORDS, 3).expand(B, K, -1, -1).reshape(B * K, L * NUM_PREDICTED_COORDS, 3)
    lddt_ca = lddt_batch(flat, truth, seq[:, None].expand(B, K, L).reshape(B * K, L))[1][:, :, 1].view(B, K, L)
    ok = torch.isfinite(rmsd)[:, :, None]                        # the usable samples
    conf = 100.0 * torch.where(ok, lddt_ca, torch.zeros_like(lddt_ca)).sum(1) / usable[:, None].float()
    if not aligned_error:
        return Ensemble(angles, crd, rmsd, rmsf, conf, usable, hidden=hidden)
    ae, ae_stats, _ = _aligned_error(crd, sample_crd, seq)
    return Ensemble(angles, crd, rmsd, rmsf, conf, usable, ae, ae_stats, hidden)
