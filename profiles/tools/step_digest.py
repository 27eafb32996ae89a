"""What profiles/host_launch/NOTES.md compares: SHA-256 of the flat parameter buffer and of the flat gradient buffer after 3
training steps of a 2-layer d_model 512 / d_ff 2048 / 8-head encoder (fixed seed, dropout 0.1, dRMSD loss, clip 1, default
arithmetic), for batches of 4 x 512 (split-K, 64-row tiles, deferred reductions) and of 16 x 512 (grouped weight gradients), with
FusedSGD and with FusedAdam.  Eight digests, one JSON line each; two commits that launch the same kernels on the same arguments
print the same eight.

    python profiles/tools/step_digest.py
"""
import hashlib
import json
import os
import sys
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from protein_transformer_amd import synthetic                                        # noqa: E402
from protein_transformer_amd.models.encoder_only import EncoderOnlyTransformer      # noqa: E402
from protein_transformer_amd.optim import FusedAdam, FusedSGD                        # noqa: E402
from protein_transformer_amd.protein.Sequence import VOCAB                          # noqa: E402
from protein_transformer_amd.protein.Structure import nerf_forward                  # noqa: E402
from protein_transformer_amd.train import train_step                                # noqa: E402

dev = torch.device("cuda:0")
L, STEPS = 512, 3
args = types.SimpleNamespace(loss="drmsd", combined_drmsd_weight=0.5, backbone_loss=False, clip=1.0)
sha = lambda t: hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()          # noqa: E731
for B in (4, 16):
    batches = [synthetic.make_batch([L] * B, L_pad=L, seed=11 + i, build_coords=lambda a, s: nerf_forward(a.to(dev), s.to(dev))[0])
               for i in range(STEPS)]
    am = synthetic.angle_means(batches[0]["true_ang"])
    for name in ("sgd", "adam"):
        torch.manual_seed(1234)
        model = EncoderOnlyTransformer(2, 8, 512, 2048, L, VOCAB, am, True, dropout=0.1).to(dev).train()
        opt = (FusedAdam(model, lr=1e-4, betas=(0.9, 0.98), eps=1e-9, weight_decay=10e-3) if name == "adam"
               else FusedSGD(model, lr=1e-4, weight_decay=10e-3))
        for b in batches:
            seq, ang, crd = (b[k].to(dev) for k in ("seq", "true_ang", "true_crd"))
            losses = train_step(model, opt, args, seq, ang, crd)
        torch.cuda.synchronize()
        flat, grad = model.flat_parameters()
        print(json.dumps(dict(batch=B, length=L, optimizer=name, steps=STEPS, drmsd=float(losses["drmsd-full"]),
                              params_sha256=sha(flat), grads_sha256=sha(grad))), flush=True)
