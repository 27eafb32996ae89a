"""What profiles/pae_head/NOTES.md times: fitting steps of the PAE head (`confidence.fit_pae_head`) on one batch of 32 proteins of
512 residues, on the d_model 512, 6-layer, 8-head, d_ff 2048 encoder of BASELINE.json configs[3] with random weights, H = 32,
nbins = 64.  Run it under the kernel trace, which gives the time of every kernel of a step - the pair sweeps of csrc/pae_head.hip
next to the encoder's deterministic pass on the same batch:

    rocprofv3 --kernel-trace --stats -d OUT_DIR -- python profiles/tools/time_pae_head.py

Three steps (the first one warms up: code objects, allocator), then four inference passes of the head (the first one warms up);
prints one JSON line with the host-clock times."""
import json
import os
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from protein_transformer_amd import confidence as CF, synthetic                     # noqa: E402
from protein_transformer_amd.protein.Structure import nerf_forward                  # noqa: E402
from protein_transformer_amd.train import make_model                                # noqa: E402

dev = torch.device("cuda:0")
B, L, STEPS = 32, 512, 3
build = lambda ang, seq: nerf_forward(ang.to(dev), seq.to(dev))[0]                  # noqa: E731
batch = synthetic.make_batch([L] * B, L_pad=L, seed=5, build_coords=build)
am = synthetic.angle_means(batch["true_ang"])
settings = types.SimpleNamespace(model="enc-only", n_layers=6, n_head=8, d_model=512, d_inner_hid=2048, max_seq_len=L, dropout=0.1)
torch.manual_seed(1)
m = make_model(settings, dev, am)
with torch.no_grad():
    m.output_projection.weight.normal_(0, 0.02)
m = m.to(dev)
batches = [(batch["seq"].to(dev), None, batch["true_crd"].to(dev))]
head = CF.PaeHead(512, device=dev)
times = []
for step in range(STEPS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    head, hist = CF.fit_pae_head(m, batches, head=head, epochs=1)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
x, seq, _ = CF.hidden_and_aligned_error(m, batches[0][0], batches[0][2])
inference = []
for rep in range(4):                                                                # (the first one warms up)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    head.forward(x, seq)
    torch.cuda.synchronize()
    inference.append(time.perf_counter() - t0)
print(json.dumps({"B": B, "L": L, "hidden": head.hidden, "nbins": head.nbins, "step_ms": [round(1e3 * t, 2) for t in times],
                  "inference_head_ms": [round(1e3 * t, 2) for t in inference], "ce": hist[-1]["ce"], "pairs": hist[-1]["pairs"]}))
