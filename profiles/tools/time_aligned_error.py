"""What rocprofv3 traces for profiles/aligned_error/NOTES.md: predict_ensemble(..., aligned_error=True) at 32 x 512 on the d_model
512, 6-layer, 8-head encoder (BASELINE.json configs[3]) with K = 8 samples, six calls (all are in the trace; the first loads the
code objects).

    rocprofv3 --kernel-trace --stats -d OUT -o ae -- python profiles/tools/time_aligned_error.py
"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from protein_transformer_amd import synthetic                                    # noqa: E402
from protein_transformer_amd.ensemble import predict_ensemble                      # noqa: E402
from protein_transformer_amd.models.encoder_only import EncoderOnlyTransformer     # noqa: E402
from protein_transformer_amd.protein.Sequence import VOCAB                         # noqa: E402

dev = torch.device("cuda:0")
B, L, K, CALLS = 32, 512, 8, 6
batch = synthetic.make_batch([L] * B, L_pad=L, seed=5)
am = synthetic.angle_means(batch["true_ang"])
torch.manual_seed(1)
m = EncoderOnlyTransformer(6, 8, 512, 2048, L, VOCAB, am, True, dropout=0.1)
with torch.no_grad():
    m.output_projection.weight.normal_(0, 0.02)
m = m.to(dev)
seq = batch["seq"].to(dev)
times = []
for i in range(CALLS):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ens = predict_ensemble(m, seq, samples=K, seed=0, aligned_error=True)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
print("calls", CALLS, "B", B, "L", L, "K", K, "wall ms per call", [round(1e3 * t, 2) for t in times])
stats = ens.ae_stats.cpu().numpy()
print("usable", ens.usable[:4].tolist(), "mean ae", float(np.nanmean(stats[:, 0])), "mean tm", float(np.nanmean(stats[:, 1])),
      "ae bytes", ens.ae.numel() * 4)
