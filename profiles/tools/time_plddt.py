"""What profiles/plddt/NOTES.md times: `predict --samples 0 --plddt` (one pass and the head) against `predict --samples 8` (nine
passes and the ensemble kernels) on one FASTA file of 32 sequences of 512 residues, on the d_model 512, 6-layer, 8-head, d_ff 2048
encoder of BASELINE.json configs[3] with random weights and an UNFITTED head (the time of a head does not depend on its weights).

    python profiles/tools/time_plddt.py OUT_DIR

Both commands run in this process through `predict.main` (checkpoint load, device work, one read back, 32 PDB files), alternating,
REPEATS times each after one warm-up of each; then the device part alone (`predict.predict_records` on the loaded model, a device
synchronise behind it).  Host clock; prints one JSON line."""
import contextlib
import io
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from protein_transformer_amd import confidence as CF, predict, synthetic            # noqa: E402
from protein_transformer_amd.protein.Sequence import VOCAB                          # noqa: E402
from protein_transformer_amd.train import make_model                                # noqa: E402

out_dir = sys.argv[1]
os.makedirs(out_dir, exist_ok=True)
dev = torch.device("cuda:0")
B, L, K, REPEATS = 32, 512, 8, 5
batch = synthetic.make_batch([L] * B, L_pad=L, seed=5)
am = synthetic.angle_means(batch["true_ang"])
settings = types.SimpleNamespace(model="enc-only", n_layers=6, n_head=8, d_model=512, d_inner_hid=2048, max_seq_len=L, dropout=0.1)
torch.manual_seed(1)
m = make_model(settings, dev, am)
with torch.no_grad():
    m.output_projection.weight.normal_(0, 0.02)
plain = os.path.join(out_dir, "bench.chkpt")
torch.save({"model_state_dict": m.state_dict(), "settings": settings}, plain)
with_head = os.path.join(out_dir, "bench_head.chkpt")
CF.save_with_head(plain, with_head, CF.ConfidenceHead(512, device=dev))
fasta = os.path.join(out_dir, "seqs.fasta")
with open(fasta, "w") as f:
    for i, row in enumerate(batch["seq"]):
        f.write(f">s{i}\n{VOCAB.ints2str(row.tolist())}\n")
records = predict.read_fasta(fasta)
assert len(records) == B and all(len(s) == L for _, s in records)

commands = {"plddt_samples0": [with_head, fasta, "--out", os.path.join(out_dir, "a"), "--samples", "0", "--plddt"],
            "samples8": [plain, fasta, "--out", os.path.join(out_dir, "b"), "--samples", str(K)]}


def command(argv):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        assert predict.main(argv) == 0
    torch.cuda.synchronize()
    return time.perf_counter() - t0


model = predict.load_checkpoint(with_head, dev)
head = CF.load_head(with_head, dev)


def device_part(name):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if name == "plddt_samples0":
        predict.predict_records(model, records, samples=0, head=head)
    else:
        predict.predict_records(model, records, samples=K)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


whole, part = {k: [] for k in commands}, {k: [] for k in commands}
for rep in range(REPEATS + 1):                      # (the first round warms up: code objects, allocator, file system)
    for name, argv in commands.items():
        t = command(argv)
        if rep:
            whole[name].append(t)
for rep in range(REPEATS + 1):
    for name in commands:
        t = device_part(name)
        if rep:
            part[name].append(t)
ms = lambda v: {"min": round(1e3 * min(v), 2), "median": round(1e3 * statistics.median(v), 2), "max": round(1e3 * max(v), 2)}  # noqa: E731
print(json.dumps({"B": B, "L": L, "K": K, "repeats": REPEATS, "command_ms": {k: ms(v) for k, v in whole.items()},
                  "predict_records_ms": {k: ms(v) for k, v in part.items()},
                  "ratio_command": round(statistics.median(whole["samples8"]) / statistics.median(whole["plddt_samples0"]), 2),
                  "ratio_predict_records": round(statistics.median(part["samples8"]) / statistics.median(part["plddt_samples0"]), 2)}))
