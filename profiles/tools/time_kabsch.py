"""The timings of profiles/kabsch/NOTES.md, on one MI355X:

    python profiles/tools/time_kabsch.py [--root CHECKOUT] [--out FILE.json] [--skip-steps]

1. `losses.kabsch_forward_backward` (with the gradient and forward only) at 32 x 512 and 4 x 512 on one synthetic batch (lengths
   256 ... 512, 2 % of the residues missing; truth by the NeRF kernels from the true angles, prediction from the noisy start angles),
   beside `eval_metrics.kabsch_rmsd_batch` (the metric's kernel) and `losses.drmsd_forward_backward` (the pair sweep) on the same
   batch: HIP events around 100 back-to-back calls after 10 warm-up calls, five windows.
2. A training step of `train.py --synthetic 32,512,12 -l <loss>` from train.py's own step timing: the `speed` column (residues / s
   between two batch rows, log.py) of the `.train` file it writes, as ms per step over the batch rows of the second and third epoch
   (the first is warm-up); `-l drmsd` and `-l kabsch` run twice each, alternating.

`--root`: time the package of another checkout of this repository (built there) instead - the parent commit, for the `-l drmsd`
step; a checkout without the loss reports what it has.  One JSON document on stdout (and in --out)."""
import argparse
import csv
import json
import os
import subprocess
import sys
import tempfile

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ap.add_argument("--out", default=None)
ap.add_argument("--skip-steps", action="store_true")
opt = ap.parse_args()
opt.root = os.path.abspath(opt.root)
sys.path.insert(0, opt.root)

import numpy as np      # noqa: E402
import torch            # noqa: E402

from protein_transformer_amd import eval_metrics, losses, synthetic         # noqa: E402
from protein_transformer_amd.protein.Structure import nerf_forward          # noqa: E402

dev = torch.device("cuda:0")
L = 512
has_kabsch = hasattr(losses, "kabsch_forward_backward")


def timed(fn, warm=10, reps=100, windows=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / reps * 1e3)
    return dict(us_median=float(np.median(times)), us_min=float(min(times)), us_max=float(max(times)))


out = {"kabsch": has_kabsch}
for B in (32, 4):
    rng = np.random.default_rng(0)
    lens = [L] + [int(x) for x in rng.integers(L // 2, L + 1, B - 1)]
    batch = synthetic.make_batch(lens, L_pad=L, seed=3, build_coords=lambda a, s: nerf_forward(a.to(dev), s.to(dev))[0], frac_missing=0.02)
    seq, true = batch["seq"].to(dev), batch["true_crd"].to(dev)
    pred = nerf_forward(batch["start_ang_rad"].to(dev), seq)[0]
    present = (~torch.isnan(true).any(-1)) & (seq != synthetic.PAD_ID).repeat_interleave(14, dim=1)
    res = {"atoms_per_protein": float(present.sum(1).double().mean())}
    if has_kabsch:
        res["kabsch_fwd_bwd_us"] = timed(lambda: losses.kabsch_forward_backward(pred, true, seq))
        res["kabsch_fwd_us"] = timed(lambda: losses.kabsch_forward_backward(pred, true, seq, need_grad=False))
        stats = losses.kabsch_forward_backward(pred, true, seq)[0]
        res["loss_mean_A"] = float(stats[:, 0].double().mean())
    res["kabsch_rmsd_metric_us"] = timed(lambda: eval_metrics.kabsch_rmsd_batch(pred, true, seq))
    res["drmsd_fwd_bwd_us"] = timed(lambda: losses.drmsd_forward_backward(pred, true, seq))
    res["drmsd_fwd_us"] = timed(lambda: losses.drmsd_forward_backward(pred, true, seq, need_grad=False))
    out[f"{B}x{L}"] = res


def step_ms(loss, tmp, tag, B=32):
    """ms per step of `train.py -l <loss>` from the speed column of its own log, in a child process."""
    cmd = [sys.executable, "-m", "protein_transformer_amd.train", "--synthetic", f"{B},{L},12", "--name", tag, "-l", loss, "-b", str(B),
           "--max_seq_len", str(L), "--train_only", "-e", "3", "--log_dir", os.path.join(tmp, "logs"), "--chkpt_dir", os.path.join(tmp, "ck")]
    r = subprocess.run(cmd, cwd=opt.root, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=opt.root))
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    rows = list(csv.reader(open(os.path.join(tmp, "logs", tag + ".train"))))
    # (a row ends in mode, granularity, time, speed; counted from the end: the `combined` value is written whatever the header lists)
    speeds = [float(r[-1]) for r in rows[1:] if r[-3] == "batch"][12:]
    ms = np.array([B * L / s * 1e3 for s in speeds])
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()), steps=len(ms))


if not opt.skip_steps:
    with tempfile.TemporaryDirectory() as tmp:
        for k, loss in enumerate(("drmsd", "kabsch", "drmsd", "kabsch") if has_kabsch else ("drmsd", "drmsd")):
            out.setdefault(f"step_{loss}_ms", []).append(step_ms(loss, tmp, f"t{k}"))
text = json.dumps(out, indent=1)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text)
print(text)
