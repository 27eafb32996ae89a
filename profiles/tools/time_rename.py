"""The timings of profiles/rename/NOTES.md, on one MI355X:

    python profiles/tools/time_rename.py [--root CHECKOUT] [--out FILE.json]

1. `losses.rename_symmetric`, `losses.slddt_forward_backward`, `losses.fape_forward_backward` at 32 x 512 on one synthetic batch
   (lengths 256 ... 512, 2 % of the residues missing; truth by the NeRF kernels from the true angles, prediction from the noisy start
   angles): HIP events around 100 back-to-back calls after 10 warm-up calls, five windows, with the pair counts per protein.
2. A training step of `train.py --synthetic 32,512,12 -l fape`, with and without `--rename_symmetric`, from train.py's own step
   timing: the `speed` column (residues / s between two batch rows, log.py) of the `.train` file it writes, as ms per step over the
   batch rows of the second and third epoch (the first is warm-up); each variant runs twice, alternating.

`--root`: time the package of another checkout of this repository (built there) instead - the parent commit, for the flag-off
step; a checkout without the renaming reports what it has.  One JSON document on stdout (and in --out)."""
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

from protein_transformer_amd import losses, synthetic                       # noqa: E402
from protein_transformer_amd.protein.Structure import nerf_forward          # noqa: E402

dev = torch.device("cuda:0")
B, L = 32, 512
has_rename = hasattr(losses, "rename_symmetric")


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


out = {"rename": has_rename}
rng = np.random.default_rng(0)
lens = [L] + [int(x) for x in rng.integers(L // 2, L + 1, B - 1)]
batch = synthetic.make_batch(lens, L_pad=L, seed=3, build_coords=lambda a, s: nerf_forward(a.to(dev), s.to(dev))[0], frac_missing=0.02)
seq, ang, true = (batch[k].to(dev) for k in ("seq", "true_ang", "true_crd"))
pred = nerf_forward(batch["start_ang_rad"].to(dev), seq)[0]
present = (~torch.isnan(true).any(-1)) & (seq != synthetic.PAD_ID).repeat_interleave(14, dim=1)
natoms = present.sum(1).double()
out["atoms_per_protein"] = float(natoms.mean())
out["slddt_pairs_per_protein"] = float((natoms * (natoms - 1) / 2).mean())
out["fape_pairs_per_protein_per_sweep"] = float((torch.tensor(lens, dtype=torch.float64, device=dev) * natoms).mean())
if has_rename:
    _, _, swapped, cost = losses.rename_symmetric(pred, true, seq, ang)
    cand = cost[..., 1] > 0
    rows = sum(((seq == r) & cand).sum(1).double() * len(pairs) for r, (pairs, _) in losses.SYMMETRIC_SWAPS.items())
    out["candidates_per_protein"] = float(cand.sum(1).double().mean())
    out["swapped_per_protein"] = float(swapped.sum(1).double().mean())
    out["rename_lane_iterations_per_protein"] = float((rows * natoms).mean())      # swap pair x present atom: 4 distances each
    out["rename_us"] = timed(lambda: losses.rename_symmetric(pred, true, seq, ang))
    out["rename_without_angles_us"] = timed(lambda: losses.rename_symmetric(pred, true, seq))
out["slddt_fwd_bwd_us"] = timed(lambda: losses.slddt_forward_backward(pred, true, seq))
out["fape_fwd_bwd_us"] = timed(lambda: losses.fape_forward_backward(pred, true, seq))


def step_ms(flag, tmp, tag):
    """ms per step of `train.py -l fape` from the speed column of its own log, in a child process."""
    cmd = [sys.executable, "-m", "protein_transformer_amd.train", "--synthetic", f"{B},{L},12", "--name", tag, "-l", "fape", "-b", str(B),
           "--max_seq_len", str(L), "--train_only", "-e", "3", "--log_dir", os.path.join(tmp, "logs"), "--chkpt_dir", os.path.join(tmp, "ck")]
    r = subprocess.run(cmd + (["--rename_symmetric"] if flag else []), cwd=opt.root, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=opt.root))
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    rows = list(csv.reader(open(os.path.join(tmp, "logs", tag + ".train"))))
    # (a row ends in mode, granularity, time, speed; counted from the end: the `combined` value is written whatever the header lists)
    speeds = [float(r[-1]) for r in rows[1:] if r[-3] == "batch"][12:]
    ms = np.array([B * L / s * 1e3 for s in speeds])
    return dict(ms_median=float(np.median(ms)), ms_min=float(ms.min()), ms_max=float(ms.max()), steps=len(ms))


if not opt.skip_steps:
    with tempfile.TemporaryDirectory() as tmp:
        for k, flag in enumerate((False, True, False, True) if has_rename else (False, False)):
            out.setdefault("step_fape_flag_on_ms" if flag else "step_fape_flag_off_ms", []).append(step_ms(flag, tmp, f"t{k}"))
text = json.dumps(out, indent=1)
if opt.out:
    with open(opt.out, "w") as f:
        f.write(text)
print(text)
