"""`train.py --clash_weight W` and `--eval_clash` end to end on the device: the term joins the gradient of whichever structural
loss trains the structure, `loss` gains W x clash-full, the report carries the value to the host (also from two ranks, one of
them idle), and a run with neither flag is, key for key and bit for bit, the run of before.

Bars.  Parameter gradient: rel-L2 < 1e-3 against the gradient without the flag plus the clash gradient pushed through the same
NeRF adjoint and the same model backward - the chain bar of tests/test_gpu_loss_path.py (the adjoint is linear; the two sides
differ by fp32 rounding along the chain).  `loss`: the same two host numbers added; under `-l combined` the reference's `loss`
is an fp32 tensor and the sum is rounded to fp32 once more - half an ulp, 6e-8 relative: rel 2e-7."""
import csv
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

import clash_ref as R
from test_gpu_dp import _free_port, _shard

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENS = [24, 19, 13]
W = 0.5


def _setup(loss, lens=LENS, **flags):
    """A tiny model (d_model 64, 2 layers), B = len(lens), rows of 24; truth built by the project's NeRF."""
    from protein_transformer_amd import synthetic
    from protein_transformer_amd.models.encoder_only import EncoderOnlyTransformer
    from protein_transformer_amd.optim import FusedSGD
    from protein_transformer_amd.protein.Sequence import VOCAB
    from protein_transformer_amd.protein.Structure import nerf_forward
    dev = torch.device(DEV)
    build = lambda ang, seq: nerf_forward(ang.to(dev), seq.to(dev))[0]           # noqa: E731
    batch = synthetic.make_batch(lens, L_pad=24, seed=21, build_coords=build, frac_missing=0.05)
    torch.manual_seed(123)
    model = EncoderOnlyTransformer(2, 4, 64, 128, 64, VOCAB, synthetic.angle_means(batch["true_ang"]), True, dropout=0.0)
    with torch.no_grad():
        model.output_projection.weight.normal_(0, 0.05)
    model.set_dropout(0.0)
    model = model.to(dev).train()
    opt = FusedSGD(model, lr=1e-2, weight_decay=10e-3)
    args = types.SimpleNamespace(loss=loss, combined_drmsd_weight=0.5, backbone_loss=False, clip=1.0, lr_scheduling="plateau", **flags)
    return model, opt, args, tuple(batch[k] for k in ("seq", "true_ang", "true_crd"))


def _step(model, args, data, **kw):
    """get_losses on a fresh forward pass -> (dictionary, flat parameter gradient as numpy, the prediction)."""
    from protein_transformer_amd.train import get_losses
    seq, ang, crd = data
    model.zero_grad()
    pred = model(seq, ang)
    out = get_losses(args, pred, ang, crd, seq, **kw)
    return out, model.flat_parameters()[1].cpu().numpy().copy(), pred


def _clash_alone(model, data, weight, tolerance=R.TOLERANCE):
    """weight * d(sum_i clash_i) pushed through the NeRF adjoint and the model: (flat parameter gradient, per-protein values)."""
    from protein_transformer_amd.losses import angles_backward, angles_forward, clash_forward_backward
    from protein_transformer_amd.protein.Structure import nerf_backward, nerf_forward
    seq, ang, _ = data
    model.zero_grad()
    pred = model(seq, ang)
    sc = pred.detach().float().contiguous().view(*seq.shape, 24)
    a = angles_forward(sc)
    built, _ = nerf_forward(a, seq)
    stats, _, dcrd = clash_forward_backward(built, seq, need_grad=True, tolerance=tolerance, weight=weight)
    pred.backward(gradient=angles_backward(sc, nerf_backward(a, seq, built, dcrd)).view_as(pred))
    return model.flat_parameters()[1].cpu().numpy().copy(), stats[:, 0].cpu().numpy().astype(np.float64)


@pytest.mark.parametrize("loss", ["drmsd", "combined", "fape"])
def test_the_term_joins_the_gradient_and_the_loss(loss):
    model, _, args, batch = _setup(loss)
    data = tuple(t.to(DEV) for t in batch)
    base, g_base, _ = _step(model, args, data)
    g_clash, values = _clash_alone(model, data, W)
    args.clash_weight = W
    with_term, g_both, _ = _step(model, args, data)
    assert np.isfinite(values).all() and values.min() > 0                # every chain of random side chains clashes somewhere
    assert set(with_term) == set(base) | {"clash-full"}
    assert float(with_term["clash-full"]) == pytest.approx(values.mean(), rel=1e-6)
    assert float(with_term["loss"]) == pytest.approx(float(base["loss"]) + W * float(with_term["clash-full"]), rel=2e-7)
    for k in base:
        if k != "loss":
            assert np.array_equal(np.asarray(with_term[k], np.float64), np.asarray(base[k], np.float64), equal_nan=True), k
    err = R.rel_l2(g_both, g_base + g_clash)
    print(f"{loss}: parameter gradient rel-L2 {err:.2e}; |base| {np.linalg.norm(g_base):.3e}, |clash| {np.linalg.norm(g_clash):.3e}")
    assert err < 1e-3 and np.linalg.norm(g_clash) > 1e-3 * np.linalg.norm(g_base)      # (the term is not lost in the sum)
    # another tolerance is another term
    args.clash_tolerance = 0.5
    wider = _step(model, args, data)[0]
    assert float(wider["clash-full"]) > float(with_term["clash-full"])
    # evaluation under the weight: forward only, the same key
    ev = _step(model, args, data, do_backwards=False, eval_mode=True, return_rmsd=True)[0]
    assert float(ev["clash-full"]) == float(wider["clash-full"])


def test_with_neither_flag_nothing_changes():
    """Keys and bits of a run without the flags: W = 0 given explicitly is the run that does not know the flags at all."""
    keys = ["loss", "drmsd-full", "lndrmsd-full", "drmsd-bb", "lndrmsd-bb", "combined-full", "mse-full", "mse-bb", "mse-sc", "rmsd-full"]
    for loss in ("drmsd", "fape"):
        model, _, args, batch = _setup(loss)
        data = tuple(t.to(DEV) for t in batch)
        before, g_before, _ = _step(model, args, data)
        args.clash_weight, args.clash_tolerance, args.eval_clash = 0.0, 1.5, False
        after, g_after, _ = _step(model, args, data)
        assert list(after) == list(before) == keys + ([f"{loss}-full"] if loss == "fape" else [])
        assert np.array_equal(g_before, g_after) and np.abs(g_before).max() > 0
        assert all(np.asarray(after[k], np.float64).tobytes() == np.asarray(before[k], np.float64).tobytes() for k in keys[:-1])
        # --eval_clash reports in evaluation only, and changes no other number there
        args.eval_clash = True
        assert list(_step(model, args, data)[0]) == list(before)
        kw = dict(do_backwards=False, eval_mode=True, return_rmsd=True)
        ev = _step(model, args, data, **kw)[0]
        args.eval_clash = False
        plain = _step(model, args, data, **kw)[0]
        assert list(ev) == list(plain) + ["clash-full"] and np.isfinite(float(ev["clash-full"]))
        assert all(np.asarray(ev[k], np.float64).tobytes() == np.asarray(plain[k], np.float64).tobytes() for k in plain)
        assert float(ev["clash-full"]) == pytest.approx(_clash_alone(model, data, 1.0)[1].mean(), rel=1e-6)


def test_the_flag_is_refused_where_no_side_chains_are_trained():
    model, _, args, batch = _setup("drmsd", clash_weight=W)
    data = tuple(t.to(DEV) for t in batch)
    args.backbone_loss = True
    with pytest.raises(ValueError, match="no side chains are built"):
        _step(model, args, data)
    args.backbone_loss, args.loss = False, "mse"
    with pytest.raises(ValueError, match="build no structure"):
        _step(model, args, data)


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      PTAMD_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from protein_transformer_amd import dp
    from protein_transformer_amd.train import get_losses, train_step
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dp.init_from_env()
    model, opt, args, batch = _setup("drmsd", lens=LENS[:1], clash_weight=W, eval_clash=True)
    dp.attach(model)
    (seq, ang, crd), n_res = _shard(batch, LENS[:1], world, rank)
    assert seq.shape[0] == (1 if rank == 0 else 0)                       # rank 1 is idle: its vector must be as long as rank 0's
    seq, ang, crd = seq.to(dev), ang.to(dev), crd.to(dev)
    step = train_step(model, opt, args, seq, ang, crd, n_res=n_res)
    with torch.no_grad():
        pred = model(seq, ang) if seq.shape[0] else None
        args.clash_weight = 0.0                                          # evaluation under --eval_clash alone
        ev = get_losses(args, pred, ang, crd, seq, do_backwards=False, eval_mode=True, return_rmsd=True, n_res=n_res)
    np.save(os.path.join(out_dir, f"clash{rank}.npy"), np.array([float(step["clash-full"]), float(step["loss"]), float(step["drmsd-full"]),
                                                                  float(ev["clash-full"]), float(ev["drmsd-full"])]))
    dp.barrier()
    dp.shutdown()


def test_two_ranks_one_of_them_idle_report_the_single_process_value(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    from protein_transformer_amd.train import get_losses, train_step
    model, opt, args, batch = _setup("drmsd", lens=LENS[:1], clash_weight=W, eval_clash=True)
    seq, ang, crd = (t.to(DEV) for t in batch)
    step = train_step(model, opt, args, seq, ang, crd)
    with torch.no_grad():
        args.clash_weight = 0.0
        ev = get_losses(args, model(seq, ang), ang, crd, seq, do_backwards=False, eval_mode=True, return_rmsd=True)
    want = np.array([float(step["clash-full"]), float(step["loss"]), float(step["drmsd-full"]), float(ev["clash-full"]),
                     float(ev["drmsd-full"])])
    r0, r1 = np.load(tmp_path / "clash0.npy"), np.load(tmp_path / "clash1.npy")
    print("single process", want, "ranks", r0, r1)
    assert np.array_equal(r0, r1) and np.isfinite(r0).all() and r0[0] > 0
    assert r0[0] == want[0] and r0[1:3] == pytest.approx(want[1:3], rel=1e-6)     # one protein: its fp32 value, exactly
    assert r0[3:] == pytest.approx(want[3:], rel=2e-4)                   # (after one step each: the bar of tests/test_gpu_dp.py)


def test_train_cli_with_both_flags(tmp_path, monkeypatch):
    """`train.py --synthetic 4,32,2 -e 1 -l drmsd --clash_weight 1 --eval_clash` runs to its end and leaves the extra column."""
    from protein_transformer_amd import train as TR
    from protein_transformer_amd.log import prepare_log_header
    monkeypatch.setattr(TR, "START_EPOCH", 0)
    monkeypatch.setattr(sys, "argv", ["train", "--synthetic", "4,32,2", "-e", "1", "-l", "drmsd", "--clash_weight", "1", "--eval_clash",
                                      "--name", "cl", "-dm", "64", "-nl", "2", "-nh", "4", "-dih", "128", "-b", "4", "--max_seq_len", "32",
                                      "--log_dir", str(tmp_path / "logs"), "--chkpt_dir", str(tmp_path / "ck")])
    TR.main()                                                            # (an exit code other than 0 would raise SystemExit)
    rows = list(csv.reader(open(tmp_path / "logs" / "cl.train")))
    plain = prepare_log_header(types.SimpleNamespace(loss="drmsd")).split(",")
    assert rows[0] == plain + ["clash"]
    # (a row always carries the `combined` value, whatever the header lists: log.log_batch)
    columns = prepare_log_header(types.SimpleNamespace(loss="combined")).split(",")
    assert all(len(r) == len(columns) + 1 for r in rows[1:])
    mode, gran = columns.index("mode"), columns.index("granularity")
    steps = [r for r in rows[1:] if r[gran] == "batch"]
    evals = [r for r in rows[1:] if r[gran] == "epoch" and r[mode] != "train"]
    assert len(steps) >= 2 and len(evals) >= 1
    for r in steps + evals:                                              # a value in Angstrom per atom on every such row
        assert np.isfinite(float(r[-1])) and float(r[-1]) >= 0, r
    assert all(np.isfinite([float(v) for v in r[:3]]).all() for r in rows[1:])
