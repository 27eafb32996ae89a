"""Data parallelism under `--backbone_loss`, as tests/test_gpu_dp.py does it for the full-atom loss: two ranks share cuda:0
and exchange gradients and loss statistics through gloo; the sharded, SUM-reduced step must reproduce the single-process step
on the whole batch - same bar (update within 1e-4 of its norm, identical statistics on both ranks)."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu


def _worker(rank, world, port, out_dir, loss, case):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", PTAMD_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import test_gpu_dp as base
    from protein_transformer_amd import dp
    from protein_transformer_amd.train import train_step
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dp.init_from_env()
    model, opt, args, batch, lens = base._make(dev, loss, case)
    args.backbone_loss = True
    dp.attach(model)
    (seq, ang, crd), n_res = base._shard(batch, lens, world, rank)
    losses = train_step(model, opt, args, seq.to(dev), ang.to(dev), crd.to(dev), n_res=n_res)
    assert losses["n-residues"] == sum(lens)
    np.save(os.path.join(out_dir, f"flat{rank}.npy"), model.flat_parameters()[0].cpu().numpy())
    np.save(os.path.join(out_dir, f"loss{rank}.npy"), np.array([float(losses[k]) for k in base.KEYS]))
    dp.barrier()
    dp.shutdown()


@pytest.mark.parametrize("loss,case", [("drmsd", "ragged"), ("combined", "ragged")])
def test_two_rank_backbone_step_equals_full_batch(tmp_path, loss, case):
    import test_gpu_dp as base
    from protein_transformer_amd.train import train_step
    assert torch.cuda.is_available()
    mp.spawn(_worker, args=(2, base._free_port(), str(tmp_path), loss, case), nprocs=2, join=True)
    dev = torch.device("cuda:0")
    model, opt, args, batch, lens = base._make(dev, loss, case)
    args.backbone_loss = True
    start = model.flat_parameters()[0].cpu().numpy().copy()
    losses = train_step(model, opt, args, *(t.to(dev) for t in batch))
    full = model.flat_parameters()[0].cpu().numpy()
    f0, f1 = np.load(tmp_path / "flat0.npy"), np.load(tmp_path / "flat1.npy")
    assert np.array_equal(f0, f1)                                   # ranks stay in lock step (also an idle one)
    upd, upd_dp = full - start, f0 - start
    assert np.linalg.norm(upd) > 0
    assert np.linalg.norm(upd_dp - upd) <= 1e-4 * np.linalg.norm(upd)
    l0, l1 = np.load(tmp_path / "loss0.npy"), np.load(tmp_path / "loss1.npy")
    assert np.array_equal(l0, l1)                                   # every rank reports the GLOBAL statistics
    assert l0 == pytest.approx(np.array([float(losses[k]) for k in base.KEYS]), rel=1e-5, abs=1e-7)
    # under the flag the step really was the backbone one: `loss` is a backbone number and the `-full` keys repeat it
    k = {"drmsd": "drmsd-bb", "lndrmsd": "lndrmsd-bb"}.get(loss)
    if k:
        assert float(losses["loss"]) == float(losses[k])
    assert float(losses["drmsd-full"]) == float(losses["drmsd-bb"])
