"""The host logic of losses.LossReport without a GPU: `pack_local` / `unpack_local` (what a single process reports) and
`reduce_vector` / `unpack_global` (what the ranks of a data-parallel job reduce) on CPU tensors.

Every input is a multiple of 1/8 that is exact in fp32, every sum of them is exact in fp64 and every expected mean is formed by
the same single fp64 division, so every comparison is `==`: no tolerance is involved."""
import itertools
import json
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from protein_transformer_amd.losses import VECTOR_SIZE, VECTOR_SLOTS, pack_local, reduce_vector, unpack_global, unpack_local
from test_dp_gloo import _free_port, _join_gloo

NAN = float("nan")
B = 3
STATS = (torch.arange(B * 8, dtype=torch.float32).reshape(B, 8) * 3 + 4) / 8
MSE = torch.tensor([1.5, 4.0, 0.75, 2.0, 0.25, 2.0])
STATUS = torch.tensor([0b1001], dtype=torch.int32)                 # bit 3 and bit 0
RMSD = torch.tensor([1.25, 2.5, 0.375])
CHANNELS = {"lddt": torch.tensor([[0.5, 0.25], [NAN, 0.75], [0.875, NAN]]), "slddt": torch.tensor([0.125, NAN, 0.625]),
            "fape": torch.tensor([1.5, 2.25, NAN])}
KEYS = {"lddt": ("lddt", "lddt-ca"), "slddt": ("slddt",), "fape": ("fape",)}      # field -> the keys of its columns


def finite_mean(x):
    """np.mean of the fp64-cast values over their finite entries; NaN when there is none."""
    x = np.asarray(x, np.float32).astype(np.float64)
    return float(np.mean(x[np.isfinite(x)])) if np.isfinite(x).any() else NAN


def plain(report):
    """A `wait()` dictionary with its one array turned into a list, so that two of them compare with ==."""
    return {k: (np.asarray(v).tolist() if k == "mse" and v is not None else v) for k, v in report.items()}


# ----------------------------------------------------------------------------- a single process
@pytest.mark.parametrize("with_stats", [True, False])
@pytest.mark.parametrize("present", list(itertools.product([False, True], repeat=4)), ids=lambda p: "".join("ny"[x] for x in p))
def test_round_trip_of_a_single_process(with_stats, present):
    has = dict(zip(("rmsd", "lddt", "slddt", "fape"), present))
    channels = {field: (t if has[field] else None) for field, t in CHANNELS.items()}
    buf, layout = pack_local(STATS if with_stats else None, MSE, STATUS, RMSD if has["rmsd"] else None, channels)
    rows = B if with_stats or any(present) else 0
    assert buf.dtype == torch.float32
    assert buf.numel() == rows * 8 + 7 + rows + sum(len(KEYS[f]) * B for f in CHANNELS if has[f])
    out = unpack_local(buf.numpy(), layout, n_res=41)
    assert list(out) == ["drmsd", "lndrmsd", "drmsd-bb", "lndrmsd-bb", "rmsd", "n_proteins", "status", "n_res", "mse", "lddt",
                         "lddt-ca", "slddt", "fape"]
    st = STATS.numpy().astype(np.float64)
    for k, key in enumerate(("drmsd", "lndrmsd", "drmsd-bb", "lndrmsd-bb")):
        assert out[key] == (np.mean(st[:, k]) if with_stats else 0.0)
    assert out["n_proteins"] == (B if with_stats else 0) and out["n_res"] == 41
    assert out["status"] == 0b1001 and isinstance(out["status"], int)                    # the word survives bit for bit
    assert out["mse"].dtype == np.float64 and out["mse"].tolist() == MSE.tolist()
    assert out["rmsd"] == (np.mean(RMSD.numpy().astype(np.float64)) if has["rmsd"] else None)
    for field, keys in KEYS.items():
        for k, key in enumerate(keys):
            want = finite_mean(CHANNELS[field].reshape(B, -1)[:, k]) if has[field] else None
            assert out[key] == want and (want is None or np.isfinite(want)), key
    # the fields lie in the declared order, each behind the one before it
    at = layout[1]
    assert list(at) == [f for f in ("stats", "mse", "status", "rmsd", "lddt", "slddt", "fape") if f == "mse" or f == "status"
                        or (f == "stats" and with_stats) or has.get(f)]
    assert layout[0] == rows and at["mse"] == slice(rows * 8, rows * 8 + 6) and at["status"] == slice(rows * 8 + 6, rows * 8 + 7)
    ends = [rows * 9 + 7] + [at[f].stop for f in CHANNELS if has[f]]
    assert [at[f].start for f in CHANNELS if has[f]] == ends[:-1] and ends[-1] == buf.numel()


def test_nothing_passed_and_channels_without_a_finite_value():
    buf, layout = pack_local()
    assert buf.numel() == 7 and layout == (0, {})
    out = unpack_local(buf.numpy(), layout)
    assert plain(out) == {"drmsd": 0.0, "lndrmsd": 0.0, "drmsd-bb": 0.0, "lndrmsd-bb": 0.0, "rmsd": None, "n_proteins": 0,
                          "status": 0, "n_res": None, "mse": None, "lddt": None, "lddt-ca": None, "slddt": None, "fape": None}
    hollow = {"lddt": torch.tensor([[NAN, 1.0], [NAN, 0.5], [NAN, NAN]]), "slddt": torch.full((B,), NAN),
              "fape": torch.tensor([NAN, float("inf"), -float("inf")])}
    buf, layout = pack_local(STATS, MSE, STATUS, RMSD, hollow)
    out = unpack_local(buf.numpy(), layout)
    assert np.isnan(out["lddt"]) and out["lddt-ca"] == 0.75 and np.isnan(out["slddt"]) and np.isnan(out["fape"])
    for word in (0, 0b1000, 0b1111, -2 ** 31, 2 ** 31 - 1, 0x7FC00000):        # bit patterns of -0.0, a NaN, a denormal among them
        buf, layout = pack_local(STATS, MSE, torch.tensor([word], dtype=torch.int32), RMSD)
        assert unpack_local(buf.numpy(), layout)["status"] == word


# ----------------------------------------------------------------------------- the layouts
def test_the_reduced_vector_keeps_its_slots():
    assert VECTOR_SIZE == 27 and list(VECTOR_SLOTS.items()) == [
        ("sums", slice(0, 4)), ("proteins", slice(4, 5)), ("rmsd_sum", slice(5, 6)), ("mse", slice(6, 12)),
        ("status_bits", slice(12, 16)), ("residues", slice(16, 17)), ("rmsd_proteins", slice(17, 18)),
        ("ranks_counted", slice(18, 19)), ("lddt", slice(19, 23)), ("slddt", slice(23, 25)), ("fape", slice(25, 27))]
    v = reduce_vector(STATS, MSE, STATUS, RMSD, 41, CHANNELS)
    assert v.dtype == torch.float64 and v.shape == (27,)
    assert v.tolist() == (STATS[:, :4].double().sum(0).tolist() + [3.0, 4.125] + MSE.tolist() + [1.0, 0.0, 0.0, 1.0]
                          + [41.0, 3.0, 1.0] + [1.375, 1.0, 2.0, 2.0] + [0.75, 2.0] + [3.75, 2.0])
    assert reduce_vector().tolist() == [0.0] * 27                  # an empty shard adds nothing


def test_the_columns_of_lddt_are_two_channels():
    lddt = torch.tensor([[0.5, 0.125], [0.75, 0.25], [1.0, 0.375]])
    buf, layout = pack_local(STATS, MSE, STATUS, RMSD, {"lddt": lddt})
    assert layout[1]["lddt"] == slice(B * 9 + 7, B * 11 + 7) and buf[layout[1]["lddt"]].tolist() == lddt.reshape(-1).tolist()
    out = unpack_local(buf.numpy(), layout)
    assert (out["lddt"], out["lddt-ca"], out["slddt"], out["fape"]) == (0.75, 0.25, None, None)
    v = reduce_vector(channels={"lddt": lddt}).numpy()
    assert v[19:23].tolist() == [2.25, 0.75, 3.0, 3.0]
    out = unpack_global(v, passed={"lddt"})
    assert (out["lddt"], out["lddt-ca"]) == (0.75, 0.25)


# ----------------------------------------------------------------------------- the global batch
def rank_inputs(rank, with_n_res=True):
    """(arguments of reduce_vector, fields passed) of three contributors: two proteins (one without a smooth lDDT, one without a
    FAPE), one protein, and an empty shard that passes None for everything."""
    if rank == 2:
        return {}, set()
    rows = slice(0, 2) if rank == 0 else slice(2, 3)
    channels = {"lddt": CHANNELS["lddt"][rows], "slddt": torch.tensor([[NAN, 0.625], [0.125]][rank]),
                "fape": torch.tensor([[1.5, NAN], [2.25]][rank])}
    return dict(stats=STATS[rows], mse=MSE * (rank + 1), status=torch.tensor([[0b0001], [0b1000]][rank], dtype=torch.int32),
                rmsd=RMSD[rows], n_res=[17, 5][rank] if with_n_res else None, channels=channels), set(channels)


def global_by_hand(n_res):
    sums = STATS[:, :4].double().sum(0).numpy()
    return {"drmsd": sums[0] / 3.0, "lndrmsd": sums[1] / 3.0, "drmsd-bb": sums[2] / 3.0, "lndrmsd-bb": sums[3] / 3.0,
            "rmsd": 4.125 / 3.0, "n_proteins": 3, "status": 0b1001, "n_res": n_res, "mse": (MSE.double() * 3).tolist(),
            "lddt": 1.375 / 2.0, "lddt-ca": 1.0 / 2.0, "slddt": 0.75 / 2.0, "fape": 3.75 / 2.0}


@pytest.mark.parametrize("with_n_res", [True, False])
def test_the_global_batch_in_one_process(with_n_res):
    parts = [rank_inputs(r, with_n_res) for r in range(3)]
    v = sum(reduce_vector(**kw) for kw, _ in parts).numpy()
    want = global_by_hand(22 if with_n_res else None)
    for _, passed in parts:                  # the empty shard reads the same numbers, `slddt` and `fape` it never passed included
        assert plain(unpack_global(v, passed)) == want
    assert not any(isinstance(x, float) and x != x for x in want.values())


def test_a_channel_nobody_asked_for_stays_none_and_one_without_a_value_is_nan():
    kw, _ = rank_inputs(0)
    kw["channels"] = {"slddt": torch.tensor([NAN, NAN])}
    v = (reduce_vector(**kw) + reduce_vector()).numpy()
    out = unpack_global(v, {"slddt"})
    assert out["lddt"] is None and out["lddt-ca"] is None and out["fape"] is None and np.isnan(out["slddt"])
    assert unpack_global(v)["slddt"] is None and unpack_global(v)["n_proteins"] == 2       # the rank that passed nothing


def _report_worker(rank, world, port, out_dir):
    dp = _join_gloo(rank, world, port)
    kw, passed = rank_inputs(rank)
    out = unpack_global(dp.all_reduce_sum_(reduce_vector(**kw)).numpy(), passed)
    with open(os.path.join(out_dir, f"report{rank}.json"), "w") as f:
        json.dump(plain(out), f)
    dp.barrier()
    dp.shutdown()


def test_the_global_batch_through_gloo(tmp_path):
    mp.spawn(_report_worker, args=(3, _free_port(), str(tmp_path)), nprocs=3, join=True)
    for rank in range(3):
        with open(tmp_path / f"report{rank}.json") as f:
            assert json.load(f) == global_by_hand(22), rank
