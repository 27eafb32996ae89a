"""What `-l kabsch` needs without a GPU: the choice on the command line, the refusal of `--backbone_loss` with it, the
early-stopping target, the metrics dictionaries with and without it (those of every other run unchanged), the loss report's
`kabsch` field - it travels in the report's tail, so that the layout of every other run stays what it was, and reduces like
`fape`'s channel - and the entry point's host-side checks and the host mirror's signatures."""
import csv
import inspect
import io
import types

import numpy as np
import pytest
import torch

OLD_LOSSES = ("mse", "drmsd", "lndrmsd", "combined", "slddt", "fape")
NAN = float("nan")
B = 3
STATS = (torch.arange(B * 8, dtype=torch.float32).reshape(B, 8) * 3 + 4) / 8
MSE = torch.tensor([1.5, 4.0, 0.75, 2.0, 0.25, 2.0])
STATUS = torch.tensor([0b1001], dtype=torch.int32)
VALUES = torch.tensor([1.5, 2.25, NAN])                                 # exact in fp32, their sums exact in fp64: comparisons are ==


@pytest.fixture(scope="module")
def built_lib():
    from protein_transformer_amd import _lib, build
    build.build()                       # hipcc cross-compiles gfx950 without a GPU
    return _lib


def test_parser_accepts_the_loss():
    from protein_transformer_amd.train import create_parser
    a = create_parser().parse_args(["-l", "kabsch"])
    assert a.loss == "kabsch" and a.backbone_loss is False
    a = create_parser().parse_args(["--loss", "kabsch", "--eval_lddt", "--clash_weight", "0.5", "--rename_symmetric", "--eval_tm"])
    assert (a.loss, a.eval_lddt, a.clash_weight, a.rename_symmetric, a.eval_tm) == ("kabsch", True, 0.5, True, True)
    assert create_parser().parse_args([]).loss == "combined"
    assert "rmsd-full as a loss" in " ".join(create_parser().format_help().split())


def test_parser_refuses_the_backbone_flag(capsys):
    from protein_transformer_amd.losses import EXTRA_LOSSES
    from protein_transformer_amd.train import KABSCH_BACKBONE_MESSAGE, create_parser
    with pytest.raises(SystemExit) as e:
        create_parser().parse_args(["-l", "kabsch", "--backbone_loss"])
    assert e.value.code == 2
    err = " ".join(capsys.readouterr().err.split())
    assert KABSCH_BACKBONE_MESSAGE in err and KABSCH_BACKBONE_MESSAGE == EXTRA_LOSSES["kabsch"].backbone_message
    assert KABSCH_BACKBONE_MESSAGE.startswith("-l kabsch is an all-atom loss: it cannot be combined with --backbone_loss")
    for loss in ("mse", "drmsd", "lndrmsd", "combined"):    # the flag keeps working where it did
        assert create_parser().parse_args(["-l", loss, "--backbone_loss"]).backbone_loss is True
    extra = EXTRA_LOSSES["kabsch"]                           # no parameters: nothing to complain about
    assert extra.check(extra.params(types.SimpleNamespace())) is None and extra.params(types.SimpleNamespace()) is True


def test_get_losses_refuses_the_backbone_flag_before_any_device_work():
    from protein_transformer_amd.train import get_losses
    args = types.SimpleNamespace(loss="kabsch", backbone_loss=True)
    with pytest.raises(ValueError, match="-l kabsch is an all-atom loss"):
        get_losses(args, None, None, None, torch.zeros(0, 4, dtype=torch.int64))


def test_early_stopping_target():
    from protein_transformer_amd.train import create_parser, early_stopping_target
    assert early_stopping_target(create_parser().parse_args(["-l", "kabsch"])) == ("train", "kabsch")
    assert early_stopping_target(create_parser().parse_args(["-l", "kabsch", "-esm", "valid-10-kabsch"])) == ("valid-10", "kabsch")
    assert early_stopping_target(create_parser().parse_args(["-l", "kabsch", "-esm", "valid-70-drmsd"])) == ("valid-70", "drmsd")
    for loss in OLD_LOSSES:
        assert early_stopping_target(create_parser().parse_args(["-l", loss])) == ("train", loss)


def _losses(extra=None, value=None):
    out = {"loss": 1.5, "drmsd-full": 1.5, "lndrmsd-full": 0.01, "drmsd-bb": 1.0, "lndrmsd-bb": 0.02, "combined-full": 0.7,
           "mse-full": 0.25, "mse-bb": 0.2, "mse-sc": 0.3, "rmsd-full": None, "n-residues": 100}
    if extra is not None:
        out.update({"loss": value, f"{extra}-full": value})
    return out


def _epoch(loss, values, mode="train"):
    from protein_transformer_amd import log
    args = types.SimpleNamespace(loss=loss, lr_scheduling="plateau")
    metrics = log.init_metrics(args)
    log.reset_metrics_for_epoch(metrics, mode)
    for v in values:
        log.update_metrics(metrics, _losses(loss if loss in ("slddt", "fape", "kabsch") else None, v), mode, None, tracking_loss=0.0)
    log.update_metrics_end_of_epoch(metrics, mode)
    return metrics


def test_metrics_track_the_loss_only_in_its_own_runs():
    from protein_transformer_amd import log
    m = _epoch("kabsch", [4.5, 2.25])
    t = m["train"]
    assert t["batch-kabsch-full"] == 2.25 and t["epoch-kabsch-full"] == 3.375 and t["epoch-history-kabsch"] == [3.375]
    assert t["epoch-drmsd-full"] == 1.5 and t["epoch-history-drmsd"] == [1.5]
    for split in m:
        if isinstance(m[split], dict) and split != "train":
            assert m[split]["epoch-history-kabsch"] == []
    # early stopping, the plateau scheduler and the checkpoint policy read `epoch-<es_metric>-full` and the history: lower is better
    args = types.SimpleNamespace(es_mode="train", es_metric="kabsch", early_stopping_threshold=0.001, early_stopping=1)
    log.update_loss_trackers(args, 0, m)
    assert m["loss_to_compare"] == 3.375 and m["losses_to_compare"] == [3.375] and m["epoch_last_improved"] == 0
    v = _epoch("kabsch", [4.5], mode="valid-10")            # -esm valid-10-kabsch reads these
    assert v["valid-10"]["epoch-kabsch-full"] == 4.5 and v["valid-10"]["epoch-history-kabsch"] == [4.5]
    log.reset_metrics_for_epoch(m, "valid-extra")           # a split that appears later is tracked the same way
    assert m["valid-extra"]["epoch-history-kabsch"] == [] and m["valid-extra"]["epoch-kabsch-full"] == 0


def test_every_other_run_keeps_its_keys():
    today = {"epoch-history-drmsd", "epoch-history-combined", "epoch-history-lndrmsd", "epoch-history-mse", "batch-history",
             "speed-history", "batch-time", "speed", "speeds"}
    for k in ("drmsd-full", "lndrmsd-full", "mse-full", "combined-full", "rmsd-full", "drmsd-bb", "lndrmsd-bb", "mse-bb", "mse-sc"):
        today |= {f"epoch-{k}", f"batch-{k}"}
    for loss in OLD_LOSSES:
        m = _epoch(loss, [0.5, 0.5])
        own = {f"epoch-history-{loss}", f"epoch-{loss}-full", f"batch-{loss}-full"} if loss in ("slddt", "fape") else set()
        assert set(m["train"]) == today | own, loss
        assert not any("kabsch" in k for split in m.values() if isinstance(split, dict) for k in split), loss
        assert set(m) == set(_epoch("kabsch", [0.5])), loss           # the top level is the same in every kind of run
    assert set(_epoch("kabsch", [0.5])["train"]) == today | {"epoch-history-kabsch", "epoch-kabsch-full", "batch-kabsch-full"}


def test_the_log_keeps_its_columns():
    """As under `-l slddt` and `-l fape` the `.train` file keeps the reference's columns - the run's loss is in the metrics, the
    rmsd column carries the same quantity from the metric's kernel at every evaluation."""
    from protein_transformer_amd import log
    header = log.prepare_log_header(types.SimpleNamespace(loss="kabsch"))
    assert header == log.prepare_log_header(types.SimpleNamespace(loss="drmsd")) and "rmsd" in header.split(",")
    m = _epoch("kabsch", [4.5, 2.25])
    m["train"]["epoch-rmsd-full"] = 3.25
    out = io.StringIO()
    log.log_batch(csv.writer(out), m, 0.0, mode="train", end_of_epoch=True, t=5.0)
    row = out.getvalue().strip().split(",")
    assert len(row) == len(log.prepare_log_header(types.SimpleNamespace(loss="combined")).split(","))
    assert float(row[header.split(",").index("rmsd")]) == 3.25


def test_the_report_field_in_a_single_process():
    from protein_transformer_amd.losses import pack_local, unpack_local
    plain_buf, plain_layout = pack_local(STATS, MSE, STATUS)
    buf, layout = pack_local(STATS, MSE, STATUS, tail={"kabsch": VALUES})
    assert buf.numel() == plain_buf.numel() + B and list(layout[1]) == list(plain_layout[1]) + ["kabsch"]
    for field, at in plain_layout[1].items():                # everything in front lies where it lay
        assert layout[1][field] == at and torch.equal(buf[at].view(torch.int32), plain_buf[at].view(torch.int32)), field
    out, plain = unpack_local(buf.numpy(), layout), unpack_local(plain_buf.numpy(), plain_layout)
    assert "kabsch" not in plain and list(out) == list(plain) + ["kabsch"] and out["kabsch"] == 1.875
    # ... the value `fape`'s channel reports for the same per-protein losses
    fape = pack_local(STATS, MSE, STATUS, None, {"fape": VALUES})
    assert unpack_local(fape[0].numpy(), fape[1])["fape"] == out["kabsch"]
    # behind the other tail fields; asked for without a value: None; without a finite value: NaN
    buf, layout = pack_local(STATS, MSE, STATUS, tail={"clash": VALUES, "kabsch": VALUES})
    assert list(layout[1])[-2:] == ["clash", "kabsch"] and list(unpack_local(buf.numpy(), layout))[-2:] == ["clash", "kabsch"]
    buf, layout = pack_local(tail={"kabsch": None})
    assert buf.numel() == 7 and unpack_local(buf.numpy(), layout)["kabsch"] is None
    buf, layout = pack_local(STATS, MSE, STATUS, tail={"kabsch": torch.full((B,), NAN)})
    assert np.isnan(unpack_local(buf.numpy(), layout)["kabsch"])


def test_the_report_field_over_ranks_reduces_like_fape():
    from protein_transformer_amd.losses import VECTOR_SIZE, VECTOR_SLOTS, reduce_vector, unpack_global
    assert VECTOR_SIZE == 27 and "kabsch" not in VECTOR_SLOTS and reduce_vector(STATS, MSE, STATUS).shape == (27,)
    ranks = [dict(stats=STATS[:2], mse=MSE, status=STATUS, channels={"fape": VALUES[:2]}, tail={"kabsch": VALUES[:2]}),
             dict(stats=STATS[2:], mse=MSE, status=STATUS, channels={"fape": VALUES[2:]}, tail={"kabsch": VALUES[2:]}),
             dict(tail={"kabsch": None})]                     # an empty shard: same length, adds nothing
    vs = [reduce_vector(**kw) for kw in ranks]
    assert [v.shape for v in vs] == [(29,)] * 3 and vs[2].tolist() == [0.0] * 29
    assert vs[0][27:].tolist() == vs[0][VECTOR_SLOTS["fape"]].tolist() == [3.75, 2.0]         # sum and count of the finite values
    assert vs[1][27:].tolist() == vs[1][VECTOR_SLOTS["fape"]].tolist() == [0.0, 0.0]
    v = sum(vs).numpy()
    for passed in ({"fape", "kabsch"}, set()):               # the empty shard reads the same numbers
        out = unpack_global(v, passed, ("kabsch",))
        assert out["kabsch"] == out["fape"] == 1.875 and out["n_proteins"] == 3 and list(out)[-1] == "kabsch"
    assert "kabsch" not in unpack_global(v[:27], {"fape"})
    v = (reduce_vector(stats=STATS, tail={"kabsch": torch.full((B,), NAN)}) + reduce_vector(tail={"kabsch": None})).numpy()
    assert np.isnan(unpack_global(v, {"kabsch"}, ("kabsch",))["kabsch"]) and unpack_global(v, set(), ("kabsch",))["kabsch"] is None


def test_entry_point_host_side_checks(built_lib):
    lib = built_lib.lib()
    assert not built_lib.MISSING and len(built_lib.SIGNATURES["ptamd_kabsch_loss_fwd_bwd"][1]) == 8
    one = torch.zeros(64).data_ptr()
    assert lib.ptamd_kabsch_loss_fwd_bwd(None, None, None, 0, 8, None, None, None) == -1         # PTAMD_ERR_BAD_SHAPE
    assert lib.ptamd_kabsch_loss_fwd_bwd(one, one, one, 0, 8, one, one, None) == -1
    assert lib.ptamd_kabsch_loss_fwd_bwd(one, one, one, 2, 0, one, one, None) == -1
    assert lib.ptamd_kabsch_loss_fwd_bwd(one, one, one, -2, 8, one, None, None) == -1
    assert lib.ptamd_kabsch_loss_fwd_bwd(one, one, one, 1, (2 ** 31 - 1) // 28 + 1, one, None, None) == -1
    for missing in range(3):                                 # a null input array
        arrays = [None if k == missing else one for k in range(3)]
        assert lib.ptamd_kabsch_loss_fwd_bwd(*arrays, 2, 8, one, one, None) == -1
    assert lib.ptamd_kabsch_loss_fwd_bwd(one, one, one, 2, 8, None, one, None) == -1             # stats is not optional


def test_host_mirror_signatures_and_no_cpu_path(built_lib):
    from protein_transformer_amd import losses
    sig = inspect.signature(losses.kabsch_forward_backward).parameters
    assert list(sig) == ["crd", "true_crds", "seq", "need_grad"] and sig["need_grad"].default is True
    assert inspect.signature(losses.batch_loss).parameters["kabsch"].default is None          # today's calls are untouched
    report = inspect.signature(losses.LossReport.__init__).parameters
    assert report["fields"].default is None and "kabsch" not in report    # asked for without a value: fields={"kabsch": None}
    assert list(losses.EXTRA_LOSSES) == ["slddt", "fape", "kabsch"] and losses.REPORT_KEYS["kabsch"] == ("kabsch",)
    assert [f.name for f in losses.REPORT_FIELDS if not f.fixed and f.name in losses.EXTRA_LOSSES] == ["kabsch"]      # in the tail
    with pytest.raises(RuntimeError, match="device tensors only"):      # a missing GPU is an error, never a CPU fall-back
        losses.kabsch_forward_backward(torch.zeros(1, 28, 3), torch.zeros(1, 28, 3), torch.zeros(1, 2, dtype=torch.int64))
    with pytest.raises(AssertionError, match="-l kabsch is an all-atom loss"):
        losses.batch_loss(torch.zeros(1, 2, 24), torch.zeros(1, 28, 3), torch.zeros(1, 2, dtype=torch.int64), backbone_only=True,
                          kabsch=True)
