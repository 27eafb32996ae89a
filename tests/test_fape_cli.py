"""What `-l fape` needs without a GPU: the choice and its flag on the command line, the refusal of `--backbone_loss` with it, the
early-stopping target, the metrics dictionaries with and without it (those of `-l slddt` runs unchanged), the entry points'
host-side checks and the host mirror's signatures."""
import inspect
import types

import pytest
import torch

OLD_LOSSES = ("mse", "drmsd", "lndrmsd", "combined", "slddt")


@pytest.fixture(scope="module")
def built_lib():
    from protein_transformer_amd import _lib, build
    build.build()                       # hipcc cross-compiles gfx950 without a GPU
    return _lib


def test_parser_accepts_the_loss_and_its_flag():
    from protein_transformer_amd.train import create_parser
    a = create_parser().parse_args(["-l", "fape"])
    assert a.loss == "fape" and a.fape_clamp == 10.0 and a.backbone_loss is False
    a = create_parser().parse_args(["--loss", "fape", "--fape_clamp", "12.5", "--eval_lddt"])
    assert (a.fape_clamp, a.eval_lddt) == (12.5, True)
    assert create_parser().parse_args(["-l", "fape", "--fape_clamp", "inf"]).fape_clamp == float("inf")      # unclamped
    d = create_parser().parse_args([])                      # the flag exists under every loss and changes nothing there
    assert d.loss == "combined" and d.fape_clamp == 10.0


def test_parser_refuses_the_backbone_flag_and_bad_numbers(capsys):
    from protein_transformer_amd.train import create_parser
    with pytest.raises(SystemExit) as e:
        create_parser().parse_args(["-l", "fape", "--backbone_loss"])
    assert e.value.code == 2
    assert "fape" in capsys.readouterr().err
    for bad in ("0", "-1", "nan", "-inf"):
        with pytest.raises(SystemExit):
            create_parser().parse_args(["-l", "fape", "--fape_clamp", bad])
    for loss in ("mse", "drmsd", "lndrmsd", "combined"):    # the flag keeps working where it did
        assert create_parser().parse_args(["-l", loss, "--backbone_loss"]).backbone_loss is True


def test_get_losses_refuses_the_backbone_flag_before_any_device_work():
    from protein_transformer_amd.train import get_losses
    args = types.SimpleNamespace(loss="fape", backbone_loss=True, fape_clamp=10.0)
    with pytest.raises(ValueError, match="fape"):
        get_losses(args, None, None, None, torch.zeros(0, 4, dtype=torch.int64))


def test_early_stopping_target():
    from protein_transformer_amd.train import create_parser, early_stopping_target
    assert early_stopping_target(create_parser().parse_args(["-l", "fape"])) == ("train", "fape")
    assert early_stopping_target(create_parser().parse_args(["-l", "fape", "-esm", "valid-70-fape"])) == ("valid-70", "fape")
    assert early_stopping_target(create_parser().parse_args(["-l", "fape", "-esm", "valid-70-drmsd"])) == ("valid-70", "drmsd")
    for loss in OLD_LOSSES:
        assert early_stopping_target(create_parser().parse_args(["-l", loss])) == ("train", loss)


def _losses(extra=None, value=None):
    out = {"loss": 1.5, "drmsd-full": 1.5, "lndrmsd-full": 0.01, "drmsd-bb": 1.0, "lndrmsd-bb": 0.02, "combined-full": 0.7,
           "mse-full": 0.25, "mse-bb": 0.2, "mse-sc": 0.3, "rmsd-full": None, "n-residues": 100}
    if extra is not None:
        out.update({"loss": value, f"{extra}-full": value})
    return out


def _epoch(loss, values):
    from protein_transformer_amd import log
    args = types.SimpleNamespace(loss=loss, lr_scheduling="plateau")
    metrics = log.init_metrics(args)
    log.reset_metrics_for_epoch(metrics, "train")
    for v in values:
        log.update_metrics(metrics, _losses(loss if loss in ("slddt", "fape") else None, v), "train", None, tracking_loss=0.0)
    log.update_metrics_end_of_epoch(metrics, "train")
    return metrics


def test_metrics_track_the_loss_only_in_its_own_runs():
    from protein_transformer_amd import log
    m = _epoch("fape", [0.5, 0.25])
    t = m["train"]
    assert t["batch-fape-full"] == 0.25 and t["epoch-fape-full"] == 0.375 and t["epoch-history-fape"] == [0.375]
    assert t["epoch-drmsd-full"] == 1.5 and t["epoch-history-drmsd"] == [1.5]
    for split in m:
        if isinstance(m[split], dict) and split != "train":
            assert m[split]["epoch-history-fape"] == []
    # early stopping, the plateau scheduler and the checkpoint policy read `epoch-<es_metric>-full` and the history: lower is better
    args = types.SimpleNamespace(es_mode="train", es_metric="fape", early_stopping_threshold=0.001, early_stopping=1)
    log.update_loss_trackers(args, 0, m)
    assert m["loss_to_compare"] == 0.375 and m["losses_to_compare"] == [0.375] and m["epoch_last_improved"] == 0
    log.reset_metrics_for_epoch(m, "train")
    assert m["train"]["epoch-fape-full"] == 0 and m["train"]["epoch-history-fape"] == [0.375]
    # a split that appears later (an evaluation mode of its own) is tracked the same way
    log.reset_metrics_for_epoch(m, "valid-extra")
    assert m["valid-extra"]["epoch-history-fape"] == [] and m["valid-extra"]["epoch-fape-full"] == 0
    assert log.prepare_log_header(types.SimpleNamespace(loss="fape")) == log.prepare_log_header(types.SimpleNamespace(loss="drmsd"))


def test_every_other_run_keeps_its_keys():
    today = {"epoch-history-drmsd", "epoch-history-combined", "epoch-history-lndrmsd", "epoch-history-mse", "batch-history",
             "speed-history", "batch-time", "speed", "speeds"}
    for k in ("drmsd-full", "lndrmsd-full", "mse-full", "combined-full", "rmsd-full", "drmsd-bb", "lndrmsd-bb", "mse-bb", "mse-sc"):
        today |= {f"epoch-{k}", f"batch-{k}"}
    for loss in OLD_LOSSES:
        m = _epoch(loss, [0.5, 0.5])
        own = {"epoch-history-slddt", "epoch-slddt-full", "batch-slddt-full"} if loss == "slddt" else set()
        assert set(m["train"]) == today | own, loss
        assert not any("fape" in k for split in m.values() if isinstance(split, dict) for k in split), loss
        assert set(m) == set(_epoch("fape", [0.5])), loss              # the top level is the same in every kind of run
    fape = _epoch("fape", [0.5])
    assert set(fape["train"]) == today | {"epoch-history-fape", "epoch-fape-full", "batch-fape-full"}
    assert list(_epoch("slddt", [0.5])["train"])[:5] == ["epoch-history-drmsd", "epoch-history-combined", "epoch-history-lndrmsd",
                                                         "epoch-history-mse", "epoch-history-slddt"]     # and their order


def test_entry_points_host_side_checks(built_lib):
    lib = built_lib.lib()
    assert not built_lib.MISSING and "ptamd_fape_fwd_bwd" in built_lib.SIGNATURES and "ptamd_fape_workspace_bytes" in built_lib.SIGNATURES
    need = lib.ptamd_fape_workspace_bytes(32, 512)
    assert 32 * 512 * (14 * 32 + 100) < need < 64 << 20        # 32 B per atom slot, 100 B per residue + the frame-side partial sums
    assert need == lib.ptamd_fape_workspace_bytes(32, 512)     # a function of (B, L) only
    assert lib.ptamd_fape_workspace_bytes(1, 1) > 0
    assert lib.ptamd_fape_workspace_bytes(0, 512) == 0 and lib.ptamd_fape_workspace_bytes(32, 0) == 0
    assert lib.ptamd_fape_workspace_bytes(-1, 8) == 0 and lib.ptamd_fape_workspace_bytes(1, (2 ** 31 - 1) // 28 + 1) == 0
    one = torch.zeros(64).data_ptr()
    null3, ok3 = (None,) * 3, (one,) * 3
    assert lib.ptamd_fape_fwd_bwd(*null3, 0, 8, 10.0, None, None, None, None, None, 0, None) == -1        # PTAMD_ERR_BAD_SHAPE
    assert lib.ptamd_fape_fwd_bwd(*null3, 2, 8, 10.0, None, None, None, None, None, 0, None) == -1        # null arrays
    assert lib.ptamd_fape_fwd_bwd(*ok3, 2, 8, 10.0, one, None, one, one, one, 1 << 30, None) == -1        # npairs is not optional
    assert lib.ptamd_fape_fwd_bwd(*ok3, 2, 8, 10.0, one, one, None, one, one, 1 << 30, None) == -1        # nor is nclamped
    for clamp in (float("nan"), 0.0, -10.0, -float("inf")):
        assert lib.ptamd_fape_fwd_bwd(*ok3, 2, 8, clamp, one, one, one, one, one, 1 << 30, None) == -1
    assert lib.ptamd_fape_fwd_bwd(*ok3, 2, 8, 10.0, one, one, one, None, None, 1 << 30, None) == -3       # PTAMD_ERR_WORKSPACE
    assert lib.ptamd_fape_fwd_bwd(*ok3, 2, 8, float("inf"), one, one, one, None, one, lib.ptamd_fape_workspace_bytes(2, 8) - 1, None) == -3


def test_host_mirror_signatures_and_no_cpu_path(built_lib):
    from protein_transformer_amd import losses
    sig = inspect.signature(losses.fape_forward_backward).parameters
    assert list(sig) == ["crd", "true_crds", "seq", "need_grad", "clamp"]
    assert sig["clamp"].default == 10.0 and sig["need_grad"].default is True
    assert inspect.signature(losses.batch_loss).parameters["fape"].default is None        # today's calls are untouched
    fixed = [f.name for f in losses.REPORT_FIELDS if f.fixed]
    assert fixed[-1] == "fape" and fixed[-2] == "slddt"                                   # behind the existing ones
    assert inspect.signature(losses.LossReport.__init__).parameters["fields"].default is None      # (fields={"fape": values})
    with pytest.raises(RuntimeError, match="device tensors only"):      # a missing GPU is an error, never a CPU fall-back
        losses.fape_forward_backward(torch.zeros(1, 28, 3), torch.zeros(1, 28, 3), torch.zeros(1, 2, dtype=torch.int64))
