"""What `-l slddt` needs without a GPU: the choice and its two flags on the command line, the refusal of `--backbone_loss` with
it, the early-stopping target, the metrics dictionaries with and without it, the entry points' host-side checks and the host
mirror's signatures."""
import inspect
import types

import pytest
import torch

OLD_LOSSES = ("mse", "drmsd", "lndrmsd", "combined")


@pytest.fixture(scope="module")
def built_lib():
    from protein_transformer_amd import _lib, build
    build.build()                       # hipcc cross-compiles gfx950 without a GPU
    return _lib


def test_parser_accepts_the_loss_and_its_flags():
    from protein_transformer_amd.train import create_parser
    a = create_parser().parse_args(["-l", "slddt"])
    assert a.loss == "slddt" and a.slddt_cutoff == 15.0 and a.slddt_temperature == 1.0 and a.backbone_loss is False
    a = create_parser().parse_args(["--loss", "slddt", "--slddt_cutoff", "12.5", "--slddt_temperature", "0.25", "--eval_lddt"])
    assert (a.slddt_cutoff, a.slddt_temperature, a.eval_lddt) == (12.5, 0.25, True)
    d = create_parser().parse_args([])                      # the flags exist under every loss and change nothing there
    assert d.loss == "combined" and d.slddt_cutoff == 15.0 and d.slddt_temperature == 1.0


def test_parser_refuses_the_backbone_flag_and_bad_numbers(capsys):
    from protein_transformer_amd.train import create_parser
    with pytest.raises(SystemExit) as e:
        create_parser().parse_args(["-l", "slddt", "--backbone_loss"])
    assert e.value.code == 2
    assert "slddt" in capsys.readouterr().err
    for bad in (["--slddt_cutoff", "0"], ["--slddt_temperature", "-1"], ["--slddt_temperature", "nan"], ["--slddt_cutoff", "inf"]):
        with pytest.raises(SystemExit):
            create_parser().parse_args(["-l", "slddt"] + bad)
    for loss in OLD_LOSSES:                                 # the flag keeps working where it did
        assert create_parser().parse_args(["-l", loss, "--backbone_loss"]).backbone_loss is True


def test_early_stopping_target():
    from protein_transformer_amd.train import create_parser, early_stopping_target
    assert early_stopping_target(create_parser().parse_args(["-l", "slddt"])) == ("train", "slddt")
    assert early_stopping_target(create_parser().parse_args(["-l", "slddt", "-esm", "valid-70-slddt"])) == ("valid-70", "slddt")
    assert early_stopping_target(create_parser().parse_args(["-l", "slddt", "-esm", "valid-70-drmsd"])) == ("valid-70", "drmsd")
    for loss in OLD_LOSSES:
        assert early_stopping_target(create_parser().parse_args(["-l", loss])) == ("train", loss)


def _losses(slddt=None):
    out = {"loss": 1.5, "drmsd-full": 1.5, "lndrmsd-full": 0.01, "drmsd-bb": 1.0, "lndrmsd-bb": 0.02, "combined-full": 0.7,
           "mse-full": 0.25, "mse-bb": 0.2, "mse-sc": 0.3, "rmsd-full": None, "n-residues": 100}
    if slddt is not None:
        out.update({"loss": slddt, "slddt-full": slddt})
    return out


def _epoch(loss, values):
    from protein_transformer_amd import log
    args = types.SimpleNamespace(loss=loss, lr_scheduling="plateau")
    metrics = log.init_metrics(args)
    log.reset_metrics_for_epoch(metrics, "train")
    for v in values:
        log.update_metrics(metrics, _losses(v if loss == "slddt" else None), "train", None, tracking_loss=0.0)
    log.update_metrics_end_of_epoch(metrics, "train")
    return metrics


def test_metrics_track_the_loss_only_in_its_own_runs():
    from protein_transformer_amd import log
    m = _epoch("slddt", [0.5, 0.25])
    t = m["train"]
    assert t["batch-slddt-full"] == 0.25 and t["epoch-slddt-full"] == 0.375 and t["epoch-history-slddt"] == [0.375]
    assert t["epoch-drmsd-full"] == 1.5 and t["epoch-history-drmsd"] == [1.5]
    for split in m:
        if isinstance(m[split], dict) and split != "train":
            assert m[split]["epoch-history-slddt"] == []
    # early stopping, the plateau scheduler and the checkpoint policy read `epoch-<es_metric>-full` and the history: lower is better
    args = types.SimpleNamespace(es_mode="train", es_metric="slddt", early_stopping_threshold=0.001, early_stopping=1)
    log.update_loss_trackers(args, 0, m)
    assert m["loss_to_compare"] == 0.375 and m["losses_to_compare"] == [0.375] and m["best_valid_loss_so_far"] == 0.375
    assert m["epoch_last_improved"] == 0
    log.reset_metrics_for_epoch(m, "train")
    assert m["train"]["epoch-slddt-full"] == 0 and m["train"]["epoch-history-slddt"] == [0.375]
    log.update_metrics(m, _losses(0.125), "train", None, tracking_loss=0.0)
    log.update_metrics_end_of_epoch(m, "train")
    log.update_loss_trackers(args, 1, m)
    assert m["best_valid_loss_so_far"] == 0.125 and m["epoch_last_improved"] == 1 and m["losses_to_compare"] == [0.375, 0.125]
    # a split that appears later (an evaluation mode of its own) is tracked the same way
    log.reset_metrics_for_epoch(m, "valid-extra")
    assert m["valid-extra"]["epoch-history-slddt"] == [] and m["valid-extra"]["epoch-slddt-full"] == 0
    # the CSV is what it is for every loss but `combined`
    assert log.prepare_log_header(types.SimpleNamespace(loss="slddt")) == log.prepare_log_header(types.SimpleNamespace(loss="drmsd"))


def test_the_four_existing_losses_keep_their_keys():
    today = {"epoch-history-drmsd", "epoch-history-combined", "epoch-history-lndrmsd", "epoch-history-mse", "batch-history",
             "speed-history", "batch-time", "speed", "speeds"}
    for k in ("drmsd-full", "lndrmsd-full", "mse-full", "combined-full", "rmsd-full", "drmsd-bb", "lndrmsd-bb", "mse-bb", "mse-sc"):
        today |= {f"epoch-{k}", f"batch-{k}"}
    for loss in OLD_LOSSES:
        m = _epoch(loss, [None, None])
        assert set(m["train"]) == today, loss
        assert not any("slddt" in k for split in m.values() if isinstance(split, dict) for k in split), loss
        assert set(m) == set(_epoch("slddt", [0.5])), loss            # the top level is the same in both kinds of run
    assert set(_epoch("slddt", [0.5])["train"]) == today | {"epoch-history-slddt", "epoch-slddt-full", "batch-slddt-full"}


def test_entry_points_host_side_checks(built_lib):
    lib = built_lib.lib()
    assert not built_lib.MISSING and "ptamd_slddt_fwd_bwd" in built_lib.SIGNATURES and "ptamd_slddt_workspace_bytes" in built_lib.SIGNATURES
    need = lib.ptamd_slddt_workspace_bytes(32, 512)
    assert 32 * 512 * 14 * 32 < need < 200 << 20               # 32 B per atom slot + the partial sums of the triangle
    assert need == lib.ptamd_slddt_workspace_bytes(32, 512)    # a function of (B, L) only
    assert lib.ptamd_slddt_workspace_bytes(0, 512) == 0 and lib.ptamd_slddt_workspace_bytes(32, 0) == 0
    assert lib.ptamd_slddt_workspace_bytes(1, (2 ** 31 - 1) // 28 + 1) == 0
    one = torch.zeros(64).data_ptr()
    null3, ok3 = (None,) * 3, (one,) * 3
    assert lib.ptamd_slddt_fwd_bwd(*null3, 0, 8, 15.0, 1.0, None, None, None, None, 0, None) == -1        # PTAMD_ERR_BAD_SHAPE
    assert lib.ptamd_slddt_fwd_bwd(*null3, 2, 8, 15.0, 1.0, None, None, None, None, 0, None) == -1        # null arrays
    assert lib.ptamd_slddt_fwd_bwd(*ok3, 2, 8, 15.0, 1.0, one, None, one, one, 1 << 30, None) == -1       # npairs is not optional
    for cutoff, tau in ((float("nan"), 1.0), (0.0, 1.0), (15.0, 0.0), (15.0, float("inf")), (-15.0, 1.0), (15.0, -1.0)):
        assert lib.ptamd_slddt_fwd_bwd(*ok3, 2, 8, cutoff, tau, one, one, one, one, 1 << 30, None) == -1
    assert lib.ptamd_slddt_fwd_bwd(*ok3, 2, 8, 15.0, 1.0, one, one, None, None, 1 << 30, None) == -3      # PTAMD_ERR_WORKSPACE
    assert lib.ptamd_slddt_fwd_bwd(*ok3, 2, 8, 15.0, 1.0, one, one, None, one, lib.ptamd_slddt_workspace_bytes(2, 8) - 1, None) == -3


def test_host_mirror_signatures_and_no_cpu_path(built_lib):
    from protein_transformer_amd import losses
    sig = inspect.signature(losses.slddt_forward_backward).parameters
    assert list(sig) == ["crd", "true_crds", "seq", "need_grad", "cutoff", "temperature"]
    assert sig["cutoff"].default == 15.0 and sig["temperature"].default == 1.0
    assert inspect.signature(losses.batch_loss).parameters["slddt"].default is None       # today's calls are untouched
    assert inspect.signature(losses.LossReport.__init__).parameters["fields"].default is None      # (fields={"slddt": values})
    assert losses.REPORT_KEYS["slddt"] == ("slddt",)
    assert losses.VECTOR_SIZE == 27 and losses.VECTOR_SLOTS == {        # the reduced vector: every slot where it has always been
        "sums": slice(0, 4), "proteins": slice(4, 5), "rmsd_sum": slice(5, 6), "mse": slice(6, 12), "status_bits": slice(12, 16),
        "residues": slice(16, 17), "rmsd_proteins": slice(17, 18), "ranks_counted": slice(18, 19), "lddt": slice(19, 23),
        "slddt": slice(23, 25), "fape": slice(25, 27)}
    with pytest.raises(RuntimeError, match="device tensors only"):      # a missing GPU is an error, never a CPU fall-back
        losses.slddt_forward_backward(torch.zeros(1, 28, 3), torch.zeros(1, 28, 3), torch.zeros(1, 2, dtype=torch.int64))
