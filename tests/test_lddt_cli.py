"""What `--eval_lddt` needs without a GPU: the flag on the command line, the CSV header and rows with and without it, the entry
points' host-side checks - and the yardstick of tests/test_gpu_lddt.py itself: its fp64 reference reproduces the known answers
exactly, and for every random case its brackets cover at most 0.1 % of the included pairs."""
import csv
import io
import types

import numpy as np
import pytest

import test_gpu_lddt as G


def test_parser_accepts_the_flag():
    from protein_transformer_amd.train import create_parser
    assert create_parser().parse_args([]).eval_lddt is False
    a = create_parser().parse_args(["--eval_lddt", "-l", "drmsd"])
    assert a.eval_lddt is True and a.loss == "drmsd" and a.backbone_loss is False


def _metrics(with_lddt):
    from protein_transformer_amd import log
    args = types.SimpleNamespace(lr_scheduling="plateau")
    metrics = log.init_metrics(args)
    losses = {k: 0.5 for k in log._TRACKED}
    losses["n-residues"] = 100
    if with_lddt:
        losses.update({"lddt-full": 0.75, "lddt-ca": 0.5})
    log.reset_metrics_for_epoch(metrics, "valid-70")
    log.update_metrics(metrics, losses, "valid-70", None, batch_level=False)
    if with_lddt:                                   # a batch without a scored protein is left out of the epoch's mean
        log.update_metrics(metrics, dict(losses, **{"lddt-full": float("nan"), "lddt-ca": 0.25}), "valid-70", None, batch_level=False)
    return metrics


def _row(metrics, **kw):
    from protein_transformer_amd import log
    out = io.StringIO()
    log.log_batch(csv.writer(out), metrics, 0.0, mode="valid-70", end_of_epoch=True, t=1.0, **kw)
    return out.getvalue().strip().split(",")


def test_csv_header_and_row_without_the_flag_are_unchanged():
    from protein_transformer_amd import log
    for loss, want in (("combined", "drmsd,ln_drmsd,rmse,rmsd,combined,lr,mode,granularity,time,speed"),
                       ("drmsd", "drmsd,ln_drmsd,rmse,rmsd,lr,mode,granularity,time,speed")):
        assert log.prepare_log_header(types.SimpleNamespace(loss=loss)) == want
        assert log.prepare_log_header(types.SimpleNamespace(loss=loss, eval_lddt=False)) == want
        assert log.prepare_log_header(types.SimpleNamespace(loss=loss, eval_lddt=True)) == want + ",lddt,lddt_ca"
    m = _metrics(False)
    log.update_metrics_end_of_epoch(m, "valid-70")
    assert not any("lddt" in k for k in m["valid-70"])
    row = _row(m)
    assert len(row) == 10 and row[6:8] == ["valid-70", "epoch"] and row[0] == "0.5"
    assert _row(m, lddt=False) == row


def test_csv_row_with_the_flag_gains_two_trailing_columns(capsys):
    from protein_transformer_amd import log
    m = _metrics(True)
    log.do_eval_epoch_logging(m, "valid-70")
    assert m["valid-70"]["epoch-lddt-full"] == 0.75 and m["valid-70"]["epoch-lddt-ca"] == 0.375
    assert "lddt-full 0.7500  lddt-ca 0.3750" in capsys.readouterr().out
    row, plain = _row(m, lddt=True), _row(m)
    assert len(row) == 12 and row[:10] == plain and [float(x) for x in row[10:]] == [0.75, 0.375]
    log.reset_metrics_for_epoch(m, "valid-70")                      # nothing stale in the next epoch
    assert not any("lddt" in k for k in m["valid-70"])
    # a row of a split that reported none (training steps never compute it) still has the header's length
    m2 = _metrics(False)
    log.do_eval_epoch_logging(m2, "valid-70")
    assert "lddt" not in capsys.readouterr().out
    row = _row(m2, lddt=True)
    assert len(row) == 12 and all(np.isnan(float(x)) for x in row[10:])


def test_entry_points_check_their_arguments_on_the_host():
    from protein_transformer_amd import _lib, build
    build.build()
    lib = _lib.lib()
    assert not _lib.MISSING and "ptamd_lddt" in _lib.SIGNATURES and "ptamd_lddt_workspace_bytes" in _lib.SIGNATURES
    need = lib.ptamd_lddt_workspace_bytes(32, 512)
    assert 32 * 512 * 14 * 32 <= need <= 32 * 512 * 14 * 36          # 32 B per atom slot + the tiles' boxes
    assert lib.ptamd_lddt_workspace_bytes(0, 512) == 0 and lib.ptamd_lddt_workspace_bytes(32, 0) == 0
    null = (None,) * 3
    assert lib.ptamd_lddt(*null, 0, 8, 15.0, *null, None, 0, None) == -1                 # PTAMD_ERR_BAD_SHAPE
    assert lib.ptamd_lddt(*null, 2, 8, 15.0, *null, None, 0, None) == -1                 # null arrays
    one = 16                                                                             # any non-null address: nothing is touched
    assert lib.ptamd_lddt(one, one, one, 2, 8, float("nan"), one, one, one, one, 1 << 30, None) == -1
    assert lib.ptamd_lddt(one, one, one, 2, 8, 0.0, one, one, one, one, 1 << 30, None) == -1
    assert lib.ptamd_lddt(one, one, one, 2, 8, 15.0, one, one, one, None, 1 << 30, None) == -3      # PTAMD_ERR_WORKSPACE
    assert lib.ptamd_lddt(one, one, one, 2, 8, 15.0, one, one, one, one, lib.ptamd_lddt_workspace_bytes(2, 8) - 1, None) == -3
    with pytest.raises(RuntimeError, match="device tensors only"):
        import torch
        from protein_transformer_amd.eval_metrics import lddt_batch
        lddt_batch(torch.zeros(1, 28, 3), torch.zeros(1, 28, 3), torch.zeros(1, 2, dtype=torch.int64))


# ----------------------------------------------------------------------------- the reference of tests/test_gpu_lddt.py
def test_reference_reproduces_the_known_answers():
    true, seq, want = G.lattice_case()
    lo, hi = G.lddt_reference(G.finite_pred(true), true, seq)
    assert np.array_equal(lo, want) and np.array_equal(hi, want)
    assert np.all(G.scores_of(lo) == 1.0)
    true, seq, wants = G.line_case()
    for scale, want in wants.items():
        # x 2 is exact and holds a tie (|dp - dt| = 4 exactly, strictly not preserved): no bracket; x 1.1 is far from every bound
        for eps in ((0.0,) if scale == 2.0 else (0.0, G.EPS)):
            lo, hi = G.lddt_reference(G.finite_pred(true, scale), true, seq, eps=eps)
            assert np.array_equal(lo, want) and np.array_equal(hi, want), (scale, eps)
    assert np.allclose(G.scores_of(wants[2.0].sum(0)), [2 / 32, 2 / 8])
    for dist, total in ((14.9, 1), (15.1, 0)):
        true, seq = G.two_atom_case(dist)
        lo, hi = G.lddt_reference(G.finite_pred(true), true, seq, eps=G.EPS)
        assert np.array_equal(lo, np.full((2, 2, 5), total)) and np.array_equal(hi, lo)


@pytest.mark.parametrize("case", G.CASES, ids=G.case_id)
def test_brackets_cover_at_most_a_thousandth_of_the_included_pairs(case):
    pred, true, seq, lo, hi = G.case_with_reference(case)
    assert np.all(hi >= lo)
    assert np.abs(pred).max() <= 64 and np.nanmax(np.abs(true)) <= 64          # what the tolerance assumes
    assert int((~np.isnan(true).any(1)).sum()) == case[0]
    width, included = int((hi - lo).sum()), int(lo[:, :, 0].sum())
    assert width <= 1e-3 * included, (width, included)
