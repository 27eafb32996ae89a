"""What `--eval_tm` needs without a GPU: the flag on the command line, the CSV header and rows with and without it (byte for byte
the old ones without), a batch without a scored protein left out of the epoch's mean, the loss report's layout - unchanged when
nobody asks for the new tail field - and the entry point's host-side refusals."""
import csv
import inspect
import io
import os
import re
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
KEYS = ("tm-ca", "gdt-ts", "gdt-ha")


@pytest.fixture(scope="module")
def built_lib():
    from protein_transformer_amd import _lib, build
    build.build()                       # hipcc cross-compiles gfx950 without a GPU
    return _lib


def test_parser_accepts_the_flag():
    from protein_transformer_amd.train import create_parser
    assert create_parser().parse_args([]).eval_tm is False
    for extra in ([], ["--eval_lddt", "--eval_clash"], ["--backbone_loss"], ["-l", "mse"], ["-l", "fape", "--rename_symmetric"]):
        a = create_parser().parse_args(["--eval_tm", *extra])          # evaluation builds every atom whatever trains
        assert a.eval_tm is True
    with pytest.raises(SystemExit):
        create_parser().parse_args(["--eval_tm", "1"])                 # a store-true flag


def _metrics(values):
    """A split's metrics after one batch per entry of `values` ({key: value} or None for a batch without the keys)."""
    from protein_transformer_amd import log
    metrics = log.init_metrics(types.SimpleNamespace(lr_scheduling="plateau"))
    losses = {k: 0.5 for k in log._TRACKED}
    losses["n-residues"] = 100
    log.reset_metrics_for_epoch(metrics, "valid-70")
    for v in values:
        log.update_metrics(metrics, dict(losses, **(v or {})), "valid-70", None, batch_level=False)
    return metrics


def _row(metrics, **kw):
    from protein_transformer_amd import log
    out = io.StringIO()
    log.log_batch(csv.writer(out), metrics, 0.0, mode="valid-70", end_of_epoch=True, t=1.0, **kw)
    return out.getvalue()


def test_header_and_rows_without_the_flag_are_byte_identical():
    from protein_transformer_amd import log
    for loss, want in (("combined", "drmsd,ln_drmsd,rmse,rmsd,combined,lr,mode,granularity,time,speed"),
                       ("drmsd", "drmsd,ln_drmsd,rmse,rmsd,lr,mode,granularity,time,speed")):
        ns = lambda **kw: types.SimpleNamespace(loss=loss, **kw)      # noqa: E731
        assert log.prepare_log_header(ns()) == log.prepare_log_header(ns(eval_tm=False)) == want
        assert log.prepare_log_header(ns(eval_tm=True)) == want + ",tm,gdt_ts,gdt_ha"
        assert log.prepare_log_header(ns(eval_lddt=True, eval_clash=True, eval_tm=True)) == want + ",lddt,lddt_ca,clash,tm,gdt_ts,gdt_ha"
        assert log.prepare_log_header(ns(eval_lddt=True, eval_clash=True)) == want + ",lddt,lddt_ca,clash"
    m = _metrics([None])
    log.update_metrics_end_of_epoch(m, "valid-70")
    assert not any(k.endswith(KEYS) for k in m["valid-70"])
    row = _row(m)
    assert row == _row(m, tm=False) and row.strip().split(",")[6:8] == ["valid-70", "epoch"] and row.startswith("0.5,")
    assert len(row.strip().split(",")) == 10 and _row(m, lddt=True, clash=True) == _row(m, lddt=True, clash=True, tm=False)


def test_rows_with_the_flag_and_the_epoch_line(capsys):
    from protein_transformer_amd import log
    from protein_transformer_amd.eval_metrics import EVAL_METRICS, METRIC_KEYS
    assert [m.field for m in EVAL_METRICS[:3]] == ["lddt", "clash", "tm"]                # behind lddt and clash, in front of ss
    assert tuple(k for k, _ in EVAL_METRICS[2].columns) == KEYS and METRIC_KEYS[3:6] == KEYS
    scored = {"tm-ca": 0.75, "gdt-ts": 0.5, "gdt-ha": 0.25}
    # the second batch has no scored protein: NaN, left out of the epoch's mean; the third has
    m = _metrics([scored, dict.fromkeys(KEYS, NAN), {"tm-ca": 0.25, "gdt-ts": 0.25, "gdt-ha": 0.125}])
    log.do_eval_epoch_logging(m, "valid-70")
    assert [m["valid-70"][f"epoch-{k}"] for k in KEYS] == [0.5, 0.375, 0.1875] and m["valid-70"]["n-tm-ca"] == 2
    assert "tm-ca 0.5000  gdt-ts 0.3750  gdt-ha 0.1875" in capsys.readouterr().out
    plain, row = _row(m).strip().split(","), _row(m, tm=True).strip().split(",")
    assert row[:10] == plain and [float(x) for x in row[10:]] == [0.5, 0.375, 0.1875]
    full = _row(m, lddt=True, clash=True, tm=True).strip().split(",")
    assert len(full) == 16 and full[10:13] == ["nan"] * 3 and full[13:] == row[10:]         # behind the lDDT and clash columns
    log.reset_metrics_for_epoch(m, "valid-70")                        # nothing stale in the next epoch
    assert not any(k.endswith(KEYS) for k in m["valid-70"])
    # a split that reported none (training steps never compute it): the row still has the header's length, the line no word
    m2 = _metrics([None])
    log.do_eval_epoch_logging(m2, "valid-70")
    assert "tm-ca" not in capsys.readouterr().out
    row = _row(m2, tm=True).strip().split(",")
    assert len(row) == 13 and row[10:] == ["nan"] * 3
    # only NaN batches: the epoch's value is NaN, not 0
    m3 = _metrics([dict.fromkeys(KEYS, NAN)])
    log.do_eval_epoch_logging(m3, "valid-70")
    assert all(np.isnan(m3["valid-70"][f"epoch-{k}"]) for k in KEYS)


# ----------------------------------------------------------------------------- the report
B = 3
STATS = (torch.arange(B * 8, dtype=torch.float32).reshape(B, 8) * 3 + 4) / 8
MSE = torch.tensor([1.5, 4.0, 0.75, 2.0, 0.25, 2.0])
STATUS = torch.tensor([0b1001], dtype=torch.int32)
RMSD = torch.tensor([1.0, 2.0, 4.0])
LDDT = torch.tensor([[0.5, 0.25], [NAN, NAN], [0.75, 0.5]])
CLASH = torch.tensor([0.125, NAN, 0.625])
TM = torch.tensor([[0.5, 0.75, 0.25], [NAN, NAN, NAN], [0.25, 0.5, 0.125]])


def test_the_report_of_a_single_process():
    from protein_transformer_amd.losses import REPORT_FIELDS, REPORT_KEYS, LossReport, pack_local, unpack_local
    assert REPORT_KEYS["tm"] == KEYS and [f.name for f in REPORT_FIELDS if not f.fixed][:2] == ["clash", "tm"]
    sig = inspect.signature(LossReport.__init__).parameters
    assert sig["fields"].default is None and "tm" not in sig          # asked for without a value: fields={"tm": None}
    for channels, tail in (({"lddt": LDDT}, None), ({"lddt": LDDT}, {"clash": CLASH}), (None, None)):
        plain_buf, plain_layout = pack_local(STATS, MSE, STATUS, RMSD, channels, tail=tail)
        buf, layout = pack_local(STATS, MSE, STATUS, RMSD, channels, tail={**(tail or {}), "tm": TM})
        assert buf.numel() == plain_buf.numel() + 3 * B               # the three columns, behind everything
        for field, at in plain_layout[1].items():                     # what lay in front lies where it lay, bit for bit
            assert layout[1][field] == at and torch.equal(buf[at].view(torch.int32), plain_buf[at].view(torch.int32)), field
        assert list(layout[1]) == list(plain_layout[1]) + ["tm"] and layout[1]["tm"] == slice(buf.numel() - 3 * B, buf.numel())
        out, plain = unpack_local(buf.numpy(), layout), unpack_local(plain_buf.numpy(), plain_layout)
        assert list(out) == list(plain) + list(KEYS) and not any(k in plain for k in KEYS)
        assert [out[k] for k in KEYS] == [0.375, 0.625, 0.1875]       # the protein without a score is left out
        assert all(np.array_equal(np.asarray(out[k], np.float64), np.asarray(plain[k], np.float64), equal_nan=True) for k in plain)
    # asked for without a value (an empty shard): the keys exist and are None; only NaN: NaN
    buf, layout = pack_local(tail={"tm": None})
    assert buf.numel() == 7 and [unpack_local(buf.numpy(), layout)[k] for k in KEYS] == [None] * 3
    buf, layout = pack_local(STATS, MSE, STATUS, tail={"tm": torch.full((B, 3), NAN)})
    assert all(np.isnan(unpack_local(buf.numpy(), layout)[k]) for k in KEYS)


def test_the_reduced_vector_of_data_parallel_ranks():
    from protein_transformer_amd.losses import VECTOR_SIZE, reduce_vector, unpack_global
    assert VECTOR_SIZE == 27 and reduce_vector(STATS, MSE, STATUS).shape == (27,)             # nobody asked: the vector of before
    assert reduce_vector(STATS, MSE, STATUS, tail={"clash": CLASH}).shape == (29,)            # the clash tail alone: as before
    ranks = [dict(stats=STATS[:2], mse=MSE, status=STATUS, tail={"clash": CLASH[:2], "tm": TM[:2]}),
             dict(stats=STATS[2:], mse=MSE, status=STATUS, tail={"clash": CLASH[2:], "tm": TM[2:]}),
             dict(tail={"clash": None, "tm": None})]                  # an empty shard: same length, adds nothing
    vs = [reduce_vector(**kw) for kw in ranks]
    assert [v.shape for v in vs] == [(35,)] * 3 and vs[2].tolist() == [0.0] * 35
    assert vs[0][29:].tolist() == [0.5, 0.75, 0.25, 1.0, 1.0, 1.0] and vs[0][27:29].tolist() == [0.125, 1.0]
    assert torch.equal(vs[0][:27], reduce_vector(stats=STATS[:2], mse=MSE, status=STATUS))    # the slots in front are untouched
    v = sum(vs).numpy()
    for passed in ({"clash", "tm"}, set()):                           # the empty shard reads the same numbers
        out = unpack_global(v, passed, ("clash", "tm"))
        assert [out[k] for k in KEYS] == [0.375, 0.625, 0.1875] and out["clash"] == 0.375 and list(out)[-3:] == list(KEYS)
    assert not any(k in unpack_global(v[:27]) for k in KEYS)
    only = sum(reduce_vector(**{**kw, "tail": {"tm": kw["tail"]["tm"]}}) for kw in ranks).numpy()
    assert only.shape == (33,) and unpack_global(only, {"tm"}, ("tm",))["tm-ca"] == 0.375
    v = (reduce_vector(stats=STATS, tail={"tm": torch.full((B, 3), NAN)}) + reduce_vector(tail={"tm": None})).numpy()
    assert np.isnan(unpack_global(v, {"tm"}, ("tm",))["gdt-ts"]) and unpack_global(v, set(), ("tm",))["gdt-ts"] is None


# ----------------------------------------------------------------------------- the entry point
def test_header_library_and_ctypes_table_agree(built_lib):
    import ctypes
    text = open(os.path.join(ROOT, "include", "ptamd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = ctypes.CDLL(built_lib.LIB_PATH)
    built_lib.lib()
    kinds = {built_lib._p: "ptr", built_lib._i: "int", built_lib._sz: "size_t"}
    for name in ("ptamd_tm_workspace_bytes", "ptamd_tm_score"):
        decl = re.search(r"\b(size_t|int)\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert decl and hasattr(handle, name) and name in built_lib.SIGNATURES and name not in built_lib.MISSING, name
        want = ["ptr" if "*" in a else a.split()[0] for a in decl.group(2).split(",")]
        res, args = built_lib.SIGNATURES[name]
        assert [kinds[a] for a in args] == want and kinds[res] == decl.group(1), name
    assert len(built_lib.SIGNATURES["ptamd_tm_score"][1]) == 11
    assert "PARITY UNPINNED" in text and "Proteins 57:702" in text and "TMscore program" in text
    for doc in ("PAPERS.md", "INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "--eval_tm" in open(os.path.join(ROOT, doc)).read() or doc == "PAPERS.md", doc
    assert "Proteins 57" in open(os.path.join(ROOT, "PAPERS.md")).read()


def test_entry_point_refusals(built_lib):
    lib = built_lib.lib()
    ws = lib.ptamd_tm_workspace_bytes
    assert ws(32, 512) == ws(32, 512) and ws(1, 1) > 0 and ws(1, 4096) > 0       # a function of (B, L) only; only a size
    assert 32 * 512 * 24 <= ws(32, 512) <= 4 << 20                                # 24 B per residue + 32 B per possible seed
    assert ws(0, 8) == 0 and ws(2, 0) == 0 and ws(-1, 8) == 0 and ws(1, 4097) == 0
    B, L = 2, 8
    buf = torch.full((8 * B * L * 42,), 77.0)                 # host memory: every call below is refused before any launch
    at = lambda k: buf.data_ptr() + 4 * k * B * L * 42        # noqa: E731  (disjoint pieces, each large enough for any array)
    ok = dict(pred=at(0), true=at(1), seq=at(2), B=B, L=L, score=at(3), counts=at(4), xform=at(5), ws=at(6), wb=1 << 30)

    def run(**kw):
        a = dict(ok, **kw)
        return lib.ptamd_tm_score(a["pred"], a["true"], a["seq"], a["B"], a["L"], a["score"], a["counts"], a["xform"], a["ws"],
                                  a["wb"], None)

    for kw in (dict(B=0), dict(L=0), dict(B=-1), dict(L=-3), dict(L=4097)):
        assert run(**kw) == -1, kw                            # PTAMD_ERR_BAD_SHAPE
    for kw in (dict(pred=None), dict(true=None), dict(seq=None), dict(score=None), dict(counts=None)):
        assert run(**kw) == -1, kw                            # a NULL array other than xform
    assert run(ws=None) == -3 and run(wb=ws(B, L) - 1) == -3 and run(wb=0) == -3          # PTAMD_ERR_WORKSPACE
    assert run(xform=None, ws=None) == -3                     # xform may be NULL: a valid call up to the workspace
    assert (buf == 77.0).all()                                # nothing was written
    from protein_transformer_amd.eval_metrics import batch_tm, tm_batch
    assert list(inspect.signature(tm_batch).parameters) == ["pred_crd", "true_crd", "seq"]
    assert list(inspect.signature(batch_tm).parameters) == ["pred_sincos", "true_crds", "input_seqs"]
    with pytest.raises(RuntimeError, match="device tensors only"):      # a missing GPU is an error, never a CPU fall-back
        tm_batch(torch.zeros(1, 28, 3), torch.zeros(1, 28, 3), torch.zeros(1, 2, dtype=torch.int64))
