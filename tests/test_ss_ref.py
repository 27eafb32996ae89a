"""What `--eval_ss` needs without a GPU: the fp64 reference of tests/ss_ref.py pinned by the structures it must label and by its
own second form, the exclusion band on every fixture of tests/test_gpu_ss.py, the flag on the command line, the CSV header and
rows with and without it, the loss report's layout - unchanged when nobody asks for the new tail field - and the entry point's
host-side refusals."""
import csv
import inspect
import io
import os
import re
import types

import numpy as np
import pytest
import torch

import ss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float("nan")
KEYS = ("ss-q3", "ss-h", "ss-e")


@pytest.fixture(scope="module")
def built_lib():
    from protein_transformer_amd import _lib, build
    build.build()                       # hipcc cross-compiles gfx950 without a GPU
    return _lib


def all_fixtures():
    return {**R.cases(), **{f"edge{L}": v for L, v in R.edge_cases().items()}}


# ----------------------------------------------------------------------------- the reference
def test_the_reference_labels_helix_and_ladders():
    """An all-coil implementation cannot pass: the interior of the ideal alpha-helix is H, six residues of each strand of both
    ladders are E (the end residues have no neighbour on one side and cannot bridge)."""
    true, seq = R.helix_case(24)
    ref = R.reference(true, true, seq)
    assert (ref["states"][1:-1, 1] == R.ST_H).all() and ref["states"][[0, -1], 1].tolist() == [R.ST_C, R.ST_C]
    i, j = np.nonzero(ref["hb"][1])
    assert len(i) == 20 and (j - i == 4).all()                        # the i -> i+4 bonds and nothing else
    assert ref["score"].tolist()[:2] == [1.0, 1.0] and np.isnan(ref["score"][2])
    want = [R.ST_C] + [R.ST_E] * 6 + [R.ST_C]
    for kind in ("anti", "par"):
        true, seq = R.ladder_case(kind)
        ref = R.reference(true, true, seq)
        assert ref["states"][:, 1].tolist() == want + [-1] + want, kind
        i, j = np.nonzero(ref["hb"][1])
        assert ((i < R.STRAND) & (j > R.STRAND)).any() and ((j < R.STRAND) & (i > R.STRAND)).any(), kind   # bonds in both directions
        a, b = (x.astype(np.float64).reshape(R.STRAND, R.NUM_SLOTS, 3)[:, :4].reshape(-1, 3) for x in R.ladder_segments(kind))
        assert np.sqrt(((a[:, None] - b[None]) ** 2).sum(2)).min() >= 2.8, kind                             # no steric overlap
        assert np.isnan(ref["score"][1]) and ref["score"][2] == 1.0
    # the antiparallel ladder holds the pattern hb(i,j) and hb(j,i); the parallel one cannot
    true, seq = R.ladder_case("anti")
    hb = R.reference(true, true, seq)["hb"][1]
    assert (hb & hb.T).any()
    true, seq = R.ladder_case("par")
    hb = R.reference(true, true, seq)["hb"][1]
    assert not (hb & hb.T).any()


def test_vectorised_and_loop_forms_agree():
    for name, (pred, true, seq) in all_fixtures().items():
        present = R.presence(true, seq)
        for x in (pred, true):
            bb = R.backbone(x, present)
            hb = R.hbonds(bb, present)
            assert np.array_equal(hb, R.hbonds_loop(bb, present)), name
            assert np.array_equal(R.states_from_bits(hb, present), R.states_from_bits_loop(hb, present)), name
    rng = np.random.default_rng(0)                                    # the pattern logic on dense random bits and breaks
    for _ in range(40):
        L = int(rng.integers(1, 48))
        present = rng.random(L) > 0.1
        hb = (rng.random((L, L)) < 0.25) & present[:, None] & present[None, :]
        assert np.array_equal(R.states_from_bits(hb, present), R.states_from_bits_loop(hb, present))


def test_exclusion_band_and_coordinate_range():
    """No candidate pair of any fixture, prediction or truth, has an fp64 energy within BAND of -0.5, and every coordinate lies
    within +-64 A: the condition under which tests/test_gpu_ss.py demands exact equality (derivation: ss_ref's docstring)."""
    assert R.BAND == 2.0e-3 and R.COORD_MAX == 64.0
    ht, hs = R.helix_case(24)
    extra = {"edges/pred": (R.noised(ht, 22), ht, hs)}                # (test_edges_of_the_definition builds on these)
    for name, (pred, true, seq) in {**all_fixtures(), **extra}.items():
        margin = min(R.min_margin(pred, true, seq), R.min_margin(true, true, seq))
        assert margin > R.BAND, (name, margin)
        assert np.nanmax(np.abs(true)) <= R.COORD_MAX and np.abs(pred).max() <= R.COORD_MAX, name


def test_scores_counts_and_packing():
    states = np.array([[0, 0], [2, 0], [1, 1], [2, 2], [-1, -1], [0, 2]], np.int8)       # {pred, true}
    present = states[:, 1] >= 0
    c = R.confusion_of(states, present)
    assert c.tolist() == [[1, 0, 1], [0, 1, 0], [1, 0, 1]] and c.sum() == 5
    assert R.scores_of(c).tolist() == [np.float32(3 / 5), 0.5, 1.0]
    assert np.isnan(R.scores_of(np.zeros((3, 3), int))).all() and np.isnan(R.scores_of(c, bad=True)).all()
    hb = np.random.default_rng(1).random((70, 70)) < 0.3
    words = R.pack_bits(hb)
    assert words.shape == (70, 2) and words.dtype == np.uint64 and np.array_equal(R.unpack_bits(words, 70), hb)
    assert int(words[3, 1]) >> 6 == 0 and bool((int(words[3, 0]) >> 5) & 1) == bool(hb[3, 5])
    # a non-finite prediction on a present residue: NaN scores, no counts, no predicted string
    pred, true, seq = R.cases()["helix"]
    bad = pred.copy()
    bad[3 * R.NUM_SLOTS + R.SLOT_CA, 0] = np.nan
    ref = R.reference(bad, true, seq)
    assert ref["bad"] and np.isnan(ref["score"]).all() and not ref["confusion"].any() and (ref["states"][:, 0] == -1).all()
    bad = pred.copy()
    bad[3 * R.NUM_SLOTS + 4, 0] = np.nan                              # a side-chain atom does not count
    assert not R.reference(bad, true, seq)["bad"]


# ----------------------------------------------------------------------------- flag, log, early stopping
def test_parser_accepts_the_flag():
    from protein_transformer_amd.train import SS_ESM_MESSAGE, create_parser, early_stopping_target
    assert create_parser().parse_args([]).eval_ss is False
    for extra in ([], ["--eval_lddt", "--eval_clash", "--eval_tm"], ["--backbone_loss"], ["-l", "mse"],
                  ["-l", "fape", "--rename_symmetric"]):
        assert create_parser().parse_args(["--eval_ss", *extra]).eval_ss is True
    with pytest.raises(SystemExit):
        create_parser().parse_args(["--eval_ss", "1"])                 # a store-true flag
    # the keys as early-stopping metrics: split and key are told apart although the key carries a hyphen
    for key in KEYS:
        a = create_parser().parse_args(["--eval_ss", "-esm", f"valid-70-{key}"])
        assert early_stopping_target(a) == ("valid-70", key)
    assert early_stopping_target(create_parser().parse_args(["-esm", "valid-70-drmsd"])) == ("valid-70", "drmsd")
    assert early_stopping_target(create_parser().parse_args(["-l", "kabsch"])) == ("train", "kabsch")
    with pytest.raises(SystemExit):
        create_parser().parse_args(["-esm", "valid-70-ss-q3"])         # nothing computes it without --eval_ss
    assert "--eval_ss" in SS_ESM_MESSAGE


def _metrics(values):
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
        assert log.prepare_log_header(ns()) == log.prepare_log_header(ns(eval_ss=False)) == want
        assert log.prepare_log_header(ns(eval_ss=True)) == want + ",ss_q3,ss_h,ss_e"
        assert log.prepare_log_header(ns(eval_lddt=True, eval_clash=True, eval_tm=True, eval_ss=True)) == \
            want + ",lddt,lddt_ca,clash,tm,gdt_ts,gdt_ha,ss_q3,ss_h,ss_e"
        assert log.prepare_log_header(ns(eval_tm=True)) == want + ",tm,gdt_ts,gdt_ha"
    m = _metrics([None])
    log.update_metrics_end_of_epoch(m, "valid-70")
    assert not any(k.endswith(KEYS) for k in m["valid-70"])           # no key, no history
    row = _row(m)
    assert row == _row(m, ss=False) and len(row.strip().split(",")) == 10
    assert _row(m, lddt=True, clash=True, tm=True) == _row(m, lddt=True, clash=True, tm=True, ss=False)


def test_rows_with_the_flag_the_epoch_line_and_early_stopping(capsys):
    from protein_transformer_amd import log
    from protein_transformer_amd.eval_metrics import ESM_KEYS, EVAL_METRICS, METRIC_KEYS
    assert [m.field for m in EVAL_METRICS] == ["lddt", "clash", "tm", "ss"]              # the log's order: ss behind every older one
    assert tuple(k for k, _ in EVAL_METRICS[-1].columns) == KEYS and ESM_KEYS == KEYS and METRIC_KEYS[-3:] == KEYS
    assert METRIC_KEYS[-6:-3] == tuple(k for k, _ in EVAL_METRICS[2].columns) == ("tm-ca", "gdt-ts", "gdt-ha")
    scored = {"ss-q3": 0.75, "ss-h": 0.5, "ss-e": 0.25}
    m = _metrics([scored, dict.fromkeys(KEYS, NAN), {"ss-q3": 0.25, "ss-h": 0.25, "ss-e": NAN}])
    log.do_eval_epoch_logging(m, "valid-70")
    assert [m["valid-70"][f"epoch-{k}"] for k in KEYS] == [0.5, 0.375, 0.25] and m["valid-70"]["n-ss-e"] == 1
    assert "ss-q3 0.5000  ss-h 0.3750  ss-e 0.2500" in capsys.readouterr().out
    plain, row = _row(m).strip().split(","), _row(m, ss=True).strip().split(",")
    assert row[:10] == plain and [float(x) for x in row[10:]] == [0.5, 0.375, 0.25]
    full = _row(m, lddt=True, clash=True, tm=True, ss=True).strip().split(",")
    assert len(full) == 19 and full[10:16] == ["nan"] * 6 and full[16:] == row[10:]       # behind every older column
    # higher is better: early stopping, the scheduler and the checkpoint policy see the negative
    args = types.SimpleNamespace(es_mode="valid-70", es_metric="ss-q3", early_stopping_threshold=0.001, early_stopping=1)
    assert log.es_value(args, m) == (-0.5, [-0.5])
    m = log.update_loss_trackers(args, 0, m)
    assert m["loss_to_compare"] == -0.5 and m["losses_to_compare"] == [-0.5] and m["best_valid_loss_so_far"] == -0.5
    log.reset_metrics_for_epoch(m, "valid-70")                        # nothing stale in the next epoch; the history stays
    assert not any(k.endswith(KEYS) and not k.startswith("epoch-history") for k in m["valid-70"])
    log.update_metrics(m, dict({k: 0.5 for k in log._TRACKED}, **{"n-residues": 1, "ss-q3": 0.625}), "valid-70", None, batch_level=False)
    log.do_eval_epoch_logging(m, "valid-70")
    m = log.update_loss_trackers(args, 1, m)                          # 0.625 > 0.5: an improvement
    assert m["epoch_last_improved"] == 1 and m["losses_to_compare"] == [-0.5, -0.625]
    # the losses are compared as before
    args = types.SimpleNamespace(es_mode="valid-70", es_metric="drmsd", early_stopping_threshold=0.001, early_stopping=1)
    assert log.es_value(args, m) == (m["valid-70"]["epoch-drmsd-full"], m["valid-70"]["epoch-history-drmsd"])
    # a split that reported none: the row still has the header's length; only NaN batches: NaN, not 0
    m2 = _metrics([None])
    capsys.readouterr()
    log.do_eval_epoch_logging(m2, "valid-70")
    assert "ss-q3" not in capsys.readouterr().out and _row(m2, ss=True).strip().split(",")[10:] == ["nan"] * 3
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
KABSCH = torch.tensor([1.5, 2.5, NAN])
SS = torch.tensor([[0.5, 0.75, NAN], [NAN, NAN, NAN], [0.25, 0.5, 0.125]])


def test_the_report_of_a_single_process():
    from protein_transformer_amd.losses import REPORT_FIELDS, REPORT_KEYS, LossReport, pack_local, unpack_local
    assert [f.name for f in REPORT_FIELDS if not f.fixed] == ["clash", "tm", "kabsch", "ss"]      # the tail's order is what it was
    assert [f.name for f in REPORT_FIELDS if f.fixed] == ["lddt", "slddt", "fape"] and REPORT_KEYS["ss"] == KEYS
    sig = inspect.signature(LossReport.__init__).parameters
    assert sig["fields"].default is None and "ss" not in sig          # asked for without a value: fields={"ss": None}
    for channels, tail in (({"lddt": LDDT}, None), ({"lddt": LDDT}, {"clash": CLASH, "tm": TM, "kabsch": KABSCH}), (None, {"tm": TM}),
                           (None, None)):
        plain_buf, plain_layout = pack_local(STATS, MSE, STATUS, RMSD, channels, tail=tail)
        buf, layout = pack_local(STATS, MSE, STATUS, RMSD, channels, tail={**(tail or {}), "ss": SS})
        assert buf.numel() == plain_buf.numel() + 3 * B               # the three columns, behind everything
        for field, at in plain_layout[1].items():                     # what lay in front lies where it lay, bit for bit
            assert layout[1][field] == at and torch.equal(buf[at].view(torch.int32), plain_buf[at].view(torch.int32)), field
        assert list(layout[1]) == list(plain_layout[1]) + ["ss"] and layout[1]["ss"] == slice(buf.numel() - 3 * B, buf.numel())
        out, plain = unpack_local(buf.numpy(), layout), unpack_local(plain_buf.numpy(), plain_layout)
        assert list(out) == list(plain) + list(KEYS) and not any(k in plain for k in KEYS)
        assert [out[k] for k in KEYS] == [0.375, 0.625, 0.125]        # per column, the proteins without a score are left out
        assert all(np.array_equal(np.asarray(out[k], np.float64), np.asarray(plain[k], np.float64), equal_nan=True) for k in plain)
    # asked for without a value (an empty shard): the keys exist and are None; only NaN: NaN
    buf, layout = pack_local(tail={"ss": None})
    assert buf.numel() == 7 and [unpack_local(buf.numpy(), layout)[k] for k in KEYS] == [None] * 3
    buf, layout = pack_local(STATS, MSE, STATUS, tail={"ss": torch.full((B, 3), NAN)})
    assert all(np.isnan(unpack_local(buf.numpy(), layout)[k]) for k in KEYS)


def test_the_reduced_vector_of_data_parallel_ranks():
    from protein_transformer_amd.losses import VECTOR_SIZE, reduce_vector, unpack_global
    assert VECTOR_SIZE == 27 and reduce_vector(STATS, MSE, STATUS).shape == (27,)             # nobody asked: the vector of before
    assert reduce_vector(STATS, MSE, STATUS, tail={"clash": CLASH, "tm": TM}).shape == (35,)  # the older tails alone: as before
    ranks = [dict(stats=STATS[:2], mse=MSE, status=STATUS, tail={"clash": CLASH[:2], "tm": TM[:2], "ss": SS[:2]}),
             dict(stats=STATS[2:], mse=MSE, status=STATUS, tail={"clash": CLASH[2:], "tm": TM[2:], "ss": SS[2:]}),
             dict(tail={"clash": None, "tm": None, "ss": None})]      # an empty shard: same length, adds nothing
    vs = [reduce_vector(**kw) for kw in ranks]
    assert [v.shape for v in vs] == [(41,)] * 3 and vs[2].tolist() == [0.0] * 41
    assert vs[0][35:].tolist() == [0.5, 0.75, 0.0, 1.0, 1.0, 0.0]                             # the field lies last
    assert torch.equal(vs[0][:35], reduce_vector(stats=STATS[:2], mse=MSE, status=STATUS, tail={"clash": CLASH[:2], "tm": TM[:2]}))
    v = sum(vs).numpy()
    for passed in ({"clash", "tm", "ss"}, set()):                     # the empty shard reads the same numbers
        out = unpack_global(v, passed, ("clash", "tm", "ss"))
        assert [out[k] for k in KEYS] == [0.375, 0.625, 0.125] and out["tm-ca"] == 0.375 and list(out)[-3:] == list(KEYS)
    assert not any(k in unpack_global(v[:27]) for k in KEYS)
    only = sum(reduce_vector(**{**kw, "tail": {"ss": kw["tail"]["ss"]}}) for kw in ranks).numpy()
    assert only.shape == (33,) and unpack_global(only, {"ss"}, ("ss",))["ss-q3"] == 0.375
    v = (reduce_vector(stats=STATS, tail={"ss": torch.full((B, 3), NAN)}) + reduce_vector(tail={"ss": None})).numpy()
    assert np.isnan(unpack_global(v, {"ss"}, ("ss",))["ss-h"]) and unpack_global(v, set(), ("ss",))["ss-h"] is None


# ----------------------------------------------------------------------------- the entry point
def test_header_library_and_ctypes_table_agree(built_lib):
    import ctypes
    text = open(os.path.join(ROOT, "include", "ptamd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    handle = ctypes.CDLL(built_lib.LIB_PATH)
    built_lib.lib()
    kinds = {built_lib._p: "ptr", built_lib._i: "int", built_lib._sz: "size_t"}
    for name in ("ptamd_ss_workspace_bytes", "ptamd_ss"):
        decl = re.search(r"\b(size_t|int)\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert decl and hasattr(handle, name) and name in built_lib.SIGNATURES and name not in built_lib.MISSING, name
        want = ["ptr" if "*" in a else a.split()[0] for a in decl.group(2).split(",")]
        res, args = built_lib.SIGNATURES[name]
        assert [kinds[a] for a in args] == want and kinds[res] == decl.group(1), name
    assert len(built_lib.SIGNATURES["ptamd_ss"][1]) == 12
    assert "DSSP SIMPLIFIED" in text and "Biopolymers 22:2577" in text and "two strongest" in text
    for doc in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        assert "--eval_ss" in open(os.path.join(ROOT, doc)).read(), doc
    assert "Biopolymers 22" in open(os.path.join(ROOT, "PAPERS.md")).read()


def test_entry_point_refusals(built_lib):
    lib = built_lib.lib()
    ws = lib.ptamd_ss_workspace_bytes
    assert ws(32, 512) == ws(32, 512) and ws(1, 1) > 0                            # a function of (B, L) only; only a size
    assert 32 * 2 * 512 * 512 // 8 <= ws(32, 512) <= 5 << 20                      # the bits of both structures + 128 B per residue
    l_max = (2 ** 31 - 1) // 28
    assert ws(0, 8) == 0 and ws(2, 0) == 0 and ws(-1, 8) == 0 and ws(1, l_max + 1) == 0 and ws(1, l_max) > 0
    B, L = 2, 8
    buf = torch.full((10 * B * L * 42,), 77.0)                # host memory: every call below is refused before any launch
    at = lambda k: buf.data_ptr() + 4 * k * B * L * 42        # noqa: E731  (disjoint pieces, each large enough for any array)
    ok = dict(pred=at(0), true=at(1), seq=at(2), B=B, L=L, score=at(3), conf=at(4), states=at(5), bits=at(6), ws=at(7), wb=1 << 30)

    def run(**kw):
        a = dict(ok, **kw)
        return lib.ptamd_ss(a["pred"], a["true"], a["seq"], a["B"], a["L"], a["score"], a["conf"], a["states"], a["bits"], a["ws"],
                            a["wb"], None)

    for kw in (dict(B=0), dict(L=0), dict(B=-1), dict(L=-3), dict(L=l_max + 1)):
        assert run(**kw) == -1, kw                            # PTAMD_ERR_BAD_SHAPE
    for kw in (dict(pred=None), dict(true=None), dict(seq=None), dict(score=None), dict(conf=None)):
        assert run(**kw) == -1, kw                            # a NULL required array
    assert run(ws=None) == -3 and run(wb=ws(B, L) - 1) == -3 and run(wb=0) == -3          # PTAMD_ERR_WORKSPACE
    assert run(states=None, bits=None, ws=None) == -3         # states and hbonds may be NULL: a valid call up to the workspace
    assert (buf == 77.0).all()                                # nothing was written
    from protein_transformer_amd.eval_metrics import ss_batch
    assert list(inspect.signature(ss_batch).parameters)[:3] == ["crd", "true_crds", "seq"]
    with pytest.raises(RuntimeError, match="device tensors only"):      # a missing GPU is an error, never a CPU fall-back
        ss_batch(torch.zeros(1, 28, 3), torch.zeros(1, 28, 3), torch.zeros(1, 2, dtype=torch.int64))
