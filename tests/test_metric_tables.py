"""The two tables every optional metric is declared in - losses.REPORT_FIELDS (how a value travels to the host) and
eval_metrics.EVAL_METRICS (flag, dictionary keys, CSV columns) - against the layouts, keys and rows written down here as literals
and formulas: every subset of the tail fields, every subset of the --eval_* flags.  No GPU.

The inputs are those of test_loss_report.py (multiples of 1/8, exact in fp32; their sums exact in fp64), so every comparison is ==."""
import csv
import io
import itertools
import types

import numpy as np
import pytest
import torch

from protein_transformer_amd.losses import pack_local, reduce_vector, unpack_global, unpack_local
from test_loss_report import CHANNELS, MSE, RMSD, STATS, STATUS, B

NAN = float("nan")
FIXED_KEYS = ["drmsd", "lndrmsd", "drmsd-bb", "lndrmsd-bb", "rmsd", "n_proteins", "status", "n_res", "mse", "lddt", "lddt-ca",
              "slddt", "fape"]
FIXED_VECTOR = (STATS[:, :4].double().sum(0).tolist() + [3.0, 4.125] + MSE.tolist() + [1.0, 0.0, 0.0, 1.0] + [41.0, 3.0, 1.0]
                + [1.375, 1.0, 2.0, 2.0] + [0.75, 2.0] + [3.75, 2.0])            # (test_the_reduced_vector_keeps_its_slots)
# the tail, in its order: field -> (keys, a value, the means of its columns over the finite entries, their sums then counts)
TAIL = {"clash": (("clash",), torch.tensor([0.125, NAN, 0.625]), [0.375], [0.75, 2.0]),
        "tm": (("tm-ca", "gdt-ts", "gdt-ha"), torch.tensor([[0.5, 0.75, 0.25], [NAN, NAN, NAN], [0.25, 0.5, 0.125]]),
               [0.375, 0.625, 0.1875], [0.75, 1.25, 0.375, 2.0, 2.0, 2.0]),
        "kabsch": (("kabsch",), torch.tensor([1.5, 2.5, NAN]), [2.0], [4.0, 2.0]),
        "ss": (("ss-q3", "ss-h", "ss-e"), torch.tensor([[0.5, 0.75, NAN], [NAN, NAN, NAN], [0.25, 0.5, 0.125]]),
               [0.375, 0.625, 0.125], [0.75, 1.25, 0.125, 2.0, 2.0, 1.0])}
SUBSETS = [tuple(f for f, on in zip(TAIL, bits) if on) for bits in itertools.product([False, True], repeat=4)]


def same(a, b):
    return a is b is None or (a is not None and b is not None and (a == b or (a != a and b != b)))


@pytest.mark.parametrize("asked", SUBSETS, ids=lambda s: "+".join(s) or "none")
def test_every_subset_of_the_tail_fields(asked):
    for states in itertools.product(("none", "value", "nan"), repeat=len(asked)):
        state = dict(zip(asked, states))
        tail = {f: None if s == "none" else TAIL[f][1] if s == "value" else torch.full_like(TAIL[f][1], NAN)
                for f, s in state.items()}
        want = {f: [None] * len(TAIL[f][0]) if s == "none" else TAIL[f][2] if s == "value" else [NAN] * len(TAIL[f][0])
                for f, s in state.items()}
        # a single process: the fixed part (every channel passed: 13 B + 7 words), then per asked field k B words - none for None
        buf, (rows, at) = pack_local(STATS, MSE, STATUS, RMSD, CHANNELS, tail=tail or None)
        assert rows == B and list(at) == ["stats", "mse", "status", "rmsd", "lddt", "slddt", "fape", *asked]
        cursor = 13 * B + 7
        assert at["fape"].stop == cursor
        for f in asked:
            width = 0 if tail[f] is None else len(TAIL[f][0]) * B
            assert at[f] == slice(cursor, cursor + width), (f, state)
            if width:
                assert torch.equal(buf[at[f]].view(torch.int32), tail[f].reshape(-1).view(torch.int32))
            cursor += width
        assert buf.numel() == cursor
        out = unpack_local(buf.numpy(), (rows, at), n_res=41)
        assert list(out) == FIXED_KEYS + [k for f in asked for k in TAIL[f][0]]
        assert out["lddt"] == 0.6875 and out["fape"] == 1.875 and out["n_res"] == 41      # what lies in front is what it was
        for f in asked:
            assert all(same(out[k], w) for k, w in zip(TAIL[f][0], want[f])), (f, state, out)
        # data parallel: 27 slots, then per asked field 2 k words whether or not the rank has a value
        v = reduce_vector(STATS, MSE, STATUS, RMSD, 41, CHANNELS, tail=tail or None)
        assert v.dtype == torch.float64 and v.numel() == 27 + 2 * sum(len(TAIL[f][0]) for f in asked)
        assert v[:27].tolist() == FIXED_VECTOR
        cursor = 27
        for f in asked:
            k = len(TAIL[f][0])
            assert v[cursor:cursor + 2 * k].tolist() == (TAIL[f][3] if state[f] == "value" else [0.0] * 2 * k), (f, state)
            cursor += 2 * k
        passed = set(CHANNELS) | {f for f in asked if tail[f] is not None}
        out = unpack_global(v.numpy(), passed, asked)
        assert list(out) == FIXED_KEYS + [k for f in asked for k in TAIL[f][0]]
        assert out["lddt"] == 0.6875 and out["fape"] == 1.875 and out["n_res"] == 41 and out["n_proteins"] == 3
        for f in asked:
            assert all(same(out[k], w) for k, w in zip(TAIL[f][0], want[f])), (f, state, out)
    # nothing but the tail: still 7 words, and a vector as long as everyone else's that adds nothing
    buf, layout = pack_local(tail=dict.fromkeys(asked))
    assert buf.numel() == 7 and layout == (0, {f: slice(7, 7) for f in asked})
    assert reduce_vector(tail=dict.fromkeys(asked)).tolist() == [0.0] * (27 + 2 * sum(len(TAIL[f][0]) for f in asked))


# ----------------------------------------------------------------------------- the log
METRICS = {"lddt": ("eval_lddt", ",lddt,lddt_ca", {"lddt-full": 0.75, "lddt-ca": 0.5}),
           "clash": ("eval_clash", ",clash", {"clash-full": 0.125}),
           "tm": ("eval_tm", ",tm,gdt_ts,gdt_ha", {"tm-ca": 0.625, "gdt-ts": 0.375, "gdt-ha": 0.25}),
           "ss": ("eval_ss", ",ss_q3,ss_h,ss_e", {"ss-q3": 0.875, "ss-h": 0.0625, "ss-e": 0.4375})}
FLAG_SUBSETS = [tuple(f for f, on in zip(METRICS, bits) if on) for bits in itertools.product([False, True], repeat=4)]


def _row(metrics, **kw):
    from protein_transformer_amd import log
    out = io.StringIO()
    log.log_batch(csv.writer(out), metrics, 0.0, mode="valid-70", end_of_epoch=True, t=1.0, **kw)
    return out.getvalue().strip().split(",")


@pytest.mark.parametrize("flagged", FLAG_SUBSETS, ids=lambda s: "+".join(s) or "none")
def test_every_subset_of_the_evaluation_flags(flagged):
    from protein_transformer_amd import log
    for loss, head in (("combined", "drmsd,ln_drmsd,rmse,rmsd,combined,lr,mode,granularity,time,speed"),
                       ("drmsd", "drmsd,ln_drmsd,rmse,rmsd,lr,mode,granularity,time,speed")):
        args = types.SimpleNamespace(loss=loss, **{METRICS[f][0]: True for f in flagged})
        assert log.prepare_log_header(args) == head + "".join(METRICS[f][1] for f in flagged)
        assert log.log_columns(args) == {f: f in flagged for f in METRICS}
    for reported in FLAG_SUBSETS:
        metrics = log.init_metrics(types.SimpleNamespace(lr_scheduling="plateau"))
        log.reset_metrics_for_epoch(metrics, "valid-70")
        losses = dict({k: 0.5 for k in log._TRACKED}, **{"n-residues": 100})
        for f in reported:
            losses.update(METRICS[f][2])
        log.update_metrics(metrics, losses, "valid-70", None, batch_level=False)
        metrics["n_batches"] = 1
        log.update_metrics_end_of_epoch(metrics, "valid-70")
        row = _row(metrics, **{f: True for f in flagged})
        assert len(row) == 10 + sum(len(METRICS[f][2]) for f in flagged) and row[:10] == _row(metrics)
        want = [str(v) if f in reported else "nan" for f in flagged for v in METRICS[f][2].values()]
        assert row[10:] == want, (flagged, reported)
        assert row == _row(metrics, **{f: f in flagged for f in METRICS})                 # False is the flag being off
        kept = {k for k in metrics["valid-70"] if k.startswith("epoch-history-")}
        assert kept == {f"epoch-history-{h}" for h in ("drmsd", "combined", "lndrmsd", "mse")} \
            | ({"epoch-history-ss-q3", "epoch-history-ss-h", "epoch-history-ss-e"} if "ss" in reported else set())
    with pytest.raises(TypeError, match="nope"):
        _row(metrics, nope=True)


# ----------------------------------------------------------------------------- the tables
def test_the_two_tables_agree():
    from protein_transformer_amd.eval_metrics import ESM_KEYS, EVAL_METRICS, METRIC_KEYS
    from protein_transformer_amd.losses import REPORT_FIELDS
    from protein_transformer_amd.train import create_parser, early_stopping_target
    fields = {f.name: f for f in REPORT_FIELDS}
    assert [(f.name, f.keys, f.fixed) for f in REPORT_FIELDS] == \
        [("lddt", ("lddt", "lddt-ca"), True), ("slddt", ("slddt",), True), ("fape", ("fape",), True)] \
        + [(name, keys, False) for name, (keys, *_) in TAIL.items()]
    defaults = vars(create_parser().parse_args([]))
    assert [(m.flag, m.field) for m in EVAL_METRICS] == [(flag, field) for field, (flag, _, _) in METRICS.items()]
    for m in EVAL_METRICS:
        assert len(fields[m.field].keys) == len(m.columns) and defaults[m.flag] is False and callable(m.run)
        assert [key for key, _ in m.columns] == list(METRICS[m.field][2])
        assert "".join(f",{name}" for _, name in m.columns) == METRICS[m.field][1]
        assert m.esm is (m.field == "ss")
    for names in ([key for m in EVAL_METRICS for key, _ in m.columns], [name for m in EVAL_METRICS for _, name in m.columns],
                  [key for m in EVAL_METRICS for key in fields[m.field].keys], [key for f in REPORT_FIELDS for key in f.keys]):
        assert len(set(names)) == len(names), names
    assert METRIC_KEYS == tuple(k for _, _, values in METRICS.values() for k in values) and ESM_KEYS == ("ss-q3", "ss-h", "ss-e")
    parse = create_parser().parse_args
    assert early_stopping_target(parse(["--eval_ss", "-esm", "valid-70-ss-q3"])) == ("valid-70", "ss-q3")
    assert early_stopping_target(parse(["-esm", "valid-70-drmsd"])) == ("valid-70", "drmsd")
    assert early_stopping_target(parse(["-esm", "train-kabsch"])) == ("train", "kabsch")
    assert early_stopping_target(parse(["-l", "kabsch"])) == ("train", "kabsch")
    for key in ("lddt-full", "clash-full", "tm-ca"):                  # the other metrics are no targets: the split stays a split
        assert early_stopping_target(parse(["-esm", f"valid-70-{key}"]))[1] != key


def test_a_report_refuses_a_field_it_does_not_know():
    from protein_transformer_amd.losses import LossReport
    with pytest.raises(ValueError, match="nope"):                     # before anything touches a device
        LossReport(torch.device("cpu"), fields={"nope": None})
    with pytest.raises(ValueError, match="nope"):
        LossReport(torch.device("cpu"), stats=STATS, fields={"clash": None, "nope": np.zeros(B)})
