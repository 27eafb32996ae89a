"""What `--clash_weight` / `--eval_clash` need without a GPU: the entry points in the header, the library and the ctypes table,
their host-side refusals, the kernel's radius table against the atom names and against the side-chain build tables, the flags on
the command line with their refusals, the defaults, the extra log column, and the tail of the loss report."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import clash_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ptamd_clash_fwd_bwd", "ptamd_clash_workspace_bytes", "ptamd_clash_radius")
NAN = float("nan")


@pytest.fixture(scope="module")
def built_lib():
    from protein_transformer_amd import _lib, build
    build.build()                       # hipcc cross-compiles gfx950 without a GPU
    return _lib


def test_header_exports_and_ctypes_table_agree(built_lib):
    import ctypes
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptamd.h")).read(), flags=re.S)
    handle = ctypes.CDLL(built_lib.LIB_PATH)
    built_lib.lib()
    assert not built_lib.MISSING
    kinds = {built_lib._p: "ptr", built_lib._i: "int", built_lib._sz: "size_t", built_lib._f: "float"}
    for name in NAMES:
        decl = re.search(r"\b(size_t|int|float)\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert decl and hasattr(handle, name) and name in built_lib.SIGNATURES, name
        want = ["ptr" if "*" in a else a.split()[0] for a in decl.group(2).split(",")]
        res, args = built_lib.SIGNATURES[name]
        assert [kinds[a] for a in args] == want, name
        assert kinds[res] == decl.group(1), name
    assert len(built_lib.SIGNATURES["ptamd_clash_fwd_bwd"][1]) == 13
    assert "include/ptamd.h" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_radius_table_against_atom_names_and_build_tables(built_lib):
    """ptamd_clash_radius is the table the compaction kernel gets: against ATOM_MAP_14 (which slots exist, which element), against
    h_pt_nsc of csrc/nerf_tables.h (how many side-chain atoms a type has) and against the host-side constants of losses.py."""
    from protein_transformer_amd import losses
    from protein_transformer_amd.protein.PDB_Creator import ATOM_MAP_14
    from protein_transformer_amd.protein.Sequence import VOCAB
    lib = built_lib.lib()
    assert losses.CLASH_RADII == R.RADII == {"C": 1.7, "N": 1.55, "O": 1.52, "S": 1.8} and losses.CLASH_TOLERANCE == 1.5
    assert VOCAB.ints2str(list(range(20))) == R.AA
    src = open(os.path.join(ROOT, "protein_transformer_amd", "csrc", "nerf_tables.h")).read()
    nsc = [int(x) for x in re.search(r"h_pt_nsc\[20\] = \{(.*?)\}", src).group(1).split(",")]
    tab = R.radius_table()
    for r, one in enumerate(R.AA):
        names = ATOM_MAP_14[one]
        assert sum(n != "PAD" for n in names) == 4 + nsc[r] == 4 + lib.ptamd_sidechain_atoms(r), one
        for s, name in enumerate(names):
            got = lib.ptamd_clash_radius(r, s)
            if name == "PAD":
                assert got == -1.0 and np.isnan(tab[r, s]), (one, s)
            else:
                assert got == np.float32(losses.CLASH_RADII[name[0]]) == np.float32(tab[r, s]), (one, name)
        assert lib.ptamd_clash_radius(r, 14) == -1.0 and lib.ptamd_clash_radius(r, -1) == -1.0
    assert lib.ptamd_clash_radius(20, 0) == -1.0 and lib.ptamd_clash_radius(-1, 0) == -1.0 and lib.ptamd_clash_radius(21, 1) == -1.0


def test_entry_points_host_side_checks(built_lib):
    lib = built_lib.lib()
    ws = lib.ptamd_clash_workspace_bytes
    assert ws(32, 512) == lib.ptamd_slddt_workspace_bytes(32, 512) + 256          # the smooth lDDT's and one int per protein
    assert ws(32, 512) == ws(32, 512) and ws(1, 1) > 0                            # a function of (B, L) only
    l_max = (2 ** 31 - 1) // 28
    assert ws(0, 8) == 0 and ws(2, 0) == 0 and ws(-1, 8) == 0 and ws(1, l_max + 1) == 0 and ws(1, l_max) > 0
    B, L = 2, 8
    buf = torch.full((8 * B * L * 42,), 77.0)                 # host memory: every call below is refused before any launch
    at = lambda k: buf.data_ptr() + 4 * k * B * L * 42        # noqa: E731  (disjoint pieces, each large enough for any array)
    pred, seq, stats, nclash, dcrd, wsp = (at(k) for k in range(6))
    ok = dict(pred=pred, seq=seq, B=B, L=L, tol=1.5, w=1.0, acc=0, stats=stats, nclash=nclash, dcrd=dcrd, ws=wsp, wb=1 << 30)

    def run(**kw):
        a = dict(ok, **kw)
        return lib.ptamd_clash_fwd_bwd(a["pred"], a["seq"], a["B"], a["L"], a["tol"], a["w"], a["acc"], a["stats"], a["nclash"],
                                       a["dcrd"], a["ws"], a["wb"], None)

    for kw in (dict(B=0), dict(L=0), dict(B=-1), dict(L=l_max + 1)):
        assert run(**kw) == -1, kw                            # PTAMD_ERR_BAD_SHAPE
    for kw in (dict(tol=-0.5), dict(tol=NAN), dict(tol=float("inf")), dict(w=NAN), dict(w=float("inf")), dict(w=-float("inf"))):
        assert run(**kw) == -1, kw                            # a bad tolerance, a weight that is not finite
    for kw in (dict(pred=None), dict(seq=None), dict(stats=None), dict(nclash=None)):
        assert run(**kw) == -1, kw                            # a NULL array other than dcrd
    for acc in (0, 1):
        assert run(ws=None, acc=acc) == -3 and run(wb=ws(B, L) - 1, acc=acc) == -3 and run(wb=0, acc=acc) == -3
    assert run(dcrd=None, ws=None) == -3                      # the forward-only form is a valid call up to the workspace
    assert run(tol=0.0, w=0.0, ws=None) == -3 and run(w=-2.0, ws=None) == -3      # tolerance 0 and any finite weight are valid
    assert (buf == 77.0).all()                                # nothing was written


def test_defaults_and_no_cpu_path(built_lib):
    from protein_transformer_amd import eval_metrics, losses
    sig = inspect.signature(losses.clash_forward_backward).parameters
    assert list(sig) == ["crd", "seq", "need_grad", "tolerance", "weight", "accumulate_into"]
    assert sig["tolerance"].default == 1.5 and sig["weight"].default == 1.0 and sig["accumulate_into"].default is None
    assert list(inspect.signature(eval_metrics.clash_batch).parameters) == ["crd", "seq", "tolerance"]
    assert inspect.signature(losses.batch_loss).parameters["clash"].default is None            # today's calls are untouched
    report = inspect.signature(losses.LossReport.__init__).parameters
    assert report["fields"].default is None and "clash" not in report     # asked for without a value: fields={"clash": None}
    assert losses.REPORT_KEYS["clash"] == ("clash",)
    with pytest.raises(RuntimeError, match="device tensors only"):      # a missing GPU is an error, never a CPU fall-back
        losses.clash_forward_backward(torch.zeros(1, 28, 3), torch.zeros(1, 2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="device tensors only"):
        eval_metrics.clash_batch(torch.zeros(1, 28, 3), torch.zeros(1, 2, dtype=torch.int64))
    with pytest.raises(AssertionError, match="no side chains are built"):
        losses.batch_loss(torch.zeros(1, 2, 24), torch.zeros(1, 28, 3), torch.zeros(1, 2, dtype=torch.int64), backbone_only=True,
                          clash=(1.0, 1.5))


def test_parser_flags_and_refusals(capsys):
    from protein_transformer_amd.train import create_parser
    a = create_parser().parse_args([])
    assert a.clash_weight == 0.0 and a.clash_tolerance == 1.5 and a.eval_clash is False
    for loss in ("drmsd", "lndrmsd", "combined", "slddt", "fape"):
        a = create_parser().parse_args(["-l", loss, "--clash_weight", "0.5", "--clash_tolerance", "1.25", "--eval_clash",
                                        "--rename_symmetric"])
        assert (a.clash_weight, a.clash_tolerance, a.eval_clash, a.loss) == (0.5, 1.25, True, loss)
    refused = [(["--clash_weight", "1", "--backbone_loss"], "no side chains are built"),
               (["--clash_weight", "1", "-l", "mse"], "build no structure"),
               (["--clash_weight", "1", "-l", "mse", "--train_only"], "build no structure"),
               (["--clash_weight", "-1"], "--clash_weight must be finite and not negative"),
               (["--clash_weight", "nan"], "--clash_weight must be finite and not negative"),
               (["--clash_weight", "inf"], "--clash_weight must be finite and not negative"),
               (["--clash_tolerance", "-0.1"], "--clash_tolerance must be finite and not negative"),
               (["--clash_tolerance", "nan", "--eval_clash"], "--clash_tolerance must be finite and not negative"),
               (["--clash_tolerance", "inf", "--clash_weight", "1"], "--clash_tolerance must be finite and not negative")]
    for argv, message in refused:
        with pytest.raises(SystemExit) as e:
            create_parser().parse_args(argv)
        assert e.value.code == 2, argv
        err = capsys.readouterr().err
        assert message in err and ("--clash_weight" in err or "--clash_tolerance" in err), argv
    # the metric alone needs no side-chain loss: evaluation builds every atom whatever trains
    for argv in (["--eval_clash", "--backbone_loss"], ["--eval_clash", "-l", "mse"], ["--clash_weight", "0", "-l", "mse"],
                 ["--clash_weight", "0", "--backbone_loss"], ["--clash_tolerance", "0"]):
        create_parser().parse_args(argv)


def test_get_losses_refuses_before_any_device_work():
    from protein_transformer_amd.train import get_losses
    none = torch.zeros(0, 4, dtype=torch.int64)
    args = types.SimpleNamespace(loss="drmsd", backbone_loss=True, clash_weight=0.5)
    with pytest.raises(ValueError, match="no side chains are built"):
        get_losses(args, None, None, None, none)
    args = types.SimpleNamespace(loss="mse", backbone_loss=False, clash_weight=0.5)
    with pytest.raises(ValueError, match="build no structure"):
        get_losses(args, None, None, None, none)


def test_the_log_gains_one_trailing_column():
    import csv
    import io
    from protein_transformer_amd import log
    ns = lambda **kw: types.SimpleNamespace(loss="drmsd", lr_scheduling="plateau", **kw)      # noqa: E731
    plain = log.prepare_log_header(ns())
    assert log.prepare_log_header(ns(eval_clash=True)) == plain + ",clash"
    assert log.prepare_log_header(ns(eval_clash=True, eval_lddt=True)) == plain + ",lddt,lddt_ca,clash"
    assert log.prepare_log_header(ns(eval_clash=False, clash_weight=1.0)) == plain      # the training term alone adds no column
    metrics = log.init_metrics(ns())
    losses = {k: 1.0 for k in log._TRACKED}
    for mode, value in (("valid-10", 0.25), ("valid-10", NAN), ("valid-10", 0.75)):
        if value == 0.25:
            log.reset_metrics_for_epoch(metrics, mode)
        log.update_metrics(metrics, dict(losses, **{"clash-full": value}), mode, torch.zeros(1, 4, dtype=torch.int64),
                           batch_level=False)
    log.do_eval_epoch_logging(metrics, "valid-10")
    assert metrics["valid-10"]["epoch-clash-full"] == 0.5                     # the batch without a value is left out
    rows = []
    for kw in ({}, {"clash": True}, {"lddt": True, "clash": True}):
        out = io.StringIO()
        log.log_batch(csv.writer(out), metrics, 0.0, mode="valid-10", end_of_epoch=True, t=5.0, **kw)
        rows.append(out.getvalue().strip().split(","))
    assert len(rows[1]) == len(rows[0]) + 1 and rows[1][:-1] == rows[0][:len(rows[0])] and float(rows[1][-1]) == 0.5
    assert len(rows[2]) == len(rows[0]) + 3 and rows[2][-3:-1] == ["nan", "nan"] and float(rows[2][-1]) == 0.5
    log.reset_metrics_for_epoch(metrics, "valid-10")
    assert not any("clash" in k for k in metrics["valid-10"])


# ----------------------------------------------------------------------------- the tail of the loss report
B = 3
STATS = (torch.arange(B * 8, dtype=torch.float32).reshape(B, 8) * 3 + 4) / 8
MSE = torch.tensor([1.5, 4.0, 0.75, 2.0, 0.25, 2.0])
STATUS = torch.tensor([0b1001], dtype=torch.int32)
CLASH = torch.tensor([0.125, NAN, 0.625])
FAPE = torch.tensor([1.5, 2.25, NAN])


def test_the_tail_of_a_single_process():
    from protein_transformer_amd.losses import pack_local, unpack_local
    plain_buf, plain_layout = pack_local(STATS, MSE, STATUS, None, {"fape": FAPE})
    buf, layout = pack_local(STATS, MSE, STATUS, None, {"fape": FAPE}, tail={"clash": CLASH})
    assert buf.numel() == plain_buf.numel() + B
    for field, at in plain_layout[1].items():                                # everything in front lies where it lay, bit for bit
        assert layout[1][field] == at and torch.equal(buf[at].view(torch.int32), plain_buf[at].view(torch.int32)), field
    assert list(layout[1]) == list(plain_layout[1]) + ["clash"] and layout[1]["clash"] == slice(buf.numel() - B, buf.numel())
    out, plain = unpack_local(buf.numpy(), layout), unpack_local(plain_buf.numpy(), plain_layout)
    assert "clash" not in plain and list(out) == list(plain) + ["clash"]     # without a tail: exactly the keys of before
    assert out["clash"] == 0.375 and out["fape"] == plain["fape"] == 1.875
    # asked for, no value: the key exists and is None; a value without a finite entry: NaN
    buf, layout = pack_local(STATS, MSE, STATUS, tail={"clash": None})
    assert buf.numel() == B * 9 + 7 and unpack_local(buf.numpy(), layout)["clash"] is None
    buf, layout = pack_local(tail={"clash": None})
    assert buf.numel() == 7 and unpack_local(buf.numpy(), layout)["clash"] is None
    buf, layout = pack_local(STATS, MSE, STATUS, tail={"clash": torch.full((B,), NAN)})
    assert np.isnan(unpack_local(buf.numpy(), layout)["clash"])
    buf, layout = pack_local(tail={"clash": CLASH})                          # the value alone still knows its B
    assert layout[0] == B and unpack_local(buf.numpy(), layout)["clash"] == 0.375


def test_the_tail_of_the_reduced_vector():
    from protein_transformer_amd.losses import VECTOR_SIZE, reduce_vector, unpack_global
    assert VECTOR_SIZE == 27 and reduce_vector(STATS, MSE, STATUS).shape == (27,)             # nobody asked: the vector of before
    ranks = [dict(stats=STATS[:2], mse=MSE, status=STATUS, channels={"fape": FAPE[:2]}, tail={"clash": CLASH[:2]}),
             dict(stats=STATS[2:], mse=MSE, status=STATUS, channels={"fape": FAPE[2:]}, tail={"clash": CLASH[2:]}),
             dict(tail={"clash": None})]                                      # an empty shard: same length, adds nothing
    vs = [reduce_vector(**kw) for kw in ranks]
    assert [v.shape for v in vs] == [(29,)] * 3 and vs[2].tolist() == [0.0] * 29
    assert vs[0][27:].tolist() == [0.125, 1.0] and vs[1][27:].tolist() == [0.625, 1.0]
    plain = reduce_vector(**{k: v for k, v in ranks[0].items() if k != "tail"})
    assert torch.equal(vs[0][:27], plain)                                     # the slots in front are untouched
    v = sum(vs).numpy()
    for passed in ({"fape", "clash"}, set()):                                 # the empty shard reads the same numbers
        out = unpack_global(v, passed, ("clash",))
        assert out["clash"] == 0.375 and out["fape"] == 1.875 and out["n_proteins"] == 3
    assert "clash" not in unpack_global(v[:27], {"fape"}) and list(out)[-1] == "clash"
    # nobody has a value: None on a rank that passed nothing, NaN on one that passed NaNs
    v = (reduce_vector(stats=STATS, tail={"clash": torch.full((B,), NAN)}) + reduce_vector(tail={"clash": None})).numpy()
    assert np.isnan(unpack_global(v, {"clash"}, ("clash",))["clash"]) and unpack_global(v, set(), ("clash",))["clash"] is None
