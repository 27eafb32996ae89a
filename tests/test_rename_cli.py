"""What `--rename_symmetric` needs without a GPU: the two entry points in the header, the library and the ctypes table, their
host-side refusals, the swap table against the atom names and against the side-chain build, the flag on the command line with its
refusals, the defaults, and the fp64 reference of the GPU tests against a plain triple loop."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

import rename_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ptamd_rename_symmetric", "ptamd_rename_symmetric_workspace_bytes")


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
    kinds = {built_lib._p: "ptr", built_lib._i: "int", built_lib._sz: "size_t"}
    for name in NAMES:
        decl = re.search(r"\b(size_t|int)\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert decl and hasattr(handle, name) and name in built_lib.SIGNATURES, name
        want = ["ptr" if "*" in a else "size_t" if a.strip().startswith("size_t") else "int" for a in decl.group(2).split(",")]
        res, args = built_lib.SIGNATURES[name]
        assert [kinds[a] for a in args] == want, name
        assert kinds[res] == decl.group(1), name
    assert len(built_lib.SIGNATURES["ptamd_rename_symmetric"][1]) == 13


def test_entry_points_host_side_checks(built_lib):
    lib = built_lib.lib()
    ws = lib.ptamd_rename_symmetric_workspace_bytes
    need = ws(32, 512)
    assert 32 * 512 * (14 * 32 + 40) < need < 64 << 20        # 32 B per atom slot, 40 B per residue + the partial sums
    assert need == ws(32, 512) and ws(1, 1) > 0               # a function of (B, L) only
    assert ws(0, 512) == 0 and ws(32, 0) == 0 and ws(-1, 8) == 0 and ws(1, (2 ** 31 - 1) // 28 + 1) == 0
    B, L = 2, 8
    big = 1 << 30
    buf = torch.zeros(16 * B * L * 42)                        # host memory: every call below is refused before any launch
    at = lambda k: buf.data_ptr() + 4 * k * B * L * 42        # noqa: E731  (disjoint pieces, each large enough for any array)
    pred, true, ang, seq, out, ang_out, swapped, cost, wsp = (at(k) for k in range(9))
    call = lib.ptamd_rename_symmetric
    ok = dict(pred=pred, true=true, ang=ang, seq=seq, out=out, ang_out=ang_out, swapped=swapped, cost=cost, ws=wsp, wb=big, B=B, L=L)

    def run(**kw):
        a = dict(ok, **kw)
        return call(a["pred"], a["true"], a["ang"], a["seq"], a["B"], a["L"], a["out"], a["ang_out"], a["swapped"], a["cost"],
                    a["ws"], a["wb"], None)

    for kw in (dict(B=0), dict(L=0), dict(B=-1), dict(L=(2 ** 31 - 1) // 28 + 1)):
        assert run(**kw) == -1, kw                            # tile_shape_ok: PTAMD_ERR_BAD_SHAPE
    for kw in (dict(pred=None), dict(true=None), dict(seq=None), dict(out=None), dict(swapped=None), dict(cost=None)):
        assert run(**kw) == -1, kw                            # a NULL array
    assert run(ang=None) == -1 and run(ang_out=None) == -1    # only one of the angle pair
    assert run(out=true) == -1 and run(out=pred) == -1 and run(ang_out=ang) == -1           # an output on its input
    assert run(out=true + 12) == -1 and run(out=pred - 12) == -1 and run(ang_out=ang + 4) == -1       # ... or overlapping it
    assert run(ws=None) == -3 and run(wb=ws(B, L) - 1) == -3 and run(wb=0) == -3            # PTAMD_ERR_WORKSPACE
    assert run(ang=None, ang_out=None, ws=None) == -3         # both angle arrays NULL is a valid call up to the workspace
    assert run(ws=wsp + 4) == -5 and run(ws=wsp + 8) == -5    # PTAMD_ERR_ALIGN: the workspace is 16-byte aligned
    assert not buf.any()                                      # nothing was written


def test_swap_table_equals_the_one_derived_from_atom_names():
    from protein_transformer_amd import losses
    from protein_transformer_amd.protein.PDB_Creator import ATOM_MAP_14
    derived = R.swaps_from_atom_names(ATOM_MAP_14)
    assert derived == losses.SYMMETRIC_SWAPS == R.SWAPS
    assert sorted(R.AA[r] for r in derived) == ["D", "E", "F", "Y"]
    names = lambda r: [tuple(ATOM_MAP_14[R.AA[r]][s] for s in pair) for pair in derived[r][0]]      # noqa: E731
    assert names(2) == [("OD1", "OD2")] and names(3) == [("OE1", "OE2")]
    assert names(4) == names(19) == [("CD1", "CD2"), ("CE1", "CE2")]


@pytest.mark.parametrize("res", sorted(R.SWAPS))
def test_turning_the_chi_column_by_pi_exchanges_the_names(res):
    """The side-chain build itself: side-chain atom k is placed with angle column 6 + k, so the column that exchanges OD1/OD2 of ASP
    is 8 (not 7, which turns CG and everything behind it).  Built twice by the CPU oracle, the second time with the table's column
    turned by pi: the swap pairs change places (exactly symmetric build constants for ASP, GLU, PHE; TYR's ring closes to 0.03 A),
    every other atom stays."""
    from oracle import geometry
    from protein_transformer_amd import synthetic
    pairs, col = R.SWAPS[res]
    seq = torch.tensor([0, res, 9])
    ang = torch.from_numpy(synthetic.sample_angles(np.random.default_rng(res), 3))
    a = geometry.generate_coords(ang, seq).numpy().reshape(3, 14, 3)
    turned = ang.clone()
    turned[1, col] += np.pi
    b = geometry.generate_coords(turned, seq).numpy().reshape(3, 14, 3)
    expect = a.copy()
    for x, y in pairs:
        expect[1, [x, y]] = expect[1, [y, x]]
    tol = 0.05 if res == 19 else 1e-4
    assert np.abs(b - expect).max() < tol
    assert np.abs(b - a).max() > 1.0                        # and the turn did move the pair
    wrong = ang.clone()
    wrong[1, col - 1] += np.pi
    assert np.abs(geometry.generate_coords(wrong, seq).numpy().reshape(3, 14, 3) - expect).max() > 1.0


def test_parser_flag_and_refusals(capsys):
    from protein_transformer_amd.train import create_parser
    assert create_parser().parse_args([]).rename_symmetric is False
    for loss in ("drmsd", "lndrmsd", "combined", "slddt", "fape"):
        a = create_parser().parse_args(["-l", loss, "--rename_symmetric", "--eval_lddt"])
        assert a.rename_symmetric is True and a.loss == loss
    with pytest.raises(SystemExit) as e:
        create_parser().parse_args(["--rename_symmetric", "--backbone_loss"])
    assert e.value.code == 2
    assert "no side chains are built" in capsys.readouterr().err
    for more in ([], ["--train_only"]):
        with pytest.raises(SystemExit) as e:
            create_parser().parse_args(["-l", "mse", "--rename_symmetric", *more])
        assert e.value.code == 2
        assert "build no structure" in capsys.readouterr().err
    assert create_parser().parse_args(["-l", "mse"]).rename_symmetric is False       # -l mse itself keeps working


def test_get_losses_refuses_before_any_device_work():
    from protein_transformer_amd.train import get_losses
    none = torch.zeros(0, 4, dtype=torch.int64)
    args = types.SimpleNamespace(loss="drmsd", backbone_loss=True, rename_symmetric=True)
    with pytest.raises(ValueError, match="no side chains are built"):
        get_losses(args, None, None, None, none)
    args = types.SimpleNamespace(loss="mse", backbone_loss=False, rename_symmetric=True)
    with pytest.raises(ValueError, match="build no structure"):
        get_losses(args, None, None, None, none)


def test_defaults_are_off_and_no_cpu_path(built_lib):
    from protein_transformer_amd import losses
    sig = inspect.signature(losses.batch_loss).parameters
    assert sig["rename_symmetric"].default is False and sig["true_ang"].default is None
    assert list(sig)[-2:] == ["rename_symmetric", "true_ang"]                         # behind the existing ones
    assert list(inspect.signature(losses.rename_symmetric).parameters) == ["crd", "true_crds", "seq", "true_ang"]
    assert inspect.signature(losses.rename_symmetric).parameters["true_ang"].default is None
    assert not any("rename" in p for p in inspect.signature(losses.LossReport.__init__).parameters)     # nothing new is reported
    with pytest.raises(RuntimeError, match="device tensors only"):      # a missing GPU is an error, never a CPU fall-back
        losses.rename_symmetric(torch.zeros(1, 28, 3), torch.zeros(1, 28, 3), torch.zeros(1, 2, dtype=torch.int64))
    with pytest.raises(AssertionError, match="no side chains are built"):
        losses.batch_loss(torch.zeros(1, 2, 24), torch.zeros(1, 28, 3), torch.zeros(1, 2, dtype=torch.int64), backbone_only=True,
                          rename_symmetric=True)


HAND = [("DA", None), ("GFYE", (2, 7)), ("WDEYF", (3, 10))]      # (sequence, a NaN atom (residue, slot) or None)


@pytest.mark.parametrize("text,missing", HAND)
def test_vectorised_reference_agrees_with_a_plain_triple_loop(text, missing):
    from protein_transformer_amd import synthetic
    rng = np.random.default_rng(len(text))
    seq = np.array([R.AA.index(c) for c in text] + [R.PAD_ID])
    L = len(seq)
    own = synthetic.slot_mask(torch.from_numpy(seq)[None])[0].numpy()
    truth = rng.normal(0, 4, (L * 14, 3)).astype(np.float32)
    truth[~own] = np.nan
    truth[(L - 1) * 14:] = 0                                      # batch padding carries zeros
    if missing:
        truth[missing[0] * 14 + missing[1]] = np.nan
    pred = (truth + rng.normal(0, 1.5, truth.shape)).astype(np.float32)
    pred[np.isnan(pred)] = 0
    ang = rng.normal(0, 1, (L, 24)).astype(np.float32)
    out, ang_out, swapped, cost = R.rename_reference(pred, truth, seq, ang)
    swapped2, cost2 = R.rename_loops(pred, truth, seq)
    assert (swapped == swapped2).all() and np.allclose(cost, cost2, rtol=1e-12, atol=0)
    cand = R.candidates(truth, seq)
    assert cand and all(cost[r, 0] > 0 for r in cand) and not cost[[r for r in range(L) if r not in cand]].any()
    if missing:                                                   # the residue whose swap partner is missing is no candidate
        assert missing[0] not in cand and int(seq[missing[0]]) in R.SWAPS
    # the application, by hand: a swapped residue has its pairs exchanged and its chi column negated, nothing else moves
    t3, o3 = truth.reshape(L, 14, 3), out.reshape(L, 14, 3)
    for r in range(L):
        pairs, col = R.SWAPS.get(int(seq[r]), ((), 0))
        moved = {s: s for s in range(14)}
        if swapped[r]:
            moved.update({a: b for a, b in pairs} | {b: a for a, b in pairs})
        for s in range(14):
            assert o3[r, s].tobytes() == t3[r, moved[s]].tobytes()
        want = ang[r].copy().reshape(12, 2)
        if swapped[r]:
            want[col] = -want[col]
        assert ang_out[r].tobytes() == want.tobytes()
    # prediction = the truth under the other naming of every candidate: all swapped, alt exactly zero
    flipped, _ = R.apply(truth, None, seq, np.isin(np.arange(L), cand).astype(np.int32))
    p2 = np.where(np.isnan(flipped), 0, flipped).astype(np.float32)
    out2, _, swapped3, cost3 = R.rename_reference(p2, truth, seq)
    assert all(swapped3[r] == 1 and cost3[r, 1] == 0 for r in cand) and swapped3.sum() == len(cand)
    assert out2.tobytes() == flipped.tobytes()
