"""CPU checks of the confidence head's host side: tests/plddt_ref.py (the fp64 restatement of csrc/plddt.hip and of the head) against
central differences of its own loss, the fp32 bin rule at its edges, `confidence.calibration` on hand-built arrays, the checkpoint
round trip of the `confidence_head` key, the four entry points of include/ptamd.h, and `predict --plddt` refusing a checkpoint
without a head.  The kernels and the fit need the GPU: tests/test_gpu_plddt.py, tests/test_gpu_confidence.py."""
import math
import os
import types

import numpy as np
import pytest
import torch

import plddt_ref as R


def random_head(rng, d=12, h=8, nbins=7):
    return {"ln.gamma": rng.normal(1, 0.2, d), "ln.beta": rng.normal(0, 0.2, d), "w1": rng.normal(0, 0.5, (h, d)),
            "b1": rng.normal(0, 0.2, h), "w2": rng.normal(0, 0.5, (nbins, h)), "b2": rng.normal(0, 0.2, nbins)}


# ------------------------------------------------------------------------------------------------ the reference itself
def test_bin_rule_is_fp32_at_the_edges():
    for nbins in (2, 50, 63, 64):
        edges = (np.arange(nbins + 1, dtype=np.float64) / nbins).astype(np.float32)
        counted, b = R.bin_index(edges, nbins)
        assert counted.all()
        # the fp32 product k / nbins * nbins, rounded once, decides - not the real number
        want = np.clip(np.floor(edges * np.float32(nbins)).astype(np.int64), 0, nbins - 1)
        assert (b == want).all() and b[0] == 0 and b[-1] == nbins - 1
        below = np.nextafter(edges[1:], np.float32(-1))
        above = np.nextafter(edges[:-1], np.float32(2))
        assert (R.bin_index(above, nbins)[1] >= b[:-1]).all() and (R.bin_index(below, nbins)[1] <= b[1:]).all()
    counted, b = R.bin_index(np.array([np.nan, np.inf, -np.inf, -0.25, 1.5, 3e38, 0.5], np.float32), 50)
    assert list(counted) == [False, False, False, True, True, True, True] and list(b[3:]) == [0, 49, 49, 25]


def test_bin_loss_on_known_rows():
    nbins = 50
    uniform = np.zeros((3, nbins))
    r = R.bin_loss(uniform, np.array([0.0, 0.37, np.nan], np.float32))
    assert np.allclose(r["plddt"], 50.0, rtol=0, atol=1e-12)
    assert np.allclose(r["ce"][:2], math.log(nbins), rtol=1e-15) and np.isnan(r["ce"][2])
    assert r["sums"][1] == 2 and abs(r["sums"][0] - math.log(nbins)) < 1e-14
    # a confident, correct row: the loss is the others' mass, not log(1 + tiny) = 0
    x = np.zeros((1, nbins))
    x[0, 10] = 80.0
    r = R.bin_loss(x, np.array([10.5 / nbins], np.float32))
    assert r["ce"][0] == pytest.approx(49 * math.exp(-80.0), rel=1e-12) and r["plddt"][0] == pytest.approx(21.0, rel=1e-12)
    # ... and a confident, wrong one
    r = R.bin_loss(x, np.array([0.0], np.float32))
    assert r["ce"][0] == pytest.approx(80.0, rel=1e-12)
    none = R.bin_loss(uniform, np.full(3, np.nan, np.float32))
    assert np.isnan(none["sums"][0]) and none["sums"][1] == 0 and np.isnan(none["ce"]).all()
    assert (R.bin_loss_grad(uniform, np.full(3, np.nan, np.float32)) == 0).all()
    assert set(R.bin_loss(uniform)) == {"plddt"}


def test_bin_loss_gradient_against_central_differences():
    rng = np.random.default_rng(1)
    T, nbins = 9, 11
    x = rng.normal(0, 2, (T, nbins))
    target = rng.random(T).astype(np.float32)
    target[[2, 5]] = [np.nan, np.inf]
    g = R.bin_loss_grad(x, target, coef=0.7)
    assert (g[[2, 5]] == 0).all() and np.abs(g.sum(axis=1)).max() < 1e-15
    num = np.zeros_like(g)
    for t in range(T):
        for k in range(nbins):
            hi, lo = x.copy(), x.copy()
            hi[t, k] += 1e-5
            lo[t, k] -= 1e-5
            num[t, k] = 0.7 * (R.bin_loss(hi, target)["sums"][0] - R.bin_loss(lo, target)["sums"][0]) / 2e-5
    assert np.abs(g - num).max() < 1e-9 * max(1.0, np.abs(g).max())


def test_head_gradients_against_central_differences():
    rng = np.random.default_rng(2)
    P = random_head(rng)
    x = rng.normal(0, 1, (10, 12))
    target = rng.random(10).astype(np.float32)
    target[3] = np.nan
    a = R.head_logits(P, x)
    assert np.abs(a["z"]).min() > 1e-4                       # no unit sits on the kink of its ReLU: the differences are clean
    g = R.head_grads(P, x, target)
    for name in R.NAMES:
        num = np.zeros_like(P[name])
        it = np.nditer(P[name], flags=["multi_index"])
        for _ in it:
            i = it.multi_index
            keep = P[name][i]
            P[name][i] = keep + 1e-6
            hi = R.head_loss(P, x, target)
            P[name][i] = keep - 1e-6
            lo = R.head_loss(P, x, target)
            P[name][i] = keep
            num[i] = (hi - lo) / 2e-6
        assert np.abs(g[name] - num).max() < 1e-8 * max(1.0, np.abs(num).max()), name


def test_unfitted_head_is_uniform():
    rng = np.random.default_rng(3)
    P = random_head(rng, nbins=50)
    P["w2"][:] = 0
    P["b2"][:] = 0
    x = rng.normal(0, 3, (5, 12))
    r = R.bin_loss(R.head_logits(P, x)["logits"], rng.random(5).astype(np.float32))
    assert np.allclose(r["ce"], math.log(50), rtol=1e-15) and np.allclose(r["plddt"], 50.0, rtol=1e-15)


# ------------------------------------------------------------------------------------------------ calibration
def test_calibration_perfect_constant_and_anticorrelated():
    from protein_transformer_amd.confidence import calibration
    truth = np.array([5.0, 15.0, 25.0, 35.0, 45.0, 55.0, 65.0, 75.0, 85.0, 95.0, 100.0])
    c = calibration(truth, truth)
    assert c["n"] == 11 and c["pearson"] == pytest.approx(1.0, abs=1e-15) and c["mae"] == 0 and c["bias"] == 0
    assert [r["n"] for r in c["reliability"]] == [1] * 9 + [2]                          # 100 closes the last row
    assert [(r["lo"], r["hi"]) for r in c["reliability"]] == [(10 * i, 10 * i + 10) for i in range(10)]
    assert c["reliability"][3]["mean_truth"] == 35.0 and c["reliability"][9]["mean_truth"] == 97.5
    const = calibration(np.full(11, 50.0), truth)
    assert const["pearson"] is None and const["bias"] == pytest.approx(50.0 - truth.mean())
    assert const["mae"] == pytest.approx(np.abs(50.0 - truth).mean())
    assert [r["n"] for r in const["reliability"]] == [0] * 5 + [11] + [0] * 4
    assert const["reliability"][5]["mean_truth"] == pytest.approx(truth.mean()) and const["reliability"][0]["mean_truth"] is None
    anti = calibration(100.0 - truth, truth)
    assert anti["pearson"] == pytest.approx(-1.0, abs=1e-15) and anti["bias"] == pytest.approx(100.0 - 2 * truth.mean())
    assert anti["reliability"][0]["mean_truth"] == 97.5 and anti["reliability"][9]["mean_truth"] == 5.0
    assert sum(r["n"] for r in anti["reliability"]) == anti["n"] == 11


def test_calibration_drops_what_is_not_finite_and_survives_nothing():
    from protein_transformer_amd.confidence import calibration
    c = calibration([10.0, np.nan, 30.0, 70.0, np.inf], [20.0, 50.0, np.nan, 60.0, 5.0])
    assert c["n"] == 2 and c["bias"] == pytest.approx(0.0) and c["mae"] == pytest.approx(10.0) and c["pearson"] == pytest.approx(1.0)
    assert sum(r["n"] for r in c["reliability"]) == 2
    empty = calibration([np.nan], [1.0])
    assert empty["n"] == 0 and empty["pearson"] is None and empty["mae"] is None and empty["bias"] is None
    assert all(r["n"] == 0 and r["mean_truth"] is None for r in empty["reliability"]) and len(empty["reliability"]) == 10
    one = calibration([42.0], [40.0])
    assert one["n"] == 1 and one["pearson"] is None and one["bias"] == 2.0
    with pytest.raises(ValueError):
        calibration([1.0, 2.0], [1.0])
    assert calibration([-5.0, 130.0], [0.0, 100.0])["reliability"][0]["n"] == 1           # clamped into the end rows


# ------------------------------------------------------------------------------------------------ checkpoints and the CLI
def fake_checkpoint(path):
    ck = {"model_state_dict": {"w": torch.arange(6.0).view(2, 3)}, "settings": types.SimpleNamespace(model="enc-only", d_model=64),
          "epoch": 3, "optimizer_state_dict": {"state": {}}, "scheduler_state_dict": None, "loss": 1.5, "metrics": {"a": [1, 2]},
          "elapsed_time": 12.0}
    torch.save(ck, path)
    return ck


def test_checkpoint_round_trip_of_the_head(tmp_path):
    from protein_transformer_amd import confidence as CF
    src, dst = str(tmp_path / "a.chkpt"), str(tmp_path / "b.chkpt")
    ck = fake_checkpoint(src)
    assert CF.read_head_entry(src) is None and CF.load_head(src, "cpu") is None
    head = CF.ConfidenceHead(64, hidden=16, nbins=50, device="cpu", seed=4)
    assert (head.params["w2"] == 0).all() and (head.params["b2"] == 0).all() and (head.params["ln.gamma"] == 1).all()
    assert head.params["w2"].shape == (50, 16) and float(head.params["w1"].abs().max()) <= math.sqrt(6.0 / 80)
    same = CF.ConfidenceHead(64, hidden=16, nbins=50, device="cpu", seed=4)
    assert torch.equal(head.flat, same.flat) and not torch.equal(head.flat, CF.ConfidenceHead(64, 16, 50, "cpu", seed=5).flat)
    g = torch.Generator().manual_seed(0)
    for v in head.params.values():
        v.copy_(torch.randn(v.shape, generator=g))
    head.steps = 17
    CF.save_with_head(src, dst, head)
    back = torch.load(dst, map_location="cpu", weights_only=False)
    assert set(back) == set(ck) | {"confidence_head"}
    assert torch.equal(back["model_state_dict"]["w"], ck["model_state_dict"]["w"]) and list(back["model_state_dict"]) == ["w"]
    assert back["epoch"] == 3 and back["metrics"] == {"a": [1, 2]} and vars(back["settings"]) == vars(ck["settings"])
    entry = back["confidence_head"]
    assert set(entry) == {"state_dict", "settings"} and tuple(entry["state_dict"]) == CF.NAMES
    assert entry["settings"] == {"d_in": 64, "hidden": 16, "nbins": 50, "lddt_cutoff": 15.0, "steps": 17}
    again = CF.load_head(dst, "cpu")
    assert again.steps == 17 and torch.equal(again.flat, head.flat)                        # the spare rows of w2 / b2: zero in both
    assert all(v.device.type == "cpu" for v in entry["state_dict"].values())
    with pytest.raises(ValueError, match="w1"):
        CF.ConfidenceHead(64, hidden=32, nbins=50, device="cpu").load_state_dict(entry["state_dict"])
    with pytest.raises(ValueError, match="not a checkpoint"):
        CF.read_head_entry(str(tmp_path / "missing.chkpt"))
    for bad in [dict(d_in=62), dict(hidden=6), dict(nbins=1), dict(nbins=65)]:
        with pytest.raises(ValueError):
            CF.ConfidenceHead(**{"d_in": 64, "hidden": 16, "nbins": 50, "device": "cpu", **bad})


def test_predict_plddt_refuses_a_checkpoint_without_a_head(tmp_path, capsys):
    from protein_transformer_amd import predict
    ckpt = str(tmp_path / "plain.chkpt")
    fake_checkpoint(ckpt)
    fasta = tmp_path / "s.fasta"
    fasta.write_text(">a\nMKV\n")
    rc = predict.main([ckpt, str(fasta), "--out", str(tmp_path / "never"), "--samples", "0", "--plddt"])
    err = capsys.readouterr().err
    assert rc == 2 and err.startswith("predict: ") and err.count("\n") == 1 and "confidence head" in err
    assert not os.path.exists(tmp_path / "never")
    assert predict.KEYS == ("id", "n-res", "ens-lddt", "ens-rmsd", "ens-rmsf-ca", "usable", "samples")
    assert predict.PER_RESIDUE_HEADER == ("resnum", "resname", "conf", "rmsf_ca", "rmsf_all") and predict.PLDDT_KEYS == ("plddt",)


def test_confidence_cli_refusals(tmp_path, capsys):
    from protein_transformer_amd import confidence as CF
    ckpt = str(tmp_path / "plain.chkpt")
    fake_checkpoint(ckpt)
    for argv in (["calibrate", ckpt, "--synthetic", "2,16,1"],                              # no head, no samples: no score
                 ["calibrate", str(tmp_path / "none.chkpt"), "--synthetic", "2,16,1", "--samples", "2"],
                 ["fit", ckpt, "--synthetic", "2,16,1", "--out", str(tmp_path / "o.chkpt"), "--nbins", "65"],
                 ["fit", ckpt, "--synthetic", "2,16,1", "--out", str(tmp_path / "o.chkpt"), "--hidden", "30"]):
        assert CF.main(argv) == 2
        err = capsys.readouterr().err
        assert err.startswith("confidence: ") and err.count("\n") == 1
    assert not os.path.exists(tmp_path / "o.chkpt")


# ------------------------------------------------------------------------------------------------ the C ABI
def test_plddt_entry_points_validate_on_the_host():
    from protein_transformer_amd import _lib, build
    build.build()
    lib = _lib.lib()
    R_ = lib.ptamd_plddt_rows_per_block()
    assert R_ >= 1
    assert lib.ptamd_plddt_workspace_bytes(0) == 0 and lib.ptamd_plddt_workspace_bytes(-3) == 0
    assert lib.ptamd_plddt_workspace_bytes(1) == lib.ptamd_plddt_workspace_bytes(R_) == 16
    assert lib.ptamd_plddt_workspace_bytes(R_ + 1) == 32 and lib.ptamd_plddt_workspace_bytes(5 * R_ + 1) == 96
    fwd = lambda **kw: lib.ptamd_plddt_fwd(*[{**dict(logits=16, ld=52, target=16, stride=1, T=4, nbins=50, plddt=16, ce=16, sums=16,  # noqa: E731
                                                     ws=16, ws_bytes=16, stream=None), **kw}[k] for k in
                                             ("logits", "ld", "target", "stride", "T", "nbins", "plddt", "ce", "sums", "ws", "ws_bytes",
                                              "stream")])
    for kw in (dict(T=0), dict(T=-1), dict(nbins=1), dict(nbins=65), dict(ld=49), dict(logits=None), dict(plddt=None),
               dict(ce=None), dict(sums=None), dict(stride=0)):
        assert fwd(**kw) == -1, kw                                                          # PTAMD_ERR_BAD_SHAPE
    assert fwd(ws=None) == -3 and fwd(ws_bytes=15) == -3 and fwd(T=R_ + 1, ws_bytes=16) == -3   # PTAMD_ERR_WORKSPACE
    assert fwd(ws=24) == -5                                                                 # PTAMD_ERR_ALIGN
    bwd = lambda **kw: lib.ptamd_plddt_bwd(*[{**dict(logits=16, ld=52, target=16, stride=2, T=4, nbins=50, sums=16, coef=1.0,  # noqa: E731
                                                     dlogits=16, ldd=52, stream=None), **kw}[k] for k in
                                             ("logits", "ld", "target", "stride", "T", "nbins", "sums", "coef", "dlogits", "ldd", "stream")])
    for kw in (dict(T=0), dict(nbins=1), dict(nbins=65), dict(ld=49), dict(ldd=49), dict(logits=None), dict(target=None),
               dict(sums=None), dict(dlogits=None), dict(stride=0)):
        assert bwd(**kw) == -1, kw
