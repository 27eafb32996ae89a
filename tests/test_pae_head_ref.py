"""CPU checks of tests/pae_head_ref.py, the fp64 restatement the MI355X tests of the PAE head are held against, and of what the
command lines decide on the host: the reference's gradients against central finite differences, its pTM term against the tm formula
of tests/aligned_error_ref.py, an unfitted head, the exactness of the device tests' inputs, `calibration(top=)`, and the refusals of
`predict --ptm` and `confidence calibrate --pae` on a checkpoint without the head (exit 2, no device touched)."""
import json

import numpy as np
import pytest
import torch

import pae_head_ref as R


def small_head(rng, d=8, H=4, nbins=5):
    return {"ln.gamma": rng.normal(1, 0.2, d), "ln.beta": rng.normal(0, 0.2, d), "w1": rng.normal(0, 0.6, (2 * H, d)),
            "b1": rng.normal(0, 0.3, 2 * H), "w2": rng.normal(0, 0.8, (nbins, H)), "b2": rng.normal(0, 0.5, nbins)}


def small_batch(rng, B=2, L=5, d=8, nbins=5, bpa=0.5):
    seq = rng.integers(0, 20, (B, L))
    seq[1, 3:] = 20
    seq[0, 2] = 21
    x = rng.normal(0, 1, (B * L, d))
    target = (rng.random((B, L, L)) * 1.2 * nbins / bpa).astype(np.float32)
    target[0, 1, 3], target[1, 0, 0] = np.nan, np.inf
    return x, seq, target


def test_gradients_against_central_differences():
    rng = np.random.default_rng(1)
    P = small_head(rng)
    x, seq, target = small_batch(rng)
    g = R.head_grads(P, x, seq, target, bpa=0.5, coef=0.7)
    eps = 1e-6
    for name in R.NAMES:
        flat = P[name].reshape(-1)
        for idx in rng.choice(flat.size, min(flat.size, 6), replace=False):
            keep = flat[idx]
            flat[idx] = keep + eps
            up = R.head_loss(P, x, seq, target, 0.5)
            flat[idx] = keep - eps
            down = R.head_loss(P, x, seq, target, 0.5)
            flat[idx] = keep
            assert 0.7 * (up - down) / (2 * eps) == pytest.approx(g[name].reshape(-1)[idx], rel=2e-5, abs=1e-8), (name, idx)


def test_pair_gradient_against_central_differences_of_uv():
    rng = np.random.default_rng(2)
    B, L, H, nbins = 2, 4, 4, 6
    uv = rng.normal(0, 1, (B, L, 2 * H))
    w2, b2 = rng.normal(0, 1, (nbins, H)), rng.normal(0, 1, nbins)
    seq = rng.integers(0, 20, (B, L))
    target = (rng.random((B, L, L)) * 4).astype(np.float32)
    r = R.pair_head(uv, w2, b2, seq, target, 2.0)
    assert (r["abs_duv"] >= np.abs(r["duv"]) - 1e-15).all() and (r["abs_dw2"] >= np.abs(r["dw2"]) - 1e-15).all()
    flat = uv.reshape(-1)
    for idx in range(0, flat.size, 5):
        keep = flat[idx]
        flat[idx] = keep + 1e-6
        up = R.pair_head(uv, w2, b2, seq, target, 2.0)["sums"][0]
        flat[idx] = keep - 1e-6
        down = R.pair_head(uv, w2, b2, seq, target, 2.0)["sums"][0]
        flat[idx] = keep
        assert (up - down) / 2e-6 == pytest.approx(r["duv"].reshape(-1)[idx], rel=2e-5, abs=1e-8)


def test_ptm_of_a_one_hot_distribution_is_the_tm_formula_on_the_bin_centres():
    import aligned_error_ref as A
    nbins, bpa, L, H = 16, 2.0, 23, 4
    rng = np.random.default_rng(3)
    seq = rng.integers(0, 20, (1, L))
    # u = v = 0 -> z = 0 -> the logits are b2 for every pair: one bin at +60 is one-hot to fp64
    for k in (0, 7, nbins - 1):
        b2 = np.zeros(nbins)
        b2[k] = 800.0
        r = R.pair_head(np.zeros((1, L, 2 * H)), np.zeros((nbins, H)), b2, seq, None, bpa)
        centre = (k + 0.5) / bpa
        assert r["pae"][0] == pytest.approx(np.full((L, L), centre), rel=1e-12)
        everyone = np.ones(L, bool)
        mean, tm = A.stats_of(np.full((L, L), centre), everyone, everyone)     # the mean-error formula on a constant matrix
        assert r["stats"][0, 0] == pytest.approx(mean, rel=1e-12) and r["stats"][0, 1] == pytest.approx(tm, rel=1e-12)
    assert R.d0_of(7) == A.d0_of(7) and R.d0_of(300) == A.d0_of(300)


def test_an_unfitted_head_is_flat():
    rng = np.random.default_rng(4)
    P = small_head(rng, nbins=7)
    P["w2"][:], P["b2"][:] = 0.0, 0.0
    x, seq, target = small_batch(rng, nbins=7)
    r = R.head_forward(P, x, seq, target, 0.5)
    assert r["sums"][0] == pytest.approx(np.log(7), rel=1e-14)
    assert r["pae"][r["defined"]] == pytest.approx(np.mean(R.centres(7, 0.5)), rel=1e-14)
    assert np.isnan(r["pae"][~r["defined"]]).all() and not r["defined"][0, 2].any() and not r["defined"][1, :, 3:].any()


def test_the_device_inputs_add_exactly_in_fp32():
    rng = np.random.default_rng(5)
    uv = R.grid_uv(rng, 3, 65, 32)
    u, v = uv[:, :, None, :32], uv[:, None, :, 32:]
    assert np.array_equal((u + v).astype(np.float64), u.astype(np.float64) + v.astype(np.float64))
    assert ((u + v) == 0).sum() > 65 and np.abs(uv).max() <= 4.0
    finite, bins = R.bin_index(np.array([0.5, np.nextafter(np.float32(0.5), np.float32(0)), np.nan, -1.0, 1e30], np.float32), 64, 2.0)
    assert finite.tolist() == [True, True, False, True, True] and bins.tolist() == [1, 0, 0, 0, 63]


def test_a_gradient_below_the_normal_range_needs_the_floor_of_its_measure():
    """Why tests/test_gpu_pae_head.py floors the sum of the summands at 2^-126: one of two bins at +80 and every target in it makes
    du and dv sums of terms ~e^-80 / n, far below fp32's normal range, and the reference ROUNDED TO fp32 - the best an fp32 output
    can be - misses 1e-6 of the unfloored sum; with the floor it is within half an ulp."""
    rng = np.random.default_rng(7)
    L, H = 12, 8
    uv = R.grid_uv(rng, 1, L, H)
    w2 = (rng.normal(0, 0.1, (2, H)) / np.sqrt(H)).astype(np.float32)
    seq = rng.integers(0, 20, (1, L))
    r = R.pair_head(uv, w2, np.array([80.0, -3.0], np.float32), seq, np.full((1, L, L), 0.25, np.float32), 2.0)
    scale, want = r["abs_duv"], r["duv"]
    assert (r["bin"] == 0).all() and 0 < scale[scale > 0].max() < 2.0 ** -126
    miss = np.abs(want.astype(np.float32).astype(np.float64) - want)[scale > 0]
    assert (miss / scale[scale > 0]).max() > 1e-6 and (miss / np.maximum(scale[scale > 0], 2.0 ** -126)).max() <= 2.0 ** -24


def test_calibration_top_scales_the_rows_and_the_default_is_unchanged():
    from protein_transformer_amd.confidence import calibration
    rng = np.random.default_rng(6)
    s, t = rng.random(200) * 100, rng.random(200) * 100
    a = calibration(s, t)
    assert json.dumps(a) == json.dumps(calibration(s, t, top=100.0))
    assert [r["lo"] for r in a["reliability"]] == [10 * i for i in range(10)] and isinstance(a["reliability"][0]["lo"], int)
    b = calibration(s * 0.32, t * 0.32, top=32.0)
    assert [r["n"] for r in b["reliability"]] == [r["n"] for r in a["reliability"]]
    assert b["reliability"][3]["lo"] == pytest.approx(9.6) and b["reliability"][9]["hi"] == pytest.approx(32.0)
    assert b["pearson"] == pytest.approx(a["pearson"], rel=1e-12)


@pytest.fixture()
def headless_checkpoint(tmp_path):
    path = tmp_path / "model.chkpt"
    torch.save({"settings": {}, "model_state_dict": {}}, path)
    return str(path)


def test_predict_ptm_refuses_a_checkpoint_without_the_head(headless_checkpoint, tmp_path, capsys, monkeypatch):
    from protein_transformer_amd import predict
    monkeypatch.setattr(predict, "load_checkpoint", lambda *a, **k: pytest.fail("the model was built"))
    fasta = tmp_path / "s.fasta"
    fasta.write_text(">a\nACDEFGHIK\n")
    assert predict.parser().parse_args([headless_checkpoint, str(fasta), "--out", "x", "--ptm"]).ptm
    assert predict.main([headless_checkpoint, str(fasta), "--out", str(tmp_path / "out"), "--ptm", "--samples", "0"]) == 2
    assert "fit-pae" in capsys.readouterr().err and not (tmp_path / "out").exists()


def test_calibrate_pae_refuses_a_checkpoint_without_head_and_samples(headless_checkpoint, capsys, monkeypatch):
    from protein_transformer_amd import confidence, predict
    monkeypatch.setattr(predict, "load_checkpoint", lambda *a, **k: pytest.fail("the model was built"))
    assert confidence.main(["calibrate", headless_checkpoint, "--synthetic", "2,16,4", "--pae"]) == 2
    assert "fit-pae" in capsys.readouterr().err
    args = confidence.parser().parse_args(["fit-pae", headless_checkpoint, "--synthetic", "2,16,4", "--out", "y"])
    assert (args.hidden, args.nbins, args.epochs) == (32, 64, 1)
    assert confidence.main(["fit-pae", headless_checkpoint, "--synthetic", "2,16,4", "--out", "y", "--hidden", "68"]) == 2
