"""MI355X tests of the PAE head above its kernels (protein_transformer_amd/confidence.py: PaeHead, fit_pae_head, `fit-pae`,
`calibrate --pae`; predict.py: `--ptm`) on a one-layer, d_model 32 encoder and synthetic proteins of L <= 48: one forward and
backward of the head against its fp64 restatement (tests/pae_head_ref.py) on the same hidden state with a non-zero last layer,
the unfitted head, the fit (it learns, it is deterministic) and the commands end to end.

BARS of the head.  uv: max |got - ref| / max(1, max |ref|), the form of the project's 1e-5 parity bar and
never above it; every one of the six gradients by its own rel-L2 (the largest of the six is held), never above the project's 1e-3 gradient bar (README.md); both 8 x the value measured
on the MI355X (profiles/pae_head/NOTES.md).  pae, stats and the mean CE are held to the kernel's own bars
(tests/test_gpu_pae_head.py) plus what uv's error can move them: |d logit| <= 2 max|d uv| sum_h |w2[k,h]|, d(ce) <= 2 max|d logit|,
d(pae) <= (nbins / bins_per_angstrom) max|d logit|, d(ptm) <= 2 max|d logit|."""
import contextlib
import io
import json
import math

import numpy as np
import pytest
import torch

import pae_head_ref as R
from test_gpu_pae_head import BARS as KERNEL_BARS
from test_gpu_predict import make_model, settings

pytestmark = pytest.mark.gpu

BARS = {"uv": 8 * 1.139e-7, "grad": 8 * 1.274e-7}        # 8 x measured on the MI355X (profiles/pae_head/NOTES.md)
WORST = {k: 0.0 for k in BARS}
SPEC = "2,24,2"                                       # --synthetic: 2 proteins of 24 residues per batch, 2 training batches
MAX_LEN = 48


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert BARS["uv"] <= 1e-5 and BARS["grad"] <= 1e-3
    yield torch.device("cuda:0")
    print(f"\n[pae fit] uv max|got - ref| / max(1, max|ref|): {WORST['uv']:.3e} (bar {BARS['uv']:.1e}); "
          f"gradient rel-L2: {WORST['grad']:.3e} (bar {BARS['grad']:.1e})")


@pytest.fixture(scope="module")
def world(dev, tmp_path_factory):
    """A one-layer model, its checkpoint, and one fixed batch B = 2, L = 20 with ragged lengths and absent truth residues."""
    import types
    from protein_transformer_amd import synthetic, train as TR
    from protein_transformer_amd.optim import FusedSGD
    from protein_transformer_amd.protein.Structure import nerf_forward
    tmp = tmp_path_factory.mktemp("pae_fit")
    args = settings(tmp, n_layers=1, n_head=2, d_model=32, d_inner_hid=64, max_seq_len=MAX_LEN)
    model = make_model(args, dev)
    metrics = {"loss_to_compare": 1.0, "losses_to_compare": [1.0], "last_chkpt_time": 0.0}
    assert TR.checkpoint_model(args, FusedSGD(model, lr=1e-2), model, metrics, 0, None)
    build = lambda ang, seq: nerf_forward(ang.to(dev), seq.to(dev))[0]                      # noqa: E731
    batch = synthetic.make_batch([20, 13], L_pad=20, seed=8, build_coords=build, frac_missing=0.1)
    return types.SimpleNamespace(tmp=tmp, args=args, model=model, ckpt=args.chkpt_path + "_best.chkpt", seq=batch["seq"].to(dev),
                                 crd=batch["true_crd"].to(dev))


def run(main, argv):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = main(argv)
    return rc, out.getvalue()


def test_forward_and_backward_against_fp64(world, dev):
    from protein_transformer_amd import confidence as CF
    x, seq, target = CF.hidden_and_aligned_error(world.model, world.seq, world.crd)
    assert x.shape == (40, 32) and target.shape == (2, 20, 20)
    t_host, s_host = target.cpu().numpy(), seq.cpu().numpy()
    assert 0 < np.isfinite(t_host).sum() < R.present(s_host).sum() ** 2 and np.isnan(t_host[1, 13:]).all()
    head = CF.PaeHead(32, device=dev, seed=1)
    g = torch.Generator().manual_seed(2)
    for name in ("w2", "b2", "ln.beta", "b1"):                                               # a head in the middle of a fit
        head.params[name].copy_(torch.randn(head.params[name].shape, generator=g).to(dev) * 0.3)
    pae, stats, sums = (t.cpu().numpy() for t in head.forward(x, seq, target))
    uv = head._saved[4].cpu().numpy()
    head.backward()
    P = {n: v.detach().cpu().numpy().astype(np.float64) for n, v in head.params.items()}
    ref = R.head_forward(P, x.cpu().numpy(), s_host, t_host, 2.0)
    e_uv = float(np.abs(uv - ref["uv"]).max() / max(1.0, np.abs(ref["uv"]).max()))
    slack = 2 * 2 * np.abs(uv - ref["uv"]).max() * np.abs(P["w2"]).sum(axis=1).max()          # 2 max |d logit|
    d = ref["defined"]
    assert np.isnan(pae[~d]).all()
    assert np.abs(pae[d] - ref["pae"][d]).max() <= KERNEL_BARS["pae"] * 32.0 + 16.0 * slack
    assert np.abs(stats - ref["stats"]).max() <= KERNEL_BARS["stats"] * 32.0 + 16.0 * slack
    assert sums[1] == ref["counted"].sum() and abs(sums[0] - ref["sums"][0]) <= KERNEL_BARS["sums0"] * ref["sums"][0] + slack
    want = R.head_grads(P, x.cpu().numpy(), s_host, t_host, 2.0)
    e_grad = 0.0                                                                              # the largest rel-L2 of the six
    for name in R.NAMES:
        got = head.grads[name].cpu().numpy().astype(np.float64)
        assert np.abs(want[name]).max() > 0, name
        e_grad = max(e_grad, math.sqrt(float(((got - want[name]) ** 2).sum()) / float((want[name] ** 2).sum())))
    WORST["uv"], WORST["grad"] = max(WORST["uv"], e_uv), max(WORST["grad"], e_grad)
    assert e_uv <= BARS["uv"] and e_grad <= BARS["grad"], (e_uv, e_grad)


def test_fit_starts_at_ln_nbins_learns_and_is_deterministic(world, dev):
    from protein_transformer_amd import confidence as CF
    batches = [(world.seq, None, world.crd)]
    state0 = {k: v.clone() for k, v in world.model.state_dict().items()}
    head, hist = CF.fit_pae_head(world.model, batches, epochs=30, lr=3e-3, seed=0)
    assert head.steps == 30 and len(hist) == 30
    assert hist[0]["ce"] == pytest.approx(math.log(64), rel=8 * 2.0 ** -23)                    # fp32: the first step's CE
    assert hist[-1]["ce"] < hist[0]["ce"] and all(h["pairs"] == hist[0]["pairs"] > 0 for h in hist)
    again, hist2 = CF.fit_pae_head(world.model, batches, epochs=30, lr=3e-3, seed=0)
    assert hist == hist2 and torch.equal(head.flat, again.flat)
    assert all(torch.equal(v, state0[k]) for k, v in world.model.state_dict().items())         # the encoder stays frozen


@pytest.fixture(scope="module")
def fitted(world):
    """`confidence fit` then `confidence fit-pae` on the world's checkpoint, and a FASTA file of two sequences."""
    from protein_transformer_amd import confidence as CF
    import ensemble_ref as er
    ckpt1, ckpt2 = str(world.tmp / "with_plddt.chkpt"), str(world.tmp / "with_both.chkpt")
    rc, _ = run(CF.main, ["fit", world.ckpt, "--synthetic", SPEC, "--out", ckpt1, "--batch_size", "2"])
    assert rc == 0
    rc, out = run(CF.main, ["fit-pae", ckpt1, "--synthetic", SPEC, "--out", ckpt2, "--epochs", "2", "--batch_size", "2", "--lr", "3e-3"])
    assert rc == 0
    lines = [json.loads(l) for l in out.strip().split("\n")]
    assert [l["steps"] for l in lines] == [2, 4] and all(set(l) == {"epoch", "ce", "pairs", "steps"} and l["pairs"] > 0 for l in lines)
    rng = np.random.default_rng(6)
    seqs = ["".join(er.AA[i] for i in rng.integers(0, 20, n)) for n in (30, 7)]
    fasta = world.tmp / "two.fasta"
    fasta.write_text("".join(f">{n}\n{s}\n" for n, s in zip(("mid", "short"), seqs)))
    return ckpt1, ckpt2, str(fasta), ("mid", "short"), seqs


def test_fit_pae_then_predict_ptm(world, fitted):
    from protein_transformer_amd import predict
    ckpt1, ckpt2, fasta, names, seqs = fitted
    a = torch.load(ckpt1, map_location="cpu", weights_only=False)
    b = torch.load(ckpt2, map_location="cpu", weights_only=False)
    assert set(b) == set(a) | {"pae_head"} and "confidence_head" in b                          # the other head survives
    assert all(torch.equal(v, b["confidence_head"]["state_dict"][k]) for k, v in a["confidence_head"]["state_dict"].items())
    assert b["pae_head"]["settings"] == {"d_in": 32, "hidden": 32, "nbins": 64, "bins_per_angstrom": 2.0, "steps": 4}
    out_dir = world.tmp / "p"
    rc, out = run(predict.main, [ckpt2, fasta, "--out", str(out_dir), "--samples", "0", "--ptm", "--plddt"])
    assert rc == 0
    lines = [json.loads(l) for l in out.strip().split("\n")]
    assert all(tuple(l) == predict.KEYS + predict.PLDDT_KEYS + predict.PTM_KEYS for l in lines)
    for name, s, line in zip(names, seqs, lines):
        n = len(s)
        assert (out_dir / f"{name}.pdb").exists() and not (out_dir / f"{name}.pae.json").exists()
        doc = json.load(open(out_dir / f"{name}.head_pae.json"))
        m = np.array(doc[0]["predicted_aligned_error"], np.float64)
        assert m.shape == (n, n) and np.isfinite(m).all() and m.min() >= 0 and m.max() <= 32.0
        assert doc[0]["max_predicted_aligned_error"] == m.max()
        assert 0 < line["ptm"] <= 1 and line["pae"] == pytest.approx(m.mean(), abs=0.01)


def test_predict_ptm_refuses_a_checkpoint_without_the_head(world, fitted, capsys):
    from protein_transformer_amd import predict
    rc, out = run(predict.main, [fitted[0], fitted[2], "--out", str(world.tmp / "never"), "--samples", "0", "--ptm"])
    err = capsys.readouterr().err
    assert rc == 2 and out == "" and "fit-pae" in err and not (world.tmp / "never").exists()


def test_calibrate_pae_counts_every_finite_true_entry(world, fitted, dev):
    from protein_transformer_amd import confidence as CF, predict
    from protein_transformer_amd.synthetic_data import make_synthetic_dataset
    ckpt2 = fitted[1]
    rc, plain = run(CF.main, ["calibrate", ckpt2, "--synthetic", SPEC, "--samples", "2", "--batch_size", "2"])
    rc2, out = run(CF.main, ["calibrate", ckpt2, "--synthetic", SPEC, "--samples", "2", "--batch_size", "2", "--pae"])
    assert rc == rc2 == 0 and out.count("\n") == 1
    report, before = json.loads(out), json.loads(plain)
    assert set(before) == {"plddt", "ens-lddt"} and set(report) == set(before) | {"pae", "ptm", "ens-pae", "ens-ptm"}
    assert all(report[k] == before[k] for k in before)                                        # today's keys are unchanged
    model = predict.load_checkpoint(ckpt2, dev)
    data = make_synthetic_dataset(SPEC, 0, dev)
    n = prots = 0
    for batch in CF.data_batches(data, "test", 2, MAX_LEN):
        _, _, target = CF.hidden_and_aligned_error(model, batch[0].to(dev), batch[-1].to(dev))
        n += int(torch.isfinite(target).sum())
        prots += batch[0].shape[0]
    assert n > 0
    for k in ("pae", "ens-pae"):
        assert report[k]["n"] == n and sum(r["n"] for r in report[k]["reliability"]) == n
        assert report[k]["reliability"][9]["hi"] == pytest.approx(32.0)
    for k in ("ptm", "ens-ptm"):
        assert report[k]["n"] == prots and report[k]["reliability"][9]["hi"] == 100
