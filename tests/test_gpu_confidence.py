"""MI355X tests of the confidence head (protein_transformer_amd/confidence.py) on the smallest model the encoder accepts (2 layers,
4 heads, d_model 64, d_ff 128 - tests/test_gpu_predict.py), B = 4, L <= 32, ragged lengths, a tenth of the truth residues absent:
one forward and backward of the head against its fp64 restatement (tests/plddt_ref.py) on the same hidden state, the unfitted
head, the fit (it learns, it is deterministic, it leaves the encoder alone), the hidden-state tap, that a prediction leaves a
training run where it found it, and the three commands end to end: `confidence fit` -> `predict --plddt` -> `confidence calibrate`.

BARS of the head: logits, max |got - ref| / max(1, max |ref|) - absolute on values of order one, the form of the project's 1e-5 parity
bar and never above it; the whole gradient by rel-L2, never above the project's 1e-3 gradient bar (README.md);
both 8 x the value measured on the MI355X (profiles/plddt/NOTES.md).  pLDDT, CE and their mean are held to the kernel's own bars
(tests/test_gpu_plddt.py) plus what the logits' error can move them: d(ce) <= 2 max|d logit|, d(plddt) <= 100 max|d logit|."""
import contextlib
import csv
import io
import json
import math

import numpy as np
import pytest
import torch

import plddt_ref as R
from test_gpu_plddt import BARS as KERNEL_BARS
from test_gpu_predict import MAX_LEN, atoms_of, make_model, settings

pytestmark = pytest.mark.gpu

LENS = (32, 21, 9, 27)
BARS = {"logits": 8 * 3.234e-7, "grad": 8 * 1.795e-7}   # 8 x measured on the MI355X (profiles/plddt/NOTES.md)
WORST = {k: 0.0 for k in BARS}
SPEC = "4,32,2"                                       # --synthetic: 4 proteins of 32 residues per batch, 2 training batches


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert BARS["logits"] <= 1e-5 and BARS["grad"] <= 1e-3
    yield torch.device("cuda:0")
    print(f"\n[confidence] logits max|got - ref| / max(1, max|ref|): {WORST['logits']:.3e} (bar {BARS['logits']:.1e}); "
          f"gradient rel-L2: {WORST['grad']:.3e} (bar {BARS['grad']:.1e})")


@pytest.fixture(scope="module")
def world(dev, tmp_path_factory):
    """A model, its checkpoint, and one fixed batch with ragged lengths and absent truth residues."""
    import types
    from protein_transformer_amd import synthetic, train as TR
    from protein_transformer_amd.optim import FusedSGD
    from protein_transformer_amd.protein.Structure import nerf_forward
    tmp = tmp_path_factory.mktemp("confidence")
    args = settings(tmp)
    model = make_model(args, dev)
    metrics = {"loss_to_compare": 1.0, "losses_to_compare": [1.0], "last_chkpt_time": 0.0}
    assert TR.checkpoint_model(args, FusedSGD(model, lr=1e-2), model, metrics, 0, None)
    build = lambda ang, seq: nerf_forward(ang.to(dev), seq.to(dev))[0]                      # noqa: E731
    batch = synthetic.make_batch(list(LENS), L_pad=32, seed=8, build_coords=build, frac_missing=0.1)
    w = types.SimpleNamespace(tmp=tmp, args=args, model=model, ckpt=args.chkpt_path + "_best.chkpt",
                              seq=batch["seq"].to(dev), crd=batch["true_crd"].to(dev), raw=batch)
    return w


def run(main, argv):
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = main(argv)
    return rc, out.getvalue()


def host_params(head):
    return {n: v.detach().cpu().numpy().astype(np.float64) for n, v in head.params.items()}


# ------------------------------------------------------------------------------------------------ the head against fp64
def test_forward_and_backward_against_fp64(world, dev):
    from protein_transformer_amd import confidence as CF
    x, target = CF.hidden_and_target(world.model, world.seq, world.crd)
    T = x.shape[0]
    assert x.shape == (4 * 32, 64) and target.numel() == 2 * T - 1
    t_host = target.cpu().numpy()[::2].copy()
    seq = world.seq.cpu().numpy().reshape(-1)
    assert np.isnan(t_host[seq == 20]).all() and 0 < np.isfinite(t_host).sum() < (seq != 20).sum()   # padding and absent residues
    head = CF.ConfidenceHead(64, device=dev, seed=1)
    g = torch.Generator().manual_seed(2)
    for name in ("w2", "b2", "ln.beta", "b1"):                                               # a head in the middle of a fit
        head.params[name].copy_(torch.randn(head.params[name].shape, generator=g).to(dev) * 0.3)
    plddt, ce, sums = head.forward(x, target, 2)
    grad = head.backward().clone()
    P, xh = host_params(head), x.cpu().numpy()
    ref = R.head_logits(P, xh)["logits"]
    logits = head.logits.cpu().numpy()
    assert logits.shape == (T, 52) and (logits[:, 50:] == 0).all()                           # the spare rows of w2 / b2 are zero
    e_logits = float(np.abs(logits[:, :50] - ref).max() / max(1.0, np.abs(ref).max()))
    loss = R.bin_loss(ref, t_host)
    counted = loss["counted"]
    slack = 2 * np.abs(logits[:, :50] - ref).max()
    got_ce = ce.cpu().numpy()
    assert np.isnan(got_ce[~counted]).all()
    assert np.abs(got_ce[counted] - loss["ce"][counted]).max() <= KERNEL_BARS["ce"] * loss["ce"][counted].max() + slack
    assert np.abs(plddt.cpu().numpy() - loss["plddt"]).max() <= KERNEL_BARS["plddt"] * 100 + 50 * slack
    s = sums.cpu().numpy()
    assert s[1] == counted.sum() and abs(s[0] - loss["sums"][0]) <= KERNEL_BARS["sums0"] * loss["sums"][0] + slack
    want = R.head_grads(P, xh, t_host)
    num = den = 0.0
    for name in R.NAMES:
        got = head.grads[name].cpu().numpy().astype(np.float64)
        num += float(((got - want[name]) ** 2).sum())
        den += float((want[name] ** 2).sum())
        assert np.abs(want[name]).max() > 0, name
    e_grad = math.sqrt(num / den)
    # the spare rows of w2 / b2 got an exactly zero gradient
    o, shape = head._layout["w2"]
    assert (grad[o + 50 * 128:o + 52 * 128] == 0).all() and (grad[head._layout["b2"][0] + 50:] == 0).all()
    WORST["logits"], WORST["grad"] = max(WORST["logits"], e_logits), max(WORST["grad"], e_grad)
    assert e_logits <= BARS["logits"] and e_grad <= BARS["grad"], (e_logits, e_grad)


def test_unfitted_head_is_uniform(world, dev):
    from protein_transformer_amd import confidence as CF
    x, target = CF.hidden_and_target(world.model, world.seq, world.crd)
    head = CF.ConfidenceHead(64, device=dev, seed=3)
    plddt, ce, sums = (t.cpu().numpy().astype(np.float64) for t in head.forward(x, target, 2))
    counted = np.isfinite(target.cpu().numpy()[::2])
    assert np.abs(plddt - 50.0).max() <= KERNEL_BARS["plddt"] * 50.0
    assert np.abs(ce[counted] - math.log(50)).max() <= KERNEL_BARS["ce"] * math.log(50) and np.isnan(ce[~counted]).all()
    assert abs(sums[0] - math.log(50)) <= KERNEL_BARS["sums0"] * math.log(50) and sums[1] == counted.sum()
    p = CF.predict_plddt(world.model, head, world.seq).cpu().numpy()
    pad = world.seq.cpu().numpy() == 20
    assert p.shape == (4, 32) and np.isnan(p[pad]).all() and np.abs(p[~pad] - 50.0).max() <= KERNEL_BARS["plddt"] * 50.0


# ------------------------------------------------------------------------------------------------ the fit
def test_fit_learns_is_deterministic_and_leaves_the_encoder_alone(world, dev):
    from protein_transformer_amd import confidence as CF
    m = world.model
    flat0 = m.flat_parameters()[0].clone()
    state0 = {k: v.clone() for k, v in m.state_dict().items()}
    was = (m.training, m.keep_hidden, m.dropout_seed, m._step_counter)
    batches = [(world.seq, None, world.crd)]
    head, hist = CF.fit_head(m, batches, epochs=200, lr=1e-3, seed=0)
    assert head.steps == 200 and len(hist) == 200 and hist[0]["ce"] == pytest.approx(math.log(50), rel=1e-5)
    assert hist[-1]["ce"] < hist[0]["ce"] and all(h["residues"] == hist[0]["residues"] > 0 for h in hist)
    a, _ = CF.fit_head(m, batches, epochs=5, lr=1e-3, seed=0)
    b, _ = CF.fit_head(m, batches, epochs=5, lr=1e-3, seed=0)
    assert torch.equal(a.flat, b.flat) and torch.equal(a._m, b._m) and torch.equal(a._v, b._v)
    assert not torch.equal(a.flat, CF.fit_head(m, batches, epochs=5, lr=1e-3, seed=1)[0].flat)
    assert torch.equal(m.flat_parameters()[0], flat0)
    assert all(torch.equal(v, state0[k]) for k, v in m.state_dict().items()) and list(m.state_dict()) == list(state0)
    assert (m.training, m.keep_hidden, m.dropout_seed, m._step_counter) == was and not hasattr(m, "last_hidden")
    o = a._layout["w2"][0]
    assert (a.flat[o + 50 * 128:o + 52 * 128] == 0).all() and (a.flat[a._layout["b2"][0] + 50:] == 0).all()   # the spare rows stay 0


def test_hidden_state_tap(world, dev):
    from protein_transformer_amd import confidence as CF
    m = make_model(world.args, dev).eval()
    assert m.keep_hidden is False
    with torch.no_grad():
        pred = m(world.seq)
        assert not hasattr(m, "last_hidden")
        m.keep_hidden = True
        again = m(world.seq)
        assert m.last_hidden.shape == (4 * 32, 64) and torch.equal(pred, again)
        del m.last_hidden
        m.keep_hidden = False
    pred2, x, _ = CF.hidden_state(m, world.seq)
    assert torch.equal(pred2, pred) and not hasattr(m, "last_hidden") and m.keep_hidden is False and m.training is False


def test_prediction_leaves_a_training_run_where_it_found_it(world, dev):
    """Three training steps, with and without a `predict_plddt` call after the first: the losses and the parameters after step
    three are bit-identical (the pattern of tests/test_gpu_predict.py for the ensemble)."""
    from protein_transformer_amd import confidence as CF, synthetic
    from protein_transformer_amd.optim import FusedSGD
    from protein_transformer_amd.protein.Structure import nerf_forward
    from protein_transformer_amd.train import train_step
    build = lambda ang, seq: nerf_forward(ang.to(dev), seq.to(dev))[0]                      # noqa: E731
    batch = synthetic.make_batch([48, 31, 17, 40], L_pad=48, seed=5, build_coords=build, frac_missing=0.05)
    data = tuple(batch[k].to(dev) for k in ("seq", "true_ang", "true_crd"))
    head = CF.ConfidenceHead(64, device=dev, seed=0)

    def trajectory(call):
        m = make_model(world.args, dev, seed=9).train()
        m.dropout_seed = 12345
        opt = FusedSGD(m, lr=1e-2, weight_decay=10e-3)
        losses = [float(train_step(m, opt, world.args, *data)["loss"])]
        if call:
            before = (m.training, m.keep_hidden, m.dropout_seed, m._step_counter, m.auto_guard, m.auto_guard.passes,
                      m.auto_guard.eval_passes, m.auto_guard.train_steps, m.auto_guard._pending)
            p = CF.predict_plddt(m, head, world.seq)
            assert p.shape == (4, 32) and not hasattr(m, "last_hidden")
            after = (m.training, m.keep_hidden, m.dropout_seed, m._step_counter, m.auto_guard, m.auto_guard.passes,
                     m.auto_guard.eval_passes, m.auto_guard.train_steps, m.auto_guard._pending)
            assert all(a is b or a == b for a, b in zip(before, after)) and before[0] is True
        losses += [float(train_step(m, opt, world.args, *data)["loss"]) for _ in range(2)]
        return losses, m.flat_parameters()[0].clone()

    plain, with_call = trajectory(False), trajectory(True)
    assert plain[0] == with_call[0] and torch.equal(plain[1], with_call[1])


# ------------------------------------------------------------------------------------------------ the commands, end to end
@pytest.fixture(scope="module")
def fitted(world):
    """`confidence fit` on the world's checkpoint, and a FASTA file of three sequences of different length."""
    from protein_transformer_amd import confidence as CF
    import ensemble_ref as er
    ckpt2 = str(world.tmp / "with_head.chkpt")
    rc, out = run(CF.main, ["fit", world.ckpt, "--synthetic", SPEC, "--out", ckpt2, "--epochs", "3", "--batch_size", "4", "--lr", "3e-3"])
    assert rc == 0
    lines = [json.loads(l) for l in out.strip().split("\n")]
    assert [l["epoch"] for l in lines] == [0, 1, 2] and [l["steps"] for l in lines] == [2, 4, 6]
    assert all(set(l) == {"epoch", "ce", "residues", "steps"} and l["residues"] > 0 for l in lines) and lines[-1]["ce"] < lines[0]["ce"]
    rng = np.random.default_rng(6)
    seqs = ["".join(er.AA[i] for i in rng.integers(0, 20, n)) for n in (30, 7, 19)]
    names = ("mid", "short", "other")
    fasta = world.tmp / "three.fasta"
    fasta.write_text("".join(f">{n}\n{s}\n" for n, s in zip(names, seqs)))
    return ckpt2, str(fasta), names, seqs


def test_fit_writes_the_head_beside_an_unchanged_checkpoint(world, fitted, dev):
    from protein_transformer_amd import confidence as CF, predict
    ckpt2 = fitted[0]
    a = torch.load(world.ckpt, map_location="cpu", weights_only=False)
    b = torch.load(ckpt2, map_location="cpu", weights_only=False)
    assert set(b) == set(a) | {"confidence_head"} and list(b["model_state_dict"]) == list(a["model_state_dict"])
    assert all(torch.equal(v, b["model_state_dict"][k]) for k, v in a["model_state_dict"].items())
    assert b["confidence_head"]["settings"] == {"d_in": 64, "hidden": 128, "nbins": 50, "lddt_cutoff": 15.0, "steps": 6}
    assert CF.load_head(world.ckpt, dev) is None and CF.load_head(ckpt2, dev).steps == 6
    m = predict.load_checkpoint(ckpt2, dev)                                               # a reader that does not know the key
    assert all(torch.equal(x, y) for x, y in zip(m.state_dict().values(), world.model.state_dict().values()))


def test_predict_plddt_end_to_end(world, fitted, dev):
    from protein_transformer_amd import confidence as CF, predict
    from protein_transformer_amd.protein.Sequence import AA_MAP
    ckpt2, fasta, names, seqs = fitted
    out_dir = world.tmp / "p"
    rc, out = run(predict.main, [ckpt2, fasta, "--out", str(out_dir), "--samples", "0", "--plddt", "--per_residue"])
    assert rc == 0
    lines = [json.loads(l) for l in out.strip().split("\n")]
    assert all(tuple(l) == predict.KEYS + predict.PLDDT_KEYS for l in lines) and [l["id"] for l in lines] == list(names)
    model, head = predict.load_checkpoint(ckpt2, dev), CF.load_head(ckpt2, dev)
    spread = 0.0
    for name, s, line in zip(names, seqs, lines):
        n = len(s)
        rows = list(csv.reader(open(out_dir / f"{name}.csv")))
        assert tuple(rows[0]) == predict.PER_RESIDUE_HEADER + ("plddt",) and len(rows) == n + 1
        col = np.array([float(r[-1]) for r in rows[1:]])
        assert np.isfinite(col).all() and (col > 0).all() and (col < 100).all()
        assert all(r[2:5] == ["nan", "nan", "nan"] for r in rows[1:])                         # no ensemble: --samples 0
        atoms = atoms_of(out_dir / f"{name}.pdb")
        b = np.array([float(l[60:66]) for l in atoms])
        res = np.array([int(l[22:26]) - 1 for l in atoms])
        assert np.abs(b - col[res]).max() <= 0.005 + 5e-5 + 1e-12                            # %6.2f of the value the CSV has to 4 decimals
        assert line["plddt"] == pytest.approx(col.mean(), abs=1e-4) and line["samples"] == 0 and line["ens-lddt"] is None
        # padding never leaks: the sequence alone, unpadded, gets the same pLDDT as in the batch of three lengths
        alone = torch.tensor([[AA_MAP[c] for c in s]], device=dev)
        p = CF.predict_plddt(model, head, alone).cpu().numpy()[0]
        assert np.abs(p - col).max() <= 5e-3, name
        spread = max(spread, float(np.ptp(col)))
    assert spread > 0                                                                     # the head does look at its input


def test_predict_without_the_flag_is_what_it_was(world, fitted):
    from protein_transformer_amd import predict
    ckpt2, fasta, names, _ = fitted
    rc_a, out_a = run(predict.main, [world.ckpt, fasta, "--out", str(world.tmp / "qa"), "--samples", "2", "--per_residue"])
    rc_b, out_b = run(predict.main, [ckpt2, fasta, "--out", str(world.tmp / "qb"), "--samples", "2", "--per_residue"])
    assert rc_a == rc_b == 0 and out_a == out_b and all(tuple(json.loads(l)) == predict.KEYS for l in out_a.strip().split("\n"))
    for name in names:
        for ext in ("pdb", "csv"):
            assert open(world.tmp / "qa" / f"{name}.{ext}", "rb").read() == open(world.tmp / "qb" / f"{name}.{ext}", "rb").read()
        assert open(world.tmp / "qa" / f"{name}.csv").readline().strip() == ",".join(predict.PER_RESIDUE_HEADER)


def test_predict_plddt_refuses_the_plain_checkpoint(world, fitted, capsys):
    from protein_transformer_amd import predict
    rc, out = run(predict.main, [world.ckpt, fitted[1], "--out", str(world.tmp / "never"), "--samples", "0", "--plddt"])
    err = capsys.readouterr().err
    assert rc == 2 and out == "" and err.count("\n") == 1 and "confidence head" in err and not (world.tmp / "never").exists()


def test_calibrate_counts_every_residue_with_a_target(world, fitted, dev):
    from protein_transformer_amd import confidence as CF, predict
    from protein_transformer_amd.synthetic_data import make_synthetic_dataset
    ckpt2 = fitted[0]
    rc, out = run(CF.main, ["calibrate", ckpt2, "--synthetic", SPEC, "--samples", "2", "--batch_size", "4"])
    assert rc == 0 and out.count("\n") == 1
    report = json.loads(out)
    assert set(report) == {"plddt", "ens-lddt"}
    model = predict.load_checkpoint(ckpt2, dev)
    data = make_synthetic_dataset(SPEC, 0, dev)
    n = 0
    for batch in CF.data_batches(data, "test", 4, MAX_LEN):
        _, target = CF.hidden_and_target(model, batch[0].to(dev), batch[-1].to(dev))
        n += int(torch.isfinite(target[::2]).sum())
    assert n > 0
    for score in report.values():
        assert score["n"] == n and sum(r["n"] for r in score["reliability"]) == n and len(score["reliability"]) == 10
        assert set(score) == {"n", "pearson", "mae", "bias", "reliability"} and score["mae"] >= abs(score["bias"])
