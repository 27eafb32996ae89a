"""MI355X tests of `python -m protein_transformer_amd.predict` and `ensemble.predict_ensemble` on the smallest model the encoder
accepts (2 layers, 4 heads, d_model 64, d_ff 128 - the sizes of tests/test_gpu_eval_ckpt.py): checkpoint -> FASTA -> PDB files with
the ensemble's confidence as temperature factors, the determinism of the run, and that a prediction leaves a training run where
it found it."""
import contextlib
import io
import json
import os
import types

import numpy as np
import pytest
import torch

import ensemble_ref as er

pytestmark = pytest.mark.gpu

MAX_LEN = 80
NAMES = ("mid", "short", "long")                                     # input order is not length order
LENGTHS = (64, 5, 70)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def settings(tmp, **kw):
    d = dict(model="enc-only", n_layers=2, n_head=4, d_model=64, d_inner_hid=128, max_seq_len=MAX_LEN, dropout=0.1,
             chkpt_path=str(tmp / "model"), checkpoint_time_interval=0, loss="drmsd", combined_drmsd_weight=0.5,
             backbone_loss=False, clip=1.0)
    d.update(kw)
    return types.SimpleNamespace(**d)


def make_model(args, dev, seed=3):
    from protein_transformer_amd import synthetic, train as TR
    rng = np.random.default_rng(seed)
    ang = torch.from_numpy(np.stack([synthetic.sample_angles(rng, 40)]))
    am = synthetic.angle_means(torch.stack([torch.cos(ang), torch.sin(ang)], -1).reshape(1, 40, 24))
    torch.manual_seed(seed)
    m = TR.make_model(args, dev, am)
    with torch.no_grad():
        m.output_projection.weight.normal_(0, 0.05)
    return m.to(dev)


def run(argv):
    from protein_transformer_amd import predict
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = predict.main(argv)
    return rc, out.getvalue()


def atoms_of(path):
    return [l for l in open(path).read().split("\n") if l.startswith("ATOM")]


@pytest.fixture(scope="module")
def world(dev, tmp_path_factory):
    """A checkpoint, a FASTA file of three sequences, and one run of the command with 4 samples."""
    from protein_transformer_amd import train as TR
    from protein_transformer_amd.optim import FusedSGD
    tmp = tmp_path_factory.mktemp("predict")
    args = settings(tmp)
    model = make_model(args, dev)
    metrics = {"loss_to_compare": 1.0, "losses_to_compare": [1.0], "last_chkpt_time": 0.0}
    assert TR.checkpoint_model(args, FusedSGD(model, lr=1e-2), model, metrics, 0, None)
    rng = np.random.default_rng(5)
    seqs = ["".join(er.AA[i] for i in rng.integers(0, 20, n)) for n in LENGTHS]
    fasta = tmp / "seqs.fasta"
    fasta.write_text("".join(f">{n} some words\n{s[:30].lower()}\n{s[30:]}*\n" for n, s in zip(NAMES, seqs)))
    w = types.SimpleNamespace(tmp=tmp, ckpt=args.chkpt_path + "_best.chkpt", fasta=str(fasta), seqs=seqs, model=model)
    w.argv = lambda out, *more: [w.ckpt, w.fasta, "--out", str(tmp / out), *more]
    w.rc, w.stdout = run(w.argv("a", "--samples", "4", "--per_residue"))
    return w


def batch_of(seqs, dev):
    """The one batch the command makes of these sequences (sorted by length, padded to the longest)."""
    from protein_transformer_amd.protein.Sequence import AA_MAP
    order = sorted(range(len(seqs)), key=lambda i: len(seqs[i]))
    ids = np.full((len(seqs), max(map(len, seqs))), 20, np.int64)
    for row, i in enumerate(order):
        ids[row, :len(seqs[i])] = [AA_MAP[c] for c in seqs[i]]
    return order, torch.from_numpy(ids).to(dev)


def test_structures_and_confidence(world, dev):
    from protein_transformer_amd import predict
    from protein_transformer_amd.ensemble import predict_ensemble
    from protein_transformer_amd.losses import predicted_coords
    from protein_transformer_amd.protein.Sequence import AA_MAP, ONE_TO_THREE_LETTER_MAP
    from protein_transformer_amd.score import read_pdb
    assert world.rc == 0
    model = predict.load_checkpoint(world.ckpt, dev)
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), world.model.state_dict().values()))
    order, seq = batch_of(world.seqs, dev)
    with torch.no_grad():
        crd = predicted_coords(model.eval()(seq), seq)[0].cpu().numpy()
    ens = predict_ensemble(model, seq, samples=4, seed=0)
    assert torch.equal(ens.crd.cpu(), torch.from_numpy(crd))
    conf = ens.conf.cpu().numpy()
    lines = [json.loads(l) for l in world.stdout.strip().split("\n")]
    assert [l["id"] for l in lines] == list(NAMES) and all(tuple(l) == predict.KEYS for l in lines)     # input order
    for row, i in enumerate(order):
        name, s = NAMES[i], world.seqs[i]
        n = len(s)
        ids, back = read_pdb(str(world.tmp / "a" / f"{name}.pdb"))
        assert list(ids) == [AA_MAP[c] for c in s]
        want = crd[row, :n * 14]
        has = er.atom_mask(np.array(ids)).reshape(-1)
        assert (np.isnan(back).any(1) == ~has).all()
        x = float(np.abs(want[has]).max())
        assert np.abs(back[has] - want[has]).max() <= 5e-4 + er.tol(0.0, x)                # the PDB's 0.001 A rounding
        text = [l[60:66] for l in atoms_of(world.tmp / "a" / f"{name}.pdb")]
        b = np.array([float(t) for t in text])
        res = np.array([int(l[22:26]) - 1 for l in atoms_of(world.tmp / "a" / f"{name}.pdb")])
        assert (b >= 0).all() and (b <= 100).all()
        written = np.nan_to_num(conf[row, res], nan=0.0).astype(np.float64)
        assert text == ["%6.2f" % v for v in written]                                      # columns 61-66, %6.2f
        # half a unit of the second decimal (+ the fp64 rounding of the subtraction: "33.65" is not a binary number)
        assert np.abs(b - written).max() <= 0.005 + 1e-12
        line = lines[i]
        assert line["n-res"] == n and line["samples"] == 4 and line["usable"] == 4
        assert line["ens-lddt"] == pytest.approx(float(np.nanmean(conf[row, :n])), rel=1e-5)
        assert line["ens-rmsd"] == pytest.approx(float(ens.rmsd[row].double().mean()), rel=1e-5) and line["ens-rmsd"] > 0
        assert line["ens-rmsf-ca"] == pytest.approx(float(ens.rmsf[row, :n, 0].double().mean()), rel=1e-5)
        rows = open(world.tmp / "a" / f"{name}.csv").read().strip().split("\n")
        assert rows[0] == "resnum,resname,conf,rmsf_ca,rmsf_all" and len(rows) == n + 1
        assert rows[1].split(",")[:2] == ["1", ONE_TO_THREE_LETTER_MAP[s[0]]]
        assert float(rows[n].split(",")[3]) == pytest.approx(float(ens.rmsf[row, n - 1, 0]), abs=1e-4)
    assert any(0 < v < 100 for v in np.nan_to_num(conf[2, :70]))                          # dropout moved something


def test_samples_zero_writes_the_structure_alone(world):
    rc, out = run(world.argv("zero", "--samples", "0"))
    assert rc == 0
    for name, line in zip(NAMES, out.strip().split("\n")):
        d = json.loads(line)
        assert d["id"] == name and d["samples"] == 0 and d["usable"] == 0
        assert d["ens-lddt"] is None and d["ens-rmsd"] is None and d["ens-rmsf-ca"] is None
        got, was = atoms_of(world.tmp / "zero" / f"{name}.pdb"), atoms_of(world.tmp / "a" / f"{name}.pdb")
        assert all(l[60:66] == "  0.00" for l in got)
        assert [l[:60] for l in got] == [l[:60] for l in was]                              # the same structure
        assert not os.path.exists(world.tmp / "zero" / f"{name}.csv")


def test_same_command_same_bytes_other_seed_other_confidence(world):
    rc, out = run(world.argv("b", "--samples", "4", "--per_residue"))
    assert rc == 0 and out == world.stdout
    for name in NAMES:
        for ext in ("pdb", "csv"):
            assert open(world.tmp / "b" / f"{name}.{ext}", "rb").read() == open(world.tmp / "a" / f"{name}.{ext}", "rb").read()
    rc, out = run(world.argv("c", "--samples", "4", "--seed", "1"))
    assert rc == 0 and out != world.stdout
    differ = 0
    for name in NAMES:
        got, was = atoms_of(world.tmp / "c" / f"{name}.pdb"), atoms_of(world.tmp / "a" / f"{name}.pdb")
        assert [l[:60] for l in got] == [l[:60] for l in was]                              # the coordinates do not move
        differ += sum(g[60:66] != w[60:66] for g, w in zip(got, was))
    assert differ > 0


def test_too_long_for_the_checkpoint_is_refused(world, capsys):
    fasta = world.tmp / "long.fasta"
    fasta.write_text(">fits\nMKV\n>giant\n" + "A" * (MAX_LEN + 1) + "\n")
    rc, out = run([world.ckpt, str(fasta), "--out", str(world.tmp / "never")])
    err = capsys.readouterr().err
    assert rc == 2 and out == "" and "giant" in err and str(MAX_LEN) in err and err.count("\n") == 1
    assert not os.path.exists(world.tmp / "never")


def test_calpha_lddt_reads_the_calphas_of_the_truth_only(dev):
    """What `predict_ensemble` relies on when it hands `lddt_batch` a truth with every slot but the C-alpha absent: the C-alpha
    column of the per-residue lDDT has the same bits as with the whole structure as the truth."""
    from protein_transformer_amd.eval_metrics import lddt_batch
    rng = np.random.default_rng(21)
    seq = rng.integers(0, 20, (3, 70))
    seq[1, 50:] = 20
    truth = np.stack([er.random_chain(rng, s) for s in seq])
    pred = (truth + rng.normal(0, 1.5, truth.shape)).astype(np.float32)
    only_ca = np.full((3, 70, 14, 3), np.nan, np.float32)
    only_ca[:, :, 1] = truth.reshape(3, 70, 14, 3)[:, :, 1]
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)                     # noqa: E731
    full = lddt_batch(d(pred), d(truth), d(seq))[1][:, :, 1].cpu().numpy()
    ca = lddt_batch(d(pred), d(only_ca.reshape(3, -1, 3)), d(seq))[1][:, :, 1].cpu().numpy()
    assert full.tobytes() == ca.tobytes() and np.isfinite(full[0]).all() and 0 < np.nanmean(full) < 1


def test_no_dropout_no_spread(world, dev):
    from protein_transformer_amd.ensemble import predict_ensemble
    model = make_model(settings(world.tmp), dev)
    model.set_dropout(0.0)
    _, seq = batch_of(world.seqs, dev)
    ens = predict_ensemble(model, seq, samples=3, seed=0)
    x = float(ens.crd.abs().max())
    assert list(ens.usable.cpu()) == [3, 3, 3]
    assert float(ens.rmsd.max()) <= er.tol(0.0, x)
    rmsf = ens.rmsf.cpu().numpy()
    assert np.nanmax(rmsf) <= er.tol(0.0, x) and np.isnan(rmsf[0, 5:]).all() and np.isfinite(rmsf[2]).all()
    conf = ens.conf.cpu().numpy()
    assert np.isfinite(conf).sum() >= 64 + 70 and (conf[np.isfinite(conf)] == 100.0).all()
    none = predict_ensemble(model, seq, samples=0)
    assert torch.equal(none.crd, ens.crd) and torch.equal(none.angles, ens.angles) and none.angles.shape == (3, 70, 12)
    assert none.rmsd is None and none.rmsf is None and none.conf is None and none.usable is None


@pytest.mark.parametrize("arith", ["default", "f16x2"])
def test_prediction_leaves_a_training_run_where_it_found_it(world, dev, arith):
    """Three training steps, with and without a `predict_ensemble` call after the first: the losses of steps two and three and
    the parameters after step three are bit-identical.  `f16x2`: the arithmetic whose scales the AutoGuard watches (the default
    picks bf16x3 at this size, where there is no guard to disturb)."""
    from protein_transformer_amd import kernels as K, synthetic
    from protein_transformer_amd.ensemble import predict_ensemble
    from protein_transformer_amd.optim import FusedSGD
    from protein_transformer_amd.protein.Structure import nerf_forward
    from protein_transformer_amd.train import train_step
    build = lambda ang, seq: nerf_forward(ang.to(dev), seq.to(dev))[0]                      # noqa: E731
    batch = synthetic.make_batch([48, 31, 17, 40], L_pad=48, seed=5, build_coords=build, frac_missing=0.05)
    data = tuple(batch[k].to(dev) for k in ("seq", "true_ang", "true_crd"))
    args = settings(world.tmp)
    _, other = batch_of(world.seqs, dev)

    def trajectory(predict_after_first):
        m = make_model(args, dev, seed=9).train()
        m.gemm_mode = K.GEMM_F16X2 if arith == "f16x2" else None
        m.dropout_seed = 12345
        opt = FusedSGD(m, lr=1e-2, weight_decay=10e-3)
        losses = [float(train_step(m, opt, args, *data)["loss"])]
        if predict_after_first:
            before = (m.training, m.dropout_seed, m._step_counter, m.auto_guard, m.auto_guard.passes, m.auto_guard.eval_passes,
                      m.auto_guard.train_steps, m.auto_guard._pending)
            ens = predict_ensemble(m, other, samples=3, seed=7)
            assert float(ens.rmsd.min()) > 0                                              # the passes did run with dropout
            after = (m.training, m.dropout_seed, m._step_counter, m.auto_guard, m.auto_guard.passes, m.auto_guard.eval_passes,
                     m.auto_guard.train_steps, m.auto_guard._pending)
            assert all(a is b or a == b for a, b in zip(before, after))
            assert before[0] is True and before[2] == 1
        losses += [float(train_step(m, opt, args, *data)["loss"]) for _ in range(2)]
        return losses, m.flat_parameters()[0].clone()

    plain, with_call = trajectory(False), trajectory(True)
    assert plain[0] == with_call[0]
    assert torch.equal(plain[1], with_call[1])
