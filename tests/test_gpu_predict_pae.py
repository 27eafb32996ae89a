"""MI355X tests of `python -m protein_transformer_amd.predict --pae` and `ensemble.predict_ensemble(..., aligned_error=True)` on the
smallest model the encoder accepts (2 layers, 4 heads, d_model 64, d_ff 128) and three sequences of 64, 5 and 70 residues: the
aligned-error files, the two further keys of the JSON line, that the run is deterministic, and that nothing changes without the
option."""
import contextlib
import io
import json
import os
import types

import numpy as np
import pytest
import torch

import aligned_error_ref as ar
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


def make_checkpoint(tmp, dev, seed=3, **kw):
    from protein_transformer_amd import synthetic, train as TR
    from protein_transformer_amd.optim import FusedSGD
    args = settings(tmp, **kw)
    rng = np.random.default_rng(seed)
    ang = torch.from_numpy(np.stack([synthetic.sample_angles(rng, 40)]))
    am = synthetic.angle_means(torch.stack([torch.cos(ang), torch.sin(ang)], -1).reshape(1, 40, 24))
    torch.manual_seed(seed)
    model = TR.make_model(args, dev, am)
    with torch.no_grad():
        model.output_projection.weight.normal_(0, 0.05)
    model = model.to(dev)
    metrics = {"loss_to_compare": 1.0, "losses_to_compare": [1.0], "last_chkpt_time": 0.0}
    assert TR.checkpoint_model(args, FusedSGD(model, lr=1e-2), model, metrics, 0, None)
    return args.chkpt_path + "_best.chkpt"


def run(argv):
    from protein_transformer_amd import predict
    out, err = io.StringIO(), io.StringIO()
    with contextlib.redirect_stdout(out), contextlib.redirect_stderr(err):
        rc = predict.main(argv)
    return rc, out.getvalue(), err.getvalue()


@pytest.fixture(scope="module")
def world(dev, tmp_path_factory):
    """A checkpoint, a FASTA file of three sequences, and one run of the command with 4 samples and --pae."""
    tmp = tmp_path_factory.mktemp("pae")
    rng = np.random.default_rng(5)
    seqs = ["".join(er.AA[i] for i in rng.integers(0, 20, n)) for n in LENGTHS]
    fasta = tmp / "seqs.fasta"
    fasta.write_text("".join(f">{n}\n{s}\n" for n, s in zip(NAMES, seqs)))
    w = types.SimpleNamespace(tmp=tmp, ckpt=make_checkpoint(tmp, dev), fasta=str(fasta), seqs=seqs)
    w.argv = lambda out, *more: [w.ckpt, w.fasta, "--out", str(tmp / out), *more]
    w.rc, w.stdout, _ = run(w.argv("a", "--samples", "4", "--pae"))
    return w


def batch_of(seqs, dev):
    """The one batch the command makes of these sequences (sorted by length, padded to the longest)."""
    from protein_transformer_amd.protein.Sequence import AA_MAP
    order = sorted(range(len(seqs)), key=lambda i: len(seqs[i]))
    ids = np.full((len(seqs), max(map(len, seqs))), 20, np.int64)
    for row, i in enumerate(order):
        ids[row, :len(seqs[i])] = [AA_MAP[c] for c in seqs[i]]
    return order, torch.from_numpy(ids).to(dev)


def test_pae_files_and_json_lines(world, dev):
    from protein_transformer_amd import predict
    from protein_transformer_amd.ensemble import predict_ensemble
    assert world.rc == 0
    model = predict.load_checkpoint(world.ckpt, dev)
    order, seq = batch_of(world.seqs, dev)
    ens = predict_ensemble(model, seq, samples=4, seed=0, aligned_error=True)
    assert ens.ae.shape == (3, 70, 70) and ens.ae_stats.shape == (3, 2)
    ae, stats = ens.ae.cpu().numpy().astype(np.float64), ens.ae_stats.cpu().numpy().astype(np.float64)
    lines = [json.loads(l) for l in world.stdout.strip().split("\n")]
    assert [l["id"] for l in lines] == list(NAMES)
    assert all(tuple(l) == predict.KEYS + predict.PAE_KEYS for l in lines)
    assert predict.PAE_KEYS == ("ens-pae", "ens-ptm")
    for row, i in enumerate(order):
        name, n = NAMES[i], len(world.seqs[i])
        text = open(world.tmp / "a" / f"{name}.pae.json").read()
        assert "NaN" not in text and "Infinity" not in text
        doc = json.loads(text)
        assert isinstance(doc, list) and len(doc) == 1
        assert set(doc[0]) == {"predicted_aligned_error", "max_predicted_aligned_error"}
        m = doc[0]["predicted_aligned_error"]
        assert len(m) == n and all(len(r) == n for r in m)
        got = np.array(m, np.float64)
        want = ae[row, :n, :n]
        assert np.isfinite(want).all()
        assert np.abs(got - want).max() <= 0.005 + 1e-9              # half a unit of the second decimal
        assert doc[0]["max_predicted_aligned_error"] == got.max()
        assert (np.diagonal(got) == 0.0).all() and got.max() > 0.0   # dropout moved something
        assert lines[i]["ens-pae"] == pytest.approx(stats[row, 0], rel=1e-6)
        assert lines[i]["ens-ptm"] == pytest.approx(stats[row, 1], rel=1e-6)
        assert 0.0 < lines[i]["ens-ptm"] <= 1.0
        assert np.isnan(ae[row, n:]).all() and np.isnan(ae[row, :, n:]).all()
    # the matrix is that of the definition, on the samples the ensemble kernel saw
    none = predict_ensemble(model, seq, samples=4, seed=0, aligned_error=False)
    assert none.ae is None and none.ae_stats is None
    for a, b in zip(none[:6], ens[:6]):
        assert torch.equal(a, b) or (torch.isnan(a) == torch.isnan(b)).all() and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b))
    zero = predict_ensemble(model, seq, samples=0)
    assert zero.rmsd is None and zero.ae is None and zero.ae_stats is None and zero.crd is not None


def test_the_same_command_twice_gives_the_same_bytes(world):
    rc, out, _ = run(world.argv("b", "--samples", "4", "--pae"))
    assert rc == 0 and out == world.stdout
    for name in NAMES:
        for ext in (".pae.json", ".pdb"):
            assert open(world.tmp / "a" / (name + ext), "rb").read() == open(world.tmp / "b" / (name + ext), "rb").read()


def test_without_the_option_nothing_changes(world):
    from protein_transformer_amd import predict
    rc, out, _ = run(world.argv("c", "--samples", "4"))
    assert rc == 0
    assert sorted(os.listdir(world.tmp / "c")) == sorted(n + ".pdb" for n in NAMES)      # no .pae.json
    lines = [json.loads(l) for l in out.strip().split("\n")]
    assert all(tuple(l) == predict.KEYS for l in lines)
    with_pae = [json.loads(l) for l in world.stdout.strip().split("\n")]
    assert [{k: l[k] for k in predict.KEYS} for l in with_pae] == lines                 # the existing keys: the same values
    for name in NAMES:
        assert open(world.tmp / "a" / (name + ".pdb"), "rb").read() == open(world.tmp / "c" / (name + ".pdb"), "rb").read()


def test_without_dropout_the_matrix_is_zero_within_tol(world, dev):
    """Dropout 0 EVERYWHERE: the attention dropout is hard-wired to 0.1 whatever the checkpoint's settings say (as in the
    reference), so the model is loaded and `set_dropout(0)` switches both off; the rest is the command's own path."""
    from protein_transformer_amd import predict
    model = predict.load_checkpoint(world.ckpt, dev)
    model.set_dropout(0.0)
    records = list(zip(NAMES, world.seqs))
    results = predict.predict_records(model, records, samples=4, seed=0, pae=True)
    for (name, s), r in zip(records, results):
        x = float(np.abs(r["crd"]).max())
        line = predict.pae_summary(r)
        print(f"{name}: extent {x:.1f} A, largest entry {r['ae'].max():.3g}, tol {ar.tol(x, 4):.3g}, ens-ptm {line['ens-ptm']}")
        assert r["usable"] == 4 and np.isfinite(r["ae"]).all() and r["ae"].max() <= ar.tol(x, 4)
        assert abs(line["ens-ptm"] - 1.0) <= ar.tol_tm(x, len(s), 4) and line["ens-pae"] <= ar.tol(x, 4)


def test_pae_needs_samples(world):
    rc, out, err = run(world.argv("never", "--samples", "0", "--pae"))
    assert rc == 2 and out == ""
    assert err.startswith("predict: ") and err.count("\n") == 1 and "--pae" in err
    assert not (world.tmp / "never").exists()
