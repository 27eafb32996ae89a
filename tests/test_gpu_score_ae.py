"""MI355X tests of `python -m protein_transformer_amd.score PRED.pdb TRUE.pdb --aligned_error OUT.json`: the true frame-aligned
error matrix of two small PDB files written with `PDB_Creator`, the truth lacking the side chain of one residue and the N of
another, against tests/aligned_error_ref.py on the coordinates as read back from the files."""
import contextlib
import io
import json

import numpy as np
import pytest
import torch

import aligned_error_ref as ar
import ensemble_ref as er

pytestmark = pytest.mark.gpu

N_RES = 24
NO_SIDE_CHAIN, NO_N = 3, 7                                            # residues (0-based) of the truth that lack atoms


def run(argv):
    from protein_transformer_amd import score
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        rc = score.main(argv)
    return rc, out.getvalue()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    from protein_transformer_amd.protein.PDB_Creator import PDB_Creator
    assert torch.cuda.is_available()
    tmp = tmp_path_factory.mktemp("score_ae")
    rng = np.random.default_rng(11)
    ids = rng.integers(0, 20, N_RES)
    ids[NO_SIDE_CHAIN] = er.AA.index("W")
    seq = "".join(er.AA[i] for i in ids)
    true = ar.random_chain(rng, ids).astype(np.float64)
    R, t = ar.random_rigid(rng)
    pred = true @ R.T + 0.1 * t + rng.normal(0, 1.0, true.shape)
    pred[~er.atom_mask(ids).reshape(-1)] = 0.0
    PDB_Creator(pred.astype(np.float32), seq=seq).save_pdb(str(tmp / "pred.pdb"), title="pred")
    PDB_Creator(true.astype(np.float32), seq=seq).save_pdb(str(tmp / "full.pdb"), title="true")
    kept = []
    for line in open(tmp / "full.pdb"):
        if line.startswith("ATOM"):
            res, name = int(line[22:26]) - 1, line[12:16].strip()
            if (res == NO_SIDE_CHAIN and name not in ("N", "CA", "C", "O")) or (res == NO_N and name == "N"):
                continue
        kept.append(line)
    (tmp / "true.pdb").write_text("".join(kept))
    return tmp


def test_aligned_error_file_and_keys(files):
    from protein_transformer_amd import score
    out_json = files / "ae.json"
    rc, out = run([str(files / "pred.pdb"), str(files / "true.pdb"), "--aligned_error", str(out_json)])
    assert rc == 0
    line = json.loads(out)
    assert tuple(line) == score.KEYS + score.AE_KEYS and score.AE_KEYS == ("ae-mean", "ae-tm")
    text = out_json.read_text()
    assert "NaN" not in text
    doc = json.loads(text)
    assert isinstance(doc, list) and len(doc) == 1 and set(doc[0]) == {"predicted_aligned_error", "max_predicted_aligned_error"}
    m = doc[0]["predicted_aligned_error"]
    assert len(m) == N_RES and all(len(r) == N_RES for r in m)
    null = np.array([[v is None for v in r] for r in m])
    want_null = np.zeros((N_RES, N_RES), bool)
    want_null[NO_N, :] = True                                        # no N: no frame - its row, not its column
    assert (null == want_null).all()                                 # (a residue without a side chain keeps both)
    # the values, on the coordinates as the files give them
    pseq, pcrd = score.read_pdb(str(files / "pred.pdb"))
    tseq, tcrd = score.read_pdb(str(files / "true.pdb"))
    ae, stats, usable = ar.reference(tcrd[None], pcrd[None, None], tseq[None])
    assert usable[0] == 1 and (np.isnan(ae[0]) == want_null).all()
    x = ar.extent_of(pcrd, tcrd)
    got = np.array([[np.nan if v is None else v for v in r] for r in m])
    assert np.nanmax(np.abs(got - ae[0])) <= 0.005 + ar.tol(x, 1)
    assert doc[0]["max_predicted_aligned_error"] == np.nanmax(got)
    n = N_RES
    assert abs(line["ae-mean"] - stats[0, 0]) <= ar.tol(x, 1) and abs(line["ae-tm"] - stats[0, 1]) <= ar.tol_tm(x, n, 1)
    assert 0.0 < line["ae-tm"] < 1.0 and line["ae-mean"] > 0.1


def test_a_truth_without_a_c_alpha_loses_row_and_column(files):
    from protein_transformer_amd import score
    lines = [l for l in open(files / "true.pdb") if not (l.startswith("ATOM") and int(l[22:26]) - 1 == 5 and l[12:16].strip() == "CA")]
    (files / "noca.pdb").write_text("".join(lines))
    rc, _ = run([str(files / "pred.pdb"), str(files / "noca.pdb"), "--aligned_error", str(files / "noca.json")])
    assert rc == 0
    m = json.loads((files / "noca.json").read_text())[0]["predicted_aligned_error"]
    null = np.array([[v is None for v in r] for r in m])
    want = np.zeros((N_RES, N_RES), bool)
    want[NO_N, :] = want[5, :] = want[:, 5] = True
    assert (null == want).all()


def test_without_the_option_the_line_is_as_before(files):
    from protein_transformer_amd import score
    rc, out = run([str(files / "pred.pdb"), str(files / "true.pdb")])
    assert rc == 0
    plain = json.loads(out)
    assert tuple(plain) == score.KEYS
    rc, out = run([str(files / "pred.pdb"), str(files / "true.pdb"), "--aligned_error", str(files / "again.json")])
    both = json.loads(out)
    for k in score.KEYS:                                             # the existing keys: the same values
        assert both[k] == plain[k] or (np.isnan(both[k]) and np.isnan(plain[k])), k
