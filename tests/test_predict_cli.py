"""CPU checks of `python -m protein_transformer_amd.predict` (the FASTA reader, the batching, the argument parser), of the
temperature factors of `PDB_Creator`, and of the two ensemble entry points of include/ptamd.h against `_lib.SIGNATURES`.  The run
itself needs the GPU: tests/test_gpu_predict.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write(tmp_path, text, name="s.fasta"):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


# ------------------------------------------------------------------------------------------------ FASTA
def test_fasta_wrapped_lower_case_and_terminator(tmp_path):
    from protein_transformer_amd.predict import read_fasta
    path = write(tmp_path, ">sp|P1|ONE first protein\nmkv\nLA ac\n\n>two\nGGSW*\n>three   \nacdefghiklmnpqrstvwy\n")
    assert read_fasta(path) == [("sp|P1|ONE", "MKVLAAC"), ("two", "GGSW"), ("three", "ACDEFGHIKLMNPQRSTVWY")]


@pytest.mark.parametrize("text,names", [
    (">a\nMKV\n>empty\n>b\nGG\n", ("empty", "no sequence")),
    (">a\nMKV\n>star\n*\n", ("star", "no sequence")),
    (">a\nMKV\n>odd\nMKXV\n", ("odd", "'X'")),
    (">a\nMKV\n>inner\nMK*V\n", ("inner", "'*'")),
    (">a\nMKV\n>b\nGG\n>a other words\nAA\n", ("'a'", "second record")),
    ("MKV\n>a\nGG\n", ("line 1", "in front of the first")),
    (">\nMKV\n", ("line 1", "cannot name a file")),
    (">x/y\nMKV\n", ("x/y", "cannot name a file")),
    ("", ("no record",)),
])
def test_fasta_refusals_name_the_record(tmp_path, text, names):
    from protein_transformer_amd.predict import read_fasta
    with pytest.raises(ValueError) as e:
        read_fasta(write(tmp_path, text))
    assert "\n" not in str(e.value)
    for n in names:
        assert n in str(e.value), str(e.value)


def test_main_refuses_with_code_2_and_one_line(tmp_path, capsys):
    """The refusals that need no model: a bad FASTA file, a missing file, a file that is no checkpoint.  (A sequence longer than
    the checkpoint's max_seq_len needs the model: tests/test_gpu_predict.py.)"""
    from protein_transformer_amd import predict
    bad = write(tmp_path, ">a\nMKV\n>a\nGG\n")
    ok = write(tmp_path, ">a\nMKV\n", "good.fasta")
    for argv in ([str(tmp_path / "none.chkpt"), bad, "--out", str(tmp_path / "o")],
                 [str(tmp_path / "none.chkpt"), str(tmp_path / "none.fasta"), "--out", str(tmp_path / "o")],
                 [str(tmp_path / "none.chkpt"), ok, "--out", str(tmp_path / "o")],
                 [write(tmp_path, "not a checkpoint\n", "text.chkpt"), ok, "--out", str(tmp_path / "o")],
                 [str(tmp_path / "none.chkpt"), write(tmp_path, ">a\nMKV\n", "ok.fasta"), "--out", str(tmp_path / "o"), "--samples", "-1"]):
        assert predict.main(argv) == 2
        err = capsys.readouterr().err
        assert err.startswith("predict: ") and err.count("\n") == 1
    assert not (tmp_path / "o").exists()


def test_batches_are_sorted_by_length_and_bounded():
    from protein_transformer_amd.predict import make_batches
    lengths = [70, 5, 64, 5, 30]
    assert make_batches(lengths, 16384) == [[1, 3, 4, 2, 0]]
    assert make_batches(lengths, 128) == [[1, 3, 4], [2], [0]]                 # 3 x 30 fits, 4 x 64 and 2 x 70 do not
    assert make_batches(lengths, 1) == [[1], [3], [4], [2], [0]]               # at least one sequence per batch
    for budget in (10, 60, 140, 350):
        got = make_batches(lengths, budget)
        assert sorted(i for b in got for i in b) == list(range(5))
        assert all(len(b) == 1 or len(b) * max(lengths[i] for i in b) <= budget for b in got)


def test_parser_defaults():
    from protein_transformer_amd.predict import KEYS, parser
    a = parser().parse_args(["m.chkpt", "s.fasta", "--out", "d"])
    assert (a.checkpoint, a.fasta, a.out, a.samples, a.seed, a.batch_residues, a.per_residue) == ("m.chkpt", "s.fasta", "d", 8, 0, 16384, False)
    a = parser().parse_args(["m.chkpt", "s.fasta", "--out", "d", "--samples", "0", "--seed", "7", "--batch_residues", "512", "--per_residue"])
    assert (a.samples, a.seed, a.batch_residues, a.per_residue) == (0, 7, 512, True)
    with pytest.raises(SystemExit):
        parser().parse_args(["m.chkpt", "s.fasta"])                                # --out is required
    assert KEYS == ("id", "n-res", "ens-lddt", "ens-rmsd", "ens-rmsf-ca", "usable", "samples")


def test_summary_and_b_factors_of_host_results():
    from protein_transformer_amd import predict
    r = dict(crd=None, conf=np.array([80.0, np.nan, 60.0], np.float32), rmsf_ca=np.array([1.0, np.nan, 3.0], np.float32),
             rmsf_all=np.array([1.5, np.nan, 3.5], np.float32), rmsd=np.array([2.0, np.nan], np.float32), usable=1)
    assert predict.summary("x", "MKV", r, 2) == {"id": "x", "n-res": 3, "ens-lddt": 70.0, "ens-rmsd": 2.0, "ens-rmsf-ca": 2.0,
                                                "usable": 1, "samples": 2}
    assert list(predict.b_factors(r, 3)) == [80.0, 0.0, 60.0]
    none = dict(crd=None, conf=None, rmsf_ca=None, rmsf_all=None, rmsd=None, usable=0)
    assert predict.summary("x", "MKV", none, 0) == {"id": "x", "n-res": 3, "ens-lddt": None, "ens-rmsd": None, "ens-rmsf-ca": None,
                                                   "usable": 0, "samples": 0}
    assert list(predict.b_factors(none, 3)) == [0.0, 0.0, 0.0]


def test_sample_seeds_depend_on_seed_and_pass_only():
    from protein_transformer_amd.ensemble import sample_seed
    seeds = {sample_seed(s, k) for s in range(4) for k in range(16)}
    assert len(seeds) == 64 and all(0 <= v < 2 ** 62 for v in seeds)
    assert sample_seed(3, 5) == sample_seed(3, 5)


# ------------------------------------------------------------------------------------------------ PDB_Creator
def test_pdb_creator_b_factors(golden):
    from protein_transformer_amd.protein.PDB_Creator import PDB_Creator
    g = golden("g11_pdb")
    seq, crd, want = str(g["seq0"]), g["crd0"], str(g["pdb0"])
    assert PDB_Creator(crd, seq=seq).to_string("golden 0") == want                 # default: every line as before
    assert PDB_Creator(crd, seq=seq, b_factors=None).to_string("golden 0") == want
    zeros = PDB_Creator(crd, seq=seq, b_factors=np.zeros(len(seq))).to_string("golden 0")
    assert zeros == want                                                           # 0.00 is what the reference writes
    b = np.linspace(0.0, 100.0, len(seq)).round(3)
    b[1] = 7.125
    got = PDB_Creator(crd, seq=seq, b_factors=b).to_string("golden 0").split("\n")
    old = want.split("\n")
    assert len(got) == len(old)
    seen = set()
    for new, was in zip(got, old):
        if not was.startswith("ATOM"):
            assert new == was
            continue
        res = int(was[22:26]) - 1
        seen.add(res)
        assert new[:60] == was[:60] and new[66:] == was[66:] and was[60:66] == "  0.00"
        assert new[60:66] == "%6.2f" % b[res] and len(new) == len(was)
    assert seen == set(range(len(seq))) and any(l[60:66] == "100.00" for l in got) and any(l[60:66] == "  7.12" for l in got)
    with pytest.raises(AssertionError):
        PDB_Creator(crd, seq=seq, b_factors=np.zeros(len(seq) + 1))                # per residue, not per atom


def test_written_b_factors_read_back(tmp_path):
    from protein_transformer_amd.protein.PDB_Creator import PDB_Creator
    from protein_transformer_amd.score import read_pdb
    crd = np.arange(3 * 14 * 3, dtype=np.float32).reshape(42, 3) + 1
    path = str(tmp_path / "b.pdb")
    PDB_Creator(crd, seq="AGW", b_factors=[12.25, 0.0, 99.999]).save_pdb(path, "t")
    bs = [(int(l[22:26]), float(l[60:66])) for l in open(path) if l.startswith("ATOM")]
    assert len(bs) == 5 + 4 + 14 and {r: v for r, v in bs} == {1: 12.25, 2: 0.0, 3: 100.0}
    seq, back = read_pdb(path)
    assert list(seq) == [0, 5, 18] and np.nanmax(np.abs(back[:5] - crd[:5])) <= 5e-4 + 1e-6


# ------------------------------------------------------------------------------------------------ ABI
def test_header_declares_the_ensemble_entry_points_as_the_ctypes_table_has_them():
    from protein_transformer_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptamd.h")).read(), flags=re.S)
    kinds = {C.c_void_p: "ptr", C.c_int: "int", C.c_size_t: "size_t", C.c_int64: "int64", C.c_float: "float"}
    for name in ("ptamd_ensemble_workspace_bytes", "ptamd_ensemble_spread"):
        decl = re.search(r"(\w+)\s+" + name + r"\s*\((.*?)\)\s*;", header, flags=re.S)
        assert decl, name
        want = []
        for a in decl.group(2).split(","):
            a = " ".join(a.split())
            want.append("ptr" if "*" in a else "int64" if a.startswith("int64_t") else "size_t" if a.startswith("size_t")
                        else "float" if a.startswith("float") else "int")
        res, args = _lib.SIGNATURES[name]
        assert [kinds[a] for a in args] == want, (name, want)
        assert kinds[res] == ("size_t" if decl.group(1) == "size_t" else "int")
    names = [" ".join(a.split()).split()[-1].lstrip("*") for a in
             re.search(r"ptamd_ensemble_spread\s*\((.*?)\)\s*;", header, flags=re.S).group(1).split(",")]
    assert names == ["ref_crd", "sample_crd", "seq", "B", "K", "L", "rmsd", "rmsf", "usable", "workspace", "workspace_bytes", "stream"]


def test_ensemble_entry_points_validate_on_the_host():
    """Bad arguments and a short workspace return the existing error codes before anything is launched (no GPU here)."""
    from protein_transformer_amd import _lib, build
    build.build()
    lib = _lib.lib()
    assert lib.ptamd_ensemble_workspace_bytes(3, 5, 129) == 3 * 5 * 64
    assert lib.ptamd_ensemble_workspace_bytes(3, 5, 1) == lib.ptamd_ensemble_workspace_bytes(3, 5, 4096)   # 64 B per (protein, sample)
    for B, K, L in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 2, 2), (1, 1, (2 ** 31 - 1) // 28 + 1), (2 ** 16, 2 ** 16, 1)):
        assert lib.ptamd_ensemble_workspace_bytes(B, K, L) == 0, (B, K, L)
        assert lib.ptamd_ensemble_spread(8, 8, 8, B, K, L, 8, 8, 8, 16, 1 << 30, None) == -1, (B, K, L)
    assert lib.ptamd_ensemble_spread(None, 8, 8, 1, 1, 4, 8, 8, 8, 16, 64, None) == -1               # a NULL array
    assert lib.ptamd_ensemble_spread(8, 8, 8, 2, 3, 4, 8, 8, 8, None, 1 << 20, None) == -3           # no workspace
    assert lib.ptamd_ensemble_spread(8, 8, 8, 2, 3, 4, 8, 8, 8, 16, 2 * 3 * 64 - 1, None) == -3      # a short one
    assert lib.ptamd_ensemble_spread(8, 8, 8, 2, 3, 4, 8, 8, 8, 24, 2 * 3 * 64, None) == -5          # not 16-byte aligned
