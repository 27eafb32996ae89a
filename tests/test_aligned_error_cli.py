"""CPU checks around the frame-aligned error matrix: the two entry points of include/ptamd.h against `_lib.SIGNATURES`, their
host-side refusals on the built library (no device is touched), the `--pae` and `--aligned_error` options of the two parsers, and
the JSON writer.  The kernel itself needs the GPU: tests/test_gpu_aligned_error.py."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_entry_points_as_the_ctypes_table_has_them():
    from protein_transformer_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ptamd.h")).read(), flags=re.S)
    kinds = {C.c_void_p: "ptr", C.c_int: "int", C.c_size_t: "size_t", C.c_int64: "int64", C.c_float: "float"}
    for name in ("ptamd_aligned_error_workspace_bytes", "ptamd_aligned_error"):
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
             re.search(r"ptamd_aligned_error\s*\((.*?)\)\s*;", header, flags=re.S).group(1).split(",")]
    assert names == ["ref_crd", "sample_crd", "seq", "B", "K", "L", "ae", "stats", "usable", "workspace", "workspace_bytes", "stream"]


def test_entry_points_validate_on_the_host():
    """Bad arguments and a short workspace return the existing error codes before anything is launched (no GPU here)."""
    from protein_transformer_amd import _lib, build
    build.build()
    lib = _lib.lib()
    size = lib.ptamd_aligned_error_workspace_bytes
    assert size(3, 5, 129) > 3 * 6 * 129 * 64                        # at least the 64-byte records of K + 1 structures
    for B, K, L in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 2, 2), (1, 1, (2 ** 31 - 1) // 28 + 1), (2 ** 16, 2 ** 16, 1),
                    (1, 1, 64 * 2 ** 12), (2 ** 12, 1, 64 * 2 ** 6)):  # the last two: more tiles than one launch addresses
        assert size(B, K, L) == 0, (B, K, L)
        assert lib.ptamd_aligned_error(8, 8, 8, B, K, L, 8, 8, 8, 16, 1 << 40, None) == -1, (B, K, L)
    for B in (1, 2, 3, 32):
        for K in (1, 2, 8):
            assert size(B + 1, K, 65) > size(B, K, 65) and size(B, K + 1, 65) > size(B, K, 65)   # monotone in B and K
    assert size(2, 3, 65) == size(2, 3, 65)
    n = size(2, 3, 4)
    for null in range(3):
        a = [8, 8, 8, 2, 3, 4, 8, 8, 8, 16, n, None]
        a[null] = None
        assert lib.ptamd_aligned_error(*a) == -1                     # a NULL input
    for null in (6, 7, 8):
        a = [8, 8, 8, 2, 3, 4, 8, 8, 8, 16, n, None]
        a[null] = None
        assert lib.ptamd_aligned_error(*a) == -1                     # a NULL output
    assert lib.ptamd_aligned_error(8, 8, 8, 2, 3, 4, 8, 8, 8, None, 1 << 20, None) == -3             # no workspace
    assert lib.ptamd_aligned_error(8, 8, 8, 2, 3, 4, 8, 8, 8, 16, n - 1, None) == -3                 # a short one
    assert lib.ptamd_aligned_error(8, 8, 8, 2, 3, 4, 8, 8, 8, 24, n, None) == -5                     # not 16-byte aligned


def test_parsers_accept_the_new_options():
    from protein_transformer_amd import predict, score
    a = predict.parser().parse_args(["m.chkpt", "s.fasta", "--out", "d"])
    assert a.pae is False
    a = predict.parser().parse_args(["m.chkpt", "s.fasta", "--out", "d", "--pae", "--samples", "4"])
    assert a.pae is True and a.samples == 4
    assert predict.PAE_KEYS == ("ens-pae", "ens-ptm") and not set(predict.PAE_KEYS) & set(predict.KEYS)
    a = score.parser().parse_args(["p.pdb", "t.pdb"])
    assert a.aligned_error is None
    a = score.parser().parse_args(["p.pdb", "t.pdb", "--aligned_error", "o.json"])
    assert a.aligned_error == "o.json"
    assert score.AE_KEYS == ("ae-mean", "ae-tm") and not set(score.AE_KEYS) & set(score.KEYS)


def test_pae_without_samples_is_refused_before_anything_is_loaded(tmp_path, capsys):
    from protein_transformer_amd import predict
    fasta = tmp_path / "s.fasta"
    fasta.write_text(">a\nMKV\n")
    assert predict.main([str(tmp_path / "none.chkpt"), str(fasta), "--out", str(tmp_path / "o"), "--samples", "0", "--pae"]) == 2
    err = capsys.readouterr().err
    assert err.startswith("predict: ") and err.count("\n") == 1 and "--pae" in err and "--samples" in err
    assert not (tmp_path / "o").exists()


def test_json_writer(tmp_path):
    from protein_transformer_amd import predict
    ae = np.array([[0.0, 1.234, np.nan], [2.005001, 0.0, 31.75], [np.nan, np.inf, 0.0]], np.float32)
    doc = predict.pae_document(ae)
    assert doc == [{"predicted_aligned_error": [[0.0, 1.23, None], [2.01, 0.0, 31.75], [None, None, 0.0]],
                    "max_predicted_aligned_error": 31.75}]
    path = tmp_path / "x.pae.json"
    predict.write_pae(str(path), ae)
    text = path.read_text()
    assert "NaN" not in text and "Infinity" not in text and "null" in text and text.endswith("\n")
    assert json.loads(text) == doc
    predict.write_pae(str(path), np.full((2, 2), np.nan))
    assert json.loads(path.read_text()) == [{"predicted_aligned_error": [[None, None], [None, None]],
                                             "max_predicted_aligned_error": None}]
    summary = predict.pae_summary({"ae_stats": np.array([1.5, np.nan], np.float32)})
    assert summary == {"ens-pae": 1.5, "ens-ptm": None} and tuple(summary) == predict.PAE_KEYS
