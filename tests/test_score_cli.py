"""The structure-file scorer `python -m protein_transformer_amd.score`: the PDB reader and the command line without a GPU, one
end-to-end run in a child process with one."""
import csv
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sidechain_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"rmsd-full", "lddt-full", "lddt-ca", "tm-ca", "gdt-ts", "gdt-ha", "ss-q3", "ss-h", "ss-e", "clash-full", "sc-chi1", "sc-chi12",
        "sc-chi-mae", "sc-rmsd", "n-res"}


def structure(n=24, seed=3):
    """(one-letter sequence, ids, crd [n*14, 3] fp32 with NaN in the slots the types do not have): all twenty types."""
    seq = np.arange(n) % 20
    crd = R.centred(R.build(seq, R.angles(n, seed))).astype(np.float32)
    return "".join(R.AA[s] for s in seq), seq.astype(np.int64), crd


def write(path, crd, letters):
    from protein_transformer_amd.protein.PDB_Creator import PDB_Creator
    PDB_Creator(crd, seq=letters).save_pdb(str(path))
    return str(path)


def test_read_pdb_round_trips_what_the_writer_writes(tmp_path):
    from protein_transformer_amd.score import read_pdb
    letters, ids, crd = structure()
    crd[5 * 14 + 4] = np.nan                                       # a CB the file will not have
    crd[9 * 14 + 2] = np.nan                                       # and a C
    seq, got, numbers = read_pdb(write(tmp_path / "a.pdb", crd, letters), with_numbers=True)
    assert seq.dtype == np.int64 and got.dtype == np.float32 and got.shape == crd.shape
    assert seq.tolist() == ids.tolist() and numbers.tolist() == list(range(1, len(ids) + 1))
    assert np.array_equal(np.isnan(got), np.isnan(crd))
    assert np.nanmax(np.abs(got - crd)) <= 5e-4 + 1e-6             # three decimals


def test_read_pdb_skips_what_it_says_it_skips(tmp_path):
    from protein_transformer_amd.score import read_pdb
    letters, ids, crd = structure(6)
    text = open(write(tmp_path / "a.pdb", crd, letters)).read().split("\n")
    atoms = [l for l in text if l.startswith("ATOM")]
    ca = next(l for l in atoms if l[12:16].strip() == "CA")
    shifted = lambda l, dx: l[:30] + f"{float(l[30:38]) + dx:8.3f}" + l[38:]          # noqa: E731
    extra = [
        ca[:12] + " HA " + ca[16:76] + " H" + ca[78:],            # a hydrogen, by its element column
        ca[:12] + "1HB " + ca[16:76] + "  " + ca[78:],            # and by its name alone
        "HETATM" + ca[6:17] + "HOH" + ca[20:],                    # water
        "HETATM" + ca[6:],                                        # a HETATM record of a standard residue
        shifted(ca[:16] + "B" + ca[17:], 9.0),                    # the other alternate location
        ca[:17] + "MSE" + ca[20:22] + " 900" + ca[26:],           # a residue name outside the twenty
        shifted(ca[:21] + "B" + ca[22:], 5.0),                    # a second chain
    ]
    # residue 3 written first: the order of the file is not the order of the result
    res3 = [l for l in atoms if int(l[22:26]) == 3]
    body = res3 + [l for l in atoms if int(l[22:26]) != 3] + extra
    model2 = ["MODEL        2"] + [shifted(l, 1.0) for l in atoms] + ["ENDMDL"]
    path = tmp_path / "b.pdb"
    path.write_text("\n".join(["REMARK  test", "MODEL        1"] + body + ["ENDMDL"] + model2 + ["END"]) + "\n")
    seq, got = read_pdb(str(path))
    want_seq, want = read_pdb(str(tmp_path / "a.pdb"))
    assert seq.tolist() == want_seq.tolist() == ids.tolist()
    assert np.array_equal(np.nan_to_num(got, nan=-1e9), np.nan_to_num(want, nan=-1e9))
    # alternate location A is read like a blank one
    path.write_text("\n".join(l[:16] + "A" + l[17:] for l in atoms) + "\n")
    assert np.array_equal(np.nan_to_num(read_pdb(str(path))[1], nan=-1e9), np.nan_to_num(want, nan=-1e9))


def test_a_malformed_atom_record_is_named(tmp_path):
    from protein_transformer_amd import score
    letters, ids, crd = structure(6)
    lines = open(write(tmp_path / "a.pdb", crd, letters)).read().split("\n")
    at = next(i for i, l in enumerate(lines) if l.startswith("ATOM") and int(l[22:26]) == 2)
    for bad in (lines[at][:22] + "  x " + lines[at][26:], lines[at][:38] + "   ?.???" + lines[at][46:], lines[at][:40]):
        path = tmp_path / "bad.pdb"
        path.write_text("\n".join(lines[:at] + [bad] + lines[at + 1:]))
        with pytest.raises(ValueError, match=rf"bad\.pdb, line {at + 1}: an ATOM record"):
            score.read_pdb(str(path))
    # and the command line says it in one line, before anything touches the device
    r = subprocess.run([sys.executable, "-m", "protein_transformer_amd.score", str(path), str(tmp_path / "a.pdb")], cwd=ROOT,
                       capture_output=True, text=True)
    assert r.returncode == 2 and r.stdout == "" and f"line {at + 1}" in r.stderr and "Traceback" not in r.stderr


def test_the_kernel_tables_are_the_reference_tables():
    """The chi counts and the symmetric chi that csrc/sidechain.hip compiles in, read from its source, against the tables of
    tests/sidechain_ref.py (which tests/test_sidechain_ref.py ties to the atom names), and the atom counts behind the same kernel
    through the library."""
    from protein_transformer_amd import _lib, build
    build.build()
    src = open(os.path.join(ROOT, "protein_transformer_amd", "csrc", "sidechain.hip")).read()
    table = lambda name: [int(x) for x in re.search(name + r"\[NRES\] = \{([^}]*)\}", src).group(1).split(",")]   # noqa: E731
    assert table("h_nchi") == list(R.NCHI)
    assert table("h_sym_chi") == [R.SYM_CHI.get(r, 0) for r in range(20)]
    assert [_lib.lib().ptamd_sidechain_atoms(r) for r in range(20)] == list(R.NSC)
    pairs = {2: {6: 7, 7: 6}, 3: {7: 8, 8: 7}, 4: {6: 10, 10: 6, 7: 9, 9: 7}, 19: {6: 11, 11: 6, 7: 10, 10: 7}}
    assert {r: {a: b for pair in p for a, b in (pair, pair[::-1])} for r, (p, _) in R.SWAPS.items()} == pairs
    for r, want in pairs.items():                                  # swap_partner: `type == r` ... `c - s` on the listed slots
        m = re.search(rf"if \(type == {r}\) return ([^?]*)\? (\d+) - s : s;", src)
        slots, c = [int(x) for x in re.findall(r"s == (\d+)", m.group(1))], int(m.group(2))
        assert {s: c - s for s in slots} == want, r


def test_unequal_sequences_are_refused():
    from protein_transformer_amd.score import score_structures
    letters, ids, crd = structure(6)
    other = ids.copy()
    other[2] = (other[2] + 1) % 20
    with pytest.raises(ValueError, match="same sequence"):
        score_structures((other, crd), (ids, crd))
    with pytest.raises(ValueError, match="same sequence"):
        score_structures((ids[:5], crd[:5 * 14]), (ids, crd))


def test_help_parses_and_names_the_options():
    r = subprocess.run([sys.executable, "-m", "protein_transformer_amd.score", "--help"], cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "--threshold" in r.stdout and "--per_residue" in r.stdout and "PRED.pdb" in r.stdout and "TRUE.pdb" in r.stdout
    from protein_transformer_amd.score import KEYS as keys, parser
    assert set(keys) == KEYS and len(keys) == len(KEYS)
    args = parser().parse_args(["a.pdb", "b.pdb", "--threshold", "30"])
    assert args.threshold == 30.0 and args.per_residue is None


def test_ctypes_table_has_the_entry_point():
    from protein_transformer_amd import _lib
    res, args = _lib.SIGNATURES["ptamd_sidechain"]
    assert len(args) == 12 and args[5] is _lib._f and args[10] is _lib._sz
    assert _lib.SIGNATURES["ptamd_sidechain_workspace_bytes"] == (_lib._sz, [_lib._i, _lib._i])
    header = open(os.path.join(ROOT, "include", "ptamd.h")).read()
    decl = re.search(r"int ptamd_sidechain\((.*?)\);", header, flags=re.S)
    assert decl and len(decl.group(1).split(",")) == 12


def test_the_scorer_never_imports_the_oracle():
    src = open(os.path.join(ROOT, "protein_transformer_amd", "score.py")).read()
    assert not re.search(r"^\s*(from|import)\s+(oracle|sidechain_ref|tests)", src, flags=re.M)
    code = ("import sys; import protein_transformer_amd.score; "
            "bad = [m for m in sys.modules if m == 'oracle' or m.startswith('oracle.')]; sys.exit(1 if bad else 0)")
    assert subprocess.run([sys.executable, "-c", code], cwd=ROOT).returncode == 0


def run_main(*argv):
    """`main` in a child process -> (return code, the JSON line or None, stderr)."""
    r = subprocess.run([sys.executable, "-m", "protein_transformer_amd.score", *argv], cwd=ROOT, capture_output=True, text=True)
    lines = [l for l in r.stdout.split("\n") if l.startswith("{")]
    return r.returncode, json.loads(lines[-1]) if lines else None, r.stderr


@pytest.mark.gpu
def test_a_file_against_itself_and_against_another(tmp_path):
    letters, ids, crd = structure(24)
    ang = R.angles(24, 3)
    ang[:, 7:] += 0.9                                              # the same backbone, other side chains
    other = R.centred(R.build(ids, ang)).astype(np.float32)
    a, b = write(tmp_path / "a.pdb", crd, letters), write(tmp_path / "b.pdb", other, letters)
    out = tmp_path / "res.csv"
    rc, same, err = run_main(a, a, "--per_residue", str(out))
    assert rc == 0, err
    assert set(same) == KEYS and same["n-res"] == 24
    # identical structures: the RMSD is the root of an fp64 cancellation, TM-score a sum of N terms 1 / N; the others are exact
    assert same["rmsd-full"] <= 1e-3 and same["lddt-full"] == 1.0 and same["lddt-ca"] == 1.0
    assert same["tm-ca"] == pytest.approx(1.0, abs=1e-6) and same["gdt-ts"] == 1.0 and same["gdt-ha"] == 1.0
    assert same["sc-chi1"] == 1.0 and same["sc-chi12"] == 1.0 and same["sc-chi-mae"] == 0.0 and same["sc-rmsd"] == 0.0
    assert same["ss-q3"] == 1.0
    rows = list(csv.reader(open(out)))
    assert rows[0] == ["resnum", "resname", "lddt", "chi1_err", "chi2_err", "chi3_err", "chi4_err", "sc_rmsd"] and len(rows) == 1 + 24
    assert [r[0] for r in rows[1:]] == [str(i) for i in range(1, 25)] and rows[1][1] == "ALA" and rows[6][1] == "GLY"
    assert rows[6][3:] == ["nan"] * 5 and float(rows[9][6]) == 0.0               # GLY has nothing; LYS has a chi4
    rc, diff, err = run_main(b, a, "--threshold", "40")
    assert rc == 0, err
    read = lambda p: __import__("protein_transformer_amd.score", fromlist=["read_pdb"]).read_pdb(p)   # noqa: E731
    ref = R.reference(read(b)[1], read(a)[1], ids)
    assert diff["sc-chi1"] == pytest.approx(ref["score"][0], abs=1e-6) and diff["sc-chi12"] == pytest.approx(ref["score"][1], abs=1e-6)
    assert diff["sc-chi-mae"] == pytest.approx(ref["score"][2], abs=R.EPS_CHI) and diff["sc-rmsd"] == pytest.approx(ref["score"][3], abs=R.EPS_RMS)
    assert diff["sc-chi1"] < 1.0 and diff["sc-rmsd"] > 0.3 and diff["lddt-ca"] > 0.99 and diff["lddt-full"] < 1.0
    # unequal sequences: a message, no traceback, nothing on stdout
    c = write(tmp_path / "c.pdb", crd[:20 * 14], letters[:20])
    rc, res, err = run_main(c, a)
    assert rc == 2 and res is None and "same sequence" in err and "Traceback" not in err
