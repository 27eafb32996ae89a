"""csrc/tm_rotation.h as it ships, run on the CPU: tests/host/tm_rotation_main.cpp includes the header, is compiled host-side only
and is fed the moments of every case of tests/rotation_cases.py in BOTH forms the kernels use - raw moments relative to the first
pair (csrc/tmscore.hip; csrc/ensemble.hip without the origin) and pre-centred moments with zero sums (csrc/kabsch_loss.hip) - plus
200 seeded random sets in general position, a line with 10^-k A of off-line scatter for k = 0 .. 12, the truth of every case against
itself, lines in 50 random and 195 integer directions against themselves, and all-zero moments.  The yardstick is numpy's SVD with
the determinant correction (kabsch_loss_ref.svd_rotation).

Bars: |R^T R - I| <= 1e-14 and det R > 0; t = qbar - R pbar to 1e-12 x extent; OPTIMALITY - the residual sum of squares under the
returned R within 1e-12 e0 of the one under the SVD's R, e0 = sum |a_c|^2 + sum |b_c|^2 (fp64 rounding times a few hundred
operations); where the gap is >= 1e-5, |R - R_svd| <= 1e-9 (the bar of tests/test_kabsch_loss_ref.py); a == b with pre-centred
moments: R == I and t == 0 to the bit; every output finite.  A second build with the address and undefined-behaviour sanitizers runs
the same file and must exit cleanly with the same bits of finiteness.  Skips without hipcc; the sanitizer part skips if its
runtime does not link.  The printed figures are in profiles/rotation/NOTES.md."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import kabsch_loss_ref as KR
import metric_ref as M
import rotation_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "tm_rotation_main.cpp")
CSRC = os.path.join(ROOT, "protein_transformer_amd", "csrc")
ORTHO_BAR, T_BAR, OPT_BAR, R_BAR = 1e-14, 1e-12, 1e-12, 1e-9


def hipcc():
    return shutil.which("hipcc") or next((p for p in ("/opt/rocm/bin/hipcc",) if os.path.exists(p)), None)


def compile_program(out, extra=()):
    cmd = [hipcc(), "-x", "hip", "--cuda-host-only", "-std=c++17", f"-I{CSRC}", *extra, SRC, "-o", str(out)]
    return subprocess.run(cmd, capture_output=True, text=True)


def records():
    """[(tag, form, a, b, n, moments)]: a, b the fp64 point sets behind the moments (None for the all-zero record)"""
    sets = [(name, c["a"], c["b"]) for name, c in C.cases().items()]
    rng = np.random.default_rng(77)
    for i in range(200):
        n = int(rng.integers(3, 60))
        b = rng.normal(0, rng.uniform(1, 20), (n, 3)) + rng.normal(0, 50, 3)
        a = (b + rng.normal(0, rng.uniform(0, 3), b.shape)) @ M.rotation(rng).T + rng.normal(0, 50, 3)
        sets.append((f"random{i}", a, b))
    u = np.array([2.0, -1.0, 0.5]) / np.linalg.norm([2.0, -1.0, 0.5])
    for k in range(13):
        t = rng.normal(0, 8, 30)
        off = rng.normal(0, 10.0 ** -k, (30, 3))
        b = np.outer(t, u) + off - np.outer(off @ u, u) + [1.0, 2.0, 3.0]
        sets.append((f"scatter1e-{k}", (b + rng.normal(0, 0.3, b.shape)) @ M.rotation(rng).T + [5.0, 6.0, 7.0], b))
    out = []
    for tag, a, b in sets:
        a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
        out.append((tag, "raw", a, b, *C.raw_moments(a, b)))
        out.append((tag, "centred", a, b, *C.centred_moments(a, b)))
    same = [(f"same/{name}", c["b"]) for name, c in C.cases().items()]
    for i in range(50):                                           # a == b on a line: sigma2 = sigma3 = 0, and the identity's
        v = rng.normal(size=3)                                    # eigenvalue, trace S, TIES with the half turn about the line
        same.append((f"same/line{i}", np.outer(rng.normal(0, 8, 20), v / np.linalg.norm(v)) + rng.normal(0, 10, 3)))
    same += [(f"same/grid{d}", x) for d, x in C.grid_lines()]     # ... and exactly collinear in fp32
    for tag, b in same:
        b = np.asarray(b, np.float64)
        out.append((tag, "centred", b, b, *C.centred_moments(b, b)))
    out.append(("zero/n3", "raw", None, None, 3, np.zeros(15)))
    out.append(("zero/n40", "centred", None, None, 40, np.zeros(15)))
    return out


@pytest.fixture(scope="module")
def solved(tmp_path_factory):
    """(records, x [len(records), 12], directory with the input file) from the -O3 build"""
    if hipcc() is None:
        pytest.skip("hipcc is not installed: the shipped header cannot be compiled here")
    d = tmp_path_factory.mktemp("rotation_host")
    r = compile_program(d / "solve", ("-O3",))
    assert r.returncode == 0, r.stderr
    recs = records()
    with open(d / "in.bin", "wb") as f:
        for *_, n, m in recs:
            f.write(np.int64(n).tobytes() + np.asarray(m, np.float64).tobytes())
    r = subprocess.run([str(d / "solve"), str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr)
    x = np.fromfile(d / "out.bin", np.float64).reshape(-1, 12)
    assert len(x) == len(recs)
    return recs, x, d


def test_every_output_is_finite(solved):
    recs, x, _ = solved
    bad = [(r[0], r[1]) for r, row in zip(recs, x) if not np.isfinite(row).all()]
    assert not bad, bad


def test_proper_rotation_translation_and_optimality(solved):
    recs, x, _ = solved
    worst = dict(ortho=0.0, t=0.0, opt=0.0, R=0.0)
    where = dict(worst)
    for (tag, form, a, b, n, m), row in zip(recs, x):
        if a is None:
            continue
        R, t = row[:9].reshape(3, 3), row[9:]
        ortho = np.abs(R.T @ R - np.eye(3)).max()
        assert ortho <= ORTHO_BAR and np.linalg.det(R) > 0, (tag, form, ortho, np.linalg.det(R))
        pb, qb = m[:3] / n, m[3:6] / n
        extent = max(np.abs(a - a[0]).max(), np.abs(b - b[0]).max(), 1.0)
        et = np.abs(t - (qb - R @ pb)).max() / extent
        ac, bc = a - a.mean(0), b - b.mean(0)
        R_svd = KR.svd_rotation(ac, bc)
        e0 = (ac * ac).sum() + (bc * bc).sum()
        ss = lambda Q: ((ac @ Q.T - bc) ** 2).sum()               # noqa: E731
        eo = abs(ss(R) - ss(R_svd)) / e0 if e0 > 0 else 0.0
        for k, v in (("ortho", ortho), ("t", et), ("opt", eo)):
            if v > worst[k]:
                worst[k], where[k] = v, f"{tag}/{form}"
        g = C.gap(a, b)[0]
        if g >= C.GAP_UNIQUE:
            eR = np.abs(R - R_svd).max()
            if eR > worst["R"]:
                worst["R"], where["R"] = eR, f"{tag}/{form} (gap {g:.1e})"
        elif not tag.startswith("same/"):
            print(f"{tag:28s} {form:8s} gap {g:.1e}: |R - R_svd| {np.abs(R - R_svd).max():.2e} (not compared), "
                  f"|ss - ss_svd| / e0 {eo:.1e}")
    for k, bar in (("ortho", ORTHO_BAR), ("t", T_BAR), ("opt", OPT_BAR), ("R", R_BAR)):
        print(f"worst {k:5s} {worst[k]:.2e} (bar {bar:.0e}) at {where[k]}")
    assert worst["t"] <= T_BAR and worst["opt"] <= OPT_BAR and worst["R"] <= R_BAR


def test_a_structure_against_itself_gives_the_identity_to_the_bit(solved):
    recs, x, _ = solved
    want = np.concatenate([np.eye(3).reshape(-1), np.zeros(3)])
    seen = 0
    for (tag, form, a, b, n, m), row in zip(recs, x):
        if tag.startswith("same/"):
            seen += 1
            assert np.array_equal(row, want) and not np.signbit(row).any(), (tag, row)
    assert seen == len(C.cases()) + 50 + 195
    for (tag, *_), row in zip(recs, x):
        if tag.startswith("zero/"):
            assert np.array_equal(row, want), (tag, row)          # S = 0: the identity, not NaN


def test_the_sanitizer_build_agrees(solved):
    recs, x, d = solved
    r = compile_program(d / "solve_san", ("-O1", "-g", "-Xarch_host", "-fsanitize=address,undefined",
                                          "-fno-sanitize-recover=undefined"))
    if r.returncode != 0:
        pytest.skip("the sanitizer runtime does not link here: " + r.stderr.strip().splitlines()[-1][:200])
    r = subprocess.run([str(d / "solve_san"), str(d / "in.bin"), str(d / "out_san.bin")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), (r.returncode, r.stderr[-2000:])
    y = np.fromfile(d / "out_san.bin", np.float64).reshape(-1, 12)
    assert y.shape == x.shape and np.array_equal(np.isfinite(y), np.isfinite(x))
    print(f"largest |x(-O1, sanitizers) - x(-O3)| over the unique records: "
          f"{max(np.abs(y[i] - x[i]).max() for i, r in enumerate(recs) if r[2] is not None and C.gap(r[2], r[3])[0] >= C.GAP_UNIQUE):.2e}")
