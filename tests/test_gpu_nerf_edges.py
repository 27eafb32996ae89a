"""MI355X tests of the NeRF build and its adjoint (csrc/geometry.hip) PER ATOM and PER ANGLE against the fp64 oracle, at the
edges of the kernels' index arithmetic, and of the atan2 kernels.  Only `nerf_forward`, `nerf_backward` (both variants),
`angles_forward` and `angles_backward` are called.

Inputs: angles from `synthetic.make_batch(...)["start_ang_rad"]` (bond angles 1.9 .. 2.1 +- 0.25).
  RAGGED  lengths 2, 3, 22, 23, 64, 65, 66, 86, 129, 130 padded to L = 130 (angles behind a protein's end are garbage):
          forward scan K = 3 (len - 1): 3 (61 idle lanes), 63 -> 66 (chunk 1 -> 2, lanes from 33 up empty), 189 / 192 / 195 (chunk 3
          full; chunk 4 with a short last lane); side-chain blocks of 64 residues: 64 / 65 / 66; adjoint n = 3 len on 256 threads:
          258 (chunk 1 -> 2, lanes from 129 up and a whole wavefront idle), 387 / 390 (2 - 3 live lanes in the last wavefront)
  TYPES   20 proteins of 66 residues, every residue type at residues 0, 1, 63, 64 and 65 (asserted)

Every bound is a multiple of what the fp32 ORACLE (the same formulas, step by step, in fp32) loses against the fp64 oracle on the
same protein - two fp32 roundings of one chain - and never above the older flat bars (coord_tol, 1e-4 for an internal
coordinate, 1e-3 for a gradient).  The multiples are twice the worst ratio measured on the MI355X, rounded up; the run that set
them printed (kernel error / yardstick = ratio; the yardstick is never taken below the rounding of the fp64 answer to fp32):

  1. forward, worst atom of a protein, A           full build                        backbone_only
     RAGGED len   2                                1.07e-6 / 2.43e-6 = 0.44          4.37e-7 / 4.92e-7 = 0.89
                  3                                1.60e-6 / 3.45e-6 = 0.46          9.64e-7 / 1.27e-6 = 0.76
                 22                                2.08e-5 / 4.58e-5 = 0.45          1.27e-5 / 4.36e-5 = 0.29
                 23                                2.08e-5 / 2.41e-5 = 0.86          9.36e-6 / 2.25e-5 = 0.42
                 64                                9.71e-5 / 1.18e-4 = 0.82          3.51e-5 / 1.05e-4 = 0.33
                 65                                4.13e-5 / 2.10e-4 = 0.20          2.54e-5 / 1.95e-4 = 0.13
                 66                                8.46e-5 / 2.66e-4 = 0.32          8.05e-5 / 2.14e-4 = 0.38
                 86                                8.73e-5 / 2.30e-4 = 0.38          6.89e-5 / 2.17e-4 = 0.32
                129                                1.13e-4 / 7.85e-4 = 0.14          1.13e-4 / 7.50e-4 = 0.15
                130                                1.85e-4 / 4.34e-4 = 0.43          1.53e-4 / 4.16e-4 = 0.37
     TYPES  len  66, worst of 20 (protein 8)       6.69e-5 / 6.36e-5 = 1.05          6.44e-5 / 5.26e-5 = 1.22
                     the other 19                  ratios 0.10 .. 0.47               ratios 0.08 .. 0.40
     -> FWD_RATIO 3 and 3.  The scan is no worse than the step-by-step fp32 chain anywhere; no ratio near 10.
  2. internal coordinates, worst placement         bond, A                  angle, rad               torsion, rad
     TYPES (20 proteins)                           2.47e-5 / 7.00e-6 = 3.53 1.66e-5 / 5.64e-6 = 2.94 1.75e-5 / 1.18e-5 = 1.49
     RAGGED len 130                                1.55e-5 / 4.50e-6 = 3.44 2.22e-5 / 3.78e-6 = 5.89 3.94e-5 / 5.45e-6 = 7.24
     -> IC_RATIO 8, 12, 15.  Here the scan IS worse than the step-by-step chain, by its composition order: a backbone atom is
     the translation of a product of up to 3 len fp32 rotation matrices, which nothing keeps orthonormal (1e-5 of a 1.5 A bond
     is what a few hundred fp32 matrix products can lose), while the step-by-step build re-normalises its frame from three atoms
     at every placement and so stays on the storage floor.  2e-5 A on a bond and 4e-5 rad on a torsion at 390 placements, 2.5 x
     inside the ceiling.
  3. adjoint, dense upstream gradient, worst angle entry / max |reference| of the protein
     RAGGED len   2                                1.15e-7 / 8.42e-8 = 1.37          5.43e-8 / 1.24e-7 = 0.44
                  3                                1.27e-7 / 4.05e-7 = 0.31          1.03e-7 / 1.03e-7 = 1.00
                 22                                5.62e-7 / 1.38e-6 = 0.41          6.02e-7 / 1.06e-6 = 0.57
                 23                                6.22e-7 / 1.16e-6 = 0.53          4.70e-7 / 1.21e-6 = 0.39
                 64                                1.38e-6 / 6.31e-6 = 0.22          1.42e-6 / 1.25e-5 = 0.11
                 65                                3.69e-7 / 5.09e-6 = 0.07          3.44e-7 / 6.31e-6 = 0.05
                 66                                8.65e-7 / 9.15e-6 = 0.09          1.24e-6 / 8.24e-6 = 0.15
                 86                                7.17e-7 / 3.42e-6 = 0.21          3.87e-7 / 5.56e-6 = 0.07
                129                                1.34e-6 / 9.90e-6 = 0.14          2.30e-6 / 2.35e-5 = 0.10
                130                                2.17e-6 / 1.28e-5 = 0.17          1.55e-6 / 1.18e-5 = 0.13
     TYPES  len  66, worst of 20                   8.22e-7 / 1.94e-6 = 0.42 (19)     3.59e-6 / 3.98e-6 = 0.90 (1)
     -> ADJ_RATIO 3 and 2
  4. adjoint, one atom at a time, worst entry of a row / max |reference| of the row
     len 130 (47 probes), worst probe              ratio 1.49; the summed rows 1.05e-7 / 9.62e-6 = 0.01
     len  66 (TRP at residue 64), worst probe      ratio 1.75; the summed rows 1.41e-7 / 4.44e-6 = 0.03
     -> PROBE_RATIO 4
  6. atan2 (bars stated, not measured): worst angle error 1.91 ulp, worst gradient error 1.64 ulp

The adjoint tests feed `nerf_backward` the fp64 coordinates rounded to fp32, not the kernel's own build: forward drift is test
1's and 2's business, the adjoint is judged alone.
"""
import functools
import math

import numpy as np
import pytest
import torch

import nerf_ref
from oracle import batched
from oracle.geometry import BL_CA_C, BL_N_CA, SC_PROGRAM
from protein_transformer_amd import synthetic

pytestmark = pytest.mark.gpu

RAGGED_LENS = [2, 3, 22, 23, 64, 65, 66, 86, 129, 130]
L_RAGGED, L_TYPES = 130, 66
TYPE_POSITIONS = (0, 1, 63, 64, 65)
EPS32 = 2.0 ** -24                               # half an ulp, relative: the rounding of a stored fp32 result

# twice the worst measured ratio, rounded up (module docstring)
FWD_RATIO = {False: 3.0, True: 3.0}              # by backbone_only
IC_RATIO = {"bond": 8.0, "angle": 12.0, "torsion": 15.0}
ADJ_RATIO = {False: 3.0, True: 2.0}
PROBE_RATIO = 4.0
IC_CEILING = 1e-4                                # A / rad: two entries of the bond table differ by at least 1e-3
GRAD_CEILING = 1e-3                              # the older per-protein bar of the gradient tests


def coord_tol(L):                                # the older bar of the coordinate tests (tests/test_gpu_loss_path.py)
    return 2e-3 * max(1.0, L / 128)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def bound(ratio, yardstick, ceiling):
    return min(ratio * yardstick, ceiling)


# --------------------------------------------------------------------------- inputs and references, computed once
def compact(x):
    """[B, L*14, 3] -> the compact backbone [B, L*3, 3]"""
    B = x.shape[0]
    return x.reshape(B, -1, 14, 3)[:, :, :3].reshape(B, -1, 3).contiguous()


def make_inputs(name):
    if name == "ragged":
        lens, L = RAGGED_LENS, L_RAGGED
        batch = synthetic.make_batch(lens, L_pad=L, seed=7)
        for pos, r in ((0, 18), (63, 4), (64, 14), (129, 19)):                    # the len-130 protein: TRP first, PHE | ARG on the
            batch["seq"][RAGGED_LENS.index(130), pos] = r                         # block edge, TYR last
    else:
        lens, L = [L_TYPES] * 20, L_TYPES
        batch = synthetic.make_batch(lens, L_pad=L, seed=8)
        for b in range(20):
            for k, pos in enumerate(TYPE_POSITIONS):
                batch["seq"][b, pos] = (b + 3 * k) % 20
    ang, seq = batch["start_ang_rad"].clone(), batch["seq"].clone()
    garbage = torch.from_numpy(np.random.default_rng(1).uniform(-3.0, 3.0, ang.shape).astype(np.float32))
    pad = (seq == 20)[:, :, None].expand_as(ang)
    return lens, L, torch.where(pad, garbage, ang), seq


@functools.lru_cache(maxsize=None)
def reference(name):
    """inputs, fp64 and fp32 oracle coordinates, and both oracles' gradients of sum(w crd) for a dense normal w (all atoms) and for
    its backbone part alone; read-only for the tests"""
    lens, L, ang, seq = make_inputs(name)
    B = len(lens)
    w = torch.from_numpy(np.random.default_rng(2).normal(size=(B, L * 14, 3)).astype(np.float32))
    w_bb = torch.zeros_like(w).reshape(B, L, 14, 3)
    w_bb[:, :, :3] = w.reshape(B, L, 14, 3)[:, :, :3]
    w_bb = w_bb.reshape(B, L * 14, 3)
    out = dict(lens=lens, L=L, ang=ang, seq=seq, w=w, own=synthetic.slot_mask(seq).numpy())
    for dtype, tag in ((torch.float64, "64"), (torch.float32, "32")):
        a = ang.to(dtype).clone().requires_grad_()
        crd = batched.generate_coords_batched(a, seq, dtype)
        g, = torch.autograd.grad((crd * w.to(dtype)).sum(), a, retain_graph=True)
        g_bb, = torch.autograd.grad((crd * w_bb.to(dtype)).sum(), a)
        out["crd" + tag], out["g" + tag], out["gbb" + tag] = crd.detach(), g, g_bb
    return out


def show(test, case, kernel, yard, ratio):
    print(f"MEASURED {test:<26} {case:<22} kernel {kernel:.3e}  yardstick {yard:.3e}  ratio {ratio:.2f}")


# --------------------------------------------------------------------------- 1. forward, per atom
@pytest.mark.parametrize("backbone_only", [False, True], ids=["full", "backbone"])
@pytest.mark.parametrize("name", ["ragged", "types"])
def test_forward_per_atom(dev, name, backbone_only):
    from protein_transformer_amd.protein.Structure import nerf_forward
    ref = reference(name)
    lens, L, ang, seq = ref["lens"], ref["L"], ref["ang"], ref["seq"]
    B = len(lens)
    crd, status = nerf_forward(ang.to(dev), seq.to(dev), backbone_only=backbone_only)
    assert int(status.item()) == 0
    crd = crd.cpu()
    c64, c32, own = ref["crd64"], ref["crd32"], torch.from_numpy(ref["own"])
    if backbone_only:
        full, _ = nerf_forward(ang.to(dev), seq.to(dev))
        assert torch.equal(crd, compact(full.cpu()))                              # bit for bit slots 0..2 of the full build
        c64, c32, own = compact(c64), compact(c32), own.reshape(B, L, 14)[:, :, :3].reshape(B, L * 3)
    assert crd.shape == c64.shape
    assert torch.all(crd[~own] == 0)                                              # slots the residue does not own, padded residues
    crd = crd.double()
    stored = c64.float().double()
    worst = 0.0
    for b, n in enumerate(lens):
        o = own[b]
        err = float((crd[b] - c64[b]).abs()[o].max())
        yard = max(float((c32[b].double() - c64[b]).abs()[o].max()), float((stored[b] - c64[b]).abs()[o].max()))
        show(f"forward/{'bb' if backbone_only else 'full'}", f"{name} len {n} #{b}", err, yard, err / yard)
        worst = max(worst, err / yard)
        assert err <= bound(FWD_RATIO[backbone_only], yard, coord_tol(n)), (b, n, err, yard)
    print(f"MEASURED worst forward ratio ({name}, backbone_only={backbone_only}): {worst:.2f}")
    # init_bb: N and CA are constants, C = CA + 1.498 (cos(pi - a), sin(pi - a), 0) with a = ang[0, 3].  The kernel's C.xy may differ
    # from the fp64 formula by pi_f32 - pi (8.8e-8) and the rounding of pi - a (6e-8), both times 1.498, cosf / sinf (2 ulp of 1,
    # 2.4e-7, times 1.498), and the roundings of the product (9e-8) and of the sum (1.2e-7): 7.9e-7 in all; bar 1e-6
    per = 3 if backbone_only else 14
    first = crd.reshape(B, L, per, 3)[:, 0, :3].numpy()
    f32 = lambda v: float(np.float32(v))                                         # noqa: E731
    assert np.all(first[:, 0] == [0.0, 0.0, f32(0.001)])
    assert np.all(first[:, 1] == [f32(BL_N_CA), 0.0, f32(0.001)])
    a03 = ang[:, 0, 3].double().numpy()
    c_ref = np.stack([f32(BL_N_CA) + np.cos(math.pi - a03) * BL_CA_C, np.sin(math.pi - a03) * BL_CA_C], -1)
    assert np.all(first[:, 2, 2] == f32(0.001)) and np.abs(first[:, 2, :2] - c_ref).max() <= 1e-6


# --------------------------------------------------------------------------- 2. forward, per placement
def test_types_batch_covers_every_type_at_every_edge():
    _, _, _, seq = make_inputs("types")
    for pos in TYPE_POSITIONS:
        assert set(seq[:, pos].tolist()) == set(range(20)), pos
    assert TYPE_POSITIONS[-1] == L_TYPES - 1


def test_forward_internal_coordinates(dev):
    from protein_transformer_amd.protein.Structure import nerf_forward
    names = ("bond", "angle", "torsion")
    for name, which in (("types", range(20)), ("ragged", [RAGGED_LENS.index(130)])):
        ref = reference(name)
        if name == "types":
            for pos in TYPE_POSITIONS:
                assert set(ref["seq"][:, pos].tolist()) == set(range(20)), pos
        crd, status = nerf_forward(ref["ang"].to(dev), ref["seq"].to(dev))
        assert int(status.item()) == 0
        crd = crd.cpu().numpy()
        ang, seq = ref["ang"].numpy(), ref["seq"].numpy()
        errs = np.zeros((3, 3))                                                   # [kernel, fp32 oracle, stored fp64][bond, angle, torsion]
        for b in which:
            for row, c in enumerate((crd[b], ref["crd32"][b].numpy(), ref["crd64"][b].float().numpy())):
                ic = nerf_ref.internal_coordinates(c, seq[b], ang[b])
                errs[row] = np.maximum(errs[row], [e.max() for e in nerf_ref.internal_errors(ic)])
        for q, qn in enumerate(names):
            yard = max(errs[1, q], errs[2, q])
            show(f"internal/{qn}", f"{name} ({len(which)} proteins)", errs[0, q], yard, errs[0, q] / yard)
            print(f"         fp32 oracle {errs[1, q]:.3e}, fp64 coordinates stored as fp32 {errs[2, q]:.3e}")
            assert errs[0, q] <= bound(IC_RATIO[qn], yard, IC_CEILING), (name, qn, errs[:, q])


# --------------------------------------------------------------------------- 3. adjoint, dense upstream gradient
def structural_zeros(seq, lens, L):
    """the angle entries that sum(w crd) cannot depend on, whatever w: padding, phi and N-CA-C of residue 0, omega / CA-C-N /
    C-N-CA of the last residue, chi columns that no predicted torsion of the residue type reads"""
    z = np.zeros((len(lens), L, 12), bool)
    for b, n in enumerate(lens):
        z[b, n:] = True
        z[b, 0, [0, 3]] = True
        z[b, n - 1, [2, 4, 5]] = True
        for i in range(n):
            used = {6 + min(k, 5) for k, at in enumerate(SC_PROGRAM[int(seq[b, i])]) if at[2] == "p"}
            z[b, i, [c for c in range(6, 12) if c not in used]] = True
    return z


@pytest.mark.parametrize("backbone_only", [False, True], ids=["full", "backbone"])
@pytest.mark.parametrize("name", ["ragged", "types"])
def test_adjoint_dense_per_angle(dev, name, backbone_only):
    from protein_transformer_amd.protein.Structure import nerf_backward
    ref = reference(name)
    lens, L, ang, seq = ref["lens"], ref["L"], ref["ang"], ref["seq"]
    crd, w = ref["crd64"].float(), ref["w"]
    g64, g32 = (ref["gbb64"], ref["gbb32"]) if backbone_only else (ref["g64"], ref["g32"])
    if backbone_only:
        crd, w = compact(crd), compact(w)
    dang = nerf_backward(ang.to(dev), seq.to(dev), crd.to(dev), w.to(dev), backbone_only=backbone_only).cpu()
    zero = g64 == 0
    sz = torch.from_numpy(structural_zeros(seq.numpy(), lens, L))
    assert torch.all(zero[sz])                                                    # the reference agrees that these are zeros ...
    if backbone_only:
        assert torch.all(zero[:, :, 6:]) and all(bool(zero[b, n - 1, 1]) for b, n in enumerate(lens))
    else:
        assert torch.equal(zero, sz)                                              # ... and, with every atom weighted, has no other
    assert torch.all(dang[zero] == 0)                                             # exact zeros where the reference has exact zeros
    worst = 0.0
    for b, n in enumerate(lens):
        top = float(g64[b].abs().max())
        err = float((dang[b].double() - g64[b]).abs().max()) / top
        yard = max(float((g32[b].double() - g64[b]).abs().max()) / top, EPS32)
        show(f"adjoint/{'bb' if backbone_only else 'full'}", f"{name} len {n} #{b}", err, yard, err / yard)
        worst = max(worst, err / yard)
        assert err <= bound(ADJ_RATIO[backbone_only], yard, GRAD_CEILING), (b, n, err, yard)
    print(f"MEASURED worst adjoint ratio ({name}, backbone_only={backbone_only}): {worst:.2f}")


# --------------------------------------------------------------------------- 4. adjoint, one atom at a time
def probe_atoms(seq, n):
    out = []
    for i in sorted({0, 1, 2, 63, 64, 65, n - 2, n - 1}):
        if 0 <= i < n:
            nsc = len(SC_PROGRAM[int(seq[i])])
            out += [(i, s) for s in sorted({0, 1, 2, 3} | ({4} if nsc else set()) | ({3 + nsc} if nsc else set()))]
    return out


@pytest.mark.parametrize("name", ["ragged", "types"], ids=["len130", "len66"])
def test_adjoint_one_atom_at_a_time(dev, name):
    from protein_transformer_amd.protein.Structure import nerf_backward
    ref = reference(name)
    if name == "ragged":
        b = RAGGED_LENS.index(130)
    else:
        b = int(np.nonzero(ref["seq"][:, 64].numpy() == 18)[0][0])                # the protein with a TRP at residue 64
    n, L, ang, seq = ref["lens"][b], ref["L"], ref["ang"][b], ref["seq"][b]
    probes = probe_atoms(seq.numpy(), n)
    P = len(probes)
    assert 24 <= P <= 48 and (0, 4) in probes and (64, 0) in probes and (n - 1, 3) in probes
    w = torch.from_numpy(np.random.default_rng(3).normal(size=(P, 3)).astype(np.float32))
    rows64, crd64 = nerf_ref.jacobian_rows(ang, seq, probes, w, torch.float64)
    rows32, _ = nerf_ref.jacobian_rows(ang, seq, probes, w, torch.float32)
    assert float((crd64 - ref["crd64"][b]).abs().max()) < 1e-10
    support = rows64 != 0
    if name == "types":                                                           # the graph, not these angles, decides the support
        sets = nerf_ref.support_sets(seq, n, probes)
        for p in range(P):
            assert sets[p] == set(zip(*(nerf_ref.int_list(v) for v in np.nonzero(support[p].numpy())))), probes[p]
    flat = torch.tensor([i * 14 + s for i, s in probes])
    dcrd = torch.zeros(P, L * 14, 3)
    dcrd[torch.arange(P), flat] = w
    rep = lambda t: t[None].expand(P, *t.shape).contiguous().to(dev)             # noqa: E731
    crd = crd64.float()
    dang = nerf_backward(rep(ang), rep(seq), rep(crd), dcrd.to(dev)).cpu()
    for p in range(P):
        assert torch.all(dang[p][~support[p]] == 0), (probes[p], torch.nonzero(dang[p] * ~support[p])[:4].tolist())
    worst = 0.0
    for p, (i, s) in enumerate(probes):
        if not bool(support[p].any()):
            assert i == 0 and s < 3                                               # N, CA, C of residue 0: constants of the build
            continue
        top = float(rows64[p].abs().max())
        err = float((dang[p].double() - rows64[p]).abs().max()) / top
        yard = max(float((rows32[p].double() - rows64[p]).abs().max()) / top, EPS32)
        show("probe", f"len {n} atom ({i}, {s})", err, yard, err / yard)
        worst = max(worst, err / yard)
        assert err <= bound(PROBE_RATIO, yard, GRAD_CEILING), (probes[p], err, yard)
    print(f"MEASURED worst probe ratio (len {n}): {worst:.2f}")
    # linearity: the rows add up to the kernel's answer for the summed upstream gradient
    total = nerf_backward(ang[None].to(dev), seq[None].to(dev), crd[None].to(dev), dcrd.sum(0, keepdim=True).to(dev)).cpu()[0]
    ref_sum, ref32_sum = rows64.sum(0), rows32.double().sum(0)
    top = float(ref_sum.abs().max())
    err = float((total.double() - dang.double().sum(0)).abs().max()) / top
    yard = max(float((ref32_sum - ref_sum).abs().max()) / top, EPS32)
    show("probe sum", f"len {n}", err, yard, err / yard)
    assert err <= bound(PROBE_RATIO, yard, GRAD_CEILING), (err, yard)
    assert torch.all(total[~support.any(0)] == 0)


# --------------------------------------------------------------------------- 5. padding and batch position
def test_padding_and_batch_position_change_no_bit(dev):
    from protein_transformer_amd.protein.Structure import nerf_backward, nerf_forward
    ref = reference("ragged")
    b0, n = RAGGED_LENS.index(65), 65
    rng = np.random.default_rng(4)
    ang0, seq0 = ref["ang"][b0, :n], ref["seq"][b0, :n]
    w0 = torch.from_numpy(rng.normal(size=(n, 14, 3)).astype(np.float32))

    def run(L, lens, at):
        """the protein as number `at` of a batch of `lens` proteins padded to L; garbage angles and upstream gradients behind every
        protein's end -> its rows of (crd, crd_bb, dang, dang_bb), and whether everything behind its end is zero"""
        other = synthetic.make_batch(lens, L_pad=L, seed=9)
        ang = torch.from_numpy(rng.uniform(-3.0, 3.0, (len(lens), L, 12)).astype(np.float32))
        live = (other["seq"] != 20)[:, :, None]
        ang = torch.where(live, other["start_ang_rad"], ang)
        seq = other["seq"].clone()
        w = torch.from_numpy(rng.normal(size=(len(lens), L, 14, 3)).astype(np.float32))
        assert lens[at] == n
        ang[at, :n], seq[at, :n], w[at, :n] = ang0, seq0, w0
        ang, seq, w = ang.to(dev), seq.to(dev), w.to(dev)
        crd, st = nerf_forward(ang, seq)
        bb, st_bb = nerf_forward(ang, seq, backbone_only=True)
        assert int(st.item()) == 0 and int(st_bb.item()) == 0
        w_bb = w[:, :, :3].reshape(len(lens), L * 3, 3).contiguous()
        dang = nerf_backward(ang, seq, crd, w.reshape(len(lens), L * 14, 3))
        dang_bb = nerf_backward(ang, seq, bb, w_bb, backbone_only=True)
        outs = [t[at].cpu().reshape(L, -1) for t in (crd, bb, dang, dang_bb)]
        assert all(bool(torch.all(t[n:] == 0)) for t in outs)
        return [t[:n] for t in outs]

    base = run(65, [65], 0)
    assert all(bool(t.abs().max() > 0) for t in base)
    for L, lens, at in ((66, [65], 0), (128, [65], 0), (128, [65, 40, 128, 2, 77, 100], 0), (128, [90, 40, 128, 2, 77, 65], 5)):
        for what, t, t0 in zip(("crd", "crd_bb", "dang", "dang_bb"), run(L, lens, at), base):
            assert torch.equal(t, t0), (L, lens, at, what, float((t - t0).abs().max()))


# --------------------------------------------------------------------------- 6. atan2 and its adjoint
# Bars, stated and not measured.  angle: 6 ulp of the result - what OpenCL asks of atan2 in single precision, the loosest figure
# documented for a conforming device atan2f (the device library serves HIP and OpenCL alike; CUDA documents 2 ulp); the inputs
# are fp32 numbers, so the fp64 atan2 of them is the exact reference.
# gradient (-y, x) g / (x^2 + y^2): in units of 2^-24 relative, x^2, y^2 and their sum lose 1 each but the sum of two positive
# terms carries at most the larger relative error: 2; the reciprocal at most 2.5 ulp = 5 where it is not correctly rounded; two
# products 1 each: 9 units = 4.5 ulp; bar 5 ulp relative (5 * 2^-23 |reference|).  (0, 0): angle 0 and gradient (0, 0), exactly.
ATAN2_ULPS, ATAN2_GRAD_REL = 6, 5 * 2.0 ** -23


def atan2_inputs(n, rng):
    phi = rng.uniform(-math.pi, math.pi, n)
    r = 10.0 ** rng.uniform(-3, 3, n)
    xy = np.stack([r * np.cos(phi), r * np.sin(phi)], -1).astype(np.float32)
    special = np.array([[0, 0], [1, 0], [0, 1], [-1, 0], [0, -1], [1e-3, 0], [0, 1e3], [-1e3, 0], [0, -1e-3],
                        [1, 1], [-1, 1], [-1, -1], [1, -1], [1e3, 1e-3], [-1e-3, 1e3], [0, 0]], np.float32)
    k = min(n, len(special))
    xy[rng.permutation(n)[:k]] = special[:k]
    return xy


@pytest.mark.parametrize("n", [1, 255, 256, 257, 12 * 130 * 3])
def test_atan2_and_its_adjoint(dev, n):
    from protein_transformer_amd.losses import angles_backward, angles_forward
    rng = np.random.default_rng(n)
    xy = atan2_inputs(n, rng)
    if n > 16:
        quadrants = {(bool(x > 0), bool(y > 0)) for x, y in xy if x != 0 and y != 0}
        assert len(quadrants) == 4 and np.any((xy == 0).all(1)) and np.any((xy[:, 0] == 0) & (xy[:, 1] != 0))
        r = np.hypot(*xy.astype(np.float64).T)
        assert r[r > 0].min() < 2e-3 and r.max() > 5e2
    g = rng.normal(size=n).astype(np.float32)
    sincos = torch.from_numpy(xy).reshape(n, 2)
    ang = angles_forward(sincos.to(dev)).cpu().numpy().reshape(n)
    dsc = angles_backward(sincos.to(dev), torch.from_numpy(g).reshape(n, 1).to(dev)).cpu().numpy().reshape(n, 2)
    x, y = xy[:, 0].astype(np.float64), xy[:, 1].astype(np.float64)
    ref = np.arctan2(y, x)
    ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
    origin = (x == 0) & (y == 0)
    assert np.all(ang[origin] == 0) and np.all(dsc[origin] == 0)
    assert np.all(ang[(y == 0) & (x > 0)] == 0)
    over = np.abs(ang - ref) / ulp
    print(f"MEASURED atan2 n = {n}: worst angle error {over[~origin].max() if (~origin).any() else 0.0:.2f} ulp")
    assert np.all(np.abs(ang - ref)[~origin] <= ATAN2_ULPS * ulp[~origin])
    r2 = np.where(origin, 1.0, x * x + y * y)
    gref = np.stack([-y / r2, x / r2], -1) * g[:, None].astype(np.float64)
    gref[origin] = 0
    rel = np.abs(dsc - gref) / np.maximum(np.abs(gref), 1e-300)
    print(f"MEASURED atan2 n = {n}: worst gradient error {rel[gref != 0].max() / 2.0 ** -23 if (gref != 0).any() else 0.0:.2f} ulp")
    assert np.all(np.abs(dsc - gref) <= ATAN2_GRAD_REL * np.abs(gref))
    assert np.all(np.sign(dsc) == np.sign(gref.astype(np.float32)))
