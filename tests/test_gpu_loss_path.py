"""MI355X parity tests for the geometry + loss kernels (NeRF fwd/bwd, atan2, dRMSD, angle MSE).

The HIP path (through the C ABI of libptamd.so) is compared with
  * the golden vectors captured from the reference (tests/golden/*.npz),
  * the CPU oracle (oracle/) on seeded inputs,
  * size-independent properties at the full benchmark size (B=32, L=512).
Stated fp32 tolerances: coordinates 2e-3 A * max(1, L/128) (two fp32 NeRF chains drift apart like
that: the reference itself is 8e-4 A (L=128) / 5.9e-3 A (L=512) away from an fp64 run of its own
formulas); per-protein drmsd rel 1e-4; lndrmsd abs 1e-6; angle gradients
rel-L2 1e-3.
"""
import os

import numpy as np
import pytest
import torch
from pytest import approx

pytestmark = pytest.mark.gpu

AA = "ACDEFGHIKLMNPQRSTVWY"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def ids(s):
    return torch.tensor([AA.index(c) for c in s])


def coord_tol(L):
    return 2e-3 * max(1.0, L / 128)


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


# --------------------------------------------------------------------------- NeRF forward
def test_generate_coords_golden(golden, dev):
    from protein_transformer_amd.protein.Structure import generate_coords
    g = golden("g2_coords")
    worst = 0.0
    for n in range(int(g["n"])):
        s = str(g[f"seq{n}"])
        crd = generate_coords(torch.tensor(g[f"ang{n}"]).to(dev), ids(s).to(dev)).cpu().numpy()
        assert crd.shape == (len(s) * 14, 3)
        err = np.abs(crd - g[f"crd{n}"]).max()
        worst = max(worst, err / coord_tol(len(s)))
        assert err < coord_tol(len(s)), f"case {n} L={len(s)} err={err}"
        # unused slots are exactly zero, like stack_coords pads them
        assert np.array_equal(crd == 0, g[f"crd{n}"] == 0)
    crd = generate_coords(torch.tensor(g["ka2_ang"]), "GAS").cpu().numpy()
    assert np.abs(crd - g["ka2_crd"]).max() < 1e-5
    print("worst coordinate error / tolerance:", worst)


def test_nerf_golden(golden, dev):
    from protein_transformer_amd.protein.Structure import nerf
    g = golden("g1_nerf")
    d = nerf(g["a"], g["b"], g["c"], g["l"], g["theta"], g["chi"]).cpu().numpy()
    assert np.abs(d - g["d"]).max() < 2e-6
    ka1 = nerf([0, 0, .001], [1.442, 0, .001], [2.0, 1.39, .001], 1.229, 2.0944, 0.5).cpu().numpy()
    assert ka1 == approx([1.362117, 2.308242, 0.511273], abs=2e-6)
    with pytest.raises(AssertionError):
        nerf([0., 0, 0], [1., 1, 1], [1., 2, 0], 1.0, 3.5, 0.0)


def test_pairwise_internal_dist(golden, dev):
    # reference tests/test_losses.py:123-150
    from protein_transformer_amd.losses import pairwise_internal_dist
    g = golden("g3_drmsd")
    for n in range(3):
        out = pairwise_internal_dist(torch.tensor(g[f"pid_in{n}"])).cpu().numpy()
        ref = g[f"pid_out{n}"]
        off = ~np.eye(len(ref), dtype=bool)
        assert np.allclose(out[off], ref[off], rtol=1e-4, atol=1e-4)          # the reference's own formula cancels
        assert np.all(np.diag(out) < 1e-6)
    a = torch.tensor([[5.3, -15.2, 300], [-3.3, 234.1, 0]])
    assert pairwise_internal_dist(a)[0, 1].item() == approx(390.15951865, rel=1e-6)


def test_generate_coords_errors(dev):
    from protein_transformer_amd.protein.Structure import generate_coords
    with pytest.raises(StopIteration):
        generate_coords(torch.zeros(1, 12), torch.tensor([0]))
    with pytest.raises(KeyError):
        generate_coords(torch.zeros(3, 12), torch.tensor([0, 21, 1]))
    with pytest.raises(AssertionError):
        a = torch.zeros(3, 12)
        a[1, 4] = 3.5
        generate_coords(a, torch.tensor([0, 1, 2]))


def test_sidechain_table_matches_oracle():
    from oracle.geometry import SC_PROGRAM
    from protein_transformer_amd import _lib
    for r in range(20):
        assert _lib.lib().ptamd_sidechain_atoms(r) == len(SC_PROGRAM[r])
    assert _lib.lib().ptamd_sidechain_atoms(20) == -1


# --------------------------------------------------------------------------- NeRF backward
def test_nerf_backward_vs_oracle_autograd(dev):
    from oracle import batched
    from protein_transformer_amd import synthetic
    from protein_transformer_amd.protein.Structure import nerf_backward, nerf_forward
    lens = [40, 33, 64, 2, 17, 20]
    batch = synthetic.make_batch(lens, L_pad=64, seed=5)
    batch["seq"][5, :20] = ids(AA)              # every residue type once, incl. as first/last
    ang = batch["start_ang_rad"]
    seq = batch["seq"]
    a64 = ang.double().clone().requires_grad_()
    crd64 = batched.generate_coords_batched(a64, seq, torch.float64)
    w = torch.from_numpy(np.random.default_rng(0).normal(size=crd64.shape))
    (crd64 * w).sum().backward()
    crd, _ = nerf_forward(ang.to(dev), seq.to(dev))
    assert np.abs(crd.cpu().numpy() - crd64.detach().numpy()).max() < coord_tol(64)
    dang = nerf_backward(ang.to(dev), seq.to(dev), crd, w.float().to(dev)).cpu().numpy()
    ref = a64.grad.numpy()
    for b in range(len(lens)):
        assert rel_l2(dang[b], ref[b]) < 1e-3, (b, rel_l2(dang[b], ref[b]))
        assert np.all(dang[b, lens[b]:] == 0)
    # graph quirks of the reference: first residue's phi and N-CA-C angle get no gradient,
    # nor do the last residue's omega / CA-C-N / C-N-CA
    assert np.all(dang[0, 0, [0, 3]] == 0)
    assert np.all(dang[0, lens[0] - 1, [2, 4, 5]] == 0)


# --------------------------------------------------------------------------- dRMSD
def test_drmsd_golden(golden, dev):
    from protein_transformer_amd.losses import drmsd
    g = golden("g3_drmsd")
    for n in range(int(g["n"])):
        d = drmsd(torch.tensor(g[f"a{n}"]).float().to(dev), torch.tensor(g[f"b{n}"]).float().to(dev)).item()
        assert d == approx(float(g[f"drmsd{n}"]), rel=1e-5)


def test_drmsd_zero_and_permutation(dev):
    # reference tests/test_losses.py:153-174
    from protein_transformer_amd.losses import drmsd
    a = torch.tensor([[0, 0, 0], [0, 1, 0], [0, 0, 2], [0, 0, 0]], dtype=torch.float)
    b = torch.tensor([[0, 0, 2], [0, 1, 0], [0, 0, 0], [0, 0, 0]], dtype=torch.float)
    assert drmsd(a, a).item() == 0
    assert drmsd(a, b).item() != 0


def test_drmsd_equals_lazy_drmsd(dev):
    # reference tests/test_losses.py:58-89
    from protein_transformer_amd.losses import drmsd
    rng = np.random.default_rng(3)
    for x, y in ((np.array([[0, 0, 0], [3, 5, 2], [2, 9, 3]]), np.array([[0, 0, 0], [9, 3, 1], [4, 7, 8]])),
                 (rng.random((50, 3)) * 10, rng.random((50, 3)) * 10)):
        n = len(x)
        da = [np.linalg.norm(x[i] - x[j]) for i in range(n) for j in range(i + 1, n)]
        db = [np.linalg.norm(y[i] - y[j]) for i in range(n) for j in range(i + 1, n)]
        lazy = np.sqrt(np.mean((np.array(da) - np.array(db)) ** 2))
        assert drmsd(torch.tensor(x).float(), torch.tensor(y).float()).item() == approx(lazy, rel=1e-5)


def test_drmsd_gradient_vs_autograd(dev):
    from oracle import batched
    from protein_transformer_amd.losses import drmsd
    rng = np.random.default_rng(11)
    a = torch.tensor(rng.normal(0, 8, (300, 3)))
    b = torch.tensor(rng.normal(0, 8, (300, 3)))
    a64 = a.clone().requires_grad_()
    batched.drmsd_direct(a64, b).backward()
    ag = a.float().to(dev).requires_grad_()
    drmsd(ag, b.float().to(dev)).backward()
    assert rel_l2(ag.grad.cpu().numpy(), a64.grad.numpy()) < 1e-4


def test_drmsd_does_not_depend_on_the_batch_it_is_cut_for(dev):
    """The pair kernel cuts a protein's triangle into work items of 16, 8 or 4 column tiles by the occupancy of the WHOLE
    batch (drmsd.hip, tri_layout: 32 / 16 / 4 proteins x 512 residues take 16 / 8 / 4), and the finalize kernel adds the items'
    partials in a fixed order: per-protein losses and gradients of the same proteins must agree to rounding whatever
    batch they are computed in, and be identical from run to run."""
    from protein_transformer_amd.losses import drmsd_forward_backward
    B, L = 32, 512
    g = torch.Generator().manual_seed(17)
    pred = (torch.randn(B, L * 14, 3, generator=g) * 12).to(dev)
    true = (torch.randn(B, L * 14, 3, generator=g) * 12)
    true[torch.rand(B, L * 14, generator=g) < 0.3] = float("nan")          # absent atoms
    true = true.to(dev)
    seq = torch.randint(0, 20, (B, L), generator=g)
    seq[1, 400:] = 20
    seq[2, 77:] = 20
    seq = seq.to(dev)
    ref_s, ref_g = drmsd_forward_backward(pred, true, seq)
    ref_s, ref_g = ref_s.clone(), ref_g.clone()
    again_s, again_g = drmsd_forward_backward(pred, true, seq)
    assert torch.equal(again_s, ref_s) and torch.equal(again_g, ref_g)
    for nb in (16, 4):
        s_, g_ = drmsd_forward_backward(pred[:nb].contiguous(), true[:nb].contiguous(), seq[:nb].contiguous())
        assert torch.allclose(s_, ref_s[:nb], rtol=2e-6, atol=0), nb
        scale = ref_g[:nb].abs().max().item()
        assert torch.allclose(g_, ref_g[:nb], rtol=1e-4, atol=2e-6 * scale), nb


def test_drmsd_work_golden(golden, dev):
    from protein_transformer_amd.losses import drmsd_work
    g = golden("g4_drmsd_work")
    for b in range(4):
        r = drmsd_work(g["pred_ang"][b], g["true_crd"][b], g["seq"][b])
        vals = g[f"vals{b}"]
        assert r[1] == approx(vals[0], rel=1e-4)
        assert r[2] == approx(vals[1], abs=1e-6)
        assert r[3] == approx(vals[2], rel=1e-4)
        assert r[4] == approx(vals[3], abs=1e-6)
        assert rel_l2(r[0].numpy(), g[f"grad{b}"]) < 1e-3
    r = drmsd_work(torch.tensor(g["ka4_ang"]), torch.tensor(g["ka4_crd"]), torch.tensor(g["ka4_seq"]))
    assert r[1:] == approx((0.8574336, 0.0571622, 0.9411135, 0.1045682), abs=2e-5)
    grad = r[0].numpy()
    assert rel_l2(grad, g["ka4_grad"]) < 1e-3
    assert np.all(grad[3:] == 0)
    assert set(np.nonzero(grad[0] == 0)[0]) == {0, 3, 6, 7, 8, 9, 10, 11}
    assert set(np.nonzero(grad[2] == 0)[0]) == {2, 4, 5, 8, 9, 10, 11}


def test_batch_loss_vs_oracle_ragged(dev):
    """Ragged batch with missing residues: HIP loss path vs the serial CPU oracle."""
    from oracle import geometry, losses as olosses
    from protein_transformer_amd import synthetic
    from protein_transformer_amd.losses import batch_loss
    lens = [31, 64, 2, 47, 20, 9]
    build = lambda ang, seq: torch.stack([                                     # noqa: E731
        torch.cat([geometry.generate_coords(ang[b, :n], seq[b, :n]), torch.zeros((seq.shape[1] - n) * 14, 3)])
        for b, n in enumerate(lens)])
    batch = synthetic.make_batch(lens, L_pad=64, seed=21, build_coords=build, frac_missing=0.1)
    ang, seq, crd = batch["start_ang_rad"], batch["seq"], batch["true_crd"]
    sincos = torch.stack([torch.cos(ang), torch.sin(ang)], -1).reshape(len(lens), 64, 24) * 0.9
    stats, grad, status = batch_loss(sincos.to(dev), crd.to(dev), seq.to(dev), do_backward=True)[:3]
    assert int(status.item()) == 0
    stats = stats.cpu().numpy()
    for b in range(len(lens)):
        sc = sincos[b].clone().requires_grad_()
        a = olosses.inverse_trig_transform(sc[None])[0]
        a.retain_grad()
        g, d, ln, dbb, lnbb = olosses.drmsd_work(a.detach().numpy(), crd[b].numpy(), seq[b].numpy())
        assert stats[b, 0] == approx(d, rel=1e-4), b
        assert stats[b, 1] == approx(ln, abs=1e-6), b
        assert stats[b, 2] == approx(dbb, rel=1e-4), b
        assert stats[b, 3] == approx(lnbb, abs=1e-6), b
        a.backward(gradient=g)
        assert rel_l2(grad[b].cpu().numpy(), sc.grad.numpy()) < 1e-3, b


def test_batch_loss_result_fields_under_every_keyword_combination(dev):
    """BatchLoss: under each legal combination of the keywords exactly the documented fields are set, with the documented shapes
    and dtypes, and without `rename_symmetric` the truth comes back as the very objects that were passed."""
    import itertools
    from protein_transformer_amd.losses import BatchLoss, batch_loss
    B, L = 2, 8
    g = torch.Generator().manual_seed(5)
    seq = torch.randint(0, 20, (B, L), generator=g)
    seq[0, :4] = torch.tensor([2, 3, 4, 19])                        # (ASP, GLU, PHE, TYR: something to rename)
    seq[1, 5:] = 20                                                 # one protein of 5 residues, padded
    crd = torch.randn(B, L * 14, 3, generator=g) * 5
    crd[0, [3, 30, 33]] = float("nan")                              # a few missing atoms
    crd[1, 5 * 14:] = 0
    ang = torch.randn(B, L, 24, generator=g)
    ang[1, 5:] = 0
    pred, seq, crd, ang = torch.randn(B, L, 24, generator=g).to(dev), seq.to(dev), crd.to(dev), ang.to(dev)
    f32 = torch.float32
    cases = [dict(backbone_only=True)] + [
        dict(**loss, **clash, **rename) for loss, clash, rename in itertools.product(
            ({}, dict(slddt=(15.0, 1.0)), dict(fape=10.0)), ({}, dict(clash=(0.5, 1.5))),
            ({}, dict(rename_symmetric=True), dict(rename_symmetric=True, true_ang=ang), dict(true_ang=ang)))]
    for kw, do_backward in itertools.product(cases, (True, False)):
        res = batch_loss(pred, crd, seq, do_backward=do_backward, **kw)
        want = {"stats": ((B, 8), f32), "status": ((1,), torch.int32), "true_crds": ((B, L * 14, 3), f32),
                "crd": ((B, L * (3 if kw.get("backbone_only") else 14), 3), f32)}
        if do_backward:
            want["grad"] = ((B, L, 24), f32)
        if "slddt" in kw or "fape" in kw:
            want["per_protein"] = ((B,), f32)
        if "true_ang" in kw:
            want["true_ang"] = ((B, L, 24), f32)
        if "clash" in kw:
            want["clash"] = ((B,), f32)
        assert type(res) is BatchLoss and res._fields == ("stats", "grad", "status", "crd", "per_protein", "true_crds", "true_ang",
                                                          "clash")
        got = {f: (tuple(v.shape), v.dtype) for f, v in res._asdict().items() if v is not None}
        assert got == want, (kw, do_backward)
        if kw.get("rename_symmetric"):
            assert res.true_crds is not crd and res.true_ang is not ang
        else:
            assert res.true_crds is crd and res.true_ang is kw.get("true_ang")


# --------------------------------------------------------------------------- full benchmark size
def test_full_size_properties(dev):
    """B=32, L=512 (BASELINE config 4): properties that do not need the slow serial oracle, plus
    the vectorised fp64 oracle for values and gradients."""
    from oracle import batched
    from protein_transformer_amd import synthetic
    from protein_transformer_amd.losses import batch_loss, drmsd_forward_backward
    from protein_transformer_amd.protein.Structure import nerf_forward
    B, L = 32, 512
    hip_build = lambda ang, seq: nerf_forward(ang.to(dev), seq.to(dev))[0]      # noqa: E731
    batch = synthetic.make_batch([L] * B, seed=synthetic.DEFAULT_SEED, build_coords=hip_build)
    seq, true_crd = batch["seq"].to(dev), batch["true_crd"].to(dev)
    crd, status = nerf_forward(batch["true_ang_rad"].to(dev), seq)
    assert int(status.item()) == 0
    c = crd.view(B, L, 14, 3)
    # bond lengths along the chain are the force-field constants (SidechainBuildInfo.py:576-580)
    assert (c[:, :, 1] - c[:, :, 0]).norm(dim=-1).sub(1.442).abs().max() < 2e-4
    assert (c[:, :, 2] - c[:, :, 1]).norm(dim=-1).sub(1.498).abs().max() < 2e-4
    assert (c[:, 1:, 0] - c[:, :-1, 2]).norm(dim=-1).sub(1.379).abs().max() < 2e-4
    assert (c[:, :, 3] - c[:, :, 2]).norm(dim=-1).sub(1.229).abs().max() < 2e-4
    # a structure against itself: zero loss
    stats, _ = drmsd_forward_backward(crd, true_crd, seq, need_grad=False)
    assert float(stats[:, 0].abs().max()) == 0.0
    n_expected = synthetic.slot_mask(batch["seq"]).sum(1).float()
    assert torch.equal(stats[:, 4].cpu(), n_expected)
    assert torch.equal(stats[:, 5].cpu(), torch.full((B,), 3.0 * L))
    # rigid motion invariance of the loss: rotate + translate the truth
    q, _ = torch.linalg.qr(torch.randn(3, 3, dtype=torch.float64))
    moved = (true_crd.double() @ q.to(dev) + 7.5).float()
    sincos = torch.stack([torch.cos(batch["start_ang_rad"]), torch.sin(batch["start_ang_rad"])], -1).reshape(B, L, 24)
    s1, g1, _ = batch_loss(sincos.to(dev), true_crd, seq)[:3]
    s2, g2, _ = batch_loss(sincos.to(dev), moved, seq)[:3]
    assert torch.allclose(s1[:, :4], s2[:, :4], rtol=2e-4, atol=1e-6)
    # values and gradients against the vectorised fp64 oracle on a 4-protein slice
    sub = slice(0, 4)
    st64, crd64, g64 = batched.batch_loss_and_grads(batch["start_ang_rad"][sub], batch["seq"][sub],
                                                    batch["true_crd"][sub], torch.float64)
    dang_hip = None
    from protein_transformer_amd.losses import angles_forward, nerf_backward
    ang = angles_forward(sincos[sub].to(dev))
    crd_p, _ = nerf_forward(ang, seq[sub])
    assert np.abs(crd_p.cpu().numpy() - crd64.numpy()).max() < coord_tol(L)
    stats_p, dcrd = drmsd_forward_backward(crd_p, true_crd[sub], seq[sub])
    dang_hip = nerf_backward(ang, seq[sub], crd_p, dcrd).cpu().numpy()
    for b in range(4):
        assert float(stats_p[b, 0]) == approx(st64[b][0], rel=1e-4)
        assert float(stats_p[b, 1]) == approx(st64[b][1], abs=1e-6)
        assert float(stats_p[b, 2]) == approx(st64[b][2], rel=1e-4)
        assert rel_l2(dang_hip[b], g64[b].numpy()) < 1e-3


# --------------------------------------------------------------------------- angle MSE / atan2
def test_mse_over_angles_golden(golden, dev):
    from protein_transformer_amd.losses import inverse_trig_transform, mse_over_angles
    g = golden("g8_mse")
    p, t = torch.tensor(g["pred"]).to(dev), torch.tensor(g["true"]).to(dev)
    assert mse_over_angles(p, t).item() == approx(float(g["full"]), rel=1e-5)
    assert mse_over_angles(p, t, bb_only=True).item() == approx(float(g["bb"]), rel=1e-5)
    assert mse_over_angles(p, t, sc_only=True).item() == approx(float(g["sc"]), rel=1e-5)
    out = inverse_trig_transform(torch.tensor(g["itt_in"]).to(dev)).cpu().numpy()
    assert np.abs(out - g["itt_out"]).max() < 1e-6
    # reference tests/test_losses.py:117-120
    a = torch.zeros(8, 10, 24, device=dev)
    assert mse_over_angles(a, a - .1).item() == approx(0.01)


def test_mse_backward_vs_oracle(golden, dev):
    from oracle import losses as olosses
    from protein_transformer_amd.losses import mse_over_angles
    g = golden("g8_mse")
    p = torch.tensor(g["pred"]).requires_grad_()
    olosses.mse_over_angles(p, torch.tensor(g["true"])).backward()
    pg = torch.tensor(g["pred"]).to(dev).requires_grad_()
    mse_over_angles(pg, torch.tensor(g["true"]).to(dev)).backward()
    assert np.allclose(pg.grad.cpu().numpy(), p.grad.numpy(), rtol=1e-5, atol=1e-8)


def test_combine_drmsd_mse():
    # reference tests/test_losses.py:11-19
    from protein_transformer_amd.losses import combine_drmsd_mse
    assert combine_drmsd_mse(0.01, 0.3, 0.5, 1, 1, log=False) == 0.155
    assert combine_drmsd_mse(0.01, 0.6, 0, 1, 1, log=False) == .6
    assert combine_drmsd_mse(0.02, 0.3, 1, 1, 1, log=False) == 0.02
    assert combine_drmsd_mse(0.02, 0.3, 1, 0.02, 1, log=False) == 1


def test_long_ragged_sequences(dev):
    """BASELINE config 5 territory: variable lengths up to 1500 residues (21 000 atom slots per protein)."""
    from oracle import batched
    from protein_transformer_amd import synthetic
    from protein_transformer_amd.losses import angles_forward, drmsd_forward_backward, nerf_backward
    from protein_transformer_amd.protein.Structure import nerf_forward
    lens, L = [1500, 611], 1500          # (round 6: a third chain of 1234 was 40 % of this test's fp64 pair sums and nothing new)
    hip_build = lambda ang, seq: nerf_forward(ang.to(dev), seq.to(dev))[0]      # noqa: E731
    batch = synthetic.make_batch(lens, L_pad=L, seed=77, build_coords=hip_build, frac_missing=0.02)
    seq, true_crd = batch["seq"].to(dev), batch["true_crd"].to(dev)
    start = batch["start_ang_rad"]
    st64, crd64, g64 = batched.batch_loss_and_grads(start, batch["seq"], batch["true_crd"], torch.float64)
    crd, status = nerf_forward(start.to(dev), seq)
    assert int(status.item()) == 0
    assert np.abs(crd.cpu().numpy() - crd64.numpy()).max() < coord_tol(L)
    stats, dcrd = drmsd_forward_backward(crd, true_crd, seq)
    dang = nerf_backward(start.to(dev), seq, crd, dcrd).cpu().numpy()
    for b in range(len(lens)):
        assert float(stats[b, 0]) == approx(st64[b][0], rel=1e-4)
        assert float(stats[b, 1]) == approx(st64[b][1], abs=1e-6)
        assert float(stats[b, 2]) == approx(st64[b][2], rel=1e-4)
        assert int(stats[b, 4]) == st64[b][4] and int(stats[b, 5]) == st64[b][5]
        assert rel_l2(dang[b], g64[b].numpy()) < 1e-3
        assert np.all(dang[b, lens[b]:] == 0)


def test_integration_md_stub_runs(golden, dev):
    """INTEGRATION.md's reference-side binding, EXECUTED as printed: the python block is cut out of the document, pointed at
    the in-tree library (PTAMD_LIB) and its `batch_drmsd_and_grad` run on the inputs of golden set G4 - the per-protein
    losses and angle gradients the REFERENCE's drmsd_work returned for them (tests/golden/make_golden.py).  The stub goes
    through the C ABI only (its own five-entry ctypes table, raw pointers): nothing of protein_transformer_amd is used."""
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "INTEGRATION.md")).read()
    stub = [b for b in re.findall(r"```python\n(.*?)```", text, flags=re.S) if "def batch_drmsd_and_grad" in b]
    assert len(stub) == 1
    old = os.environ.get("PTAMD_LIB")
    os.environ["PTAMD_LIB"] = os.path.join(root, "protein_transformer_amd", "csrc", "libptamd.so")
    try:
        ns = {}
        exec(compile(stub[0], "INTEGRATION.md", "exec"), ns)
    finally:
        if old is None:
            os.environ.pop("PTAMD_LIB", None)
        else:
            os.environ["PTAMD_LIB"] = old
    g = golden("g4_drmsd_work")
    ang = torch.tensor(g["pred_ang"])                                            # [4, 16, 12] radians
    sincos = torch.stack([torch.cos(ang), torch.sin(ang)], -1).reshape(4, 16, 24).to(dev).contiguous()
    stats, dsc = ns["batch_drmsd_and_grad"](sincos, torch.tensor(g["true_crd"]).to(dev).contiguous(),
                                            torch.tensor(g["seq"]).to(dev).contiguous())
    torch.cuda.synchronize()
    stats = stats.cpu().numpy().astype(np.float64)
    d = dsc.cpu().view(4, 16, 12, 2)
    dang = (-torch.sin(ang) * d[..., 0] + torch.cos(ang) * d[..., 1]).numpy()   # chain rule through (cos, sin) at unit radius
    for b in range(4):
        vals = g[f"vals{b}"]
        assert stats[b, 0] == approx(vals[0], rel=1e-4) and stats[b, 1] == approx(vals[1], abs=1e-6)
        assert stats[b, 2] == approx(vals[2], rel=1e-4) and stats[b, 3] == approx(vals[3], abs=1e-6)
        assert rel_l2(dang[b], g[f"grad{b}"]) < 1e-3, b


def test_drmsd_in_passes_is_bit_identical(dev):
    """The fixed-order partial sums of the pair sweep grow as O(n^2 / 256) per protein (1.35 GB at 32 x 1500 in round 4).  Beyond a
    budget the strips are swept in passes over groups of strips with the same buffers (csrc/drmsd.hip `layout`): the workspace of
    (32, 1500) is below 256 MB, and the result - losses and gradient - is bit for bit that of one launch.  Forced here on a
    small batch through the *_budget entry points (the budget is an ARGUMENT: the library reads no environment)."""
    from protein_transformer_amd import _lib, synthetic
    from protein_transformer_amd.losses import drmsd_forward_backward
    from protein_transformer_amd.protein.Structure import nerf_forward
    lib = _lib.lib()
    assert lib.ptamd_drmsd_workspace_bytes(32, 1500) <= 256 << 20
    assert lib.ptamd_drmsd_workspace_bytes(32, 512) <= 200 << 20
    lens = [700, 512, 333, 64, 2]
    build = lambda ang, seq: nerf_forward(ang.to(dev), seq.to(dev))[0]  # noqa: E731
    batch = synthetic.make_batch(lens, L_pad=700, seed=77, build_coords=build, frac_missing=0.05)
    seq, true = batch["seq"].to(dev), batch["true_crd"].to(dev)
    pred = nerf_forward(batch["start_ang_rad"].to(dev), seq)[0]
    one = lib.ptamd_drmsd_workspace_bytes(len(lens), 700)
    assert lib.ptamd_drmsd_workspace_bytes_budget(len(lens), 700, 0) == one
    os.environ["PTAMD_DRMSD_PARTIAL_MB"] = "1"            # (round 5 read this at every call: it must be ignored now)
    try:
        assert lib.ptamd_drmsd_workspace_bytes(len(lens), 700) == one
    finally:
        os.environ.pop("PTAMD_DRMSD_PARTIAL_MB", None)
    s1, g1 = drmsd_forward_backward(pred, true, seq)
    s1, g1 = s1.clone(), g1.clone()
    for mb in (4, 1):
        assert lib.ptamd_drmsd_workspace_bytes_budget(len(lens), 700, mb << 20) < one
        s2, g2 = drmsd_forward_backward(pred, true, seq, partial_budget_bytes=mb << 20)
        torch.cuda.synchronize()
        assert torch.equal(s1, s2) and torch.equal(g1, g2), mb
        s3, _ = drmsd_forward_backward(pred, true, seq, need_grad=False, partial_budget_bytes=mb << 20)
        assert torch.equal(s1, s3)
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
