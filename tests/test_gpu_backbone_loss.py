"""MI355X tests of the backbone-only loss path (`--backbone_loss`): ptamd_nerf_bb_fwd / _bwd, ptamd_drmsd_bb_fwd_bwd and their
host mirror up to `train.train_step`.

Semantics under test: for protein b the atoms are the slots s % 14 < 3 (N, CA, C) whose truth is present, n_bb of them;
drmsd-bb = drmsd over them, lndrmsd-bb = drmsd-bb / n_bb; the injected gradient is d(sum_b lndrmsd-bb_b)/d(pred).

The fp64 reference is assembled HERE from oracle parts: `oracle.losses.inverse_trig_transform` (atan2),
`oracle.batched.generate_coords_batched(..., dtype=torch.float64)` (the build), `oracle.losses.backbone_of` (slots 0..2),
`oracle.batched.drmsd_direct` (the loss) and torch autograd (the gradient).

Tolerances are those the full-atom path is held to (tests/test_gpu_loss_path.py): per-protein dRMSD rel
1e-4, length-normalised abs 1e-6, per-protein gradient rel-L2 < 1e-3 against fp64 autograd, parameter gradients rel-L2 1e-3 on
the whole vector.
"""
import types

import numpy as np
import pytest
import torch
from pytest import approx

pytestmark = pytest.mark.gpu

RAGGED_LENS = [31, 64, 2, 47, 20, 9]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


def bb_loss_fp64(sincos, seq, true_crd):
    """fp64 backbone loss of a batch.  sincos [B, L, 24] fp64 (may be part of a graph), seq [B, L], true_crd [B, L*14, 3] (NaN =
    absent) -> ([(drmsd-bb, lndrmsd-bb, n_bb)] per protein, sum_b lndrmsd-bb_b as a differentiable scalar).  A protein with
    fewer than two present backbone atoms has no pair: (nan, nan, n_bb) and no term in the sum."""
    from oracle import batched
    from oracle import losses as olosses
    B, L = seq.shape
    ang = olosses.inverse_trig_transform(sincos)
    crd = batched.generate_coords_batched(ang, seq, dtype=torch.float64)
    stats, total = [], torch.zeros((), dtype=torch.float64)
    for b in range(B):
        n_res = int((seq[b] != 20).sum())
        p = olosses.backbone_of(crd[b, :n_res * 14])
        t = olosses.backbone_of(true_crd[b, :n_res * 14].double())
        ok = ~torch.isnan(t).any(dim=1)
        n_bb = int(ok.sum())
        if n_bb < 2:
            stats.append((float("nan"), float("nan"), n_bb))
            continue
        d = batched.drmsd_direct(p[ok], t[ok])
        total = total + d / n_bb
        stats.append((d.item(), (d / n_bb).item(), n_bb))
    return stats, total


def bb_reference(sincos, seq, true_crd):
    """-> (per-protein stats, d(sum lndrmsd-bb)/d(sincos) as an fp64 tensor [B, L, 24])"""
    sc = sincos.detach().double().clone().requires_grad_()
    stats, total = bb_loss_fp64(sc, seq, true_crd)
    total.backward()
    return stats, sc.grad.detach()


def ragged_batch():
    """The construction of tests/test_gpu_loss_path.py::test_batch_loss_vs_oracle_ragged."""
    from oracle import geometry
    from protein_transformer_amd import synthetic
    lens = RAGGED_LENS
    build = lambda ang, seq: torch.stack([                                     # noqa: E731
        torch.cat([geometry.generate_coords(ang[b, :n], seq[b, :n]), torch.zeros((seq.shape[1] - n) * 14, 3)])
        for b, n in enumerate(lens)])
    batch = synthetic.make_batch(lens, L_pad=64, seed=21, build_coords=build, frac_missing=0.1)
    ang, seq, crd = batch["start_ang_rad"], batch["seq"], batch["true_crd"]
    sincos = torch.stack([torch.cos(ang), torch.sin(ang)], -1).reshape(len(lens), 64, 24) * 0.9
    return sincos, seq, crd


@pytest.fixture(scope="module")
def ragged(dev):
    sincos, seq, crd = ragged_batch()
    stats64, grad64 = bb_reference(sincos, seq, crd)
    return dict(sincos=sincos, seq=seq, crd=crd, stats64=stats64, grad64=grad64)


def small_model(dev, am, seed, L=48, dm=64, nl=2, nh=4, dff=128, out_std=2e-3):
    """A small enc-only model with the REALISTIC initialisation of the parity record (tests/test_gpu_parity_record.py: output
    weights N(0, 2e-3) around the arctanh of the angle means, LayerNorm parameters off their trivial values), dropout 0.  Every
    random number is drawn on the CPU, so the same weights can be rebuilt without a GPU."""
    from protein_transformer_amd.models.encoder_only import EncoderOnlyTransformer
    from protein_transformer_amd.protein.Sequence import VOCAB
    torch.manual_seed(seed)
    m = EncoderOnlyTransformer(nl, nh, dm, dff, L, VOCAB, am, True, dropout=0.0)
    with torch.no_grad():
        P = dict(m.named_parameters())
        P["output_projection.weight"].normal_(0, out_std)
        for n, p in P.items():
            if "norm.weight" in n:
                p.add_(0.1 * torch.randn_like(p))
            elif "norm.bias" in n:
                p.add_(0.05 * torch.randn_like(p))
    m.set_dropout(0.0)
    if dev is not None:
        m = m.to(dev).train()
    return m


def bb_args(loss="drmsd", clip=1.0):
    return types.SimpleNamespace(loss=loss, combined_drmsd_weight=0.5, backbone_loss=True, clip=clip)


SMALL_LENS = [48, 31, 17, 40]


def small_batch(dev, seed=5):
    from protein_transformer_amd import synthetic
    from protein_transformer_amd.protein.Structure import nerf_forward
    build = lambda ang, seq: nerf_forward(ang.to(dev), seq.to(dev))[0]           # noqa: E731
    batch = synthetic.make_batch(SMALL_LENS, L_pad=48, seed=seed, build_coords=build, frac_missing=0.05)
    return batch


# --------------------------------------------------------------------------- 1. what used to raise
def test_backbone_flag_trains_instead_of_raising(dev):
    """`get_losses(backbone_loss=True, loss="drmsd")`, `compute_batch_drmsd(backbone_only=True)` and
    `drmsd_work(backbone_only=True)` raised NotImplementedError before this path existed."""
    from test_gpu_parity_record import realistic_angle_means
    from protein_transformer_amd.losses import compute_batch_drmsd, drmsd_work
    from protein_transformer_amd.train import get_losses
    batch = small_batch(dev)
    seq, ang, crd = (batch[k].to(dev) for k in ("seq", "true_ang", "true_crd"))
    model = small_model(dev, realistic_angle_means(3), seed=3)
    model.zero_grad()
    out = get_losses(bb_args("drmsd"), model(seq, ang), ang, crd, seq)
    assert isinstance(out, dict) and len([k for k in out if k != "n-residues"]) == 10
    g = model.flat_parameters()[1]
    assert torch.isfinite(g).all() and float(g.abs().max()) > 0
    assert float(out["loss"]) == float(out["drmsd-bb"]) and np.isfinite(float(out["loss"])) and float(out["loss"]) > 0
    # a training step builds no side chains: the `-full` keys carry the backbone values
    assert float(out["drmsd-full"]) == float(out["drmsd-bb"]) and float(out["lndrmsd-full"]) == float(out["lndrmsd-bb"])
    assert float(get_losses(bb_args("lndrmsd"), model(seq, ang), ang, crd, seq, do_backwards=False)["loss"]) \
        == approx(float(out["lndrmsd-bb"]), rel=1e-12)

    model.zero_grad()
    vals = compute_batch_drmsd(model(seq, ang), crd, seq, do_backward=True, backbone_only=True)
    assert len(vals) == 4 and vals[2] == approx(float(out["drmsd-bb"]), rel=1e-6) and vals[0] == vals[2] and vals[1] == vals[3]
    g2 = model.flat_parameters()[1]
    assert torch.isfinite(g2).all() and float(g2.abs().max()) > 0
    vals = compute_batch_drmsd(model(seq, ang), crd, seq, return_rmsd=True, backbone_only=True)
    assert len(vals) == 5 and np.isfinite(vals[4]) and vals[4] > 0

    n = SMALL_LENS[1]
    r = drmsd_work(batch["start_ang_rad"][1], batch["true_crd"][1], batch["seq"][1], backbone_only=True)
    assert len(r) == 5 and tuple(r[0].shape) == (48, 12)
    gw = r[0].numpy()
    # which angles cannot move N, CA or C comes from the fp64 reference of this protein, not from a list written down here
    start = batch["start_ang_rad"][1:2]
    sc1 = torch.stack([torch.cos(start), torch.sin(start)], -1).reshape(1, 48, 24)
    g64 = bb_reference(sc1, batch["seq"][1:2], batch["true_crd"][1:2])[1].view(48, 12, 2)
    dead = (g64 == 0).all(dim=-1).numpy()
    assert dead[:n].any() and not dead[:n].all()
    assert np.isfinite(gw).all() and np.abs(gw[~dead]).max() > 0 and np.all(gw[dead] == 0) and np.all(gw[n:] == 0)
    full = drmsd_work(batch["start_ang_rad"][1], batch["true_crd"][1], batch["seq"][1])
    assert r[3] == approx(full[3], rel=1e-4) and r[4] == approx(full[4], abs=1e-6) and (r[1], r[2]) == (r[3], r[4])
    assert len(drmsd_work(batch["start_ang_rad"][1], batch["true_crd"][1], batch["seq"][1], return_rmsd=True,
                          backbone_only=True)) == 6


# --------------------------------------------------------------------------- 2. values
def test_backbone_stats_vs_fp64_and_vs_full_call(dev, ragged):
    from protein_transformer_amd.losses import batch_loss
    sincos, seq, crd = (ragged[k].to(dev) for k in ("sincos", "seq", "crd"))
    stats, _, status = batch_loss(sincos, crd, seq, do_backward=False, backbone_only=True)[:3]
    full, _, status_full = batch_loss(sincos, crd, seq, do_backward=False)[:3]
    assert int(status.item()) == 0 and int(status_full.item()) == 0
    stats, full = stats.cpu().numpy(), full.cpu().numpy()
    for b, (d, ln, n_bb) in enumerate(ragged["stats64"]):
        print(f"protein {b}: n_bb {n_bb}  drmsd-bb {stats[b, 2]:.7f} (fp64 {d:.7f}, full call {full[b, 2]:.7f})  "
              f"lndrmsd-bb {stats[b, 3]:.3e} (fp64 {ln:.3e})")
        assert stats[b, 2] == approx(d, rel=1e-4), b
        assert stats[b, 3] == approx(ln, abs=1e-6), b
        assert stats[b, 5] == n_bb, b
        assert stats[b, 2] == approx(full[b, 2], rel=1e-4) and stats[b, 3] == approx(full[b, 3], abs=1e-6), b
        assert stats[b, 5] == full[b, 5], b
        assert (stats[b, 0], stats[b, 1], stats[b, 4]) == (stats[b, 2], stats[b, 3], stats[b, 5]), b     # the mirror
        assert stats[b, 6] == 0 and stats[b, 7] == 0


# --------------------------------------------------------------------------- 3. coordinates
@pytest.mark.parametrize("shape", ["ragged-64", "4x512"])
def test_backbone_coordinates_are_the_full_builds_bits(dev, ragged, shape):
    from protein_transformer_amd import synthetic
    from protein_transformer_amd.losses import angles_forward
    from protein_transformer_amd.protein.Structure import nerf_forward
    if shape == "ragged-64":
        seq = ragged["seq"].to(dev)
        ang = angles_forward(ragged["sincos"].to(dev))
    else:
        batch = synthetic.make_batch([512, 512, 411, 77], L_pad=512, seed=synthetic.DEFAULT_SEED)
        seq, ang = batch["seq"].to(dev), batch["start_ang_rad"].to(dev)
    B, L = seq.shape
    full, st_full = nerf_forward(ang, seq)
    bb, st_bb = nerf_forward(ang, seq, backbone_only=True)
    assert tuple(bb.shape) == (B, L * 3, 3)
    assert int(st_full.item()) == int(st_bb.item()) == 0
    assert torch.equal(bb.view(B, L, 3, 3), full.view(B, L, 14, 3)[:, :, :3])
    lens = (seq != 20).sum(1)
    for b in range(B):
        assert float(bb.view(B, L, 9)[b, int(lens[b]):].abs().max() if int(lens[b]) < L else 0.0) == 0.0
        assert float(bb.view(B, L, 9)[b, :int(lens[b])].abs().max()) > 0


def test_backbone_build_flags_what_the_full_build_flags(dev):
    from protein_transformer_amd.protein.Structure import nerf_forward
    ang = torch.zeros(2, 4, 12, device=dev)
    seq = torch.tensor([[0, 20, 20, 20], [1, 2, 3, 20]], device=dev)            # first protein: one residue
    ang[1, 1, 4] = 3.5                                                           # a bond angle outside [-pi, pi]
    full, st_full = nerf_forward(ang, seq)
    bb, st_bb = nerf_forward(ang, seq, backbone_only=True)
    assert int(st_bb.item()) == int(st_full.item()) == 2 | 4
    assert float(bb[0].abs().max()) == 0.0
    assert torch.equal(bb.view(2, 4, 3, 3), full.view(2, 4, 14, 3)[:, :, :3])


# --------------------------------------------------------------------------- 4. gradient
def check_gradient(grad_dev, grad64, lens, what):
    """per protein rel-L2 < 1e-3; exact zeros of the reference are exact zeros on the device; -> number of such entries"""
    g = grad_dev.detach().cpu().numpy()
    ref = grad64.numpy()
    assert np.isfinite(g).all()
    n_zero = 0
    for b, n in enumerate(lens):
        err = rel_l2(g[b], ref[b])
        print(f"{what}: protein {b} (L = {n}): gradient rel-L2 vs fp64 {err:.2e}")
        assert err < 1e-3, (what, b, err)
        zero = ref[b] == 0
        assert np.all(g[b][zero] == 0), (what, b)
        n_zero += int(zero[:n].sum())
    return n_zero


def test_backbone_gradient_vs_fp64_autograd_ragged(dev, ragged):
    from protein_transformer_amd.losses import batch_loss
    sincos, seq, crd = (ragged[k].to(dev) for k in ("sincos", "seq", "crd"))
    _, grad, status = batch_loss(sincos, crd, seq, do_backward=True, backbone_only=True)[:3]
    assert int(status.item()) == 0
    ref = ragged["grad64"].reshape(len(RAGGED_LENS), 64, 24)
    assert check_gradient(grad.view(len(RAGGED_LENS), 64, 24), ref, RAGGED_LENS, "ragged") > 0
    # the channels that cannot move N, CA or C - derived from the reference, not written down here
    dead = (ref == 0).all(dim=0).all(dim=0)
    assert dead.any() and not dead.all()
    print("channels of the 24 with a zero reference gradient everywhere:", torch.nonzero(dead).flatten().tolist())
    assert float(grad.view(-1, 24)[:, dead.to(dev)].abs().max()) == 0.0


def test_backbone_gradient_full_size_slice(dev):
    """A 4-protein slice of the 32 x 512 benchmark batch (as test_full_size_properties does for the full-atom path)."""
    from protein_transformer_amd import synthetic
    from protein_transformer_amd.losses import batch_loss
    from protein_transformer_amd.protein.Structure import nerf_forward
    B, L = 32, 512
    hip_build = lambda ang, seq: nerf_forward(ang.to(dev), seq.to(dev))[0]      # noqa: E731
    batch = synthetic.make_batch([L] * B, seed=synthetic.DEFAULT_SEED, build_coords=hip_build)
    start = batch["start_ang_rad"]
    sincos = torch.stack([torch.cos(start), torch.sin(start)], -1).reshape(B, L, 24)
    seq, crd = batch["seq"], batch["true_crd"]
    stats, grad, status = batch_loss(sincos.to(dev), crd.to(dev), seq.to(dev), backbone_only=True)[:3]
    assert int(status.item()) == 0
    full = batch_loss(sincos.to(dev), crd.to(dev), seq.to(dev), do_backward=False)[0]
    assert torch.allclose(stats[:, 2], full[:, 2], rtol=1e-4, atol=0) and torch.allclose(stats[:, 3], full[:, 3], rtol=0, atol=1e-6)
    assert torch.equal(stats[:, 5].cpu(), torch.full((B,), 3.0 * L))
    sub = slice(0, 4)
    stats64, grad64 = bb_reference(sincos[sub], seq[sub], crd[sub])
    st = stats.cpu().numpy()
    for b in range(4):
        assert st[b, 2] == approx(stats64[b][0], rel=1e-4) and st[b, 3] == approx(stats64[b][1], abs=1e-6)
    # a protein's loss and gradient do not depend on the batch it is computed in beyond rounding (tile cut by batch occupancy)
    s4, g4, _ = batch_loss(sincos[sub].to(dev), crd[sub].to(dev), seq[sub].to(dev), backbone_only=True)[:3]
    assert torch.allclose(s4, stats[sub], rtol=2e-6, atol=0)
    assert check_gradient(grad.view(B, L, 24)[sub], grad64, [L] * 4, "32 x 512 slice") > 0
    assert check_gradient(g4.view(4, L, 24), grad64, [L] * 4, "4 x 512") > 0


# --------------------------------------------------------------------------- 5. independence of the side-chain channels
def test_side_chain_channels_do_not_reach_the_backbone_loss(dev, ragged):
    from protein_transformer_amd.losses import batch_loss
    sincos, seq, crd = (ragged[k].to(dev) for k in ("sincos", "seq", "crd"))
    ref = ragged["grad64"].reshape(-1, 24)
    dead = (ref == 0).all(dim=0)
    assert dead.any()
    s1, g1, _ = batch_loss(sincos, crd, seq, backbone_only=True)[:3]
    s1, g1 = s1.clone(), g1.clone()
    moved = sincos.clone()
    gen = torch.Generator().manual_seed(1)
    noise = torch.randn(moved.shape, generator=gen).to(dev)
    moved[..., dead.to(dev)] = noise[..., dead.to(dev)]
    assert not torch.equal(moved, sincos)
    s2, g2, _ = batch_loss(moved, crd, seq, backbone_only=True)[:3]
    assert torch.equal(s1, s2) and torch.equal(g1, g2)
    # ... while the full-atom loss does see them
    f1 = batch_loss(sincos, crd, seq, do_backward=False)[0]
    f2 = batch_loss(moved, crd, seq, do_backward=False)[0]
    assert not torch.equal(f1[:, 0], f2[:, 0]) and torch.equal(f1[:, 2], f2[:, 2])


# --------------------------------------------------------------------------- 6. degenerate proteins
def test_proteins_without_a_backbone_pair(dev):
    from protein_transformer_amd import synthetic
    from protein_transformer_amd.losses import batch_loss
    from protein_transformer_amd.protein.Structure import nerf_forward
    lens = [20, 12, 30, 16]
    build = lambda ang, seq: nerf_forward(ang.to(dev), seq.to(dev))[0]           # noqa: E731
    batch = synthetic.make_batch(lens, L_pad=32, seed=8, build_coords=build)
    crd = batch["true_crd"].clone().view(4, 32, 14, 3)
    crd[1, :, :3] = float("nan")                     # no backbone atom present
    crd[3, :, :3] = float("nan")
    crd[3, 5, 1] = torch.tensor([1.0, 2.0, 3.0])     # exactly one
    crd = crd.view(4, 32 * 14, 3)
    start = batch["start_ang_rad"]
    sincos = torch.stack([torch.cos(start), torch.sin(start)], -1).reshape(4, 32, 24)
    stats, grad, status = batch_loss(sincos.to(dev), crd.to(dev), batch["seq"].to(dev), backbone_only=True)[:3]
    assert int(status.item()) == 0
    stats, grad = stats.cpu(), grad.view(4, 32, 24).cpu()
    assert torch.isfinite(grad).all()
    assert stats[:, 5].tolist() == [60.0, 0.0, 90.0, 1.0]
    for b in (0, 2):
        assert torch.isfinite(stats[b]).all() and float(stats[b, 2]) > 0 and float(grad[b].abs().max()) > 0
    for b in (1, 3):
        assert float(grad[b].abs().max()) == 0.0
    stats64, grad64 = bb_reference(sincos, batch["seq"], crd)
    for b in (0, 2):
        assert float(stats[b, 2]) == approx(stats64[b][0], rel=1e-4) and float(stats[b, 3]) == approx(stats64[b][1], abs=1e-6)
        assert rel_l2(grad[b].numpy(), grad64[b].numpy()) < 1e-3


# --------------------------------------------------------------------------- 7. passes and sizing
def test_backbone_sweep_in_passes_is_bit_identical_and_sized_from_3L(dev):
    from protein_transformer_amd import _lib, synthetic
    from protein_transformer_amd.losses import drmsd_forward_backward
    from protein_transformer_amd.protein.Structure import nerf_forward
    lib = _lib.lib()
    assert lib.ptamd_drmsd_bb_workspace_bytes(32, 512) < lib.ptamd_drmsd_workspace_bytes(32, 512)
    assert lib.ptamd_drmsd_bb_workspace_bytes(32, 512) * 3 < lib.ptamd_drmsd_workspace_bytes(32, 512)      # 3 L against 14 L atoms
    lens = [700, 512, 333, 64, 2]
    build = lambda ang, seq: nerf_forward(ang.to(dev), seq.to(dev))[0]  # noqa: E731
    batch = synthetic.make_batch(lens, L_pad=700, seed=77, build_coords=build, frac_missing=0.05)
    seq, true = batch["seq"].to(dev), batch["true_crd"].to(dev)
    pred = nerf_forward(batch["start_ang_rad"].to(dev), seq, backbone_only=True)[0]
    one = lib.ptamd_drmsd_bb_workspace_bytes(len(lens), 700)
    assert lib.ptamd_drmsd_bb_workspace_bytes_budget(len(lens), 700, 0) == one
    s1, g1 = drmsd_forward_backward(pred, true, seq, backbone_only=True)
    s1, g1 = s1.clone(), g1.clone()
    for budget in (1 << 20, 400 << 10):
        assert lib.ptamd_drmsd_bb_workspace_bytes_budget(len(lens), 700, budget) < one          # really in passes
        s2, g2 = drmsd_forward_backward(pred, true, seq, partial_budget_bytes=budget, backbone_only=True)
        torch.cuda.synchronize()
        assert torch.equal(s1, s2) and torch.equal(g1, g2), budget
        s3, _ = drmsd_forward_backward(pred, true, seq, need_grad=False, partial_budget_bytes=budget, backbone_only=True)
        assert torch.equal(s1, s3)
    assert torch.isfinite(g1).all() and float(g1.abs().max()) > 0
    full = drmsd_forward_backward(nerf_forward(batch["start_ang_rad"].to(dev), seq)[0], true, seq, need_grad=False)[0]
    assert torch.allclose(s1[:, 2], full[:, 2], rtol=1e-4, atol=0) and torch.equal(s1[:, 5], full[:, 5])


# --------------------------------------------------------------------------- 8. a training step
STEP_DRAWS = (11, 12, 13, 14)      # seeds of the four draws (model initialisation and batch)


def ill_conditioned(rad64, seq, lens):
    """The fp64-only criterion of DESIGN.md section 4: |sin| of a backbone bond angle below 5e-4, or a 6e-8 rad move of every
    angle (random sign) moves a coordinate by more than one unit of 1e-3 A * max(1, L / 128)."""
    from oracle import batched
    sin_bond = min(float(np.abs(np.sin(rad64[b, :n, 3:6].numpy())).min()) for b, n in enumerate(lens))
    if sin_bond < 5e-4:
        return True
    gen = torch.Generator().manual_seed(99)
    sign = torch.randint(0, 2, rad64.shape, generator=gen).double() * 2 - 1
    c0 = batched.generate_coords_batched(rad64, seq, torch.float64)
    c1 = batched.generate_coords_batched(rad64 + 6e-8 * sign, seq, torch.float64)
    unit = [1e-3 * max(1.0, n / 128) for n in lens]
    return max(float((c1[b, :n * 14] - c0[b, :n * 14]).abs().max()) / unit[b] for b, n in enumerate(lens)) > 1.0


def fp64_backbone_step(model, nhead, seq, crd):
    """The encoder's fp64 forward as tests/parity_lib.py obtains it, with the backbone loss in place of the full one:
    -> (radians [B, L, 12], per-protein stats, {name: gradient})."""
    from oracle import encoder as oenc
    B, L = seq.shape
    params = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    pe = {k: v for k, v in params.items() if k.endswith(".pe")}
    leaf = {k: v.clone().requires_grad_() for k, v in params.items() if k not in pe}
    pred = oenc.encoder_forward({**leaf, **pe}, seq.cpu(), nhead)
    cs = pred.view(B, L, 12, 2)
    rad = torch.atan2(cs[..., 1], cs[..., 0]).detach()
    stats, total = bb_loss_fp64(pred.view(B, L, 24), seq.cpu(), crd.cpu())
    total.backward()
    return rad, stats, {k: v.grad for k, v in leaf.items()}


def test_backbone_train_step_vs_fp64(dev):
    """`train.train_step` under the flag (enc-only d 64, 2 layers, 4 heads, dropout 0, SGD, clip 1) against the fp64 step: the
    parameter gradient the optimizer saw (the clip scales it inside the step kernel; `.grad` keeps what was back-propagated)."""
    import parity_lib
    from test_gpu_parity_record import realistic_angle_means
    from protein_transformer_amd.optim import FusedSGD
    from protein_transformer_amd.train import train_step
    ran = skipped = 0
    for draw in STEP_DRAWS:
        batch = small_batch(dev, seed=draw)
        seq, ang, crd = (batch[k].to(dev) for k in ("seq", "true_ang", "true_crd"))
        model = small_model(dev, realistic_angle_means(draw), seed=draw)
        before = model.flat_parameters()[0].clone()
        rad64, stats64, ref = fp64_backbone_step(model, 4, seq, crd)
        if ill_conditioned(rad64, batch["seq"], SMALL_LENS):
            skipped += 1
            print(f"draw {draw}: ill-conditioned for any fp32 chain (DESIGN.md section 4), skipped")
            continue
        opt = FusedSGD(model, lr=1e-2, weight_decay=10e-3)
        losses = train_step(model, opt, bb_args("drmsd", clip=1.0), seq, ang, crd)
        err, groups, worst = parity_lib.grad_errors({n: p.grad for n, p in model.named_parameters()}, ref)
        print(f"draw {draw}: parameter gradient rel-L2 vs fp64 {err:.2e}, worst tensor {worst}, groups {groups}")
        assert err < 1e-3, (draw, err)
        assert float(losses["loss"]) == approx(np.mean([s[0] for s in stats64]), rel=1e-4)
        assert float(losses["lndrmsd-bb"]) == approx(np.mean([s[1] for s in stats64]), abs=1e-6)
        assert not torch.equal(model.flat_parameters()[0], before)           # the step moved the weights
        # nothing flows into the output rows of the channels that cannot move N, CA or C - the rows whose fp64 gradient is zero
        gw = dict(model.named_parameters())["output_projection.weight"].grad
        dead = (ref["output_projection.weight"] == 0).all(dim=1)
        assert dead.any() and not dead.all()
        assert float(gw[dead.to(dev)].abs().max()) == 0.0 and float(gw[~dead.to(dev)].abs().max()) > 0
        ran += 1
    assert ran >= 1 and skipped <= len(STEP_DRAWS) // 4, (ran, skipped)


# --------------------------------------------------------------------------- 9. combined
def test_combined_loss_under_the_flag(dev):
    from test_gpu_parity_record import realistic_angle_means
    from protein_transformer_amd.losses import batch_loss, combine_drmsd_mse, mse_grad, mse_sums
    from protein_transformer_amd.train import get_losses
    batch = small_batch(dev, seed=6)
    seq, ang, crd = (batch[k].to(dev) for k in ("seq", "true_ang", "true_crd"))
    model = small_model(dev, realistic_angle_means(6), seed=6)
    w = 0.5
    model.zero_grad()
    pred = model(seq, ang)
    seen = []
    pred.register_hook(lambda g: seen.append(g.detach().clone()))
    out = get_losses(bb_args("combined"), pred, ang, crd, seq)
    assert len(seen) == 1
    assert float(out["loss"]) == float(combine_drmsd_mse(out["lndrmsd-bb"], out["mse-full"], w=w))
    assert float(out["loss"]) == float(out["combined-full"])
    g_bb = batch_loss(pred, crd, seq, backbone_only=True)[1].view_as(pred)
    g_mse = mse_grad(pred, ang, mse_sums(pred, ang), coef=(1 - w) / 0.01).view_as(pred)
    err = float((seen[0] - (g_bb + g_mse)).double().norm() / (g_bb + g_mse).double().norm())
    print("combined under the flag: fused gradient vs backbone + MSE added separately, rel-L2", err)
    assert err < 1e-5, err
    assert float(g_mse.abs().max()) > 0 and float(g_bb.abs().max()) > 0
    # -l mse ignores the flag
    a = get_losses(bb_args("mse"), model(seq, ang), ang, crd, seq, do_backwards=False)
    b_args = bb_args("mse")
    b_args.backbone_loss = False
    b = get_losses(b_args, model(seq, ang), ang, crd, seq, do_backwards=False)
    assert float(a["loss"]) == float(b["loss"]) == float(a["mse-full"])


def test_evaluation_under_the_flag_reports_every_metric(dev):
    """eval_mode builds the whole structure: the metrics are those without the flag, only `loss` follows the flag."""
    from test_gpu_parity_record import realistic_angle_means
    from protein_transformer_amd.train import get_losses
    batch = small_batch(dev, seed=6)
    seq, ang, crd = (batch[k].to(dev) for k in ("seq", "true_ang", "true_crd"))
    model = small_model(dev, realistic_angle_means(6), seed=6).eval()
    plain = bb_args("drmsd")
    plain.backbone_loss = False
    with torch.no_grad():
        pred = model(seq, ang)
        a = get_losses(bb_args("drmsd"), pred, ang, crd, seq, do_backwards=False, eval_mode=True, return_rmsd=True)
        b = get_losses(plain, pred, ang, crd, seq, do_backwards=False, eval_mode=True, return_rmsd=True)
    for k in ("drmsd-full", "lndrmsd-full", "drmsd-bb", "lndrmsd-bb", "combined-full", "mse-full", "mse-bb", "mse-sc", "rmsd-full"):
        assert float(a[k]) == float(b[k]), k
    assert float(a["loss"]) == float(a["drmsd-bb"]) and float(b["loss"]) == float(b["drmsd-full"])
    assert float(a["drmsd-full"]) != float(a["drmsd-bb"])
    # evaluation that also back-propagates (no caller in the tree does): the metrics stay the full ones, the gradient is the
    # backbone's - bit for bit what a training step injects
    model.train()
    model.zero_grad()
    c = get_losses(bb_args("drmsd"), model(seq, ang), ang, crd, seq, do_backwards=True, eval_mode=True)
    g_eval = model.flat_parameters()[1].clone()
    model.zero_grad()
    d = get_losses(bb_args("drmsd"), model(seq, ang), ang, crd, seq, do_backwards=True)
    assert torch.equal(g_eval, model.flat_parameters()[1]) and float(g_eval.abs().max()) > 0
    assert float(c["drmsd-full"]) == float(a["drmsd-full"]) and float(c["loss"]) == float(a["drmsd-bb"])
    assert float(d["loss"]) == approx(float(c["loss"]), rel=1e-4)      # the training step's number comes from the 3 L sweep


# --------------------------------------------------------------------------- 10. determinism
def test_backbone_step_is_bit_reproducible(dev):
    from test_gpu_parity_record import realistic_angle_means
    from protein_transformer_amd.losses import batch_loss
    from protein_transformer_amd.train import get_losses
    batch = small_batch(dev, seed=7)
    seq, ang, crd = (batch[k].to(dev) for k in ("seq", "true_ang", "true_crd"))
    model = small_model(dev, realistic_angle_means(7), seed=7)
    runs = []
    for _ in range(2):
        model.zero_grad()
        pred = model(seq, ang)
        out = get_losses(bb_args("drmsd", clip=None), pred, ang, crd, seq)
        s, g, _ = batch_loss(pred, crd, seq, backbone_only=True)[:3]
        runs.append((model.flat_parameters()[1].clone(), s.clone(), g.clone(), float(out["loss"])))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][2], runs[1][2])
    assert runs[0][3] == runs[1][3]
    assert float(runs[0][0].abs().max()) > 0
