"""The frame aligned point error on the device (csrc/fape.hip, losses.fape_forward_backward, `train.py -l fape`) against an fp64
restatement of its definition in include/ptamd.h, written here with torch autograd.

Whether a pair is clamped is a threshold on an fp32 d_ij, so no case uses 10.0 as its clamp: `well_posed_clamp` sorts the
reference d_ij of the case inside [9.5, 10.5] (the ends of the window count as neighbours), asserts that the widest gap between
neighbours is at least 1e-3 A and places the clamp in its middle; every coordinate-level case also asserts that its largest
frame-to-atom distance (the lever arm of a frame's rotation) is at most 64 A.  Both are conditions on the input, checked on the
CPU; no pair is left out of a comparison, and `npairs` and `nclamped` must equal the reference's counts exactly.

Bars.  Value: |loss - ref| <= 1e-5.  Every number below 64 A has a half ulp of at most 2^-19 = 1.9e-6 A.  One component of
x_ij = R^T (x_j - t) carries: the three subtractions, each half an ulp, weighted by a column of R (sum of |entries| <= sqrt 3):
3.3e-6; the rounding of R to fp32 (2^-25 per entry, fp64 before that) times |r| <= 64 A: 3.3e-6; the three roundings of the
multiply-adds: 5.7e-6; together 1.23e-5 A, for prediction and truth 2.5e-5 A per component of Delta, so |d - d_ref| <= sqrt(3)
2.5e-5 = 4.3e-5 A (the root is 1-Lipschitz in Delta) - a tenth of the 5e-4 A half-gap, so no pair changes sides - and 4.3e-6
after the division by Z = 10 A; the root's own ulp and the sums (fp32 over 64 values, fp64 behind them) add less than 1e-6.
dcrd: rel-L2 < 1e-4 against the fp64 gradient, the bar of tests/test_gpu_loss_path.py for a coordinate gradient.  Down to the
angles through the NeRF adjoint: rel-L2 < 1e-3, the bar of the chain tests there; the value bound of that test is derived at
its place.  Hand-computed case: value abs 1e-6 (d is off by at most an ulp of 12 A = 1e-6 A, divided by 40), gradient rel 1e-5
(Delta / d with both from exactly representable offsets: the ulps of rsq and of three products).

Measured on an MI355X (the figures every test prints): see profiles/fape/NOTES.md."""
import numpy as np
import pytest
import torch

from test_gpu_slddt import PAD, SLOTS, _chains, _dp_worker, _make, cloud, present_atoms, rel_l2, stack

pytestmark = pytest.mark.gpu

Z = 10.0
VALUE_BAR = 1e-5
TODAY_KEYS = {"loss", "drmsd-full", "lndrmsd-full", "drmsd-bb", "lndrmsd-bb", "combined-full", "mse-full", "mse-bb", "mse-sc",
              "rmsd-full"}


# ----------------------------------------------------------------------------- the fp64 reference
def frames_from_points(n, ca, c):
    """Algorithm 21 on [F,3] fp64 tensors: (R [F,3,3] with columns e1 e2 e3, t, |v1|^2, |u2|^2)."""
    v1, v2 = c - ca, n - ca
    q1 = (v1 * v1).sum(-1)
    e1 = v1 / q1.sqrt()[:, None]
    u2 = v2 - e1 * (e1 * v2).sum(-1, keepdim=True)
    q2 = (u2 * u2).sum(-1)
    e2 = u2 / q2.sqrt()[:, None]
    e3 = torch.linalg.cross(e1, e2)
    return torch.stack([e1, e2, e3], -1), ca, q1, q2


def frame_residues(true, seq):
    """Residues of one protein that carry a frame: non-pad, N, CA, C present in the truth, true frame not degenerate."""
    true, seq = np.asarray(true, np.float64), np.asarray(seq)
    bb = true.reshape(len(seq), SLOTS, 3)[:, :3]
    ok = (seq != PAD) & ~np.isnan(bb).any((1, 2))
    res = np.nonzero(ok)[0]
    if len(res) == 0:
        return res
    t = torch.tensor(bb[res])
    _, _, q1, q2 = frames_from_points(t[:, 0], t[:, 1], t[:, 2])
    return res[((q1 > 1e-8) & (q2 > 1e-8)).numpy()]


def fape_reference(pred, true, seq, clamp):
    """One protein in fp64: dict(loss, npairs, nclamped, grad [L*14,3], d [frames,atoms], lever).  `pred`: array, or an fp64 torch
    tensor inside an autograd graph (then grad is None and loss is a tensor).  An unusable prediction (a present atom that is
    not finite or beyond 1e18, a degenerate predicted frame) gives a NaN loss, a zero gradient, npairs and nclamped = 0."""
    idx, res = present_atoms(true, seq), frame_residues(true, seq)
    graph = torch.is_tensor(pred) and pred.requires_grad
    p_all = pred if graph else torch.tensor(np.asarray(pred, np.float64), requires_grad=True)
    nan = p_all.sum().detach() * 0 + float("nan")
    out = dict(loss=nan if graph else float("nan"), npairs=0, nclamped=0, grad=None if graph else np.zeros(tuple(p_all.shape)),
               d=np.zeros((0, 0)), lever=0.0)
    if len(idx) == 0 or len(res) == 0:
        return out
    out["npairs"] = len(idx) * len(res)
    p = p_all[torch.tensor(idx)]
    with torch.no_grad():
        if not bool((p.abs() <= 1e18).all()):                    # (NaN fails the comparison)
            return out
    t_all = torch.tensor(np.asarray(true, np.float64))
    bb = lambda x: [x.reshape(len(seq), SLOTS, 3)[torch.tensor(res), k] for k in range(3)]      # noqa: E731
    Rp, tp, q1, q2 = frames_from_points(*bb(p_all))
    if not bool(((q1 > 1e-8) & (q2 > 1e-8)).all()):
        return out
    Rt, tt, _, _ = frames_from_points(*bb(t_all))
    rp = p[None] - tp[:, None]                                   # [F,A,3]
    rt = t_all[torch.tensor(idx)][None] - tt[:, None]
    delta = torch.einsum("fmk,fam->fak", Rp, rp) - torch.einsum("fmk,fam->fak", Rt, rt)
    d = ((delta ** 2).sum(-1) + 1e-4).sqrt()
    is_open = d.detach() < clamp
    loss = torch.where(is_open, d, torch.full_like(d, min(clamp, 1e300)).detach()).mean() / Z
    out.update(nclamped=int((~is_open).sum()), d=d.detach().numpy(),
               lever=float(max(rp.detach().norm(dim=-1).max(), rt.norm(dim=-1).max())))
    if graph:
        out["loss"] = loss
        return out
    loss.backward()
    out.update(loss=float(loss.detach()), grad=p_all.grad.numpy())
    return out


def well_posed_clamp(ds):
    """The clamp of a case: the middle of the widest gap between neighbouring reference d_ij (a list of arrays, computed with
    clamp = inf) inside [9.5, 10.5]; asserts the gap is >= 1e-3 A.  (A case without any d in the window has the whole window as
    its gap.)"""
    near = [9.5, 10.5]
    for d in ds:
        d = np.asarray(d).ravel()
        near += d[(d >= 9.5) & (d <= 10.5)].tolist()
    near = np.sort(np.array(near))
    k = int(np.argmax(np.diff(near)))
    assert near[k + 1] - near[k] >= 1e-3, "pick another seed for this case: its deviations crowd the window"
    return float(np.float32(0.5 * (near[k] + near[k + 1])))


# ----------------------------------------------------------------------------- cases
def _tiny():
    """1 atom; a residue with N, CA, C only (1 frame, 3 atoms); two residues, the second without its CA (1 frame, 5 atoms); no
    present atom; a fully padded row; a truth with collinear N, CA, C (no frame)."""
    rng = np.random.default_rng(111)
    L = 3
    one, bb = cloud(1, 1, rng, L), cloud(3, 3, rng, L)
    no_ca = cloud(6, 3, rng, L)
    no_ca[1][SLOTS + 1] = np.nan
    none = cloud(4, 2, rng, L)
    none[1][:] = np.nan
    padded = cloud(4, 2, rng, L)
    padded[2][:] = PAD
    padded[1][:] = 0.0
    line = cloud(3, 3, rng, L)
    line[1][:3] = np.array([[-1.4, 0, 0], [0, 0, 0], [1.5, 0, 0]], np.float32) + np.float32(2.5)
    return stack([one, bb, no_ca, none, padded, line])


def _edges():
    """63, 64, 65, 128, 129 atoms (tiles are 64 compacted atoms), five atoms per residue, rows padded to the longest."""
    rng = np.random.default_rng(212)
    return stack([cloud(n, 5, rng, L=26) for n in (63, 64, 65, 128, 129)])


def _frames():
    """130 residues of five atoms: 130 frames (tiles of 64 frames: 3) x 650 atoms (11 tiles of 64 atoms: 2 chunks of 8)."""
    rng = np.random.default_rng(313)
    return stack([cloud(650, 5, rng)])


CASES = {"tiny": _tiny, "edges": _edges, "frames": _frames, "chains": lambda: _chains()[:3]}
_cache = {}


def case(name):
    """(pred, true, seq, clamp, per-protein references) of a case, built once: the clamp is placed by the unclamped reference,
    and the lever arm of every protein is checked."""
    if name not in _cache:
        pred, true, seq = CASES[name]()
        free = [fape_reference(pred[b], true[b], seq[b], float("inf")) for b in range(len(seq))]
        assert max(r["lever"] for r in free) <= 64.0, "pick another seed for this case: a frame-to-atom distance beyond 64 A"
        clamp = well_posed_clamp([r["d"] for r in free])
        _cache[name] = (pred, true, seq, clamp, [fape_reference(pred[b], true[b], seq[b], clamp) for b in range(len(seq))])
        _cache[name, "free"] = free
    return _cache[name]


def run(pred, true, seq, clamp, need_grad=True):
    """losses.fape_forward_backward on numpy inputs -> (stats [B,2], npairs [B], nclamped [B], dcrd or None) as numpy."""
    from protein_transformer_amd.losses import fape_forward_backward
    dev = torch.device("cuda:0")
    p, t, s = (torch.as_tensor(np.asarray(x)) for x in (pred, true, seq))
    if p.dim() == 2:
        p, t, s = p[None], t[None], s[None]
    st, n, c, g = fape_forward_backward(p.float().to(dev), t.float().to(dev), s.to(dev), need_grad=need_grad, clamp=clamp)
    return st.cpu().numpy(), n.cpu().numpy(), c.cpu().numpy(), (g.cpu().numpy() if g is not None else None)


def check_against(name, got, refs, true, seq):
    stats, npairs, nclamped, dcrd = got
    assert np.isfinite(dcrd).all()
    for b, ref in enumerate(refs):
        err = abs(stats[b, 0] - ref["loss"]) if ref["npairs"] else 0.0
        print(f"{name}[{b}]: npairs {npairs[b]} / {ref['npairs']}, nclamped {nclamped[b]} / {ref['nclamped']}, "
              f"loss {stats[b, 0]} / {ref['loss']} (|err| {err:.2e}), dcrd rel-L2 {rel_l2(dcrd[b], ref['grad']) if ref['npairs'] else 0.0:.2e}")
        assert npairs[b] == ref["npairs"] and nclamped[b] == ref["nclamped"]
        if ref["npairs"] == 0:
            assert np.isnan(stats[b]).all() and not dcrd[b].any()
            continue
        assert err <= VALUE_BAR
        assert stats[b, 1] == pytest.approx(ref["nclamped"] / ref["npairs"], rel=1e-6)
        assert rel_l2(dcrd[b], ref["grad"]) < 1e-4
        absent = np.setdiff1d(np.arange(dcrd.shape[1]), present_atoms(true[b], seq[b]))
        assert not dcrd[b, absent].any()                           # empty slots and padded residues get zeros


# ----------------------------------------------------------------------------- 1. value, counts, gradient against fp64
@pytest.mark.parametrize("name", list(CASES))
def test_value_counts_and_gradient_against_fp64(name):
    pred, true, seq, clamp, refs = case(name)
    check_against(name, run(pred, true, seq, clamp), refs, true, seq)


def test_the_cases_are_the_shapes_they_claim():
    shape = lambda name: [(len(frame_residues(t, s)), len(present_atoms(t, s))) for t, s in zip(*case(name)[1:3])]     # noqa: E731
    assert shape("tiny") == [(0, 1), (1, 3), (1, 5), (0, 0), (0, 0), (0, 3)]
    assert shape("edges") == [(13, 63), (13, 64), (13, 65), (26, 128), (26, 129)] and shape("frames") == [(130, 650)]
    assert [f > 15 and a > 100 for f, a in shape("chains")] == [True] * 3 + [False]      # (the last row is fully padded)
    for name in ("edges", "frames", "chains"):                     # both branches of the clamp are exercised
        for ref in case(name)[4]:
            assert 0 < ref["nclamped"] < ref["npairs"] or ref["npairs"] == 0, name


def test_unclamped_equals_the_reference_without_a_clamp():
    pred, true, seq, _, _ = case("edges")
    got = run(pred, true, seq, float("inf"))
    assert not got[2].any()
    check_against("edges, clamp inf", got, _cache["edges", "free"], true, seq)


def test_gradient_down_to_the_angles_against_fp64_autograd():
    from oracle import batched, losses as olosses
    from protein_transformer_amd.losses import batch_loss
    dev = torch.device("cuda:0")
    _, true, seq, batch = _chains()
    true, seq = true[:3], seq[:3]                                  # (without the fully padded row: the model never sees one)
    ang = batch["start_ang_rad"]
    sincos = (torch.stack([torch.cos(ang), torch.sin(ang)], -1).reshape(len(seq), -1, 24) * 0.9).float()
    sc64 = sincos.double().clone().requires_grad_()
    crd64 = batched.generate_coords_batched(olosses.inverse_trig_transform(sc64), batch["seq"], torch.float64)
    free = [fape_reference(crd64[b].detach().numpy(), true[b], seq[b], float("inf")) for b in range(len(seq))]
    clamp = well_posed_clamp([r["d"] for r in free])
    out = batch_loss(sincos.to(dev), torch.from_numpy(true).to(dev), batch["seq"].to(dev), do_backward=True, fape=clamp)
    assert {f for f, v in out._asdict().items() if v is None} == {"true_ang", "clash"} and int(out.status.item()) == 0
    grad, fa = out.grad.cpu().numpy(), out.per_protein.cpu().numpy()
    total = 0
    for b in range(len(seq)):
        ref = fape_reference(crd64[b], true[b], seq[b], clamp)
        total = total + ref["loss"]                                # the back-propagated quantity is the SUM over proteins
        # Two NeRF chains, fp32 and fp64, stand behind these: coordinates within delta = 2e-3 A (the stated tolerance of
        # tests/test_gpu_loss_path.py for L <= 128).  To first order a frame's axes move by |d e1| <= 2 delta / |v1|,
        # |d e2| <= (2 delta + 2 |v2| |d e1|) / |u2| <= 6.4 delta / m and |d e3| <= |d e1| + |d e2| <= 8.4 delta / m, with
        # m = min(|v1|, |u2|) over the frames and |v2| / |v1| <= 1.1 for a backbone (asserted); so R^T r moves by at most
        # sqrt(2^2 + 6.4^2 + 8.4^2) delta lever / m <= 11 delta lever / m, x_j and t_i by delta each, d is 1-Lipschitz in
        # Delta and min(d, clamp) in d, and the mean of the pair values / Z moves by no more than one of them.
        n_, ca_, c_ = (crd64[b].detach().reshape(-1, SLOTS, 3)[torch.tensor(frame_residues(true[b], seq[b])), k] for k in range(3))
        v1, v2 = c_ - ca_, n_ - ca_
        e1 = v1 / v1.norm(dim=-1, keepdim=True)
        m = float(torch.minimum(v1.norm(dim=-1), (v2 - e1 * (e1 * v2).sum(-1, keepdim=True)).norm(dim=-1)).min())
        assert float((v2.norm(dim=-1) / v1.norm(dim=-1)).max()) <= 1.1
        bound = (2 * 2e-3 + 11 * 2e-3 * free[b]["lever"] / m) / Z
        print(f"chains[{b}]: loss {fa[b]} / {float(ref['loss'].detach())}, bound {bound:.2e}")
        assert abs(fa[b] - float(ref["loss"].detach())) <= bound
    total.backward()
    for b in range(len(seq)):
        print(f"chains[{b}]: angle gradient rel-L2 {rel_l2(grad[b], sc64.grad[b].numpy()):.2e}")
        assert rel_l2(grad[b], sc64.grad[b].numpy()) < 1e-3


# ----------------------------------------------------------------------------- 2. closed forms
def test_prediction_equal_to_truth():
    _, true, seq, clamp, refs = case("chains")
    stats, npairs, nclamped, dcrd = run(np.nan_to_num(true, nan=0.0), true, seq, clamp)
    assert npairs[:3].all() and npairs[3] == 0 and not nclamped.any()
    assert np.abs(stats[:3, 0] - 1e-3).max() <= 1e-6 and np.isnan(stats[3, 0])
    assert not dcrd.any()                                          # exactly zero everywhere


def _rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def test_rigid_motion_scores_like_the_truth_and_a_mirror_image_does_not():
    from protein_transformer_amd.losses import drmsd_forward_backward
    pred, true, seq, clamp, refs = case("chains")
    rng = np.random.default_rng(515)
    filled = np.nan_to_num(true, nan=0.0).astype(np.float64)
    moved = (filled @ _rotation(rng).T + np.array([3.0, -7.0, 11.0])).astype(np.float32)
    mirrored = (filled * np.array([1.0, 1.0, -1.0])).astype(np.float32)
    noisy = run(pred, true, seq, clamp)
    rigid = run(moved, true, seq, clamp)
    mirror = run(mirrored, true, seq, clamp)
    dev = torch.device("cuda:0")
    dstats, _ = drmsd_forward_backward(torch.from_numpy(mirrored).to(dev), torch.from_numpy(true).to(dev), torch.from_numpy(seq).to(dev),
                                       need_grad=False)
    dstats = dstats.cpu().numpy()
    for b in range(3):                                             # (the last row is fully padded)
        gn = [float(np.linalg.norm(x[3][b])) for x in (noisy, rigid, mirror)]
        print(f"chains[{b}]: loss noisy {noisy[0][b, 0]:.6f} rigid {rigid[0][b, 0]:.7f} mirror {mirror[0][b, 0]:.6f}; "
              f"|dcrd| noisy {gn[0]:.3e} rigid {gn[1]:.3e} mirror {gn[2]:.3e}; dRMSD of the mirror image {dstats[b, 0]:.3e}")
        # the moved copy is rounded to fp32: its Delta is the rounding of the coordinates (<= 2^-19 A below 64 A) seen through
        # the value bar's chain of roundings, so d stays within that bar of sqrt(1e-4)
        assert abs(rigid[0][b, 0] - 1e-3) <= VALUE_BAR
        assert gn[1] < 0.05 * gn[0]
        # the point of the feature: the mirror image is a different structure for FAPE, the same one for the dRMSD
        assert mirror[0][b, 0] > 0.1 and mirror[0][b, 0] > 100 * rigid[0][b, 0]
        assert dstats[b, 0] < 1e-3


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_one_frame_and_one_displaced_atom_by_hand(axis):
    L, clamp = 2, 8.0                                              # d is 0.01, ~3 or ~12 here: nowhere near the clamp
    true = np.full((L * SLOTS, 3), np.nan, np.float32)
    true[0], true[1], true[2] = (-0.5, 1.5, 0), (0, 0, 0), (1.5, 0, 0)         # N, CA, C: e1 = x, e2 = y, e3 = z
    true[SLOTS + 1] = (3, 4, 5)                                    # a lone CA: an atom, no frame
    seq = np.zeros(L, np.int64)
    for off, want_d in ((3.0, np.sqrt(9.0 + 1e-4)), (-3.0, np.sqrt(9.0 + 1e-4)), (12.0, clamp)):
        pred = np.nan_to_num(true, nan=0.0)
        pred[SLOTS + 1, axis] += off
        stats, npairs, nclamped, dcrd = run(pred, true, seq, clamp)
        ref = fape_reference(pred, true, seq, clamp)
        assert npairs[0] == 4 and nclamped[0] == ref["nclamped"] == int(abs(off) > clamp)
        assert abs(stats[0, 0] - (3 * 0.01 + want_d) / (Z * 4)) <= 1e-6
        if abs(off) > clamp:                                       # the clamped pair carries no gradient, the others have Delta = 0
            assert abs(stats[0, 0] - (0.03 + clamp) / 40) <= 1e-7       # exactly the clamp, whatever d is
            assert not dcrd.any()
            continue
        g = off / want_d / (Z * 4)
        assert dcrd[0, SLOTS + 1, axis] == pytest.approx(g, rel=1e-5)
        assert np.count_nonzero(dcrd[0, SLOTS + 1]) == 1
        assert rel_l2(dcrd[0], ref["grad"]) < 1e-5                 # the frame's N, CA, C carry the reaction
        # a translation of everything changes nothing: the four rows cancel up to their own fp32 rounding (2^-24 relative each,
        # magnitudes <= |g| (1 + |r| / |v1| + |r| / |u2|) = 10.4 |g| with |r| = 7.07 A and 1.5 A bonds: 4 x 10.4 x 6e-8 = 2.5e-6)
        assert np.abs(dcrd[0].astype(np.float64).sum(0)).max() <= 3e-6 * abs(g)


# ----------------------------------------------------------------------------- 3. determinism and independence
@pytest.mark.parametrize("name", ["edges", "frames", "chains"])
def test_bits_do_not_depend_on_the_run_the_batch_or_the_padding(name):
    pred, true, seq, clamp, _ = case(name)
    first = run(pred, true, seq, clamp)
    again = run(pred, true, seq, clamp)
    for a, b in zip(first, again):
        assert np.array_equal(a, b, equal_nan=True)
    fwd = run(pred, true, seq, clamp, need_grad=False)
    assert fwd[3] is None and all(np.array_equal(a, b, equal_nan=True) for a, b in zip(fwd[:3], first[:3]))
    L = seq.shape[1]
    for b in range(len(seq)):
        alone = run(pred[b], true[b], seq[b], clamp)
        for a, w in zip(alone, first):
            assert np.array_equal(a[0], w[b], equal_nan=True), b
        wide = run(np.concatenate([pred[b], np.zeros_like(pred[b])]), np.concatenate([true[b], np.zeros_like(true[b])]),
                   np.concatenate([seq[b], np.full(L, PAD, np.int64)]), clamp)        # the padding doubled
        assert all(np.array_equal(a[0], w[b], equal_nan=True) for a, w in zip(wide[:3], first[:3])), b
        assert np.array_equal(wide[3][0, :L * SLOTS], first[3][b]) and not wide[3][0, L * SLOTS:].any()


# ----------------------------------------------------------------------------- 4. unusable predictions
@pytest.mark.parametrize("value", [float("nan"), 1e30, -float("inf")])
def test_an_unusable_predicted_atom_costs_its_protein_only(value):
    pred, true, seq, clamp, refs = case("edges")
    before = run(pred, true, seq, clamp)
    b = 3
    p = pred.copy()
    p[b, int(present_atoms(true[b], seq[b])[70]), 1] = value
    stats, npairs, nclamped, dcrd = run(p, true, seq, clamp)
    assert np.isnan(stats[b, 0]) and npairs[b] == refs[b]["npairs"] and nclamped[b] == 0 and not dcrd[b].any()
    assert np.isfinite(dcrd).all()
    for o in range(len(seq)):
        if o != b:
            assert all(np.array_equal(x[o], y[o]) for x, y in zip((stats, npairs, nclamped, dcrd), before))
    ref = fape_reference(p[b], true[b], seq[b], clamp)
    assert np.isnan(ref["loss"]) and ref["npairs"] == npairs[b]


def test_a_degenerate_predicted_frame_costs_its_protein_only():
    pred, true, seq, clamp, refs = case("edges")
    b = 1
    p = pred.copy()
    p[b, 2 * SLOTS + 2] = p[b, 2 * SLOTS + 1]                       # C on CA in residue 2
    stats, npairs, nclamped, dcrd = run(p, true, seq, clamp)
    assert np.isnan(stats[b, 0]) and npairs[b] == refs[b]["npairs"] and nclamped[b] == 0 and not dcrd[b].any()
    assert abs(stats[0, 0] - refs[0]["loss"]) <= VALUE_BAR and np.isnan(fape_reference(p[b], true[b], seq[b], clamp)["loss"])


# ----------------------------------------------------------------------------- 5. refusals
def test_refusals_leave_the_outputs_untouched():
    from protein_transformer_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    B, L = 2, 5
    crd = torch.zeros(B, L * SLOTS, 3, device=dev)
    seq = torch.zeros(B, L, dtype=torch.int64, device=dev)
    need = lib.ptamd_fape_workspace_bytes(B, L)
    assert need > 0
    # every output with a guard word behind it
    stats = torch.full((B * 2 + 1,), 77.0, device=dev)
    npairs = torch.full((B + 1,), 77, dtype=torch.int64, device=dev)
    nclamped = torch.full((B + 1,), 77, dtype=torch.int64, device=dev)
    dcrd = torch.full((B * L * SLOTS * 3 + 1,), 77.0, device=dev)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    P = _lib.ptr

    def call(pred=crd, true=crd, s=seq, b=B, l=L, clamp=9.0, st=stats, n=npairs, c=nclamped, g=dcrd, w=ws, wb=None):
        rc = lib.ptamd_fape_fwd_bwd(P(pred), P(true), P(s), b, l, clamp, P(st), P(n), P(c), P(g), P(w), need if wb is None else wb,
                                    _lib.stream())
        torch.cuda.synchronize()
        return rc

    def untouched():
        return all(bool((t == 77).all()) for t in (stats, npairs, nclamped, dcrd))
    bad_shape = ([dict(b=0), dict(b=-1), dict(l=0), dict(l=-3), dict(l=(2 ** 31 - 1) // 28 + 1), dict(pred=None), dict(true=None),
                  dict(s=None), dict(st=None), dict(n=None), dict(c=None)]
                 + [dict(clamp=v) for v in (0.0, -1.0, -float("inf"), float("nan"))])
    for kw in bad_shape:
        assert call(**kw) == -1, kw                          # PTAMD_ERR_BAD_SHAPE
        assert untouched(), kw
    for kw in (dict(w=None), dict(wb=need - 1), dict(wb=0)):
        assert call(**kw) == -3, kw                          # PTAMD_ERR_WORKSPACE
        assert untouched(), kw
    assert call(g=None) == 0 and bool((dcrd == 77).all())    # forward only: dcrd is not an output
    # every atom at the origin: no frame anywhere
    assert bool((npairs[:B] == 0).all()) and bool((nclamped[:B] == 0).all()) and bool(torch.isnan(stats[:B * 2]).all())
    assert call(clamp=float("inf")) == 0 and not bool(dcrd[:-1].any())
    assert float(stats[-1]) == 77 and int(npairs[-1]) == 77 and int(nclamped[-1]) == 77 and float(dcrd[-1]) == 77     # the guards


# ----------------------------------------------------------------------------- 6. get_losses and train_step
def test_get_losses_under_fape():
    from oracle import batched, losses as olosses
    from protein_transformer_amd.train import get_losses
    dev = torch.device("cuda:0")
    model, _, args, batch, lens = _make(dev, "fape", lens=[40, 33, 21, 37])
    seq, ang, crd = (t.to(dev) for t in batch)
    pred = model(seq, ang)
    sc64 = pred.detach().cpu().double().view(len(lens), -1, 24)
    crd64 = batched.generate_coords_batched(olosses.inverse_trig_transform(sc64), batch[0], torch.float64).numpy()
    true, s = batch[2].numpy(), batch[0].numpy()
    free = [fape_reference(crd64[b], true[b], s[b], float("inf")) for b in range(len(lens))]
    args.fape_clamp = well_posed_clamp([r["d"] for r in free])
    per = [fape_reference(crd64[b], true[b], s[b], args.fape_clamp)["loss"] for b in range(len(lens))]
    seen = []
    pred.register_hook(lambda g: seen.append(g.detach().cpu().numpy()))
    out = get_losses(args, pred, ang, crd, seq)
    assert set(out) == TODAY_KEYS | {"fape-full"} and float(out["loss"]) == float(out["fape-full"]) and len(seen) == 1
    assert np.isfinite(seen[0]).all() and np.abs(seen[0]).max() > 0
    # the mean of the per-protein references; a model's first prediction is far from the truth (lever arms of tens of A), the
    # bound is the one derived in test_gradient_down_to_the_angles_against_fp64_autograd with m >= 1.2 A for a NeRF backbone
    bound = max((2 * 2e-3 + 11 * 2e-3 * r["lever"] / 1.2) / Z for r in free)
    print(f"get_losses: fape-full {float(out['loss'])} / {np.mean(per)}, bound {bound:.2e}")
    assert abs(float(out["loss"]) - np.mean(per)) <= bound
    # the ten reference keys keep their meaning: the dRMSD numbers of an `-l lndrmsd` call on the same prediction
    args.loss = "lndrmsd"
    plain = get_losses(args, pred.detach(), ang, crd, seq, do_backwards=False)
    assert set(plain) == TODAY_KEYS                                # and without `-l fape` the key is absent
    for k in TODAY_KEYS - {"loss", "rmsd-full"}:
        assert float(out[k]) == float(plain[k]), k
    args.loss = "drmsd"
    assert "fape-full" not in get_losses(args, pred.detach(), ang, crd, seq, do_backwards=False)
    # evaluation: the key, the same value, no gradient
    args.loss = "fape"
    with torch.no_grad():
        ev = get_losses(args, pred.detach(), ang, crd, seq, do_backwards=False, eval_mode=True, return_rmsd=True)
    assert set(ev) == TODAY_KEYS | {"fape-full"} and len(seen) == 1
    assert float(ev["fape-full"]) == float(out["fape-full"]) == float(ev["loss"]) and float(ev["rmsd-full"]) > 0
    args.backbone_loss = True
    with pytest.raises(ValueError):
        get_losses(args, pred.detach(), ang, crd, seq, do_backwards=False)


def test_five_adam_steps_lower_the_loss():
    from protein_transformer_amd.train import train_step
    dev = torch.device("cuda:0")
    model, opt, args, batch, _ = _make(dev, "fape", adam=True, lens=[64, 51, 40, 58], L_pad=64)
    args.fape_clamp = 10.0
    data = tuple(t.to(dev) for t in batch)
    trace = [float(train_step(model, opt, args, *data)["fape-full"]) for _ in range(5)]
    print("fape-full trace:", " ".join(f"{v:.5f}" for v in trace))
    assert np.isfinite(trace).all()
    assert trace[-1] < trace[0]


# ----------------------------------------------------------------------------- 7. data parallel
KEYS = ("loss", "fape-full", "drmsd-full", "lndrmsd-full", "drmsd-bb", "lndrmsd-bb", "mse-full")


def test_two_ranks_reproduce_the_single_process_step(tmp_path):
    """The twin of the test of this name in tests/test_gpu_slddt.py (its worker, its 3 + 2 split, its bars): the FAPE sum and count
    travel in LossReport's vector, so every rank reports the mean over the GLOBAL batch."""
    import torch.multiprocessing as mp

    import test_gpu_dp as base
    from protein_transformer_amd.train import train_step
    mp.spawn(_dp_worker, args=(2, base._free_port(), str(tmp_path), "fape", KEYS), nprocs=2, join=True)
    dev = torch.device("cuda:0")
    model, opt, args, batch, lens = _make(dev, "fape")
    # every protein of this batch has a frame (the two-residue one keeps N, CA, C of its first residue), so both shards report
    assert all(len(frame_residues(t, s)) > 0 for t, s in zip(batch[2].numpy(), batch[0].numpy()))
    start = model.flat_parameters()[0].cpu().numpy().copy()
    losses = train_step(model, opt, args, *(t.to(dev) for t in batch))
    full = model.flat_parameters()[0].cpu().numpy()
    f0, f1 = np.load(tmp_path / "flat0.npy"), np.load(tmp_path / "flat1.npy")
    assert np.array_equal(f0, f1)                                   # ranks stay in lock step
    upd, upd_dp = full - start, f0 - start
    assert np.linalg.norm(upd) > 0
    assert np.linalg.norm(upd_dp - upd) <= 1e-4 * np.linalg.norm(upd)
    l0, l1 = np.load(tmp_path / "loss0.npy"), np.load(tmp_path / "loss1.npy")
    assert np.array_equal(l0, l1)                                   # every rank reports the GLOBAL statistics
    assert l0 == pytest.approx(np.array([float(losses[k]) for k in KEYS]), rel=1e-5, abs=1e-7)
    assert 0.0 < float(losses["loss"]) < 1.0
