"""The smooth lDDT loss on the device (csrc/slddt.hip, losses.slddt_forward_backward, `train.py -l slddt`) against an fp64
restatement of its definition in include/ptamd.h, written here with torch autograd.

Inclusion is a threshold on fp32 true distances, so no case uses 15.0 as its cutoff: `well_posed_cutoff` sorts the true
inter-residue distances of the case inside [14.5, 15.5] (the ends of the window count as neighbours), asserts that the widest gap
between neighbours is at least 1e-3 A and places the cutoff in its middle - a condition on the input, checked on the CPU; no
pair is left out of a comparison, and `npairs` must equal the reference's count exactly.

The loss has a second threshold: sign(dp - dt) in the gradient, and eps'(0) != 0, so a pair whose exact delta is below the fp32
error of delta (~3e-6 A, below) gets a gradient of either sign, in any fp32 implementation.  A NeRF-built prediction has such
pairs by construction: the C(i)-N(i+1) bond has the same length in truth and prediction, so its delta is the rounding of the
stored coordinates, ~1e-9 .. 1e-6 A, and four flipped pairs of 26717 move the rel-L2 of `dcrd` by 3e-3.  (Through the NeRF
adjoint these pairs drop out - a bond length does not depend on an angle - so the angle-gradient checks are not affected.)  The
coordinate-gradient case therefore adds a fixed 0.1 A jitter to the NeRF-built prediction, and `reference` asserts for every
case that no included pair has delta < 1e-5 A, three times that fp32 error: again a condition on the input, checked on the CPU.

Bars.  Value: |loss - ref| <= 1e-5 / tau (delta carries a few fp32 ulps of a <= ~16 A distance ~ 3e-6 A, |eps'| <= 0.25 / tau,
plus ~1e-6 from exp / rcp and a fixed-order sum of values <= 1).  dcrd: rel-L2 < 1e-4 against the fp64 gradient, the bar of
tests/test_gpu_loss_path.py for the dRMSD coordinate gradient.  Down to the angles through the NeRF adjoint: rel-L2 < 1e-3, the
bar of the chain tests there.  Hand-computed two-atom cases: value abs 1e-6 (delta is off by at most an ulp of 18 A = 2e-6 A times
|eps'| <= 0.25, plus the ulps of four logistics), gradient rel 1e-5 (the same delta error times |eps''/eps'| <= 1, plus the ulps of
exp, rcp and rsq)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SLOTS, PAD = 14, 20
THRESHOLDS = (0.5, 1.0, 2.0, 4.0)
TAUS = (1.0, 0.25)


# ----------------------------------------------------------------------------- the fp64 reference
def present_atoms(true, seq):
    """Slot indices of one protein's atoms: non-pad residue, no NaN in the true coordinate."""
    true, seq = np.asarray(true), np.asarray(seq)
    ok = ~np.isnan(true).any(-1) & np.repeat(seq != PAD, SLOTS)
    return np.nonzero(ok)[0]


def true_distances(true, seq):
    """(idx, dt [n,n] fp64 of the fp32 coordinates, other [n,n] bool: different residues)."""
    idx = present_atoms(true, seq)
    t = np.asarray(true, np.float64)[idx]
    dt = np.sqrt(((t[:, None] - t[None]) ** 2).sum(-1))
    res = idx // SLOTS
    return idx, dt, res[:, None] != res[None]


def well_posed_cutoff(true, seq):
    """The cutoff of a case (one protein or a batch): the middle of the widest gap between neighbouring true inter-residue
    distances inside [14.5, 15.5]; asserts the gap is >= 1e-3 A."""
    true, seq = np.asarray(true), np.asarray(seq)
    if true.ndim == 2:
        true, seq = true[None], seq[None]
    near = [14.5, 15.5]
    for b in range(len(seq)):
        _, dt, other = true_distances(true[b], seq[b])
        d = dt[np.triu(other, 1)]
        near += d[(d >= 14.5) & (d <= 15.5)].tolist()
    near = np.sort(np.array(near))
    k = int(np.argmax(np.diff(near)))
    assert near[k + 1] - near[k] >= 1e-3, "pick another seed for this case: its distances crowd the window"
    return float(np.float32(0.5 * (near[k] + near[k + 1])))


def slddt_reference(pred, true, seq, cutoff, tau, bad=()):
    """One protein in fp64: (loss, npairs, d loss / d pred [L*14,3], delta of the included pairs).  `pred`: array, or an fp64
    torch tensor inside an autograd graph (then the gradient slot is None and the loss is a tensor).  `bad`: slots whose
    predicted coordinate is unusable - their pairs are counted and score 0."""
    idx, dt, other = true_distances(true, seq)
    incl = np.triu(other & (dt < cutoff), 1)
    npairs = int(incl.sum())
    graph = torch.is_tensor(pred) and pred.requires_grad
    p_all = pred if graph else torch.tensor(np.asarray(pred, np.float64), requires_grad=True)
    if npairs == 0:
        return (p_all.sum() * 0 + float("nan") if graph else float("nan")), 0, (None if graph else np.zeros(p_all.shape)), np.zeros(0)
    usable = ~np.isin(idx, np.asarray(bad, np.int64))
    ii, jj = np.nonzero(incl)
    scored = torch.tensor(usable[ii] & usable[jj])
    p = p_all[torch.tensor(idx)]
    p = torch.where(torch.tensor(usable)[:, None], p, torch.zeros_like(p))
    diff = p[torch.tensor(ii)] - p[torch.tensor(jj)]
    dp = torch.sqrt((diff ** 2).sum(-1) + 1e-30)
    delta = (dp - torch.tensor(dt[ii, jj])).abs()
    eps = sum(torch.sigmoid((t - delta) / tau) for t in THRESHOLDS) / 4
    loss = 1 - torch.where(scored, eps, torch.zeros_like(eps)).sum() / npairs
    if graph:
        return loss, npairs, None, delta.detach().numpy()
    loss.backward()
    return float(loss.detach()), npairs, p_all.grad.numpy(), delta.detach().numpy()


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30)


# ----------------------------------------------------------------------------- cases
def cloud(n_atoms, per_res, rng, L=None, line=0.0, spread=8.0):
    """One protein of exactly `n_atoms` present atoms, `per_res` per residue (the last residue may hold fewer), the rest of the
    slots absent (NaN): (pred, true, seq).  `line` > 0: residues strung along x at that spacing (an extended chain)."""
    n_res = -(-n_atoms // per_res)
    L = L or n_res
    true = np.full((L * SLOTS, 3), np.nan, np.float32)
    seq = np.full(L, PAD, np.int64)
    seq[:n_res] = rng.integers(0, 20, n_res)
    slots = np.array([r * SLOTS + s for r in range(n_res) for s in range(per_res)][:n_atoms], np.int64)
    xyz = rng.normal(0, 1.5 if line else spread, (n_atoms, 3))
    if line:
        xyz[:, 0] += line * (slots // SLOTS)
    true[slots] = xyz
    true[n_res * SLOTS:] = 0.0                                    # batch padding carries zeros, not NaN
    pred = rng.normal(0, 5.0, (L * SLOTS, 3)).astype(np.float32)  # absent slots hold anything finite
    pred[slots] = true[slots] + rng.normal(0, 1.5, (n_atoms, 3))
    return pred, true, seq


def stack(items):
    return tuple(np.stack([it[k] for it in items]) for k in range(3))


def _tiny():
    """1 atom; 2 atoms in one residue (no pair); 2 atoms in two residues; no present atom; a fully padded row."""
    rng = np.random.default_rng(101)
    L = 3
    one, same, two = cloud(1, 1, rng, L), cloud(2, 2, rng, L), cloud(2, 1, rng, L, spread=3.0)
    none = cloud(4, 2, rng, L)
    none[1][:] = np.nan
    padded = cloud(4, 2, rng, L)
    padded[2][:] = PAD
    padded[1][:] = 0.0
    return stack([one, same, two, none, padded])


def _edges():
    """63, 64, 65, 128, 129 atoms (tiles are 64 compacted atoms), five atoms per residue, rows padded to the longest."""
    rng = np.random.default_rng(202)
    return stack([cloud(n, 5, rng, L=26) for n in (63, 64, 65, 128, 129)])


def _extended():
    """~200 residues strung out over 760 A, 8 atoms each: 25 tiles, most tile pairs farther apart than the cutoff."""
    rng = np.random.default_rng(303)
    return stack([cloud(1597, 8, rng, line=3.8)])


def _chains():
    """NeRF-built chains of 40, 33 and 21 residues in rows of 48 (truth with NaN atoms scattered: 10 % of the residues missing
    and, on top, single atoms; one whole residue more knocked out by hand) and a fully padded tail row.  The prediction is the
    chain built from the noised angles plus a 0.1 A jitter (module docstring: no pair may sit on delta = 0)."""
    from oracle import batched
    from protein_transformer_amd import synthetic
    build = lambda ang, seq: batched.generate_coords_batched(ang, seq, torch.float64)      # noqa: E731
    batch = synthetic.make_batch([40, 33, 21], L_pad=48, seed=77, build_coords=build, frac_missing=0.1)
    true = batch["true_crd"].numpy().copy()
    rng = np.random.default_rng(404)
    real = np.repeat(batch["seq"].numpy() != PAD, SLOTS, axis=1)
    true[(rng.random(true.shape[:2]) < 0.05) & real] = np.nan           # scattered atoms
    true[0, 7 * SLOTS:8 * SLOTS] = np.nan                               # a whole residue
    pred = batched.generate_coords_batched(batch["start_ang_rad"], batch["seq"], torch.float64).float().numpy()
    pred = pred + rng.normal(0, 0.1, pred.shape).astype(np.float32)
    tail = np.zeros_like(true[:1])                                      # the fully padded row: zeros behind pad ids
    return (np.concatenate([pred, tail]), np.concatenate([true, tail]),
            np.concatenate([batch["seq"].numpy(), np.full((1, 48), PAD, np.int64)]), batch)


CASES = {"tiny": _tiny, "edges": _edges, "extended": _extended, "chains": _chains}
_cache = {}


def case(name):
    """(pred, true, seq, cutoff) of a case, built once."""
    if name not in _cache:
        pred, true, seq = CASES[name]()[:3]
        _cache[name] = (pred, true, seq, well_posed_cutoff(true, seq))
    return _cache[name]


def reference(name, tau):
    """Per protein (loss, npairs, grad, delta), computed once per (case, tau) and shared.  Asserts the case is well-posed for
    the gradient: no included pair within 1e-5 A of delta = 0, where sign(dp - dt) is decided by rounding."""
    key = (name, tau)
    if key not in _cache:
        pred, true, seq, cutoff = case(name)
        _cache[key] = [slddt_reference(pred[b], true[b], seq[b], cutoff, tau) for b in range(len(seq))]
        for b, ref in enumerate(_cache[key]):
            assert ref[1] == 0 or ref[3].min() >= 1e-5, f"pick another seed for {name}[{b}]: a pair sits on delta = 0"
    return _cache[key]


def run(pred, true, seq, cutoff, tau, need_grad=True):
    """losses.slddt_forward_backward on numpy inputs -> (stats [B,2], npairs [B], dcrd [B,L*14,3] or None) as numpy."""
    from protein_transformer_amd.losses import slddt_forward_backward
    dev = torch.device("cuda:0")
    p, t, s = (torch.as_tensor(np.asarray(x)) for x in (pred, true, seq))
    if p.dim() == 2:
        p, t, s = p[None], t[None], s[None]
    st, n, g = slddt_forward_backward(p.float().to(dev), t.float().to(dev), s.to(dev), need_grad=need_grad, cutoff=cutoff,
                                      temperature=tau)
    return st.cpu().numpy(), n.cpu().numpy(), (g.cpu().numpy() if g is not None else None)


# ----------------------------------------------------------------------------- 1. value, count, gradient against fp64
@pytest.mark.parametrize("tau", TAUS)
@pytest.mark.parametrize("name", list(CASES))
def test_value_count_and_gradient_against_fp64(name, tau):
    pred, true, seq, cutoff = case(name)
    stats, npairs, dcrd = run(pred, true, seq, cutoff, tau)
    assert np.isfinite(dcrd).all()
    for b, (loss, n, grad, _) in enumerate(reference(name, tau)):
        print(f"{name}[{b}] tau {tau}: npairs {npairs[b]} / {n}, loss {stats[b, 0]} / {loss}, "
              f"dcrd rel-L2 {rel_l2(dcrd[b], grad) if n else 0.0:.2e}")
        assert npairs[b] == n
        if n == 0:
            assert np.isnan(stats[b]).all() and not dcrd[b].any()
            continue
        assert abs(stats[b, 0] - loss) <= 1e-5 / tau
        assert abs(stats[b, 1] - (1 - loss)) <= 1e-5 / tau
        assert rel_l2(dcrd[b], grad) < 1e-4
        absent = np.setdiff1d(np.arange(dcrd.shape[1]), present_atoms(true[b], seq[b]))
        assert not dcrd[b, absent].any()                           # empty slots and padded residues get zeros


def test_the_cases_are_the_shapes_they_claim():
    counts = lambda name: [len(present_atoms(t, s)) for t, s in zip(*case(name)[1:3])]       # noqa: E731
    assert counts("tiny") == [1, 2, 2, 0, 0] and counts("edges") == [63, 64, 65, 128, 129] and counts("extended") == [1597]
    assert [r[1] for r in reference("tiny", 1.0)] == [0, 0, 1, 0, 0]
    idx, dt, _ = true_distances(case("extended")[1][0], case("extended")[2][0])
    tiles = -(-len(idx) // 64)
    far = sum(dt[i * 64:(i + 1) * 64, j * 64:(j + 1) * 64].min() > 30.0 for i in range(tiles) for j in range(i, tiles))
    assert far > 0.7 * tiles * (tiles + 1) / 2                     # most tile pairs lie beyond any box margin


@pytest.mark.parametrize("tau", TAUS)
def test_gradient_down_to_the_angles_against_fp64_autograd(tau):
    from oracle import batched, losses as olosses
    from protein_transformer_amd.losses import batch_loss
    dev = torch.device("cuda:0")
    _, true, seq, batch = _chains()
    cutoff, true, seq = case("chains")[3], true[:3], seq[:3]         # (without the fully padded row: the model never sees one)
    ang = batch["start_ang_rad"]
    sincos = (torch.stack([torch.cos(ang), torch.sin(ang)], -1).reshape(len(seq), -1, 24) * 0.9).float()
    out = batch_loss(sincos.to(dev), torch.from_numpy(true).to(dev), batch["seq"].to(dev), do_backward=True, slddt=(cutoff, tau))
    assert {f for f, v in out._asdict().items() if v is None} == {"true_ang", "clash"} and int(out.status.item()) == 0
    grad, sl = out.grad.cpu().numpy(), out.per_protein.cpu().numpy()
    sc64 = sincos.double().clone().requires_grad_()
    crd64 = batched.generate_coords_batched(olosses.inverse_trig_transform(sc64), batch["seq"], torch.float64)
    total = 0
    for b in range(len(seq)):
        loss, n, _, _ = slddt_reference(crd64[b], true[b], seq[b], cutoff, tau)
        if n:
            total = total + loss                                   # the back-propagated quantity is the SUM over proteins
            # two NeRF chains, fp32 and fp64, stand behind these: coordinates within 2e-3 A (the stated tolerance of
            # tests/test_gpu_loss_path.py for L <= 128), so delta within 4e-3 A, times |eps'| <= 0.25 / tau
            assert abs(sl[b] - float(loss)) <= 1e-3 / tau
        else:
            assert np.isnan(sl[b])
    total.backward()
    for b in range(len(seq)):
        print(f"chains[{b}] tau {tau}: angle gradient rel-L2 {rel_l2(grad[b], sc64.grad[b].numpy()):.2e}")
        if np.isnan(sl[b]):
            assert not grad[b].any()
        else:
            assert rel_l2(grad[b], sc64.grad[b].numpy()) < 1e-3


# ----------------------------------------------------------------------------- 2. closed forms
def test_prediction_equal_to_truth():
    _, true, seq, cutoff = case("chains")
    pred = np.nan_to_num(true, nan=0.0)
    stats, npairs, dcrd = run(pred, true, seq, cutoff, 1.0)
    want = 1 - 0.25 * sum(1 / (1 + np.exp(-t)) for t in THRESHOLDS)
    assert abs(want - 0.195918) < 1e-6
    for b in range(len(seq)):
        if npairs[b]:
            assert abs(stats[b, 0] - 0.195918) <= 1e-6
    assert npairs[:3].all() and not dcrd.any()                     # exactly zero everywhere


@pytest.mark.parametrize("off", [0.25, 1.5, 3.0, 8.0])
def test_two_atoms_by_hand(off):
    L = 2
    true = np.full((L * SLOTS, 3), np.nan, np.float32)
    true[1], true[SLOTS + 1] = (0, 0, 0), (10, 0, 0)
    pred = np.zeros((L * SLOTS, 3), np.float32)
    pred[SLOTS + 1] = (10 + off, 0, 0)
    stats, npairs, dcrd = run(pred, true, np.zeros(L, np.int64), 15.0, 1.0)
    sig = np.array([1 / (1 + np.exp(off - t)) for t in THRESHOLDS])
    slope = 0.25 * (sig * (1 - sig)).sum()                         # -eps'(delta); sign(dp - dt) = +1
    assert npairs[0] == 1
    assert abs(stats[0, 0] - (1 - 0.25 * sig.sum())) <= 1e-6 and abs(stats[0, 1] - 0.25 * sig.sum()) <= 1e-6
    assert dcrd[0, SLOTS + 1, 0] == pytest.approx(slope, rel=1e-5) and dcrd[0, 1, 0] == pytest.approx(-slope, rel=1e-5)
    assert not dcrd[0, :, 1:].any() and np.count_nonzero(dcrd[0]) == 2
    # the same pair compressed instead of stretched: the two gradient vectors change sides
    pred[SLOTS + 1] = (10 - off, 0, 0)
    stats2, _, dcrd2 = run(pred, true, np.zeros(L, np.int64), 15.0, 1.0)
    assert abs(stats2[0, 0] - stats[0, 0]) <= 1e-6
    assert dcrd2[0, SLOTS + 1, 0] == pytest.approx(-slope, rel=1e-5) and dcrd2[0, 1, 0] == pytest.approx(slope, rel=1e-5)


# ----------------------------------------------------------------------------- 3. consistency with the metric
@pytest.mark.parametrize("name", ["edges", "chains"])
def test_consistent_with_the_lddt_metric(name):
    from protein_transformer_amd.eval_metrics import lddt_batch
    dev = torch.device("cuda:0")
    pred, true, seq, cutoff = case(name)
    tau = 1.0 / 64
    stats, npairs, _ = run(pred, true, seq, cutoff, tau, need_grad=False)
    score, _, counts = lddt_batch(torch.from_numpy(pred).float().to(dev), torch.from_numpy(true).float().to(dev),
                                  torch.from_numpy(seq).to(dev), cutoff)
    assert np.array_equal(2 * npairs, counts[:, :, 0, 0].sum(1).cpu().numpy().astype(np.int64))
    hard = score[:, 0].cpu().numpy()
    for b, (_, n, _, delta) in enumerate(reference(name, 1.0)):
        if n == 0:
            assert np.isnan(stats[b, 1]) and np.isnan(hard[b])
            continue
        unsure = np.mean([np.abs(delta - t) < 12 * tau for t in THRESHOLDS])
        print(f"{name}[{b}]: smooth {stats[b, 1]:.6f} hard {hard[b]:.6f} bound {unsure + np.exp(-12):.6f}")
        assert abs(stats[b, 1] - hard[b]) <= unsure + np.exp(-12)


# ----------------------------------------------------------------------------- 4. determinism and independence
@pytest.mark.parametrize("name", ["edges", "chains"])
def test_bits_do_not_depend_on_the_run_the_batch_or_the_padding(name):
    pred, true, seq, cutoff = case(name)
    first = run(pred, true, seq, cutoff, 1.0)
    again = run(pred, true, seq, cutoff, 1.0)
    for a, b in zip(first, again):
        assert np.array_equal(a, b, equal_nan=True)
    fwd = run(pred, true, seq, cutoff, 1.0, need_grad=False)
    assert fwd[2] is None and np.array_equal(fwd[0], first[0], equal_nan=True) and np.array_equal(fwd[1], first[1])
    for b in range(len(seq)):
        alone = run(pred[b], true[b], seq[b], cutoff, 1.0)
        for a, w in zip(alone, first):
            assert np.array_equal(a[0], w[b], equal_nan=True), b
        n_res = int((seq[b] != PAD).sum())
        if 0 < n_res < seq.shape[1]:                               # the same protein in a row cut to its own length
            cut = run(pred[b, :n_res * SLOTS], true[b, :n_res * SLOTS], seq[b, :n_res], cutoff, 1.0)
            assert np.array_equal(cut[0][0], first[0][b], equal_nan=True) and cut[1][0] == first[1][b]
            assert np.array_equal(cut[2][0], first[2][b, :n_res * SLOTS])


# ----------------------------------------------------------------------------- 5. non-finite prediction
@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")])
def test_a_non_finite_predicted_atom_scores_zero_and_nothing_traps(value):
    pred, true, seq, cutoff = case("edges")
    b = 4
    slot = int(present_atoms(true[b], seq[b])[70])
    p = pred[b].copy()
    p[slot, 1] = value
    stats, npairs, dcrd = run(p, true[b], seq[b], cutoff, 1.0)
    q = p.copy()
    q[slot] = 0.0
    loss, n, grad, _ = slddt_reference(q, true[b], seq[b], cutoff, 1.0, bad=[slot])
    assert npairs[0] == n == reference("edges", 1.0)[b][1]          # inclusion depends on the truth only
    assert abs(stats[0, 0] - loss) <= 1e-5 and loss > reference("edges", 1.0)[b][0]
    assert np.isfinite(dcrd).all() and not dcrd[0, slot].any()
    assert rel_l2(dcrd[0], grad) < 1e-4


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals_leave_the_outputs_untouched():
    from protein_transformer_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    B, L = 2, 5
    crd = torch.zeros(B, L * SLOTS, 3, device=dev)
    seq = torch.zeros(B, L, dtype=torch.int64, device=dev)
    stats = torch.full((B, 2), 77.0, device=dev)
    npairs = torch.full((B,), 77, dtype=torch.int64, device=dev)
    dcrd = torch.full((B, L * SLOTS, 3), 77.0, device=dev)
    need = lib.ptamd_slddt_workspace_bytes(B, L)
    assert need > 0 and lib.ptamd_slddt_workspace_bytes(0, L) == 0 and lib.ptamd_slddt_workspace_bytes(B, -1) == 0
    assert lib.ptamd_slddt_workspace_bytes(B, (2 ** 31 - 1) // 28 + 1) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    P = _lib.ptr

    def call(pred=crd, true=crd, s=seq, b=B, l=L, cutoff=15.0, tau=1.0, st=stats, n=npairs, g=dcrd, w=ws, wb=None):
        rc = lib.ptamd_slddt_fwd_bwd(P(pred), P(true), P(s), b, l, cutoff, tau, P(st), P(n), P(g), P(w), need if wb is None else wb,
                                     _lib.stream())
        torch.cuda.synchronize()
        return rc

    def untouched():
        return bool((stats == 77).all()) and bool((npairs == 77).all()) and bool((dcrd == 77).all())
    nonpos = (0.0, -1.0, float("inf"), float("nan"))
    bad_shape = ([dict(b=0), dict(b=-1), dict(l=0), dict(l=-3), dict(l=(2 ** 31 - 1) // 28 + 1), dict(pred=None), dict(true=None),
                  dict(s=None), dict(st=None), dict(n=None)] + [dict(cutoff=v) for v in nonpos] + [dict(tau=v) for v in nonpos])
    for kw in bad_shape:
        assert call(**kw) == -1, kw                          # PTAMD_ERR_BAD_SHAPE
        assert untouched(), kw
    for kw in (dict(w=None), dict(wb=need - 1), dict(wb=0)):
        assert call(**kw) == -3, kw                          # PTAMD_ERR_WORKSPACE
        assert untouched(), kw
    assert call(g=None) == 0 and bool((dcrd == 77).all())    # forward only: dcrd is not an output
    assert bool((npairs == SLOTS * SLOTS * L * (L - 1) // 2).all())      # every atom at the origin: every inter-residue pair
    assert call() == 0
    assert abs(float(stats[0, 0]) - 0.195918) <= 1e-6 and not bool(dcrd.any())


# ----------------------------------------------------------------------------- 7. get_losses
LENS = [40, 33, 2, 21, 37]            # protein 2: the atoms of its second residue are absent - no inter-residue pair, no score
TODAY_KEYS = {"loss", "drmsd-full", "lndrmsd-full", "drmsd-bb", "lndrmsd-bb", "combined-full", "mse-full", "mse-bb", "mse-sc",
              "rmsd-full"}


def _make(dev, loss, adam=False, lens=LENS, L_pad=48, well_posed=False):
    """A small enc-only model (d 64, 2 layers, dropout 0), its optimizer, args and a ragged batch on the host.  `well_posed`: the
    cutoff of the run is placed like a case's (for the comparison with fp64; seed 17 leaves a gap of 2.6e-3 A); else 15 A."""
    import types

    from protein_transformer_amd import synthetic
    from protein_transformer_amd.models.encoder_only import EncoderOnlyTransformer
    from protein_transformer_amd.optim import FusedAdam, FusedSGD
    from protein_transformer_amd.protein.Sequence import VOCAB
    from protein_transformer_amd.protein.Structure import nerf_forward
    build = lambda ang, seq: nerf_forward(ang.to(dev), seq.to(dev))[0]           # noqa: E731
    batch = synthetic.make_batch(lens, L_pad=L_pad, seed=17, build_coords=build, frac_missing=0.05)
    if 2 in lens:
        batch["true_crd"][lens.index(2), SLOTS:2 * SLOTS] = float("nan")
    am = synthetic.angle_means(batch["true_ang"])
    torch.manual_seed(123)
    model = EncoderOnlyTransformer(2, 4, 64, 128, L_pad, VOCAB, am, True, dropout=0.0)
    with torch.no_grad():
        model.output_projection.weight.normal_(0, 0.05)
    model.set_dropout(0.0)
    model = model.to(dev).train()
    opt = FusedAdam(model, lr=1e-3) if adam else FusedSGD(model, lr=1e-2, weight_decay=10e-3)
    data = tuple(batch[k] for k in ("seq", "true_ang", "true_crd"))
    args = types.SimpleNamespace(loss=loss, combined_drmsd_weight=0.5, backbone_loss=False, clip=1.0, lr_scheduling="plateau",
                                 slddt_cutoff=well_posed_cutoff(data[2].numpy(), data[0].numpy()) if well_posed else 15.0,
                                 slddt_temperature=1.0)
    return model, opt, args, data, lens


def test_get_losses_under_slddt():
    from oracle import batched, losses as olosses
    from protein_transformer_amd.train import get_losses
    dev = torch.device("cuda:0")
    model, _, args, batch, lens = _make(dev, "slddt", well_posed=True)
    seq, ang, crd = (t.to(dev) for t in batch)
    pred = model(seq, ang)
    seen = []
    pred.register_hook(lambda g: seen.append(g.detach().cpu().numpy()))
    out = get_losses(args, pred, ang, crd, seq)
    assert set(out) == TODAY_KEYS | {"slddt-full"} and float(out["loss"]) == float(out["slddt-full"]) and len(seen) == 1
    # the gradient that arrives at `pred`: fp64 autograd of the SUM over proteins, from the same (cos, sin) values
    sc64 = pred.detach().cpu().double().view(len(lens), -1, 24).requires_grad_()
    crd64 = batched.generate_coords_batched(olosses.inverse_trig_transform(sc64), batch[0], torch.float64)
    per = [slddt_reference(crd64[b], batch[2][b].numpy(), batch[0][b].numpy(), args.slddt_cutoff, 1.0) for b in range(len(lens))]
    assert [p[1] > 0 for p in per] == [True, True, False, True, True]
    sum(p[0] for p in per if p[1]).backward()
    got = seen[0].reshape(len(lens), -1, 24)
    for b in range(len(lens)):
        if per[b][1]:
            assert rel_l2(got[b], sc64.grad[b].numpy()) < 1e-3, b
        else:
            assert not got[b].any()
    # mean over the proteins with a score (bar: 4e-3 A between the fp32 and the fp64 NeRF chain times |eps'| <= 0.25, as above)
    assert abs(float(out["loss"]) - np.mean([float(p[0]) for p in per if p[1]])) <= 1e-3
    # the ten reference keys keep their meaning: the dRMSD numbers of an `-l lndrmsd` call on the same prediction
    args.loss = "lndrmsd"
    plain = get_losses(args, pred.detach(), ang, crd, seq, do_backwards=False)
    assert set(plain) == TODAY_KEYS                                # and without `-l slddt` the key is absent
    for k in TODAY_KEYS - {"loss", "rmsd-full"}:
        assert float(out[k]) == float(plain[k]), k
    assert float(out["drmsd-full"]) > 0
    # evaluation: the key, no gradient
    args.loss = "slddt"
    with torch.no_grad():
        ev = get_losses(args, pred.detach(), ang, crd, seq, do_backwards=False, eval_mode=True, return_rmsd=True)
    assert set(ev) == TODAY_KEYS | {"slddt-full"} and len(seen) == 1
    assert float(ev["slddt-full"]) == float(out["slddt-full"]) == float(ev["loss"]) and float(ev["rmsd-full"]) > 0
    args.backbone_loss = True
    with pytest.raises(ValueError):
        get_losses(args, pred.detach(), ang, crd, seq, do_backwards=False)


# ----------------------------------------------------------------------------- 8. it trains
def test_thirty_adam_steps_lower_the_loss():
    from protein_transformer_amd.train import train_step
    dev = torch.device("cuda:0")
    model, opt, args, batch, _ = _make(dev, "slddt", adam=True, lens=[64, 51, 40, 58], L_pad=64)
    data = tuple(t.to(dev) for t in batch)
    trace = [float(train_step(model, opt, args, *data)["loss"]) for _ in range(30)]
    print("loss trace:", " ".join(f"{v:.4f}" for v in trace))
    assert np.isfinite(trace).all()
    assert np.mean(trace[-5:]) < np.mean(trace[:5])


# ----------------------------------------------------------------------------- 9. data parallel
KEYS = ("loss", "slddt-full", "drmsd-full", "lndrmsd-full", "drmsd-bb", "lndrmsd-bb", "mse-full")


def _dp_worker(rank, world, port, out_dir, loss="slddt", keys=KEYS):
    """One rank of a two-process gloo job on one GPU: a `train_step` under `-l <loss>` on its shard of `_make`'s batch (shared with
    tests/test_gpu_fape.py)."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0",
                      PTAMD_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), here]
    import test_gpu_dp as base
    from protein_transformer_amd import dp
    from protein_transformer_amd.train import train_step
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    dp.init_from_env()
    model, opt, args, batch, lens = _make(dev, loss)
    dp.attach(model)
    (seq, ang, crd), n_res = base._shard(batch, lens, world, rank)
    assert seq.shape[0] == (3 if rank == 0 else 2)
    losses = train_step(model, opt, args, seq.to(dev), ang.to(dev), crd.to(dev), n_res=n_res)
    np.save(os.path.join(out_dir, f"flat{rank}.npy"), model.flat_parameters()[0].cpu().numpy())
    np.save(os.path.join(out_dir, f"loss{rank}.npy"), np.array([float(losses[k]) for k in keys]))
    np.save(os.path.join(out_dir, f"held{rank}.npy"), np.array([lens.index(2) in dp.shard_indices(lens, world, rank)]))
    dp.barrier()
    dp.shutdown()


def test_two_ranks_reproduce_the_single_process_step(tmp_path):
    import torch.multiprocessing as mp

    import test_gpu_dp as base
    from protein_transformer_amd.train import train_step
    mp.spawn(_dp_worker, args=(2, base._free_port(), str(tmp_path)), nprocs=2, join=True)
    dev = torch.device("cuda:0")
    model, opt, args, batch, lens = _make(dev, "slddt")
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
    assert np.load(tmp_path / "held0.npy")[0] != np.load(tmp_path / "held1.npy")[0]      # one shard held the protein without a score
