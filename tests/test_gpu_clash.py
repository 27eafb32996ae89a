"""The steric clash term on the device (csrc/clash.hip, losses.clash_forward_backward, eval_metrics.clash_batch) against the
fp64 restatement of its definition in tests/clash_ref.py.

The pair term has a kink, so every case satisfies a condition on its INPUT that the reference asserts: no candidate pair within
1e-4 A of r_a + r_b - tau - d = 0 (tests/clash_ref.py).  Under it `nclash` must match exactly.

Bars, all taken from the project.  Value: |loss - ref| <= 1e-5, the value bar of the smooth lDDT (a term carries a few fp32 ulps
of a distance below 3.6 A, the sum is divided by the atom count).  dcrd: rel-L2 < 1e-4 against the fp64 gradient, the bar of
tests/test_gpu_loss_path.py for the coordinate gradient.  Down to the angles through the NeRF adjoint: rel-L2 < 1e-3, the chain
bar there.  nclash and n: exact.  Hand-built cases: value abs 1e-6 (one or two terms, each off by an ulp of a distance and of the
division), gradient rel 1e-5 (a unit vector from v_rsq_f32, over n)."""
import numpy as np
import pytest
import torch

import clash_ref as R

pytestmark = pytest.mark.gpu

SLOTS, PAD = R.SLOTS, R.PAD
BIG = "WWWYRF"                 # residue types of 11 to 14 atoms: 45 residues pass 8 tiles of 64 atoms


# ----------------------------------------------------------------------------- cases: (crd [B,L*14,3], seq [B,L])
def _chain(n_atoms=None, seq=None, seed=0, L_pad=None, letters=R.AA):
    rng = np.random.default_rng(seed)
    if seq is None:
        seq = R.sequence_with_atoms(n_atoms, rng, letters)
    return R.build_chain(seq, rng, L_pad)


def _single(n_atoms, seed):
    crd, seq = _chain(n_atoms, seed=seed)
    return crd[None], seq[None]


def _long():
    """45 residues of the largest types: more than 8 column tiles (a second chunk) and more than 4 row tiles (a second strip)."""
    rng = np.random.default_rng(45)
    crd, seq = R.build_chain(np.array([R.AA.index(c) for c in rng.choice(list(BIG), 45)]), rng)
    return crd[None], seq[None]


def _folded():
    """A chain whose last residue is carried back onto residue 0 (a rigid shift: the kernel does not know the chain is broken):
    the two are tiles apart in slot order, and every tile between them is far from both."""
    crd, seq = _chain(seq=np.random.default_rng(7).integers(0, 20, 40), seed=7)
    L = len(seq)
    first, last = slice(0, SLOTS), slice((L - 1) * SLOTS, L * SLOTS)
    n_last = len(R.atoms_of(seq[-1:])[0])
    shift = crd[first][1] - crd[last][1] + np.float32([0.9, 0.7, 0.5])           # CA onto CA, a little off
    crd[(L - 1) * SLOTS:(L - 1) * SLOTS + n_last] += shift
    return crd[None], seq[None]


def _clusters():
    """The second half of a chain moved 100 A away: no pair across, boxes far apart."""
    crd, seq = _chain(seq=np.random.default_rng(8).integers(0, 20, 30), seed=8)
    idx = R.atoms_of(seq)[0]
    far = idx[idx >= 15 * SLOTS]
    crd[far, 0] += 100.0
    return crd[None], seq[None]


def _ragged():
    """B = 3: 24 and 17 residues in rows of 30, and a fully padded row."""
    a = _chain(seq=np.random.default_rng(9).integers(0, 20, 24), seed=9, L_pad=30)
    b = _chain(seq=np.random.default_rng(10).integers(0, 20, 17), seed=10, L_pad=30)
    return np.stack([a[0], b[0], np.zeros_like(a[0])]), np.stack([a[1], b[1], np.full(30, PAD, np.int64)])


CASES = {"n63": lambda: _single(63, 163), "n64": lambda: _single(64, 164), "n65": lambda: _single(65, 168),
         "n129": lambda: _single(129, 229), "long": _long, "folded": _folded, "clusters": _clusters, "ragged": _ragged}
_cache = {}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def reference(name, tau=R.TOLERANCE):
    """Per protein (loss, nclash, n, grad, margin) in fp64, computed once per (case, tau) and shared; the reference asserts the
    margin of the case."""
    key = (name, tau)
    if key not in _cache:
        crd, seq = case(name)
        _cache[key] = [R.clash_reference(crd[b], seq[b], tau) for b in range(len(seq))]
    return _cache[key]


def run(crd, seq, tau=R.TOLERANCE, need_grad=True, weight=1.0, accumulate_into=None):
    """losses.clash_forward_backward on numpy inputs -> (stats [B,2], nclash [B], dcrd [B,L*14,3] or None) as numpy."""
    from protein_transformer_amd.losses import clash_forward_backward
    dev = torch.device("cuda:0")
    c, s = torch.as_tensor(np.asarray(crd)), torch.as_tensor(np.asarray(seq))
    if c.dim() == 2:
        c, s = c[None], s[None]
    acc = None if accumulate_into is None else torch.as_tensor(accumulate_into).float().to(dev).contiguous()
    st, n, g = clash_forward_backward(c.float().to(dev), s.to(dev), need_grad=need_grad, tolerance=tau, weight=weight,
                                      accumulate_into=acc)
    return st.cpu().numpy(), n.cpu().numpy(), (g.cpu().numpy() if g is not None else None)


def absent_slots(seq_row):
    return np.setdiff1d(np.arange(len(seq_row) * SLOTS), R.atoms_of(seq_row)[0])


# ----------------------------------------------------------------------------- 1. value, count, gradient against fp64
@pytest.mark.parametrize("name", list(CASES))
def test_value_count_and_gradient_against_fp64(name):
    crd, seq = case(name)
    stats, nclash, dcrd = run(crd, seq)
    fwd_stats, fwd_nclash, none = run(crd, seq, need_grad=False)
    assert none is None and np.array_equal(stats, fwd_stats, equal_nan=True) and np.array_equal(nclash, fwd_nclash)
    assert np.isfinite(dcrd).all()
    for b, (loss, n_hit, n, grad, margin) in enumerate(reference(name)):
        print(f"{name}[{b}]: n {stats[b, 1]:.0f} / {n}, nclash {nclash[b]} / {n_hit}, loss {stats[b, 0]} / {loss}, margin {margin:.1e}, "
              f"dcrd rel-L2 {R.rel_l2(dcrd[b], grad) if n_hit else 0.0:.2e}")
        assert stats[b, 1] == n and nclash[b] == n_hit
        if n == 0:
            assert np.isnan(stats[b, 0]) and not dcrd[b].any()
            continue
        assert abs(stats[b, 0] - loss) <= 1e-5
        assert R.rel_l2(dcrd[b], grad) < 1e-4
        assert not dcrd[b, absent_slots(seq[b])].any()               # exactly zero in every slot that is not an atom


def test_the_cases_are_the_shapes_they_claim():
    n = lambda name: [r[2] for r in reference(name)]                 # noqa: E731
    assert [n(k) for k in ("n63", "n64", "n65", "n129")] == [[63], [64], [65], [129]]
    assert n("long")[0] > 8 * 64 and case("long")[1].shape[1] == 45
    assert n("ragged")[2] == 0 and n("ragged")[0] > 64 and n("ragged")[1] > 64
    assert all(r[1] > 0 for name in CASES for r in reference(name) if r[2])       # every protein with atoms has clashes
    # folded: residue 0 clashes with the last residue, and they lie in the first and the last tile
    crd, seq = case("folded")
    idx, rad, ii, jj = R.candidate_pairs(seq[0])
    d = np.linalg.norm(crd[0][idx[ii]].astype(np.float64) - crd[0][idx[jj]], axis=1)
    hit = rad[ii] + rad[jj] - R.TOLERANCE - d > 0
    ends = hit & (idx[ii] // SLOTS == 0) & (idx[jj] // SLOTS == seq.shape[1] - 1)
    assert ends.sum() >= 3 and (ii[ends] // 64).max() == 0 and (jj[ends] // 64).min() >= 3
    # clusters: nothing across the gap
    crd, seq = case("clusters")
    idx = R.atoms_of(seq[0])[0]
    x = crd[0][idx, 0]
    assert x[idx < 15 * SLOTS].max() + 50 < x[idx >= 15 * SLOTS].min()


@pytest.mark.parametrize("tau", [0.0, 2.5])
def test_other_tolerances(tau):
    crd, seq = case("n129")
    stats, nclash, dcrd = run(crd, seq, tau)
    loss, n_hit, n, grad, _ = reference("n129", tau)[0]
    print(f"tau {tau}: nclash {nclash[0]} / {n_hit}, loss {stats[0, 0]} / {loss}, dcrd rel-L2 {R.rel_l2(dcrd[0], grad):.2e}")
    assert nclash[0] == n_hit and abs(stats[0, 0] - loss) <= 1e-5 and R.rel_l2(dcrd[0], grad) < 1e-4
    # beyond 2 * 1.8 no pair can violate: zero, not NaN
    stats, nclash, dcrd = run(crd, seq, 3.7)
    assert stats[0, 0] == 0.0 and nclash[0] == 0 and not dcrd.any()


ANGLE_LENS, ANGLE_SEED = [24, 17, 12], 73


def test_gradient_down_to_the_angles_against_fp64_autograd():
    """angles -> NeRF forward -> clash -> NeRF adjoint -> angles adjoint on the device against fp64 autograd through the oracle's
    chain.  Two builds stand behind the comparison, fp32 and fp64, so the condition on the input is asked of BOTH: the margin on
    the coordinates the kernel is given (its own fp32 build, read back), and the same violating pairs in the two builds."""
    from oracle import batched, losses as olosses
    from protein_transformer_amd import synthetic
    from protein_transformer_amd.losses import angles_backward, angles_forward, batch_loss, clash_forward_backward
    from protein_transformer_amd.protein.Structure import nerf_backward, nerf_forward
    dev = torch.device("cuda:0")
    build = lambda ang, seq: batched.generate_coords_batched(ang, seq, torch.float64)      # noqa: E731
    batch = synthetic.make_batch(ANGLE_LENS, L_pad=26, seed=ANGLE_SEED, build_coords=build)
    seq, ang = batch["seq"], batch["start_ang_rad"]
    true = batch["true_crd"].float()
    sincos = (torch.stack([torch.cos(ang), torch.sin(ang)], -1).reshape(len(seq), -1, 24) * 0.9).float()
    sc, sq = sincos.to(dev), seq.to(dev)
    a32 = angles_forward(sc)
    crd32, _ = nerf_forward(a32, sq)
    stats, nclash, dcrd = clash_forward_backward(crd32, sq, need_grad=True)
    grad = angles_backward(sc, nerf_backward(a32, sq, crd32, dcrd)).cpu().numpy()
    sc64 = sincos.double().clone().requires_grad_()
    crd64 = batched.generate_coords_batched(olosses.inverse_trig_transform(sc64), seq, torch.float64)
    total = 0
    for b in range(len(seq)):
        on32 = R.clash_reference(crd32[b].cpu().numpy(), seq[b].numpy())           # asserts the margin of the kernel's input
        loss, n_hit, n, _, margin = R.clash_reference(crd64[b], seq[b].numpy())
        total = total + loss                                           # the back-propagated quantity is the SUM over proteins
        print(f"chain[{b}]: clash {float(stats[b, 0])} / {on32[0]} (fp64 chain {float(loss.detach())}), nclash {int(nclash[b])} / {on32[1]} "
              f"(fp64 chain {n_hit}), margins {on32[4]:.1e} {margin:.1e}")
        assert n_hit == on32[1], "pick another seed: a pair changes sides between the fp32 and the fp64 build"
        assert int(nclash[b]) == on32[1] and float(stats[b, 1]) == n and abs(float(stats[b, 0]) - on32[0]) <= 1e-5
    total.backward()
    want = sc64.grad.numpy()
    for b in range(len(seq)):
        print(f"chain[{b}]: angle gradient rel-L2 {R.rel_l2(grad[b], want[b]):.2e}")
        assert R.rel_l2(grad[b], want[b]) < 1e-3
    # batch_loss(clash=(W, tau)): the term joins the dRMSD gradient in front of the ONE adjoint, which is linear
    W = 0.5
    plain = batch_loss(sc, true.to(dev), sq, do_backward=True)
    out = batch_loss(sc, true.to(dev), sq, do_backward=True, clash=(W, R.TOLERANCE))
    unset = lambda r: {f for f, v in r._asdict().items() if v is None}                # noqa: E731
    assert unset(plain) == {"per_protein", "true_ang", "clash"} and unset(out) == {"per_protein", "true_ang"}
    assert int(out.status.item()) == 0
    assert torch.equal(out[0], plain[0])                               # the dRMSD statistics do not know about the term
    assert torch.equal(out.clash, stats[:, 0])                         # the unweighted per-protein values
    both = plain[1].cpu().numpy() + W * grad.reshape(plain[1].shape)
    print(f"batch_loss: rel-L2 of the joint gradient {R.rel_l2(out[1].cpu().numpy(), both):.2e}")
    assert R.rel_l2(out[1].cpu().numpy(), both) < 1e-3
    assert not torch.equal(out[1], plain[1])


# ----------------------------------------------------------------------------- 2. hand-built cases
def far_apart(seq):
    """Every slot on a 10 A grid (residue along x, slot along y), away from the origin: nothing is near anything."""
    L = len(seq)
    crd = np.zeros((L * SLOTS, 3), np.float32)
    crd[:, 0] = 10.0 * np.repeat(np.arange(L), SLOTS) + 5.0
    crd[:, 1] = 10.0 * np.tile(np.arange(SLOTS), L)
    return crd


def check_by_hand(crd, seq, pairs):
    """pairs: [(slot a, slot b, r_a + r_b)] of the only violating pairs, all along x with x_a < x_b."""
    seq = np.asarray(seq, np.int64)
    stats, nclash, dcrd = run(crd, seq)
    ref = R.clash_reference(crd, seq)
    n = len(R.atoms_of(seq)[0])
    want = sum(rr - 1.5 - float(crd[b, 0] - crd[a, 0]) for a, b, rr in pairs) / n
    assert stats[0, 1] == n == ref[2] and nclash[0] == len(pairs) == ref[1]
    assert abs(stats[0, 0] - want) <= 1e-6 and abs(ref[0] - want) <= 1e-6
    g = np.zeros((len(seq) * SLOTS, 3))
    for a, b, _ in pairs:
        g[a, 0] += 1.0 / n
        g[b, 0] -= 1.0 / n
    assert np.abs(dcrd[0] - g).max() <= 1e-5 / n and np.abs(ref[3] - g).max() < 1e-12
    return stats, nclash, dcrd


def test_peptide_bond_is_excluded_and_the_next_nitrogen_is_not():
    seq = [5, 5, 5, 5]                                                   # four GLY
    crd = far_apart(seq)
    crd[2], crd[SLOTS] = (0, 70, 3), (1.3, 70, 3)                        # C(0) - N(1) at 1.3 A: the bond, nothing
    check_by_hand(crd, seq, [])
    crd[SLOTS + 2], crd[3 * SLOTS] = (0, 80, 3), (1.3, 80, 3)            # C(1) - N(3) at 1.3 A: 1.7 + 1.55 - 1.5 - 1.3
    check_by_hand(crd, seq, [(SLOTS + 2, 3 * SLOTS, 3.25)])
    crd[SLOTS + 2], crd[3 * SLOTS] = (1.3, 80, 3), (0, 80, 3)            # the same two the other way round in space
    check_by_hand(crd, seq, [(3 * SLOTS, SLOTS + 2, 3.25)])
    crd = far_apart(seq)
    crd[SLOTS], crd[2 * SLOTS + 2] = (0, 90, 3), (1.3, 90, 3)            # N(1) - C(2): not a bond (the bond is C(i) - N(i+1))
    check_by_hand(crd, seq, [(SLOTS, 2 * SLOTS + 2, 3.25)])
    crd = far_apart(seq)
    crd[1], crd[SLOTS] = (0, 90, 3), (1.3, 90, 3)                        # CA(0) - N(1): not the bond either
    check_by_hand(crd, seq, [(1, SLOTS, 3.25)])


def test_disulfide_is_excluded_and_sulfur_to_carbon_is_not():
    seq = [R.CYS, 0, R.CYS, R.AA.index("M")]
    crd = far_apart(seq)
    crd[5], crd[2 * SLOTS + 5] = (0, 70, 3), (2.0, 70, 3)                # SG - SG at 2.0 A (threshold 2.1): nothing
    check_by_hand(crd, seq, [])
    crd[SLOTS + 4] = (-1.5, 70, 3)                                       # CB of ALA 1.5 A from the first SG: 1.7 + 1.8 - 1.5 - 1.5
    check_by_hand(crd, seq, [(SLOTS + 4, 5, 3.5)])
    crd = far_apart(seq)
    crd[5], crd[3 * SLOTS + 6] = (0, 70, 3), (2.0, 70, 3)                # SG - SD of MET: sulfur both, no disulfide
    check_by_hand(crd, seq, [(5, 3 * SLOTS + 6, 3.6)])
    crd = far_apart(seq)
    crd[5], crd[3 * SLOTS + 5] = (0, 70, 3), (1.0, 70, 3)                # SG - slot 5 of MET (CG): the exclusion asks for two CYS
    check_by_hand(crd, seq, [(5, 3 * SLOTS + 5, 3.5)])


def test_pairs_within_a_residue_do_not_count():
    seq = [R.AA.index("W"), 0]
    crd = far_apart(seq)
    crd[4:SLOTS] = crd[4] + np.float32([0.1, 0, 0]) * np.arange(10)[:, None]     # ten side-chain atoms 0.1 A apart
    check_by_hand(crd, seq, [])


def test_glycines_with_their_absent_slots_at_the_origin():
    """geometry.hip zero-fills the slots a residue does not have: ten per GLY, all at the origin.  None of them is an atom; a
    real atom AT the origin meets none of them."""
    seq = [5] * 6 + [PAD, 21]
    crd = far_apart(seq)
    absent = absent_slots(np.array(seq))
    assert len(absent) == 6 * 10 + 2 * SLOTS
    crd[absent] = 0.0
    stats, nclash, dcrd = check_by_hand(crd, seq, [])
    assert stats[0, 0] == 0.0 and stats[0, 1] == 24 and not dcrd.any()
    crd[1] = 0.0                                                         # CA of residue 0 at the origin
    check_by_hand(crd, seq, [])
    crd[SLOTS + 1] = (1.0, 0, 0)                                         # and a real neighbour: exactly this one pair
    check_by_hand(crd, seq, [(1, SLOTS + 1, 3.4)])


def test_coinciding_atoms_have_a_finite_zero_gradient():
    seq = [5, 5, 5]
    crd = far_apart(seq)
    crd[1] = crd[SLOTS + 1] = (3, 70, 3)                                 # in the row tile and the column tile of one sweep step
    crd[2 * SLOTS + 3] = (4, 70, 3)                                      # O of residue 2, 1 A from both: 1.7 + 1.52 - 1.5 - 1
    stats, nclash, dcrd = run(crd, seq)
    assert nclash[0] == 3 and abs(stats[0, 0] - (1.9 + 2 * 0.72) / 12) <= 1e-6
    want = np.zeros((3 * SLOTS, 3))
    want[1, 0] = want[SLOTS + 1, 0] = 1 / 12                             # (descent pushes the pair of them away from the O)
    want[2 * SLOTS + 3, 0] = -2 / 12
    assert np.isfinite(dcrd).all() and np.abs(dcrd[0] - want).max() <= 1e-5 / 12


# ----------------------------------------------------------------------------- 3. poison
def test_what_absent_and_pad_slots_hold_changes_no_bit():
    crd, seq = case("ragged")
    clean = run(crd, seq)
    rng = np.random.default_rng(5)
    for b in range(len(seq)):
        absent = absent_slots(seq[b])
        assert len(absent)
        dirty = crd.copy()
        dirty[b, absent] = rng.choice([np.nan, 1e30, -np.inf, 0.5], (len(absent), 3)).astype(np.float32)
        got = run(dirty, seq)
        for a, c in zip(got, clean):
            assert np.array_equal(a, c, equal_nan=True), b


@pytest.mark.parametrize("poison", [np.nan, np.inf, 2e18])
def test_an_unusable_atom_makes_its_protein_nan_and_no_other(poison):
    crd, seq = case("ragged")
    clean = run(crd, seq)
    atom = R.atoms_of(seq[1])[0][37]
    dirty = crd.copy()
    dirty[1, atom, 2] = poison
    stats, nclash, dcrd = run(dirty, seq)
    assert np.isnan(stats[1, 0]) and stats[1, 1] == clean[0][1, 1] and nclash[1] == 0 and not dcrd[1].any()
    for b in (0, 2):
        assert np.array_equal(stats[b], clean[0][b], equal_nan=True) and nclash[b] == clean[1][b]
        assert np.array_equal(dcrd[b], clean[2][b])
    # accumulating: the unusable protein's rows stay what they were
    base = np.random.default_rng(6).normal(0, 1, crd.shape).astype(np.float32)
    acc = run(dirty, seq, weight=2.0, accumulate_into=base)[2]
    assert np.array_equal(acc[1], base[1]) and np.array_equal(acc[2], base[2]) and not np.array_equal(acc[0], base[0])
    # a finite coordinate below the bound is used as it is: far from everything, no clash with it
    dirty[1, atom] = (9e17, 0, 0)
    stats, nclash, _ = run(dirty, seq)
    assert np.isfinite(stats[1, 0]) and nclash[1] <= clean[1][1]


# ----------------------------------------------------------------------------- 4. accumulate, bits, refusals
@pytest.mark.parametrize("weight", [0.37, -3.0])
def test_accumulate_with_a_weight(weight):
    crd, seq = case("ragged")
    g = run(crd, seq)[2]
    scaled = run(crd, seq, weight=weight)[2]
    base = np.random.default_rng(11).normal(0, 0.05, crd.shape).astype(np.float32)
    acc = run(crd, seq, weight=weight, accumulate_into=base)[2]
    w = float(np.float32(weight))                                        # the weight the kernel gets
    want = base.astype(np.float64) + w * g.astype(np.float64)
    # base + weight * g within 2 fp32 ulps of the sum (the kernel rounds g as the unweighted call does, then one multiply-add)
    worst = np.abs(acc - want) / np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    print(f"weight {weight}: accumulate within {worst.max():.2f} ulps")
    assert worst.max() <= 2
    assert (np.abs(scaled - w * g.astype(np.float64)) <= 2 * np.spacing(np.abs(scaled))).all()
    for b in range(len(seq)):
        absent = absent_slots(seq[b])
        assert np.array_equal(acc[b, absent], base[b, absent]) and not scaled[b, absent].any()     # untouched / exactly zero
    assert np.array_equal(run(crd, seq, weight=0.0)[2], np.zeros_like(g))


def test_two_runs_give_the_same_bits():
    for name in ("long", "ragged"):
        crd, seq = case(name)
        a, b = run(crd, seq), run(crd, seq)
        for x, y in zip(a, b):
            assert np.array_equal(x, y, equal_nan=True), name


def test_a_protein_alone_and_inside_a_wider_longer_batch():
    crd, seq = case("ragged")
    L, wide = seq.shape[1], 71
    lc, ls = case("long")
    big_crd = np.zeros((4, wide * SLOTS, 3), np.float32)
    big_seq = np.full((4, wide), PAD, np.int64)
    big_crd[0, :lc.shape[1]], big_seq[0, :ls.shape[1]] = lc[0], ls[0]
    for b in (0, 1, 2):
        big_crd[b + 1, :L * SLOTS], big_seq[b + 1, :L] = crd[b], seq[b]
    big_crd[:, L * SLOTS:][1:] = np.float32(1e30)                      # the longer padding holds anything
    inside = run(big_crd, big_seq)
    for b in (0, 1, 2):
        n_res = int((seq[b] != PAD).sum())
        alone = run(crd[b, :max(n_res, 1) * SLOTS], seq[b, :max(n_res, 1)])     # trimmed to its own length
        assert np.array_equal(alone[0][0], inside[0][b + 1], equal_nan=True) and alone[1][0] == inside[1][b + 1]
        assert np.array_equal(alone[2][0], inside[2][b + 1, :alone[2].shape[1]]) and not inside[2][b + 1, alone[2].shape[1]:].any()


def test_eval_metric_is_the_forward_pass():
    from protein_transformer_amd.eval_metrics import clash_batch
    crd, seq = case("ragged")
    dev = torch.device("cuda:0")
    loss, nclash, n = clash_batch(torch.from_numpy(crd).to(dev), torch.from_numpy(seq).to(dev), R.TOLERANCE)
    stats, hits, _ = run(crd, seq)
    assert np.array_equal(loss.cpu().numpy(), stats[:, 0], equal_nan=True) and np.array_equal(n.cpu().numpy(), stats[:, 1])
    assert np.array_equal(nclash.cpu().numpy(), hits) and nclash.dtype == torch.int64


def test_refusals_leave_the_outputs_untouched():
    from protein_transformer_amd import _lib
    lib = _lib.lib()
    dev = torch.device("cuda:0")
    crd, seq = case("ragged")
    B, L = seq.shape
    c, s = torch.from_numpy(crd).to(dev), torch.from_numpy(seq).to(dev)
    stats = torch.full((B, 2), 77.0, device=dev)
    nclash = torch.full((B,), 77, dtype=torch.int64, device=dev)
    dcrd = torch.full((B, L * SLOTS, 3), 77.0, device=dev)
    need = lib.ptamd_clash_workspace_bytes(B, L)
    ws = torch.full((need + 256,), 77, dtype=torch.uint8, device=dev)
    p = _lib.ptr
    ok = dict(pred=p(c), seq=p(s), B=B, L=L, tol=1.5, w=1.0, acc=0, stats=p(stats), nclash=p(nclash), dcrd=p(dcrd), ws=p(ws), wb=need)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.ptamd_clash_fwd_bwd(a["pred"], a["seq"], a["B"], a["L"], a["tol"], a["w"], a["acc"], a["stats"], a["nclash"],
                                       a["dcrd"], a["ws"], a["wb"], _lib.stream())

    bad_shape = [dict(B=0), dict(L=0), dict(B=-2), dict(L=(2 ** 31 - 1) // 28 + 1), dict(tol=-1.0), dict(tol=float("nan")),
                 dict(tol=float("inf")), dict(w=float("nan")), dict(w=float("inf")), dict(pred=None), dict(seq=None),
                 dict(stats=None), dict(nclash=None)]
    for acc in (0, 1):
        for kw in bad_shape:
            assert call(acc=acc, **kw) == -1, kw
        for kw in (dict(ws=None), dict(wb=need - 1), dict(wb=0)):
            assert call(acc=acc, **kw) == -3, kw
    torch.cuda.synchronize()
    assert (stats == 77).all() and (nclash == 77).all() and (dcrd == 77).all() and (ws == 77).all()
    assert call() == 0                                                   # and the same arguments, valid, do run
    torch.cuda.synchronize()
    assert (ws[need:] == 77).all() and not (dcrd == 77).any() and not (stats == 77).any()
