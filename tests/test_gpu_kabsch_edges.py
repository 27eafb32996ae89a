"""MI355X tests of csrc/kabsch.hip alone (`rmsd-full`, the headline evaluation metric) against the explicit fp64 superposition
of tests/metric_ref.py, at the edges of its slot loop, of its presence tests, of the atom count and of the geometry.  Only
`kabsch_rmsd_batch` is called, plus `rmsd` once, `batch_rmsd` once and the C entry point for its refusals.

Slots: L in {1, 18, 19, 37, 74}, 14 L = 14, 252, 266, 518, 1036 slots on 256 threads (one, two, four-plus trips; four wavefronts);
per L sparse proteins of 4 - 6 present slots out of {0, 63, 64, 255, 256, 511, 512, 14 L - 1} with prediction and truth
independent N(0, 8 A) - the reference itself shows that losing any ONE of the slots moves rmsd^2 by more than 100 bars
(asserted) - and one dense protein.  Presence: NaN in x, y or z alone, a padded residue mid-sequence (zero truth; large finite
garbage), NaN / inf / garbage predictions at absent slots.  n = 0 (NaN), 1 (exactly 0), 2, 3.  Geometry
(metric_ref.geometry_cases, each as an exact rigid motion and with 0.5 A of noise): general position; planar, axis-aligned and
rotated; planar truth against a 3-D prediction; collinear; every predicted atom on one point; a mirror image, plain and
rotated; a mirrored cube (three equal singular values, det < 0); a common offset of 1e3 and opposite offsets of +-1e4.

Bar, on rmsd^2 against `superposed_rmsd_ref` of the same fp32 inputs, eps = 2^-52 (metric_ref.kabsch_bar):
    |got^2 - want^2| <= 2^-22 want^2 + 64 eps M / n + 6 min(sqrt(16 eps) s1, 16 eps s1^2 / s3) / n
  - the fp32 rounding of the result, doubled by squaring, with a margin of 2;
  - the cancellation of the UNCENTRED fp64 moments, M = sum |a|^2 + sum |b|^2;
  - the loss in s3 from forming H^T H: an eigenvalue error of order eps s1^2 is eps s1^2 / s3 in s3, and sqrt(eps) s1 when H is
    rank-deficient (s2 in place of s3 for a rank-1 H; sqrt(16 eps) s1 when the denominator is 0).
Every constant is from this model and the reference's own s1 >= s2 >= s3, n, M; none is from the kernel's output.  The numpy
transcription of the kernel's arithmetic in tests/test_metric_ref.py meets the bar on every geometry (worst ratio 0.34).

Non-finite input (include/ptamd.h): a NaN or infinite predicted coordinate on a PRESENT atom gives that protein NaN - before
this suite the kernel's fmax(NaN, 0) reported RMSD 0.0, a perfect score, which `rmsd-full` then averaged in; a finite 1e30 is
used as it is (finite, huge, inside the bar); the same values on an absent slot change no bit; `batch_rmsd` of a batch with
such a protein is NaN.

MEASURED on the MI355X (the tests print every case; error / bar of rmsd^2, all <= 1):
  slots      L 1: sparse 0.220, dense 0.144      L 18: 0.276, 0.295      L 19: 0.018, 0.073
             L 37: sparse 0.254 / 0.123, dense 0.131                     L 74: sparse 0.277 / 0.157, dense 0.074
  presence   0.292 (n = 52)
  counts     n = 2: 0.107, two-point stretch 0.000 (got 1 exactly);  n = 3: 0.095, near 0.024
  geometry                 exact      + 0.5 A noise                            exact      + noise
    general                0.007      0.212          mirror                    0.079      0.157
    planar-axis            0.000      0.001          mirror-rotated            0.005      0.048
    planar-rotated         0.000      0.000          mirror-cube               0.000      0.275
    planar-vs-3d           0.001      0.007          mirror-cube-rotated       0.096      0.341   <- the worst
    collinear              0.000      0.018          offset-1e3                0.009      0.132
    one-point              0.201      0.201          offset-1e4-opposite       0.013      0.003
  1e30 in a present predicted coordinate: got 1.561249e+29, want 1.56125e+29, 0.158
  (0.2 - 0.34 is the fp32 rounding of the result against the first term; the rank-deficient and far-offset cases stay two
  orders of magnitude inside the second and third term.  An exact motion of a collinear set reads 0 where the reference
  reads 2.1e-6, the fp32 rounding of the inputs: e0 - 2 trace came out negative and was clamped.)
"""
import numpy as np
import pytest
import torch

import metric_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


def run(dev, proteins):
    """[(pred [L*14, 3], true, seq [L]), ...] of one L -> rmsd [B] (numpy fp32)"""
    from protein_transformer_amd.eval_metrics import kabsch_rmsd_batch
    pred, true, seq = (torch.from_numpy(np.stack([p[k] for p in proteins])).to(dev) for k in range(3))
    return kabsch_rmsd_batch(pred, true, seq).cpu().numpy()


def pad_to(protein, L, rng, truth="zeros"):
    """the protein with padded residues behind it up to L: PAD_ID, zero truth (what collate writes) or large finite garbage, and
    garbage in the prediction"""
    pred, true, seq = protein
    k = L - len(seq)
    assert k >= 0
    tail_p = rng.normal(0, 1e3, (k * 14, 3)).astype(np.float32)
    tail_t = np.zeros((k * 14, 3), np.float32) if truth == "zeros" else rng.normal(0, 1e6, (k * 14, 3)).astype(np.float32)
    return np.concatenate([pred, tail_p]), np.concatenate([true, tail_t]), np.concatenate([seq, np.full(k, R.PAD_ID)])


def ratio(got, protein):
    """|got^2 - want^2| / bar for one protein, from the reference over its present atoms -> (ratio, want, n)"""
    want, sig, n, M = R.protein_ref(*protein)
    assert n > 0 and np.isfinite(got), (got, n)
    g = float(got)
    return abs(g * g - want * want) / R.kabsch_bar(want, sig, n, M), want, n


def show(case, r, got, want, n):
    print(f"MEASURED {case:<34} n {n:5d}  got {got:.7g}  want {want:.7g}  error / bar {r:.3f}")


# --------------------------------------------------------------------------- slots
def far_atoms(n, rng):
    return rng.normal(0, 8, (n, 3)).astype(np.float32), rng.normal(0, 8, (n, 3)).astype(np.float32)


@pytest.mark.parametrize("L", R.SLOT_LS)
def test_slot_loop_sparse_and_dense(dev, L):
    rng = np.random.default_rng(100 + L)
    proteins, names, counts = [], [], []
    for slots in R.sparse_slot_sets(L):
        a, b = far_atoms(len(slots), rng)
        proteins.append(R.embed(a, b, L=L, slots=slots, rng=rng))
        names.append(f"L {L} sparse {slots}")
        counts.append(len(slots))
        want, sig, n, M = R.superposed_rmsd_ref(a, b)             # from the reference alone: every single slot matters
        bar = R.kabsch_bar(want, sig, n, M)
        for k in range(n):
            less = R.superposed_rmsd_ref(np.delete(a, k, 0), np.delete(b, k, 0))[0]
            twice = R.superposed_rmsd_ref(np.concatenate([a, a[k:k + 1]]), np.concatenate([b, b[k:k + 1]]))[0]
            assert abs(less ** 2 - want ** 2) > 100 * bar and abs(twice ** 2 - want ** 2) > 100 * bar, (L, slots, k)
    n_all = L * 14
    b = rng.normal(0, 8, (n_all, 3))
    a = b @ R.rotation(rng).T + [5.0, -60.0, 20.0] + rng.normal(0, R.NOISE, (n_all, 3))
    dense = R.embed(a.astype(np.float32), b.astype(np.float32), L=L, rng=rng)
    if L > 1:
        dense[1][[1, n_all - 2], :] = np.nan                      # two atoms absent, so that the dense count is not L * 14 either
    proteins.append(dense)
    names.append(f"L {L} dense")
    counts.append(n_all - 2 * (L > 1))
    got = run(dev, proteins)
    assert np.array_equal(got, run(dev, proteins))
    for k, (name, p) in enumerate(zip(names, proteins)):
        r, want, n = ratio(got[k], p)
        show(name, r, got[k], want, n)
        assert n == counts[k], name
        assert r <= 1.0, (name, got[k], want, r)


# --------------------------------------------------------------------------- presence
def test_presence_per_coordinate_padding_and_garbage(dev):
    rng = np.random.default_rng(7)
    L = 6
    b = rng.normal(0, 8, (L * 14, 3))
    a = b @ R.rotation(rng).T + [1.0, 2.0, 3.0] + rng.normal(0, R.NOISE, b.shape)
    pred, true, seq = a.astype(np.float32), b.astype(np.float32), rng.integers(0, 20, L)
    true[3, 0] = np.nan                                           # x only
    true[17, 1] = np.nan                                          # y only
    true[50, 2] = np.nan                                          # z only
    true[70] = np.nan
    pred[3], pred[17], pred[50], pred[70] = np.nan, np.inf, [1e30, -np.inf, 0.0], 1e6     # garbage at absent slots
    seq[2], seq[4] = R.PAD_ID, R.PAD_ID                           # padded residues in the MIDDLE of the sequence
    true[2 * 14:3 * 14] = 0.0                                     # one as collate leaves it ...
    true[4 * 14:5 * 14] = rng.normal(0, 1e6, (14, 3))             # ... one with large finite garbage in both structures
    pred[4 * 14:5 * 14] = rng.normal(0, 1e6, (14, 3))
    pred[4 * 14 + 1] = np.nan
    protein = (pred, true, seq)
    assert int(R.present_atoms(*protein).sum()) == 4 * 14 - 4     # residues 0, 1, 3, 5 less slots 3, 17, 50, 70
    got = run(dev, [protein])
    r, want, n = ratio(got[0], protein)
    show("presence", r, got[0], want, n)
    assert n == 52 and r <= 1.0 and 0.5 < want < 1.0, (got, want, r)


# --------------------------------------------------------------------------- counts
def test_atom_counts_0_1_2_3(dev):
    rng = np.random.default_rng(8)
    L = 3
    none = R.embed(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), L=L, rng=rng)
    padded = R.embed(*far_atoms(5, rng), L=L, rng=rng)
    padded = (padded[0], np.nan_to_num(padded[1], nan=0.0), np.full(L, R.PAD_ID))        # every residue padded
    one = R.embed(*far_atoms(1, rng), L=L, slots=[41], rng=rng)
    a1, b1 = far_atoms(1, rng)
    one_far = R.embed(a1 + np.float32(1e4), b1 - np.float32(1e4), L=L, slots=[0], rng=rng)
    two = R.embed(*far_atoms(2, rng), L=L, slots=[13, 14], rng=rng)
    stretch = R.embed(np.array([[0, 0, 0], [2, 0, 0]], np.float32), np.array([[5, 5, 5], [5, 9, 5]], np.float32), L=L, slots=[0, 41],
                      rng=rng)
    three = R.embed(*far_atoms(3, rng), L=L, slots=[0, 20, 41], rng=rng)
    b3 = rng.normal(0, 8, (3, 3))
    three_near = R.embed((b3 @ R.rotation(rng).T + rng.normal(0, R.NOISE, (3, 3))).astype(np.float32), b3.astype(np.float32), L=L,
                         slots=[5, 6, 7], rng=rng)
    got = run(dev, [none, padded, one, one_far, two, stretch, three, three_near])
    assert np.isnan(got[0]) and np.isnan(got[1])
    assert got[2] == 0.0 and got[3] == 0.0                        # one atom: exactly 0, wherever it is
    assert got[5] == pytest.approx(1.0, rel=1e-6)                 # centred +-1 against +-2: residual 1 per atom
    for k, name in ((4, "n = 2"), (5, "n = 2 stretch"), (6, "n = 3"), (7, "n = 3 near")):
        p = (none, padded, one, one_far, two, stretch, three, three_near)[k]
        r, want, n = ratio(got[k], p)
        show(name, r, got[k], want, n)
        assert n == int(name[4]) and r <= 1.0, (name, got[k], want, r)


# --------------------------------------------------------------------------- geometry
def test_geometry_against_the_explicit_superposition(dev):
    from protein_transformer_amd.eval_metrics import rmsd
    cases = R.geometry_cases()
    rng = np.random.default_rng(9)
    proteins = {name: pad_to(R.embed(a, b, rng=rng), 3, rng) for name, (a, b, _) in cases.items()}
    got = dict(zip(proteins, run(dev, list(proteins.values()))))
    for name, p in proteins.items():
        r, want, n = ratio(got[name], p)
        show(name, r, got[name], want, n)
        assert n == len(cases[name][0]) and r <= 1.0, (name, got[name], want, r)
        if name.startswith("mirror"):
            assert got[name] > 1.0, (name, got[name])
    assert got["mirror-rotated"] == pytest.approx(got["mirror"], rel=1e-5)
    a, b, _ = cases["general+noise"]
    assert np.float32(rmsd(a, b)) == got["general+noise"]         # the host-float convenience call: the same kernel, the same bits


# --------------------------------------------------------------------------- batch
def test_ragged_batch_equals_each_protein_alone_bit_for_bit(dev):
    rng = np.random.default_rng(10)
    cases = R.geometry_cases()
    pool = [R.embed(a, b, rng=rng) for name, (a, b, _) in cases.items()
            if name in ("general+noise", "collinear", "mirror-cube", "one-point", "offset-1e4-opposite+noise", "planar-rotated+noise")]
    pool.append(R.embed(*far_atoms(5, rng), L=37, slots=R.sparse_slot_sets(37)[1], rng=rng))
    pool.append(R.embed(*far_atoms(19 * 14, rng), L=19, rng=rng))
    pool.append(R.embed(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), L=2, rng=rng))
    alone = np.array([run(dev, [p])[0] for p in pool])
    assert np.isnan(alone[-1]) and np.isfinite(alone[:-1]).all() and len(set(alone[:-1].tolist())) == len(pool) - 1
    for L, truth in ((37, "zeros"), (74, "garbage")):
        order = rng.permutation(len(pool))
        batch = [pad_to(pool[k], L, rng, truth) for k in order]
        got = run(dev, batch)
        assert np.array_equal(got, alone[order], equal_nan=True), (L, got, alone[order])
        assert np.array_equal(got, run(dev, batch), equal_nan=True)


# --------------------------------------------------------------------------- non-finite prediction
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf"), 1e30], ids=["nan", "inf", "-inf", "1e30"])
def test_non_finite_prediction_is_no_perfect_score(dev, value):
    rng = np.random.default_rng(12)
    cases = R.geometry_cases()
    base = [pad_to(R.embed(*cases[name][:2], rng=rng), 4, rng) for name in ("general+noise", "planar-axis+noise", "mirror")]
    clean = run(dev, base)
    assert np.isfinite(clean).all()
    present = np.nonzero(R.present_atoms(*base[1]))[0]
    absent = np.nonzero(~R.present_atoms(*base[1]))[0]
    assert len(present) == R.N_GEO and len(absent) == 16
    for coord in range(3):
        hit = [tuple(x.copy() for x in p) for p in base]
        hit[1][0][present[5 + coord], coord] = value              # one coordinate of one PRESENT atom of the middle protein
        got = run(dev, hit)
        assert got[0] == clean[0] and got[2] == clean[2], (value, got, clean)        # the other two keep their bits
        if np.isfinite(value):                                    # finite, huge, and the reference's value (include/ptamd.h)
            r, want, n = ratio(got[1], hit[1])
            show(f"prediction {value:g} in coordinate {coord}", r, got[1], want, n)
            assert np.isfinite(got[1]) and got[1] > 1e28 and r <= 1.0, (value, got[1], want, r)
        else:
            assert np.isnan(got[1]), f"prediction {value} in coordinate {coord} of a present atom: got {got[1]}, want NaN"
            assert np.isnan(R.protein_ref(*hit[1])[0])
        miss = [tuple(x.copy() for x in p) for p in base]
        miss[1][0][absent[[0, 3, 15]], coord] = value             # an absent slot (NaN truth; a padded residue): nothing changes
        assert np.array_equal(run(dev, miss), clean), (value, coord)


def test_batch_rmsd_of_a_diverged_protein_is_nan(dev):
    from protein_transformer_amd import synthetic
    from protein_transformer_amd.eval_metrics import batch_rmsd, kabsch_rmsd_batch
    from protein_transformer_amd.losses import angles_forward
    from protein_transformer_amd.protein.Structure import nerf_forward
    lens, L = [12, 9, 12], 12
    batch = synthetic.make_batch(lens, L_pad=L, seed=4)
    seq = batch["seq"].to(dev)
    truth, status = nerf_forward(batch["true_ang_rad"].to(dev), seq)
    assert int(status.item()) == 0
    own = synthetic.slot_mask(batch["seq"]).to(dev)
    pad = (seq == 20).repeat_interleave(14, dim=1)
    truth = torch.where(own[:, :, None] | pad[:, :, None], truth, torch.full_like(truth, float("nan")))
    start = batch["start_ang_rad"]
    sincos = torch.stack([torch.cos(start), torch.sin(start)], -1).reshape(3, L, 24).to(dev)
    crd, _ = nerf_forward(angles_forward(sincos), seq)
    each = kabsch_rmsd_batch(crd, truth, seq).double().cpu().numpy()
    assert np.isfinite(each).all() and (each > 0.05).all()
    assert batch_rmsd(sincos, truth, seq) == pytest.approx(each.mean(), rel=1e-12)
    bad = sincos.clone()
    bad[1, 2, 0] = float("nan")                                   # one angle of one protein diverged
    got = batch_rmsd(bad, truth, seq)
    assert np.isnan(got), f"batch_rmsd with a NaN angle in one protein: got {got} (clean mean {each.mean()}), want NaN"


# --------------------------------------------------------------------------- refusals
def test_entry_point_refusals_leave_the_output_alone(dev):
    from protein_transformer_amd import _lib
    lib = _lib.lib()
    B, L = 2, 3
    pred = torch.zeros(B, L * 14, 3, device=dev)
    true = torch.zeros(B, L * 14, 3, device=dev)
    seq = torch.zeros(B, L, dtype=torch.int64, device=dev)
    out = torch.full((B,), 7.0, device=dev)
    call = lambda p, t, s, b, l, o: lib.ptamd_kabsch_rmsd(_lib.ptr(p), _lib.ptr(t), _lib.ptr(s), b, l, _lib.ptr(o), _lib.stream())  # noqa: E731
    for args in ((pred, true, seq, 0, L, out), (pred, true, seq, -1, L, out), (pred, true, seq, B, 0, out),
                 (pred, true, seq, B, -7, out), (None, true, seq, B, L, out), (pred, None, seq, B, L, out),
                 (pred, true, None, B, L, out), (pred, true, seq, B, L, None)):
        assert call(*args) == -1                                  # PTAMD_ERR_BAD_SHAPE
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(pred, true, seq, B, L, out) == 0
    assert np.array_equal(out.cpu().numpy(), np.zeros(B, np.float32))              # identical structures
