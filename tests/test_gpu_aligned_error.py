"""MI355X tests of the frame-aligned error matrix (csrc/aligned_error.hip, `ptamd_aligned_error`) against its fp64 restatement
tests/aligned_error_ref.py, through the C ABI on buffers this file owns.

Cases (built on the host by `aligned_error_ref.make_case`): L in {1, 3, 63, 64, 65, 129} x K in {1, 3}, three proteins per batch -
a full row, one padded by a residue, one of at most five residues, so a tile edge, a one-entry last tile and tiles holding only
padding are in play - with samples that are noisy moved copies, bit copies, rigidly moved copies, hinged copies and mirror images
of the reference; then one thing wrong at a time in the reference or in a sample (`aligned_error_ref.spoiled`).  Slots a residue
type does not have and padded residues hold NaN in both structures.

Outputs are pre-filled with poison inside guard bands of 64 elements; the workspace sits at offset 256 of a poisoned buffer 512
bytes longer.  In every comparison NO entry is left out: the NaN pattern and `usable` equal the reference's exactly, finite entries
and the mean lie within `tol(extent)`, the TM stat within `tol_tm` - the bounds aligned_error_ref derives from the arithmetic."""
import numpy as np
import pytest
import torch

import aligned_error_ref as ar

pytestmark = pytest.mark.gpu

GUARD = 64


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Guarded:
    """A device tensor of `shape` inside a poisoned buffer, GUARD elements of guard band on either side."""

    def __init__(self, shape, dtype, dev, poison):
        self.isz, self.poison = torch.empty(0, dtype=dtype).element_size(), poison
        n = int(np.prod(shape))
        self.raw = torch.full(((n + 2 * GUARD) * self.isz,), poison, dtype=torch.uint8, device=dev)
        self.inner = self.raw[GUARD * self.isz:(GUARD + n) * self.isz]
        self.t = self.inner.view(dtype).view(*shape)

    def guards_intact(self):
        g = GUARD * self.isz
        return bool((self.raw[:g] == self.poison).all()) and bool((self.raw[-g:] == self.poison).all())


def outputs(B, L, dev, poison):
    return dict(ae=Guarded((B, L, L), torch.float32, dev, poison), stats=Guarded((B, 2), torch.float32, dev, poison),
                usable=Guarded((B,), torch.int32, dev, poison))


def call_abi(ref, samples, seq, dev, poison=0xFF):
    """One call on poisoned buffers -> {name: host array}.  `poison`: the byte every output and the workspace hold on arrival
    (0xFF: a NaN no kernel writes; 0x7F: large finite garbage)."""
    from protein_transformer_amd import _lib
    lib, P = _lib.lib(), _lib.ptr
    ref, samples, seq = (torch.as_tensor(a).to(dev).contiguous() for a in (ref, samples, seq))
    B, K, L = samples.shape[0], samples.shape[1], seq.shape[1]
    nbytes = lib.ptamd_aligned_error_workspace_bytes(B, K, L)
    assert nbytes > 0
    whole = torch.full((nbytes + 512,), 0xCD, dtype=torch.uint8, device=dev)
    ws = whole[256:256 + nbytes]
    assert ws.data_ptr() % 16 == 0
    ws.fill_(poison)
    outs = outputs(B, L, dev, poison)
    rc = lib.ptamd_aligned_error(P(ref), P(samples), P(seq), B, K, L, P(outs["ae"].t), P(outs["stats"].t), P(outs["usable"].t),
                                 P(ws), nbytes, _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    for name, g in outs.items():
        assert g.guards_intact(), name
    assert bool((whole[:256] == 0xCD).all()) and bool((whole[256 + nbytes:] == 0xCD).all())
    return {k: g.t.cpu().numpy().copy() for k, g in outs.items()}


def check(got, want, extent, lens, K):
    """Every entry of every output against the fp64 reference; -> the worst error as a fraction of its bound."""
    ae, stats, usable = want
    assert (got["usable"] == usable).all(), (got["usable"], usable)
    g = got["ae"].astype(np.float64)
    assert (np.isnan(g) == np.isnan(ae)).all()
    assert np.isfinite(g[~np.isnan(ae)]).all()
    ok = ~np.isnan(ae)
    err = np.abs(g[ok] - ae[ok])
    bound = ar.tol(extent, K)
    worst = float(err.max(initial=0.0)) / bound
    assert (err <= bound).all(), (float(err.max()), bound)
    s = got["stats"].astype(np.float64)
    assert (np.isnan(s) == np.isnan(stats)).all()
    for b in range(len(lens)):
        if np.isnan(stats[b, 0]):
            continue
        n = int(np.isfinite(ae[b]).any(0).sum())                             # the points
        e_mean, e_tm = abs(s[b, 0] - stats[b, 0]), abs(s[b, 1] - stats[b, 1])
        worst = max(worst, e_mean / bound, e_tm / ar.tol_tm(extent, n, K))
        assert e_mean <= bound and e_tm <= ar.tol_tm(extent, n, K), (b, e_mean, e_tm)
    return worst


@pytest.mark.parametrize("K", ar.KS)
@pytest.mark.parametrize("L", ar.LENGTHS)
def test_noisy_samples_against_fp64_poison_and_repeat(L, K, dev):
    """Cases 1, 6 and 7: values, the two poisons, guard bands, the same call twice."""
    c = ar.make_case(L, K, "noise")
    a = call_abi(c["ref"], c["samples"], c["seq"], dev, 0xFF)
    b = call_abi(c["ref"], c["samples"], c["seq"], dev, 0x7F)
    again = call_abi(c["ref"], c["samples"], c["seq"], dev, 0xFF)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k                   # whatever the outputs and the workspace held
        assert a[k].tobytes() == again[k].tobytes(), k               # the same call twice
    worst = check(a, c["want"], c["extent"], c["lens"], K)
    print(f"L {L} K {K}: extent {c['extent']:.1f} A, worst error / bound {worst:.4f}, usable {list(a['usable'])}")
    assert list(a["usable"]) == [K, K, K]
    for p, n in enumerate(c["lens"]):
        assert np.isfinite(a["ae"][p, :n, :n]).all()
        assert np.isnan(a["ae"][p, n:]).all() and np.isnan(a["ae"][p, :, n:]).all()      # padded rows and columns
        assert (np.diagonal(a["ae"][p])[:n] == 0.0).all()                                # i = j: exactly 0
        if n >= 3:
            assert np.abs(a["ae"][p, :n, :n] - a["ae"][p, :n, :n].T).max() > 0.01        # not symmetric


@pytest.mark.parametrize("K", ar.KS)
@pytest.mark.parametrize("L", ar.LENGTHS)
def test_identical_sample_is_exactly_zero(L, K, dev):
    c = ar.make_case(L, K, "identical")
    a = call_abi(c["ref"], c["samples"], c["seq"], dev)
    check(a, c["want"], c["extent"], c["lens"], K)
    defined = ~np.isnan(c["want"][0])
    assert (a["ae"][defined] == 0.0).all()
    assert (a["stats"][:, 0] == 0.0).all() and (a["stats"][:, 1] == 1.0).all()


@pytest.mark.parametrize("kind", ("rigid", "hinge", "mirror"))
@pytest.mark.parametrize("L", ar.LENGTHS)
def test_rigid_hinge_and_mirror(L, kind, dev):
    K = 3
    c = ar.make_case(L, K, kind)
    a = call_abi(c["ref"], c["samples"], c["seq"], dev)
    check(a, c["want"], c["extent"], c["lens"], K)
    bound = ar.tol(c["extent"], K)
    for p, n in enumerate(c["lens"]):
        m = a["ae"][p, :n, :n].astype(np.float64)
        # a moved copy ROUNDED TO FP32 is no rigid image: `moved_copy_slack` bounds what fp64 itself gives for it, `tol` the
        # kernel's distance from fp64 (asserted entry by entry in `check` above)
        slack = bound + ar.moved_copy_slack(c["ref"][p], n, c["extent"])
        if kind == "rigid":
            assert m.max() <= slack
        elif kind == "hinge":
            h, dist = c["hinge"][p]
            lo, hi = np.arange(n) < h, np.arange(n) >= h
            assert (m[np.ix_(lo, lo)] == 0.0).all() and m[np.ix_(hi, hi)].max(initial=0.0) <= slack
            assert np.abs(m[np.ix_(lo, hi)] - dist[None, :n][:, hi]).max(initial=0.0) <= slack
            assert np.abs(m[np.ix_(hi, lo)] - dist[None, :n][:, lo]).max(initial=0.0) <= slack
        elif n >= 8:
            assert a["stats"][p, 0] > 1000 * bound                   # a mirror image keeps every distance and is far


@pytest.mark.parametrize("what", ar.SPOILS)
@pytest.mark.parametrize("L", (3, 65))
def test_validity_of_the_reference_and_of_a_sample(L, what, dev):
    """Cases 4 and 5, residue 1 of protein 0."""
    K = 3
    c = ar.make_case(L, K, "noise")
    ref, samples, seq = ar.spoiled(c, what)
    want = ar.reference(ref, samples, seq)
    a = call_abi(ref, samples, seq, dev)
    check(a, want, c["extent"], c["lens"], K)
    base = call_abi(c["ref"], c["samples"], c["seq"], dev)
    n = c["lens"][0]
    ae = a["ae"][0]
    if what in ("ref_n_nan", "ref_degenerate"):
        assert np.isnan(ae[1]).all() and np.isfinite(np.delete(ae[:n, 1], 1)).all()      # the row, not the column
        assert list(a["usable"]) == [K, K, K]
    elif what == "ref_ca_nan":
        assert np.isnan(ae[1]).all() and np.isnan(ae[:, 1]).all() and np.isfinite(ae[0, 0])
        assert list(a["usable"]) == [K, K, K]
    elif what == "smp_side_chain":
        for k in a:
            assert a[k].tobytes() == base[k].tobytes(), k            # not one bit
    elif what == "all_samples":
        assert list(a["usable"]) == [0, 0, 0] and np.isnan(a["ae"]).all() and np.isnan(a["stats"]).all()
    else:
        assert list(a["usable"]) == [K - 1, K, K]
        rest = call_abi(c["ref"], c["samples"][:, 1:], c["seq"], dev)     # the remaining samples, alone
        assert a["ae"][0].tobytes() == rest["ae"][0].tobytes() and a["stats"][0].tobytes() == rest["stats"][0].tobytes()
        assert a["ae"][1:].tobytes() == base["ae"][1:].tobytes()


def test_single_spoiled_sample_leaves_nothing(dev):
    c = ar.make_case(65, 1, "noise")
    ref, samples, seq = ar.spoiled(c, "smp_ca_huge")
    a = call_abi(ref, samples, seq, dev)
    check(a, ar.reference(ref, samples, seq), c["extent"], c["lens"], 1)
    assert list(a["usable"]) == [0, 1, 1] and np.isnan(a["ae"][0]).all() and np.isnan(a["stats"][0]).all()
    assert np.isfinite(a["stats"][1:]).all()


def test_a_protein_does_not_depend_on_its_batch_or_its_padding(dev):
    c = ar.make_case(129, 3, "noise")
    full = call_abi(c["ref"], c["samples"], c["seq"], dev)
    n = c["lens"][1]                                                 # protein 1 alone, in a row of its own length
    alone = call_abi(c["ref"][1:2, :n * 14].copy(), c["samples"][1:2, :, :n * 14].copy(), c["seq"][1:2, :n].copy(), dev)
    assert alone["ae"][0].tobytes() == np.ascontiguousarray(full["ae"][1, :n, :n]).tobytes()
    assert alone["stats"].tobytes() == full["stats"][1:2].tobytes() and alone["usable"][0] == full["usable"][1]


def test_error_codes_launch_nothing(dev):
    from protein_transformer_amd import _lib
    lib, P = _lib.lib(), _lib.ptr
    c = ar.make_case(3, 3, "noise")
    d = [torch.from_numpy(a).to(dev) for a in (c["ref"], c["samples"], c["seq"])]
    B, K, L = 3, 3, 3
    nbytes = lib.ptamd_aligned_error_workspace_bytes(B, K, L)
    whole = torch.zeros(nbytes + 32, dtype=torch.uint8, device=dev)
    ws = whole[:nbytes]
    assert ws.data_ptr() % 16 == 0
    outs = outputs(B, L, dev, 0xFF)

    def call(B_=B, K_=K, L_=L, n=nbytes, w=ws, null=None):
        a = [P(d[0]), P(d[1]), P(d[2]), B_, K_, L_, P(outs["ae"].t), P(outs["stats"].t), P(outs["usable"].t), P(w), n, _lib.stream()]
        if null is not None:
            a[null] = None
        return lib.ptamd_aligned_error(*a)

    for null in (0, 1, 2, 6, 7, 8):
        assert call(null=null) == -1                                 # PTAMD_ERR_BAD_SHAPE: a NULL array
    assert call(B_=0) == -1 and call(K_=0) == -1 and call(L_=0) == -1
    assert lib.ptamd_aligned_error_workspace_bytes(0, K, L) == 0 and lib.ptamd_aligned_error_workspace_bytes(B, 0, L) == 0
    assert lib.ptamd_aligned_error_workspace_bytes(B, K, 0) == 0
    assert call(n=nbytes - 1) == -3 and call(null=9) == -3           # PTAMD_ERR_WORKSPACE: one byte short; none
    assert call(w=whole[8:8 + nbytes]) == -5                         # PTAMD_ERR_ALIGN
    torch.cuda.synchronize()
    for name, g in outs.items():
        assert bool((g.raw == g.poison).all()), name                 # nothing was launched: every byte is still poison
    assert bool((whole == 0).all())


def test_wrapper_returns_the_bits_of_the_abi_call(dev):
    from protein_transformer_amd.ensemble import aligned_error
    c = ar.make_case(65, 3, "noise")
    d = [torch.from_numpy(a).to(dev) for a in (c["ref"], c["samples"], c["seq"])]
    a = call_abi(*d, dev)
    big = ar.make_case(129, 3, "noise")
    aligned_error(*[torch.from_numpy(big[k]).to(dev) for k in ("ref", "samples", "seq")])   # a larger batch through the cached workspace
    ae, stats, usable = aligned_error(*d)
    assert ae.shape == (3, 65, 65) and stats.shape == (3, 2) and usable.shape == (3,) and usable.dtype == torch.int32
    for k, v in (("ae", ae), ("stats", stats), ("usable", usable)):
        assert v.is_cuda and v.cpu().numpy().tobytes() == a[k].tobytes(), k
    with pytest.raises(AssertionError):
        aligned_error(d[0], d[1][:, :, :-14], d[2])
    with pytest.raises(RuntimeError, match="device tensors only"):
        aligned_error(d[0].cpu(), d[1].cpu(), d[2].cpu())


def test_true_aligned_error_is_the_k1_form_with_the_truth_as_reference(dev):
    from protein_transformer_amd.ensemble import aligned_error
    from protein_transformer_amd.eval_metrics import aligned_error_batch
    c = ar.make_case(65, 1, "noise")
    truth, pred, seq = (torch.from_numpy(c[k]).to(dev) for k in ("ref", "samples", "seq"))
    ae, stats = aligned_error_batch(pred[:, 0], truth, seq)
    want = aligned_error(truth, pred, seq)
    assert ae.cpu().numpy().tobytes() == want[0].cpu().numpy().tobytes()
    assert stats.cpu().numpy().tobytes() == want[1].cpu().numpy().tobytes()
