"""MI355X tests of the superposed ensemble spread (csrc/ensemble.hip, `ptamd_ensemble_spread`) against its fp64 restatement
tests/ensemble_ref.py, through the C ABI on buffers this file owns.

Cases: L in {1, 2, 3, 63, 64, 65, 129} x K in {1, 2, 5}, three proteins of different lengths per batch (padded residues behind
present ones, one protein with two present residues).  The reference structures are random-angle chains (`synthetic.sample_angles`
through the NeRF kernel); a sample is the reference under a rigid motion plus Gaussian displacements of 0.1 .. 3 A, except the
special ones: an identical copy, a rigidly moved copy, a mirror image, a sample with a NaN C-alpha, a sample with a NaN side-chain
atom.  Slots a residue type does not have and padded residues hold NaN in the samples: they must never reach a result.

Outputs are pre-filled with poison (0xFF bytes: a NaN no kernel writes; 0xCD bytes in the integers) inside guard bands of 64
elements; the workspace sits at offset 256 of a poisoned buffer 512 bytes longer and is handed over filled with 0xFF and with
0x00.  Asserted: every output element is written, no guard byte is touched, the two runs give the same bits, and the values are
within `ensemble_ref.tol_sq` - on the squares - of fp64, with the NaN pattern and `usable` exact."""
import numpy as np
import pytest
import torch

import ensemble_ref as er

pytestmark = pytest.mark.gpu

GUARD = 64
LENGTHS = (1, 2, 3, 63, 64, 65, 129)
SPECIAL = {   # K -> {(protein, sample): kind}; everything else is a moved, noisy copy
    1: {(0, 0): "noise", (1, 0): "mirror", (2, 0): "nan_sc"},
    2: {(0, 0): "identical", (0, 1): "nan_ca", (1, 0): "rigid", (1, 1): "mirror", (2, 0): "nan_sc"},
    5: {(0, 0): "identical", (0, 1): "rigid", (0, 2): "mirror", (0, 3): "nan_ca", (0, 4): "nan_sc", (1, 0): "mirror",
        (1, 2): "nan_ca", (2, 1): "nan_ca", (2, 3): "rigid"},
}


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

    def any_poison_left(self):
        return bool((self.inner.view(-1, self.isz) == self.poison).all(1).any())


def lens_of(L):
    return [L, max(1, (L + 1) // 2), min(L, 2)]


_cases = {}


def make_case(L, K, dev):
    """(ref [3, L*14, 3], samples [3, K, L*14, 3], seq [3, L]) fp32 / int64 numpy, the extent X of the coordinates that count, and
    the fp64 reference results; built once per (L, K)."""
    if (L, K) in _cases:
        return _cases[(L, K)]
    from protein_transformer_amd import synthetic
    from protein_transformer_amd.protein.Structure import nerf_forward
    rng = np.random.default_rng(1000 * L + K)
    lens = lens_of(L)
    seq = np.full((3, L), er.PAD_ID, np.int64)
    ang = np.zeros((3, L, 12), np.float32)
    for b, n in enumerate(lens):
        seq[b, :n] = rng.integers(0, 20, n)
        seq[b, 0] = er.AA.index("W")                                 # a residue with every side-chain slot, for `nan_sc`
        ang[b, :n] = synthetic.sample_angles(rng, n)
    ref = nerf_forward(torch.from_numpy(ang).to(dev), torch.from_numpy(seq).to(dev))[0].cpu().numpy().astype(np.float32)
    assert np.isfinite(ref).all()
    samples = np.zeros((3, K, L * er.SLOTS, 3), np.float32)
    counts = np.array([er.atom_mask(seq[b]).reshape(-1) for b in range(3)])            # [3, L*14]
    for b in range(3):
        for k in range(K):
            kind = SPECIAL[K].get((b, k), "noise")
            if kind == "mirror" and lens[b] < 4:
                kind = "noise"
            r64 = ref[b].astype(np.float64)
            R, t = er.random_rigid(rng)
            if kind == "identical":
                s = r64
            elif kind == "rigid":
                s = r64 @ R.T + t
            elif kind == "mirror":
                s = r64 * np.array([1.0, 1.0, -1.0])
            else:
                s = r64 @ R.T + t + rng.normal(0, rng.uniform(0.1, 3.0), r64.shape)
            samples[b, k] = s.astype(np.float32)
            if kind == "nan_ca":
                samples[b, k, (lens[b] - 1) * er.SLOTS + er.CA, rng.integers(0, 3)] = np.nan
            if kind == "nan_sc":
                samples[b, k, 0 * er.SLOTS + 4 + rng.integers(0, 10), rng.integers(0, 3)] = np.nan
    x = max(float(np.abs(ref[counts]).max()), float(np.nanmax(np.abs(samples[np.repeat(counts[:, None], K, 1)]))))
    samples[~np.repeat(counts[:, None], K, 1)] = np.nan               # slots without an atom, padded residues
    ref = ref.copy()
    ref[~counts] = np.nan
    want = er.reference(ref, samples, seq)
    _cases[(L, K)] = (ref, samples, seq, x, want)
    return _cases[(L, K)]


def call_abi(ref, samples, seq, ws_fill, dev):
    from protein_transformer_amd import _lib
    lib, P = _lib.lib(), _lib.ptr
    B, K, L = samples.shape[0], samples.shape[1], seq.shape[1]
    nbytes = lib.ptamd_ensemble_workspace_bytes(B, K, L)
    assert nbytes == B * K * 64
    whole = torch.full((nbytes + 512,), 0xCD, dtype=torch.uint8, device=dev)
    ws = whole[256:256 + nbytes]
    assert ws.data_ptr() % 16 == 0
    ws.fill_(ws_fill)
    outs = dict(rmsd=Guarded((B, K), torch.float32, dev, 0xFF), rmsf=Guarded((B, L, 2), torch.float32, dev, 0xFF),
                usable=Guarded((B,), torch.int32, dev, 0xCD))
    rc = lib.ptamd_ensemble_spread(P(ref), P(samples), P(seq), B, K, L, P(outs["rmsd"].t), P(outs["rmsf"].t), P(outs["usable"].t),
                                   P(ws), nbytes, _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    for name, g in outs.items():
        assert g.guards_intact(), name
        assert not g.any_poison_left(), name
    assert bool((whole[:256] == 0xCD).all()) and bool((whole[256 + nbytes:] == 0xCD).all())
    return {k: g.t.cpu().numpy().copy() for k, g in outs.items()}


def check(got, want, x):
    rmsd, rmsf, usable = want
    assert (got["usable"] == usable).all(), (got["usable"], usable)
    worst = 0.0
    for g, w in ((got["rmsd"], rmsd), (got["rmsf"], rmsf)):
        g = g.astype(np.float64)
        assert (np.isnan(g) == np.isnan(w)).all()
        ok = ~np.isnan(w)
        err, bound = np.abs(g[ok] ** 2 - w[ok] ** 2), er.tol_sq(w[ok], x)
        if err.size:
            worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (float(err.max()), float(bound[err.argmax()]))
    return worst


@pytest.mark.parametrize("K", (1, 2, 5))
@pytest.mark.parametrize("L", LENGTHS)
def test_spread_against_fp64(L, K, dev):
    ref, samples, seq, x, want = make_case(L, K, dev)
    d = [torch.from_numpy(a).to(dev) for a in (ref, samples, seq)]
    a = call_abi(*d, 0xFF, dev)
    b = call_abi(*d, 0x00, dev)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k                   # the same bits, whatever the workspace held
    worst = check(a, want, x)
    print(f"L {L} K {K}: extent {x:.1f} A, worst |gpu^2 - ref^2| / bound {worst:.3f}, usable {list(a['usable'])}")
    lens = lens_of(L)
    for b_, n in enumerate(lens):
        assert np.isnan(a["rmsf"][b_, n:]).all()                     # padded residues
        if n < 3:
            assert a["usable"][b_] == 0 and np.isnan(a["rmsd"][b_]).all() and np.isnan(a["rmsf"][b_]).all()
    if L >= 3:
        for (b_, k), kind in SPECIAL[K].items():
            if lens[b_] < 3:
                continue
            if kind == "nan_ca":
                assert np.isnan(a["rmsd"][b_, k])
            elif kind in ("identical", "rigid"):
                assert a["rmsd"][b_, k] <= er.tol(0.0, x)
            elif kind == "mirror" and lens[b_] >= 8:
                assert a["rmsd"][b_, k] > 0.5                        # not fitted by a reflection
            else:
                assert np.isfinite(a["rmsd"][b_, k])


def test_wrapper_returns_the_bits_of_the_abi_call(dev):
    from protein_transformer_amd.ensemble import ensemble_spread
    ref, samples, seq, x, want = make_case(65, 5, dev)
    d = [torch.from_numpy(a).to(dev) for a in (ref, samples, seq)]
    a = call_abi(*d, 0xFF, dev)
    ensemble_spread(*[torch.from_numpy(v).to(dev) for v in make_case(129, 5, dev)[:3]])    # a larger batch through the cached workspace
    rmsd, rmsf, usable = ensemble_spread(*d)
    assert rmsd.shape == (3, 5) and rmsf.shape == (3, 65, 2) and usable.shape == (3,) and usable.dtype == torch.int32
    for k, v in (("rmsd", rmsd), ("rmsf", rmsf), ("usable", usable)):
        assert v.is_cuda and v.cpu().numpy().tobytes() == a[k].tobytes(), k
    with pytest.raises(AssertionError):
        ensemble_spread(d[0], d[1][:, :, :-14], d[2])
    with pytest.raises(RuntimeError, match="device tensors only"):
        ensemble_spread(d[0].cpu(), d[1].cpu(), d[2].cpu())


def test_a_protein_does_not_depend_on_its_batch_or_its_padding(dev):
    from protein_transformer_amd.ensemble import ensemble_spread
    ref, samples, seq, x, want = make_case(65, 2, dev)
    full = [v.cpu().numpy() for v in ensemble_spread(*[torch.from_numpy(a).to(dev) for a in (ref, samples, seq)])]
    n = lens_of(65)[1]                                               # protein 1 alone, in a row of its own length
    alone = [v.cpu().numpy() for v in ensemble_spread(torch.from_numpy(ref[1:2, :n * 14].copy()).to(dev),
                                                      torch.from_numpy(samples[1:2, :, :n * 14].copy()).to(dev),
                                                      torch.from_numpy(seq[1:2, :n].copy()).to(dev))]
    assert alone[0].tobytes() == full[0][1:2].tobytes() and alone[1].tobytes() == full[1][1:2, :n].tobytes()
    assert alone[2][0] == full[2][1]


def test_error_codes_launch_nothing(dev):
    from protein_transformer_amd import _lib
    lib, P = _lib.lib(), _lib.ptr
    ref, samples, seq, x, want = make_case(3, 2, dev)
    d = [torch.from_numpy(a).to(dev) for a in (ref, samples, seq)]
    B, K, L = 3, 2, 3
    nbytes = lib.ptamd_ensemble_workspace_bytes(B, K, L)
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    outs = dict(rmsd=Guarded((B, K), torch.float32, dev, 0xFF), rmsf=Guarded((B, L, 2), torch.float32, dev, 0xFF),
                usable=Guarded((B,), torch.int32, dev, 0xCD))
    args = lambda B_, K_, L_, n: (P(d[0]), P(d[1]), P(d[2]), B_, K_, L_, P(outs["rmsd"].t), P(outs["rmsf"].t),   # noqa: E731
                                  P(outs["usable"].t), P(ws), n, _lib.stream())
    assert lib.ptamd_ensemble_spread(*args(B, K, L, nbytes - 1)) == -3             # PTAMD_ERR_WORKSPACE
    assert lib.ptamd_ensemble_spread(*args(B, 0, L, nbytes)) == -1                 # PTAMD_ERR_BAD_SHAPE
    assert lib.ptamd_ensemble_spread(*args(B, K, 0, nbytes)) == -1
    assert lib.ptamd_ensemble_spread(*args(0, K, L, nbytes)) == -1
    assert lib.ptamd_ensemble_workspace_bytes(B, 0, L) == 0 and lib.ptamd_ensemble_workspace_bytes(B, K, 0) == 0
    torch.cuda.synchronize()
    for name, g in outs.items():
        assert bool((g.raw == g.poison).all()), name                 # nothing was launched: every byte is still poison
