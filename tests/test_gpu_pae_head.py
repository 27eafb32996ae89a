"""MI355X tests of the pair sweep of the PAE head (csrc/pae_head.hip: `ptamd_pae_head_fwd`, `ptamd_pae_head_bwd`) against their
fp64 restatement tests/pae_head_ref.py, through the C ABI: L in {1, 2, 63, 64, 65, 130} (one point tile, its edge, three tiles),
B = 3 with the lengths {L, ceil(L / 2), nothing present} and an unknown id inside a chain, H in {4, 32, 64}, nbins in {2, 50, 63,
64}, tight and padded strides, targets on and next to every bin edge, NaN / +-inf targets, no counted pair at all, inference
without a target, logits at +-80, two calls, a protein alone and inside a batch, every bad-argument code.

Every buffer the kernels write sits between guard bands of a sentinel bit pattern and is pre-filled with it (a NaN); the spare
columns of uv hold NaN; the inputs are verified unchanged.  u and v are multiples of 2^-8 in [-4, 4] (`pae_head_ref.grid_uv`), so
u + v is exact and the relu decision, the derivative 0 at exactly 0 included, is the reference's.

ERROR MEASURE.  pae, stats and sums[0]: |got - ref| / max(|ref|, 2^-126).  The reduced gradients duv, dw2, db2: |got - ref| over
the sum of the absolute values of the summands (the reference returns it): cancellation makes an element-relative error
meaningless there; where that sum is 0 the gradient must be exactly 0.  That sum takes the same 2^-126 floor as the other
measure: with a bias of 80 on one of two bins, whole rows and columns of duv are sums of terms ~e^-80 / n and come to 1e-40 ..
1e-75 - below fp32's normal range, where the fp64 reference ROUNDED TO fp32 already misses 1e-5 of that sum (1.0e-5 at 6e-41,
all of it where it underflows to 0), so no fp32 output can be held to a sum that small.  sums[1], zeros and NaNs are exact.
BARS: 8 x the largest error measured on the MI355X over every case of this file (profiles/pae_head/NOTES.md; the kernels are
deterministic, the margin is for other inputs), none above the project's 1e-5 parity bar."""
import ctypes as C

import numpy as np
import pytest
import torch

import pae_head_ref as R
from test_gpu_plddt import FLT_MIN, PARITY, Guarded, lib, rel, stream

pytestmark = pytest.mark.gpu

# 8 x the largest error measured on the MI355X over every case of this file (profiles/pae_head/NOTES.md)
BARS = {"pae": 8 * 4.168e-7, "stats": 8 * 4.617e-7, "sums0": 8 * 4.953e-8, "duv": 8 * 5.520e-7, "dw2": 8 * 4.622e-7,
        "db2": 8 * 2.852e-7}
WORST = {k: 0.0 for k in BARS}
PAD, UNKNOWN = 20, 21


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert all(b <= PARITY for b in BARS.values())
    yield torch.device("cuda:0")
    for k in BARS:
        print(f"\n[pae_head] largest error, {k}: {WORST[k]:.3e} (bar {BARS[k]:.1e})", end="")
    print()


def call(dev, uv, w2, b2, seq, target, bpa=2.0, pad=0, coef=1.0, backward=True):
    """One forward (and backward) call: uv [B, L, 2H] fp32 laid out with the row stride 2H + pad (spare columns NaN), duv with
    2H + 2 pad.  Returns host arrays; duv as the whole [B * L, ldd]."""
    B, L, H2 = uv.shape
    H, nbins = H2 // 2, w2.shape[0]
    lduv, ldd = H2 + pad, H2 + 2 * pad
    laid = np.full((B * L, lduv), np.nan, np.float32)
    laid[:, :H2] = uv.reshape(B * L, H2)
    d_uv, d_w2, d_b2 = Guarded(dev, laid.size).set(laid), Guarded(dev, w2.size).set(w2), Guarded(dev, nbins).set(b2)
    d_seq = torch.from_numpy(np.ascontiguousarray(seq, np.int64)).to(dev)
    d_pae, d_stats, d_sums = Guarded(dev, B * L * L), Guarded(dev, 2 * B), Guarded(dev, 2)
    nws = lib().ptamd_pae_head_workspace_bytes(B, L, H, nbins)
    assert nws > 0 and nws % 16 == 0
    d_ws = Guarded(dev, nws // 4)
    d_tg = Guarded(dev, B * L * L).set(target) if target is not None else None
    sq = C.c_void_p(d_seq.data_ptr())
    rc = lib().ptamd_pae_head_fwd(d_uv.ptr(), lduv, d_w2.ptr(), d_b2.ptr(), sq, d_tg.ptr() if d_tg else None, B, L, H, nbins, bpa,
                                  d_pae.ptr(), d_stats.ptr(), d_sums.ptr() if d_tg else None, d_ws.ptr() if d_tg else None,
                                  nws if d_tg else 0, stream())
    assert rc == 0, rc
    out = {"pae": d_pae.collect().reshape(B, L, L), "stats": d_stats.collect().reshape(B, 2)}

    def inputs_unchanged():
        assert np.array_equal(d_uv.collect().view(np.int32), laid.reshape(-1).view(np.int32))
        assert np.array_equal(d_w2.collect(), w2.reshape(-1)) and np.array_equal(d_b2.collect(), b2)
        assert np.array_equal(d_seq.cpu().numpy(), seq)
    if target is None:
        assert d_sums.untouched() and d_ws.untouched()
        inputs_unchanged()
        return out
    out["sums"] = d_sums.collect()
    d_ws.collect()
    if backward:
        d_duv, d_dw2, d_db2 = Guarded(dev, B * L * ldd), Guarded(dev, w2.size), Guarded(dev, nbins)
        rc = lib().ptamd_pae_head_bwd(d_uv.ptr(), lduv, d_w2.ptr(), d_b2.ptr(), sq, d_tg.ptr(), B, L, H, nbins, bpa, d_sums.ptr(), coef,
                                      d_duv.ptr(), ldd, d_dw2.ptr(), d_db2.ptr(), d_ws.ptr(), nws, stream())
        assert rc == 0, rc
        out.update(duv=d_duv.collect().reshape(B * L, ldd), dw2=d_dw2.collect().reshape(w2.shape), db2=d_db2.collect())
        d_ws.collect()
        assert np.array_equal(d_tg.collect().view(np.int32), np.asarray(target, np.float32).reshape(-1).view(np.int32))
    inputs_unchanged()
    return out


def scaled(got, ref, scale):
    """max |got - ref| / max(scale, 2^-126) where scale > 0; exactly 0 where it is 0."""
    got, ref, scale = (np.asarray(a, np.float64) for a in (got, ref, scale))
    assert np.isfinite(got).all()
    assert (got[scale == 0] == 0).all(), "a gradient without a summand is not exactly 0"
    return float((np.abs(got - ref)[scale > 0] / np.maximum(scale[scale > 0], FLT_MIN)).max()) if (scale > 0).any() else 0.0


def check(out, uv, w2, b2, seq, target, bpa=2.0, coef=1.0):
    ref = R.pair_head(uv, w2, b2, seq, target, bpa, coef)
    B, L, H2 = uv.shape
    defined = ref["defined"]
    assert np.isnan(out["pae"][~defined]).all() and np.isfinite(out["pae"][defined]).all()
    some = R.present(seq).any(axis=1)
    assert np.isnan(out["stats"][~some]).all() and np.isfinite(out["stats"][some]).all()
    err = {"pae": rel(out["pae"][defined], ref["pae"][defined]), "stats": rel(out["stats"][some], ref["stats"][some])}
    if "sums" in out:
        n = int(ref["counted"].sum())
        assert out["sums"][1] == n
        if n:
            err["sums0"] = rel(out["sums"][0], ref["sums"][0])
        else:
            assert np.isnan(out["sums"][0])
    if "duv" in out:
        assert (out["duv"][:, H2:].view(np.int32) == 0).all(), "a spare gradient column is not +0"
        absent = ~R.present(seq).reshape(-1)
        assert (out["duv"][absent] == 0).all(), "an absent residue has a gradient"
        err["duv"] = scaled(out["duv"][:, :H2], ref["duv"].reshape(B * L, H2), ref["abs_duv"].reshape(B * L, H2))
        err["dw2"] = scaled(out["dw2"], ref["dw2"], ref["abs_dw2"])
        err["db2"] = scaled(out["db2"], ref["db2"], ref["abs_db2"])
    for k, v in err.items():
        WORST[k] = max(WORST[k], v)
    for k, v in err.items():
        assert v <= BARS[k], (k, v, BARS[k])
    return ref


def batch_of(rng, L, H, nbins, scale=0.5):
    """B = 3: lengths L, ceil(L / 2) and a protein of padding only; an unknown id inside the first chain where it has room."""
    seq = np.full((3, L), PAD, np.int64)
    seq[0] = rng.integers(0, 20, L)
    seq[1, :-(-L // 2)] = rng.integers(0, 20, -(-L // 2))
    if L >= 3:
        seq[0, L // 2] = UNKNOWN
    uv = R.grid_uv(rng, 3, L, H)
    w2 = (rng.normal(0, scale, (nbins, H)) / np.sqrt(H)).astype(np.float32)
    b2 = rng.normal(0, 1.0, nbins).astype(np.float32)
    return uv, w2, b2, seq


def edge_targets(nbins, bpa):
    edges = (np.arange(nbins + 2, dtype=np.float64) / bpa).astype(np.float32)
    below, above = np.nextafter(edges, np.float32(-1)), np.nextafter(edges, np.float32(1e9))
    return np.concatenate([edges, below, above, np.array([np.nan, np.inf, -np.inf, -0.5, 3e38], np.float32)])


def mixed_targets(rng, shape, nbins, bpa):
    pool = edge_targets(nbins, bpa)
    t = (rng.random(shape) * 1.2 * nbins / bpa).astype(np.float32)
    t = np.where(rng.random(shape) < 0.3, pool[rng.integers(0, len(pool), shape)], t).astype(np.float32)
    t[rng.random(shape) < 0.15] = np.nan
    return t


@pytest.mark.parametrize("L", (1, 2, 63, 64, 65, 130))
def test_tiles_widths_and_bins_at_their_edges(dev, L):
    rng = np.random.default_rng(1000 + L)
    for H, nbins, pad, bpa, coef in [(4, 2, 0, 0.125, 1.0), (32, 64, 3, 2.0, 0.5), (64, 50, 5, 2.0, 1.0), (32, 63, 0, 1.5, 1.0)]:
        uv, w2, b2, seq = batch_of(rng, L, H, nbins)
        target = mixed_targets(rng, (3, L, L), nbins, bpa)
        target[0, 0, 0] = np.float32(0.3 / bpa)
        check(call(dev, uv, w2, b2, seq, target, bpa, pad, coef), uv, w2, b2, seq, target, bpa, coef)


@pytest.mark.parametrize("nbins", (2, 50, 63, 64))
def test_targets_on_and_next_to_every_bin_edge(dev, nbins):
    rng = np.random.default_rng(2000 + nbins)
    bpa, L = 2.0, 15
    uv, w2, b2, seq = batch_of(rng, L, 32, nbins)
    seq[0] = rng.integers(0, 20, L)                               # every pair of the first protein is defined
    edges = edge_targets(nbins, bpa)
    assert len(edges) <= L * L
    target = mixed_targets(rng, (3, L, L), nbins, bpa)
    target[0].reshape(-1)[:len(edges)] = edges
    ref = check(call(dev, uv, w2, b2, seq, target, bpa, 1), uv, w2, b2, seq, target, bpa)
    bins = ref["bin"][0].reshape(-1)
    assert bins[0] == 0 and bins[nbins] == nbins - 1 and bins[1] == min(1, nbins - 1)
    assert not ref["counted"][0].reshape(-1)[len(edges) - 5:len(edges) - 2].any()


def test_no_pair_counts(dev):
    rng = np.random.default_rng(3000)
    uv, w2, b2, seq = batch_of(rng, 65, 32, 64)
    target = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), (3, 65, 65))
    for coef in (1.0, -2.0):
        out = call(dev, uv, w2, b2, seq, target, 2.0, 2, coef)
        check(out, uv, w2, b2, seq, target, 2.0, coef)
        assert np.isnan(out["sums"][0]) and out["sums"][1] == 0
        for k in ("duv", "dw2", "db2"):
            assert (out[k].view(np.int32) == 0).all(), k          # +0.0 everywhere, spare columns included, whatever coef's sign
    # ... and with pairs that count and a negative coef, the zeros of the spare columns, absent residues and padding are still +0
    target = mixed_targets(rng, (3, 65, 65), 64, 2.0)
    out = call(dev, uv, w2, b2, seq, target, 2.0, 2, -2.0)
    check(out, uv, w2, b2, seq, target, 2.0, -2.0)
    assert (out["duv"][:, 64:].view(np.int32) == 0).all() and (out["duv"][~R.present(seq).reshape(-1)].view(np.int32) == 0).all()


@pytest.mark.parametrize("L,H,nbins", [(1, 4, 2), (65, 32, 64), (130, 64, 50)])
def test_inference_without_a_target(dev, L, H, nbins):
    rng = np.random.default_rng(4000 + L)
    uv, w2, b2, seq = batch_of(rng, L, H, nbins)
    out = call(dev, uv, w2, b2, seq, None, 2.0, 4)
    check(out, uv, w2, b2, seq, None)
    with_target = call(dev, uv, w2, b2, seq, mixed_targets(rng, (3, L, L), nbins, 2.0), 2.0, 4, backward=False)
    assert np.array_equal(out["pae"].view(np.int32), with_target["pae"].view(np.int32))   # the same matrix either way


@pytest.mark.parametrize("nbins", (2, 50, 64))
def test_logits_at_plus_and_minus_80(dev, nbins):
    rng = np.random.default_rng(5000 + nbins)
    L, bpa = 20, 2.0
    uv, w2, b2, seq = batch_of(rng, L, 32, nbins, scale=0.1)
    hot, cold = int(rng.integers(0, nbins)), int(rng.integers(0, nbins))
    for kind in range(3):                                         # +80 on one bin / -80 on one bin / both
        b = b2.copy()
        if kind != 1:
            b[hot] = 80.0
        if kind != 0:
            b[cold] = -80.0
        # the target's bin on the hot lane (whole columns of confidently right pairs: dv_j is a sum of terms ~e^-80 alone, which
        # the kernel carries unscaled so that they stay normal fp32 numbers), on the cold one, anywhere
        target = mixed_targets(rng, (3, L, L), nbins, bpa)
        target[0, :, ::2] = np.float32((hot + 0.5) / bpa)
        target[0, :, 1::4] = np.float32((cold + 0.5) / bpa)
        out = call(dev, uv, w2, b, seq, target, bpa, 1)
        for k in ("sums", "duv", "dw2", "db2"):
            assert np.isfinite(out[k]).all(), k
        check(out, uv, w2, b, seq, target, bpa)


def test_two_calls_and_a_protein_alone(dev):
    rng = np.random.default_rng(6000)
    L, H, nbins = 130, 32, 64
    uv, w2, b2, seq = batch_of(rng, L, H, nbins)
    target = mixed_targets(rng, (3, L, L), nbins, 2.0)
    a, b = (call(dev, uv, w2, b2, seq, target, 2.0, 3) for _ in range(2))
    for k in a:
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    # the second protein alone, its row padded no further than its own length: the same bits, with a target and without one
    n = -(-L // 2)
    inference = call(dev, uv, w2, b2, seq, None, 2.0, 3)
    for tg, whole in ((np.ascontiguousarray(target[1:2, :n, :n]), a), (None, inference)):
        alone = call(dev, np.ascontiguousarray(uv[1:2, :n]), w2, b2, seq[1:2, :n], tg, 2.0, 0, backward=False)
        assert np.array_equal(alone["pae"][0].view(np.int32), whole["pae"][1, :n, :n].view(np.int32))
        assert np.array_equal(alone["stats"][0].view(np.int32), whole["stats"][1].view(np.int32))


def test_bad_arguments_return_the_code_and_write_nothing(dev):
    B, L, H, nbins = 2, 5, 8, 50
    nws = lib().ptamd_pae_head_workspace_bytes(B, L, H, nbins)
    sizes = dict(uv=B * L * 18, w2=nbins * H, b2=nbins, target=B * L * L, pae=B * L * L, stats=2 * B, sums=2, ws=nws // 4 + 4,
                 duv=B * L * 18, dw2=nbins * H, db2=nbins)
    bufs = {k: Guarded(dev, n) for k, n in sizes.items()}
    seq = torch.zeros(B, L, dtype=torch.int64, device=dev)
    good = dict(lduv=18, ldd=18, B=B, L=L, H=H, nbins=nbins, bpa=2.0, ws_bytes=nws, seq=C.c_void_p(seq.data_ptr()))

    def args(kw):
        return {**good, **{k: b.ptr() for k, b in bufs.items()}, **kw}

    def fwd(**kw):
        a = args(kw)
        return lib().ptamd_pae_head_fwd(a["uv"], a["lduv"], a["w2"], a["b2"], a["seq"], a["target"], a["B"], a["L"], a["H"], a["nbins"],
                                        a["bpa"], a["pae"], a["stats"], a["sums"], a["ws"], a["ws_bytes"], stream())

    def bwd(**kw):
        a = args(kw)
        return lib().ptamd_pae_head_bwd(a["uv"], a["lduv"], a["w2"], a["b2"], a["seq"], a["target"], a["B"], a["L"], a["H"], a["nbins"],
                                        a["bpa"], a["sums"], 1.0, a["duv"], a["ldd"], a["dw2"], a["db2"], a["ws"], a["ws_bytes"], stream())

    shapes = (dict(B=0), dict(B=-1), dict(L=0), dict(B=70000), dict(H=0), dict(H=6), dict(H=68), dict(nbins=1), dict(nbins=65),
              dict(lduv=15), dict(bpa=0.0), dict(bpa=-2.0), dict(bpa=float("nan")), dict(bpa=float("inf")), dict(uv=None),
              dict(w2=None), dict(b2=None), dict(seq=None))
    for kw in shapes + (dict(pae=None), dict(stats=None), dict(sums=None)):
        assert fwd(**kw) == -1, kw                                                      # PTAMD_ERR_BAD_SHAPE
    for kw in shapes + (dict(ldd=15), dict(target=None), dict(sums=None), dict(duv=None), dict(dw2=None), dict(db2=None)):
        assert bwd(**kw) == -1, kw
    for f in (fwd, bwd):
        assert f(ws=None) == -3 and f(ws_bytes=nws - 1) == -3 and f(ws_bytes=0) == -3   # PTAMD_ERR_WORKSPACE
        assert f(ws=bufs["ws"].ptr(2)) == -5                                            # PTAMD_ERR_ALIGN
    for ws in (lib().ptamd_pae_head_workspace_bytes(0, 5, 8, 50), lib().ptamd_pae_head_workspace_bytes(2, 5, 6, 50),
               lib().ptamd_pae_head_workspace_bytes(2, 5, 8, 65)):
        assert ws == 0
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert b.untouched(), k
