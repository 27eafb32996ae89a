"""MI355X tests of the binned-lDDT loss kernels (csrc/plddt.hip: `ptamd_plddt_fwd`, `ptamd_plddt_bwd`) against their fp64
restatement tests/plddt_ref.py, at the lane and row edges: 2 / 50 / 63 / 64 bins, 1, R - 1, R, R + 1 rows and several workspace
records with a ragged last one (R = ptamd_plddt_rows_per_block()), padded row strides, both target strides, targets on and next to
every bin edge, rows that do not count, no counted row at all, inference without a target, logits at +-80.

Every buffer the kernels write sits between guard bands of a sentinel bit pattern and is pre-filled with it (a NaN), the spare
logit columns hold NaN: a lane that reads beyond nbins, a row that is skipped or a store out of its row shows.

ERROR MEASURE.  plddt, ce, sums[0] and every element of dlogits are compared with fp64 RELATIVE TO THE REFERENCE VALUE,
|got - ref| / max(|ref|, 2^-126): fp32 holds no normal number below 2^-126, so a reference below it (the loss of a row whose other
lanes underflow, e^-160) is compared on that floor.  sums[1], the zeros of dlogits and the NaNs of ce are exact.
BARS: 8 x the largest error measured on the MI355X over every case of this file (profiles/plddt/NOTES.md; the kernels are
deterministic, the margin is for other inputs), none above the project's 1e-5 parity bar."""
import ctypes as C

import numpy as np
import pytest
import torch

import plddt_ref as R

pytestmark = pytest.mark.gpu

FLT_MIN = 2.0 ** -126
SENT = 0x7FC0BEEF                 # a NaN: guard bands and the pre-fill of every output
GUARD = 64                        # floats in front of and behind every buffer (256 bytes: the payload stays 16-byte aligned)
PARITY = 1e-5                     # no bar above it
# 8 x the largest error measured on the MI355X over every case of this file (profiles/plddt/NOTES.md)
BARS = {"plddt": 8 * 2.700e-7, "ce": 8 * 1.345e-7, "sums0": 8 * 5.572e-8, "dlogits": 8 * 2.804e-7}
WORST = {k: 0.0 for k in BARS}
NBINS = (2, 50, 63, 64)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert all(b <= PARITY for b in BARS.values())
    yield torch.device("cuda:0")
    for k in BARS:
        print(f"\n[plddt] largest |got - ref| / max(|ref|, 2^-126), {k}: {WORST[k]:.3e} (bar {BARS[k]:.1e})", end="")
    print()


def lib():
    from protein_transformer_amd._lib import lib as _lib
    return _lib()


def stream():
    from protein_transformer_amd import kernels as K_
    return K_.stream()


def rows_per_block():
    return lib().ptamd_plddt_rows_per_block()


class Guarded:
    """n floats on the device, pre-filled with the sentinel, between two guard bands of it."""

    def __init__(self, dev, n):
        self.n = n
        self.buf = torch.full((GUARD + n + GUARD,), SENT, dtype=torch.int32).to(dev)
        self.t = self.buf[GUARD:GUARD + n].view(torch.float32)

    def ptr(self, offset=0):
        return C.c_void_p(self.t.data_ptr() + 4 * offset)

    def set(self, values):
        self.t.copy_(torch.from_numpy(np.ascontiguousarray(values, np.float32).reshape(-1)))
        return self

    def collect(self):
        """The payload as fp32 (and its bits); asserts that the guard bands still hold the sentinel."""
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == SENT).all() and (b[GUARD + self.n:] == SENT).all(), "a guard band was written"
        return b[GUARD:GUARD + self.n].view(np.float32).copy()

    def untouched(self):
        return (self.collect().view(np.int32) == SENT).all()


def call(dev, logits, target, ld, ldd, stride, coef=1.0, backward=True):
    """One forward (and backward) call on logits [T, nbins] fp32 / target [T] fp32 or None, laid out with row stride ld (spare
    columns NaN) and target stride `stride` (spare slots NaN - a finite value would not matter, a read of it would show as a row
    that counts).  Returns the outputs as host arrays; dlogits as the whole [T, ldd]."""
    T, nbins = logits.shape
    lg = np.full((T, ld), np.nan, np.float32)
    lg[:, :nbins] = logits
    d_logits = Guarded(dev, T * ld).set(lg)
    d_plddt, d_ce, d_sums = Guarded(dev, T), Guarded(dev, T), Guarded(dev, 2)
    nws = lib().ptamd_plddt_workspace_bytes(T)
    assert nws == 16 * -(-T // rows_per_block())
    d_ws = Guarded(dev, nws // 4)
    d_target = None
    if target is not None:
        tg = np.full(((T - 1) * stride + 1,), np.nan, np.float32)
        tg[::stride] = target
        d_target = Guarded(dev, tg.size).set(tg)
    P = lambda g: g.ptr() if g is not None else None                                    # noqa: E731
    rc = lib().ptamd_plddt_fwd(P(d_logits), ld, P(d_target), stride, T, nbins, P(d_plddt), P(d_ce) if target is not None else None,
                               P(d_sums) if target is not None else None, P(d_ws) if target is not None else None,
                               nws if target is not None else 0, stream())
    assert rc == 0, rc
    out = {"plddt": d_plddt.collect()}
    if target is None:
        torch.cuda.synchronize()
        assert d_ce.untouched() and d_sums.untouched() and d_ws.untouched()
        assert np.array_equal(d_logits.collect().view(np.int32), lg.reshape(-1).view(np.int32))
        return out
    out.update(ce=d_ce.collect(), sums=d_sums.collect())
    d_ws.collect()
    if backward:
        d_dl = Guarded(dev, T * ldd)
        rc = lib().ptamd_plddt_bwd(P(d_logits), ld, P(d_target), stride, T, nbins, P(d_sums), coef, P(d_dl), ldd, stream())
        assert rc == 0, rc
        out["dlogits"] = d_dl.collect().reshape(T, ldd)
    assert np.array_equal(d_logits.collect().view(np.int32), lg.reshape(-1).view(np.int32))         # the inputs are inputs
    return out


def rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert np.isfinite(got).all() and np.isfinite(ref).all()
    return float((np.abs(got - ref) / np.maximum(np.abs(ref), FLT_MIN)).max()) if got.size else 0.0


def check(out, logits, target, coef=1.0):
    """Every output of `call` against the fp64 restatement; records the errors and holds them to the bars."""
    T, nbins = logits.shape
    ref = R.bin_loss(logits, target)
    err = {"plddt": rel(out["plddt"], ref["plddt"])}
    if target is not None:
        counted = ref["counted"]
        assert np.isnan(out["ce"][~counted]).all() and np.isfinite(out["ce"][counted]).all()
        err["ce"] = rel(out["ce"][counted], ref["ce"][counted])
        n = int(counted.sum())
        assert out["sums"][1] == n
        if n:
            err["sums0"] = rel(out["sums"][0], ref["sums"][0])
        else:
            assert np.isnan(out["sums"][0])
        if "dlogits" in out:
            dl = out["dlogits"]
            assert (dl[:, nbins:] == 0).all(), "a spare gradient column is not exactly 0"
            assert (dl[~counted] == 0).all(), "a row that does not count has a gradient"
            err["dlogits"] = rel(dl[:, :nbins], R.bin_loss_grad(logits, target, coef))
    for k, v in err.items():
        WORST[k] = max(WORST[k], v)
    for k, v in err.items():
        assert v <= BARS[k], (k, v, BARS[k])
    return ref


def edge_targets(nbins):
    """k / nbins as fp32 for every k (0.0 and 1.0 among them) and its two fp32 neighbours, then what does not count."""
    edges = (np.arange(nbins + 1, dtype=np.float64) / nbins).astype(np.float32)
    below, above = np.nextafter(edges, np.float32(-1)), np.nextafter(edges, np.float32(2))
    return np.concatenate([edges, below, above, np.array([np.nan, np.inf, -np.inf, -0.5, 1.5, 3e38], np.float32)])


def mixed_targets(rng, T, nbins):
    """T targets: random ones in [0, 1), edge values, and NaN / +-inf rows mixed in (about a fifth); at least one row counts
    where T > 1, and the single row of T = 1 does."""
    pool = edge_targets(nbins)
    t = rng.random(T).astype(np.float32)
    pick = rng.random(T)
    t = np.where(pick < 0.4, pool[rng.integers(0, len(pool), T)], t).astype(np.float32)
    out = rng.random(T) < 0.2
    t[out] = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), int(out.sum()))
    t[0] = np.float32(0.37)
    return t


def sizes():
    r = rows_per_block()
    return sorted({1, r - 1, r, r + 1, 3 * r + 5} - {0})


@pytest.mark.parametrize("nbins", NBINS)
def test_rows_and_lanes_at_their_edges(dev, nbins):
    """T in {1, R - 1, R, R + 1, 3 R + 5 (four workspace records, the last one ragged)}, both target strides, padded and tight
    strides, ldd beyond one wavefront of columns."""
    rng = np.random.default_rng(100 + nbins)
    for T in sizes():
        logits = rng.normal(0, 2.5, (T, nbins)).astype(np.float32)
        target = mixed_targets(rng, T, nbins)
        for stride, ld, ldd, coef in [(1, nbins + 3, nbins + 5, 1.0), (2, nbins, nbins, 0.5), (2, nbins + 9, 64 + 70, 1.0)]:
            check(call(dev, logits, target, ld, ldd, stride, coef), logits, target, coef)


@pytest.mark.parametrize("nbins", NBINS)
def test_targets_on_and_next_to_every_bin_edge(dev, nbins):
    target = edge_targets(nbins)
    T = len(target)
    rng = np.random.default_rng(200 + nbins)
    logits = rng.normal(0, 2.5, (T, nbins)).astype(np.float32)
    out = call(dev, logits, target, nbins + 1, nbins + 2, 2)
    ref = check(out, logits, target)
    # the bin the kernel took shows in the gradient: the one negative entry of a counted row
    got_bin = np.argmin(out["dlogits"][:, :nbins], axis=1)
    assert (got_bin[ref["counted"]] == ref["bin"][ref["counted"]]).all()
    assert ref["bin"][0] == 0 and ref["bin"][nbins] == nbins - 1 and not ref["counted"][-6:-3].any()


@pytest.mark.parametrize("nbins", NBINS)
def test_no_row_counts(dev, nbins):
    rng = np.random.default_rng(300 + nbins)
    T = rows_per_block() + 3
    logits = rng.normal(0, 2.5, (T, nbins)).astype(np.float32)
    target = rng.choice(np.array([np.nan, np.inf, -np.inf], np.float32), T)
    out = call(dev, logits, target, nbins + 2, nbins + 6, 1)
    check(out, logits, target)
    assert np.isnan(out["sums"][0]) and out["sums"][1] == 0 and np.isnan(out["ce"]).all()
    assert (out["dlogits"].view(np.int32) == 0).all()                                    # +0.0 everywhere, spare columns included


@pytest.mark.parametrize("nbins", NBINS)
def test_inference_without_a_target(dev, nbins):
    rng = np.random.default_rng(400 + nbins)
    for T in sizes():
        logits = rng.normal(0, 2.5, (T, nbins)).astype(np.float32)
        out = call(dev, logits, None, nbins + 4, nbins, 1)
        check(out, logits, None)
        with_target = call(dev, logits, mixed_targets(rng, T, nbins), nbins + 4, nbins, 1, backward=False)
        assert np.array_equal(out["plddt"].view(np.int32), with_target["plddt"].view(np.int32))   # the same pLDDT either way


@pytest.mark.parametrize("nbins", NBINS)
def test_logits_at_plus_and_minus_80_on_single_lanes(dev, nbins):
    rng = np.random.default_rng(500 + nbins)
    T = 2 * rows_per_block() + 1
    logits = rng.normal(0, 1.0, (T, nbins)).astype(np.float32)
    hot, cold = rng.integers(0, nbins, T), rng.integers(0, nbins, T)
    kind = np.arange(T) % 3                                   # +80 on one lane / -80 on one lane / both
    logits[kind != 1, hot[kind != 1]] = 80.0
    logits[kind != 0, cold[kind != 0]] = -80.0
    # the target's bin on the hot lane, on the cold lane, or anywhere
    where = np.where(np.arange(T) % 2 == 0, hot, cold)
    target = ((where + 0.5) / nbins).astype(np.float32)
    target[3::7] = rng.random(len(target[3::7])).astype(np.float32)
    out = call(dev, logits, target, nbins + 1, nbins + 3, 1)
    assert np.isfinite(out["plddt"]).all() and np.isfinite(out["ce"]).all() and np.isfinite(out["dlogits"]).all()
    ref = check(out, logits, target)
    assert ref["ce"].max() > 79.0 and 0 < ref["ce"].min() < 1e-30                        # both ends of the loss were seen
    # uniform rows, and a row that is one-hot to fp32: pLDDT = the bin centre, loss 0 against fp64's e^-160 (the floor)
    flat = np.zeros((3, nbins), np.float32)
    flat[1, nbins - 1], flat[1, :nbins - 1] = 80.0, -80.0
    flat[2, 0], flat[2, 1:] = -80.0, 80.0
    t3 = np.array([0.5, (nbins - 0.5) / nbins, 0.0], np.float32)
    out = call(dev, flat, t3, nbins, nbins, 1)
    check(out, flat, t3)
    assert out["plddt"][0] == pytest.approx(50.0, rel=BARS["plddt"]) and out["ce"][0] == pytest.approx(np.log(nbins), rel=BARS["ce"])
    assert out["plddt"][1] == pytest.approx(100.0 * (nbins - 0.5) / nbins, rel=BARS["plddt"])


def test_two_calls_are_bit_identical(dev):
    rng = np.random.default_rng(600)
    nbins, T = 50, 5 * rows_per_block() + 7
    logits = rng.normal(0, 2.5, (T, nbins)).astype(np.float32)
    target = mixed_targets(rng, T, nbins)
    a, b = (call(dev, logits, target, 52, 52, 2) for _ in range(2))
    for k in ("plddt", "ce", "sums", "dlogits"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32)), k
    # ... and a row's result does not depend on the rows around it or on the strides
    c = call(dev, logits[7:8], target[7:8], 64, 50, 1)
    assert c["plddt"][0].view(np.int32) == a["plddt"][7].view(np.int32) and c["ce"][0].view(np.int32) == a["ce"][7].view(np.int32)


def test_bad_arguments_return_the_code_and_write_nothing(dev):
    nbins, T = 50, rows_per_block() + 1
    bufs = {k: Guarded(dev, n) for k, n in dict(logits=T * 52, target=2 * T, plddt=T, ce=T, sums=2, ws=8, dlogits=T * 52).items()}
    good = dict(ld=52, stride=2, T=T, nbins=nbins, ws_bytes=32, ldd=52)

    def fwd(**kw):
        a = {**good, **{k: b.ptr() for k, b in bufs.items()}, **kw}
        return lib().ptamd_plddt_fwd(a["logits"], a["ld"], a["target"], a["stride"], a["T"], a["nbins"], a["plddt"], a["ce"], a["sums"],
                                     a["ws"], a["ws_bytes"], stream())

    def bwd(**kw):
        a = {**good, **{k: b.ptr() for k, b in bufs.items()}, **kw}
        return lib().ptamd_plddt_bwd(a["logits"], a["ld"], a["target"], a["stride"], a["T"], a["nbins"], a["sums"], 1.0, a["dlogits"],
                                     a["ldd"], stream())

    for kw in (dict(T=0), dict(T=-5), dict(nbins=1), dict(nbins=65), dict(nbins=0), dict(ld=49), dict(logits=None), dict(plddt=None),
               dict(ce=None), dict(sums=None), dict(stride=0), dict(stride=-1)):
        assert fwd(**kw) == -1, kw                                                      # PTAMD_ERR_BAD_SHAPE
    assert fwd(ws=None) == -3 and fwd(ws_bytes=31) == -3 and fwd(ws_bytes=0) == -3      # PTAMD_ERR_WORKSPACE
    assert fwd(ws=bufs["ws"].ptr(2)) == -5                                              # PTAMD_ERR_ALIGN
    for kw in (dict(T=0), dict(nbins=1), dict(nbins=65), dict(ld=49), dict(ldd=49), dict(logits=None), dict(target=None),
               dict(sums=None), dict(dlogits=None), dict(stride=0)):
        assert bwd(**kw) == -1, kw
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert b.untouched(), k
