"""csrc/elementwise.hip against fp64, element by element: the embedding forward and backward, the three LayerNorm kernel
families (forward, backward, backward fused with the dropout backward and the f16x2 bookkeeping), the deferred (dgamma,
dbeta) reduction over several sites, the bias column sum and the tanh / ReLU / dropout backward kernels.

The references are tests/elementwise_ref.py (plain numpy in fp64, written from the reference semantics); the first
tests of this module, which need no GPU, check THEM against torch autograd in float64.  Every comparison is per element
and in an error UNIT that follows from the operation (eps = 2^-24; xh, mean, rstd the fp64 values; kappa_t =
max(1, max_c |x_tc| rstd_t), what the rounding of the mean costs a normalised value):

    y              eps (|gamma_c| (kappa_t + |xh_tc|) + |beta_c|)
    mean           eps max_c |x_tc|
    rstd           eps rstd_t kappa_t
    dx, dropped    eps (kappa_t rstd_t max_c |gamma_c dy_tc| (1 + max_c xh_tc^2) + |dres_tc|)      (dropped: / (1 - p))
    dgamma         eps (sum_t |dy_tc| (|xh_tc| + kappa_t) + |dgamma_c before|)
    dbeta          eps (sum_t |dy_tc| + |dbeta_c before|)
    embedding out  eps x the first-order bound of an fp32 evaluation (embed_fwd_bound below), within 2 units
    demb           eps (sum_t |term| over the tokens of that vocabulary row + |demb before|)
    colsum         eps (sum_t |x_tc| + |out_c before|, accumulating)

Three of these are wider than a unit without them would be, because plain fp32 PyTorch cannot meet the narrower one:
  * the `before` terms: these outputs are accumulated INTO, and the last addition rounds at the size of what was there
    (without them fp32 PyTorch is up to 5240 units off at T = 1, where the preload dwarfs the one row that is added);
  * the embedding output: NOT eps |out|.  The bound is 3.5 to 5 times |out| (4 |x0| + |x0 + pe| + |out| without dropout,
    x0, x0 + pe and out of one sign here), so `2 units` is 7 to 10 eps |out|; fp32 PyTorch reaches 4.7 eps |out|, i.e.
    0.78 of the bound, and so does the kernel.
The multiple of its unit that a kernel may be off is not chosen here: for every input the same operation is also
evaluated with plain fp32 PyTorch on the CPU, and the kernel is allowed max(8, 4 x the multiple that evaluation
reaches) - another summation order and other fma contractions are legitimate, a wrong element, a missed row or a wrong
mean is hundreds to millions of units.  No element is left out of any comparison.

Largest multiples over all the cases below (fp32 PyTorch on the CPU / the kernel on the MI355X), from a run of this
module:

    family / output                      fp32 CPU    kernel
    colsum out                               1.74      3.78
    embed_bwd demb                           4.35      3.80
    embed_fwd out                            0.78      0.78
    layernorm_bwd dbeta                      3.85      3.54
    layernorm_bwd dgamma                     1.61      1.53
    layernorm_bwd dx                         2.64      3.49
    layernorm_bwd_dropout dbeta              3.90      3.44
    layernorm_bwd_dropout dgamma             1.55      1.53
    layernorm_bwd_dropout dropped            3.97      4.09
    layernorm_bwd_dropout dx                 3.56      3.09
    layernorm_bwd_reduce dbeta               2.26      2.11
    layernorm_bwd_reduce dgamma              0.98      0.71
    layernorm_fwd mean                       1.77      1.29
    layernorm_fwd rstd                       1.66      1.66
    layernorm_fwd y                          1.82      1.74
    tanh_bwd dx                              1.37      1.37

(relu_dropout_bwd, dropout_bwd, the dropout patterns and every f16x2 scale are compared bit for bit.)
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import elementwise_ref as R
from elementwise_ref import f64, scale_of
from test_host_logic import dropout_mask_restated

gpu = pytest.mark.gpu

EPS = 2.0 ** -24
SENTINEL = 0x7FC5A5A5               # a quiet NaN with a payload no kernel produces
SCALE_PRESET = 0x7F000000
SEED, STREAM = 0x1234_5678_9ABC, 13
FACTOR = 3.5
BAD_SHAPE = -1

# (family, output) -> [largest fp32-CPU multiple, largest kernel multiple]: bookkeeping only, printed behind the last test
# (pytest -s) so that the table in the docstring above can be written again from a run; no assertion reads it
MEASURED = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    torch.cuda.synchronize()
    if MEASURED:
        print("\n    family / output                      fp32 CPU    kernel")
        for (fam, out), (a, b) in sorted(MEASURED.items()):
            print(f"    {fam + ' ' + out:<36} {a:8.2f}  {b:8.2f}")


def multiple(got, want, unit):
    """Largest |got - want| / unit over ALL elements; where the unit is 0 only the exact value will do."""
    got, want = f64(got), f64(want)
    unit = np.broadcast_to(np.asarray(unit, np.float64), want.shape)
    assert got.shape == want.shape
    if not np.isfinite(got).all():
        return float("inf")
    err = np.abs(got - want)
    zero = unit == 0
    if (err[zero] != 0).any():
        return float("inf")
    return float((err[~zero] / unit[~zero]).max()) if (~zero).any() else 0.0


def check(family, output, got, ref32, want, unit, case, fixed=None):
    """The kernel within max(8, 4 x what fp32 PyTorch reaches) units of fp64 (`fixed`: within that many units); returns
    the allowed multiple."""
    m32, mk = multiple(ref32, want, unit), multiple(got, want, unit)
    rec = MEASURED.setdefault((family, output), [0.0, 0.0])
    rec[0], rec[1] = max(rec[0], m32), max(rec[1], mk)
    allowed = max(8.0, 4.0 * m32) if fixed is None else fixed
    print(f"{family} {output} {case}: fp32 CPU {m32:.2f} units, kernel {mk:.2f}, allowed {allowed:.2f}")
    assert mk <= allowed, f"{family} {output} {case}: kernel {mk:.3g} units from fp64, fp32 CPU {m32:.3g}, allowed {allowed:.3g}"
    return allowed


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy()


def as_float(scale_bits):
    return scale_bits.cpu().numpy().view(np.float32).astype(np.float64)


# ------------------------------------------------------------------------------------------------ LayerNorm inputs
LN_D = [4, 36, 252, 256, 260, 508, 512, 516, 1020, 1024, 1028, 2044, 2048]
LN_D_FUSED = [d for d in LN_D if d <= 1024]


def ln_refs(x, dy, gamma, beta, dres, dg0, db0):
    """fp64 results, their error units and the fp32-PyTorch results of one LayerNorm site (CPU tensors in, dict out)."""
    D = x.shape[1]
    y, mean, rstd = R.ln_fwd64(x, gamma, beta)
    x64, dy64, g64, b64, dres64 = f64(x), f64(dy), f64(gamma), f64(beta), f64(dres)
    xh = (x64 - mean[:, None]) * rstd[:, None]
    ax = np.abs(x64).max(1)
    kap = np.maximum(1.0, ax * rstd)
    u_dx0 = (EPS * kap * rstd * np.abs(dy64 * g64).max(1) * (1.0 + (xh ** 2).max(1)))[:, None] + 0 * x64
    c = dict(x=x, dy=dy, gamma=gamma, beta=beta, dres=dres, dg0=dg0, db0=db0, y=y, mean=mean, rstd=rstd,
             u_y=EPS * (np.abs(g64) * (kap[:, None] + np.abs(xh)) + np.abs(b64)), u_mean=EPS * ax, u_rstd=EPS * rstd * kap,
             u_dx={False: u_dx0, True: u_dx0 + EPS * np.abs(dres64)},
             u_dg=EPS * ((np.abs(dy64) * (np.abs(xh) + kap[:, None])).sum(0) + np.abs(f64(dg0))),
             u_db=EPS * (np.abs(dy64).sum(0) + np.abs(f64(db0))))
    dx, dg, db = R.ln_bwd64(dy, x, gamma)
    c["dx"] = {False: dx, True: dx + dres64}
    c["dg"], c["db"] = f64(dg0) + dg, f64(db0) + db
    # the same in plain fp32 PyTorch
    y32, mean32, rstd32 = torch.native_layer_norm(x, (D,), gamma, beta, R.LN_EPS)
    c["y32"], c["mean32"], c["rstd32"] = y32, mean32.reshape(-1), rstd32.reshape(-1)
    xr, gr, br = x.clone().requires_grad_(), gamma.clone().requires_grad_(), beta.clone().requires_grad_()
    F.layer_norm(xr, (D,), gr, br, R.LN_EPS).backward(dy)
    c["dx32"] = {False: xr.grad, True: xr.grad + dres}
    c["dg32"], c["db32"] = dg0 + gr.grad, db0 + br.grad
    return c


@functools.lru_cache(maxsize=None)
def ln_case(T, D):
    g = torch.Generator().manual_seed(7919 * T + D)
    rn = lambda *s: torch.randn(*s, generator=g)                          # noqa: E731
    x = rn(T, D) * torch.exp(2 * rn(T, 1))
    dy = rn(T, D) * torch.exp(2 * rn(T, 1))
    dres = rn(T, D)
    gamma = (torch.rand(D, generator=g) + 0.5) * torch.where(torch.rand(D, generator=g) < 0.1, -1.0, 1.0)
    beta = 0.3 * rn(D)
    if T >= 6:
        x[1] = rn(D) + 100                      # a large mean: conditioning about 100
        x[2] = 0.75                             # constant row: variance 0
        x[3] = 0.0
        x[4] = 1e-4 * rn(D)                     # variance far below eps
        dy[5] = 0.0
    return ln_refs(x, dy, gamma, beta, dres, rn(D), rn(D))


@functools.lru_cache(maxsize=None)
def ln_dev(T, D):
    """... on the device, with the mean and rstd that the forward kernel saved (what the backward kernels are given)."""
    from protein_transformer_amd import kernels as K
    c = ln_case(T, D)
    d = {k: c[k].cuda() for k in ("x", "dy", "gamma", "beta", "dres", "dg0", "db0")}
    _, d["mean"], d["rstd"] = K.layernorm_fwd(d["x"], d["gamma"], d["beta"])
    return d


# ------------------------------------------------------------------------------------------------ the references (no GPU)
def close64(got, want, what):
    """1e-12 relative to the LARGEST entry of the row ([T, D]) or of the vector, not to each element: an entry that cancels
    to nearly nothing carries the absolute rounding of its row in both float64 evaluations."""
    got, want = f64(got), f64(want)
    ref = np.abs(want).max(axis=-1, keepdims=True)
    assert got.shape == want.shape and bool((np.abs(got - want) <= 1e-12 * ref).all()), what


@pytest.mark.parametrize("T,D", [(1, 4), (3, 36), (37, 64), (33, 260), (40, 1020), (8, 2048)])
def test_layernorm_references_against_autograd_in_float64(T, D):
    c = ln_case(T, D)
    x, gam, bet = (c[k].double().requires_grad_() for k in ("x", "gamma", "beta"))
    y, mean, rstd = torch.native_layer_norm(x, (D,), gam, bet, R.LN_EPS)
    close64(c["y"], y, "y")
    close64(c["mean"], mean.reshape(-1), "mean")
    close64(c["rstd"], rstd.reshape(-1), "rstd")
    dy, dres = c["dy"].double(), c["dres"].double()
    (F.layer_norm(x, (D,), gam, bet, R.LN_EPS) + x).backward(dy)            # x + LN(x): dres = dy comes round the sublayer
    dx, dg, db = R.ln_bwd64(c["dy"], c["x"], c["gamma"], dres=c["dy"])
    close64(dx, x.grad, "dx")
    close64(dg, gam.grad, "dgamma")
    close64(db, bet.grad, "dbeta")
    x2 = c["x"].double().requires_grad_()
    F.layer_norm(x2, (D,), gam.detach(), bet.detach(), R.LN_EPS).backward(dy)
    close64(c["dx"][False], x2.grad, "dx without dres")
    close64(c["dx"][True], x2.grad + dres, "dx with dres")
    close64(c["dg"], c["dg0"].double() + gam.grad, "dgamma on top of what was there")
    close64(c["db"], c["db0"].double() + bet.grad, "dbeta on top of what was there")


@pytest.mark.parametrize("B,L,D", [(1, 1, 4), (3, 50, 64), (2, 301, 260)])
def test_embedding_references_against_autograd_in_float64(B, L, D):
    c = emb_case(B, L, D)
    emb = c["emb"].double().requires_grad_()
    ids = torch.from_numpy(R.embed_ids(c["seq"]))
    x0 = emb[ids] * np.sqrt(D)
    out = x0 + (x0 + c["pe"].double().repeat(B, 1))
    close64(R.embed_fwd64(c["seq"], c["emb"], c["pe"]), out, "embed fwd")
    out.backward(c["dout"].double())
    close64(R.embed_bwd64(c["seq"], c["dout"], D, 0.0, 0, c["demb0"]), c["demb0"].double() + emb.grad, "embed bwd")
    # out-of-range ids are row 21, rows without a token keep what they held
    unused = np.setdiff1d(np.arange(22), R.embed_ids(c["seq"]))
    assert len(unused) >= 2
    assert np.array_equal(R.embed_bwd64(c["seq"], c["dout"], D, 0.1, 5, c["demb0"])[unused], f64(c["demb0"])[unused])


def test_embedding_reference_with_dropout_is_the_adjoint_of_its_forward():
    """With fixed masks emb -> out is affine: <bwd(dout), delta> == <dout, fwd(emb + delta) - fwd(emb)> in fp64."""
    c = emb_case(3, 50, 64)
    delta = torch.randn(22, 64, generator=torch.Generator().manual_seed(3)).double()
    o1 = R.embed_fwd64(c["seq"], c["emb"], c["pe"], 0.1, 77)
    o2 = R.embed_fwd64(c["seq"], c["emb"].double() + delta, c["pe"], 0.1, 77)
    grad = R.embed_bwd64(c["seq"], c["dout"], 64, 0.1, 77, torch.zeros(22, 64))
    lhs, rhs = float((grad * f64(delta)).sum()), float(((o2 - o1) * f64(c["dout"])).sum())
    assert lhs == pytest.approx(rhs, rel=1e-12)
    assert ((o1 == 0) == ~R.embed_keep(150, 64, 0.1, 77, R.STREAM_EMB2)).all()


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_embedding_mask_keeps_the_stated_fraction(p):
    T, D = 4096, 64
    masks = [R.embed_keep(T, D, p, 99, s) for s in (R.STREAM_EMB1, R.STREAM_EMB2)]
    for m in masks:
        assert abs(m.mean() - (1 - p)) < 4 * np.sqrt(p * (1 - p) / m.size)
    assert abs((masks[0] & masks[1]).mean() - (1 - p) ** 2) < 0.01          # two streams, two masks


def test_small_references():
    g = torch.Generator().manual_seed(2)
    z = (torch.randn(1000, generator=g) * 3).double().requires_grad_()
    dy = torch.randn(1000, generator=g).double()
    y = torch.tanh(z)
    y.backward(dy)
    close64(R.tanh_bwd64(dy, y.detach()), z.grad, "tanh bwd")
    x = torch.randn(37, 5, generator=g)
    close64(R.colsum64(x, torch.ones(5)), 1 + x.double().sum(0), "colsum")
    assert np.array_equal(scale_of(np.array([0.0, 1.0, 3.0, 2.0 ** 14, 1e-30])), [2.0 ** 127, 2.0 ** 14, 2.0 ** 13, 1.0, 2.0 ** 114])
    d = R.dropped64(np.ones((45, 7)), 0.5, SEED, STREAM)
    assert np.array_equal(d != 0, dropout_mask_restated(45, 7, 0.5, SEED, STREAM)) and set(np.unique(d)) <= {0.0, 2.0}


# ------------------------------------------------------------------------------------------------ LayerNorm forward
@gpu
@pytest.mark.parametrize("D", LN_D)
@pytest.mark.parametrize("T", [1, 3, 4, 5, 37])
def test_layernorm_fwd(dev, T, D):
    from protein_transformer_amd import kernels as K
    c, d = ln_case(T, D), ln_dev(T, D)
    rs = torch.full((T,), SENTINEL, dtype=torch.int32, device=dev)
    y, mean, rstd = K.layernorm_fwd(d["x"], d["gamma"], d["beta"], row_scale=rs)
    case = f"T={T} D={D}"
    check("layernorm_fwd", "y", y, c["y32"], c["y"], c["u_y"], case)
    check("layernorm_fwd", "mean", mean, c["mean32"], c["mean"], c["u_mean"], case)
    check("layernorm_fwd", "rstd", rstd, c["rstd32"], c["rstd"], c["u_rstd"], case)
    assert np.array_equal(as_float(rs), scale_of(y.abs().amax(1).cpu().numpy())), case
    y0, mean0, rstd0 = K.layernorm_fwd(d["x"], d["gamma"], d["beta"])                  # the by-product changes nothing
    assert torch.equal(y0, y) and torch.equal(mean0, mean) and torch.equal(rstd0, rstd)


# ------------------------------------------------------------------------------------------------ LayerNorm backward
@gpu
@pytest.mark.parametrize("T,D", [(T, D) for T in (1, 5, 37) for D in LN_D] + [(2100, 64), (4100, 36)])
def test_layernorm_bwd(dev, T, D):
    """(2100 and 4100 rows: the second and third trip of the row loop, 2048 rows per trip)"""
    from protein_transformer_amd import kernels as K
    c, d = ln_case(T, D), ln_dev(T, D)
    for with_dres in (False, True):
        dg, db = d["dg0"].clone(), d["db0"].clone()
        dx = K.layernorm_bwd(d["dy"], d["x"], d["gamma"], d["mean"], d["rstd"], dg, db, dres=d["dres"] if with_dres else None)
        case = f"T={T} D={D} dres={with_dres}"
        check("layernorm_bwd", "dx", dx, c["dx32"][with_dres], c["dx"][with_dres], c["u_dx"][with_dres], case)
        check("layernorm_bwd", "dgamma", dg, c["dg32"], c["dg"], c["u_dg"], case)
        check("layernorm_bwd", "dbeta", db, c["db32"], c["db"], c["u_db"], case)


# ------------------------------------------------------------------------------------------------ the fused backward
def fused_outputs(dev, T, D):
    return dict(rs=torch.full((T,), SENTINEL, dtype=torch.int32, device=dev), bs=torch.full((T,), SENTINEL, dtype=torch.int32, device=dev),
                rmin=torch.full((4,), SCALE_PRESET, dtype=torch.int32, device=dev),
                bmin=torch.full((4,), SCALE_PRESET, dtype=torch.int32, device=dev))


def check_fused(dev, T, D, p, with_dres):
    from protein_transformer_amd import kernels as K
    c, d = ln_case(T, D), ln_dev(T, D)
    o = fused_outputs(dev, T, D)
    dg, db = d["dg0"].clone(), d["db0"].clone()
    factor = torch.tensor([FACTOR], device=dev)
    dx, dr = K.layernorm_bwd_dropout(d["dy"], d["x"], d["gamma"], d["mean"], d["rstd"], dg, db, d["dres"] if with_dres else None,
                                     p, SEED, STREAM, row_scale=o["rs"], bound_factor=factor, bound_scale=o["bs"],
                                     row_scale_min=o["rmin"], bound_scale_min=o["bmin"])
    case = f"T={T} D={D} p={p} dres={with_dres}"
    fam = "layernorm_bwd_dropout"
    dx64, u_dx = c["dx"][with_dres], c["u_dx"][with_dres]
    allowed = check(fam, "dx", dx, c["dx32"][with_dres], dx64, u_dx, case)
    check(fam, "dgamma", dg, c["dg32"], c["dg"], c["u_dg"], case)
    check(fam, "dbeta", db, c["db32"], c["db"], c["u_db"], case)
    drn = dr.cpu().numpy()
    assert np.isfinite(drn).all(), case
    if p > 0:
        keep = dropout_mask_restated(T, D, p, SEED, STREAM)
        ks32 = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        dr32 = np.where(keep, c["dx32"][with_dres].numpy() * ks32, np.float32(0.0))
        ks = R.keep_scale64(p)
        allowed = check(fam, "dropped", dr, dr32, R.dropped64(dx64, p, SEED, STREAM), u_dx * ks, case)
        # exactly the restated pattern (but for a dx that cancels to 0 within its tolerance)
        assert (((drn == 0) == ~keep) | (np.abs(dx64) <= allowed * u_dx)).all(), case
        assert not np.any(drn[~keep]), case
    else:
        assert dr is dx
    written = np.abs(drn)
    assert np.array_equal(as_float(o["rs"]), scale_of(written.max(1))), case                # exact maxima of what was written
    nrm = np.sqrt((written.astype(np.float64) ** 2).sum(1)) * FACTOR
    got, want = as_float(o["bs"]), scale_of(nrm.astype(np.float32))
    assert np.all((got == want) | (got == want * 2) | (got * 2 == want)), case            # fp32 rounding of the norm at a binade edge
    assert np.all(nrm * got < 2.0 ** 15 * (1 + 1e-6)), case
    assert np.array_equal(as_float(o["rmin"]), np.full(4, as_float(o["rs"]).min())), case
    assert np.array_equal(as_float(o["bmin"]), np.full(4, got.min())), case
    if T >= 6 and not with_dres:                # dy = 0 and nothing round the sublayer: a row of zeros, the largest finite power
        assert not written[5].any() and as_float(o["rs"])[5] == 2.0 ** 127 and got[5] == 2.0 ** 127, case


@gpu
@pytest.mark.parametrize("D", LN_D_FUSED)
@pytest.mark.parametrize("T", [1, 3, 5, 31, 32, 33, 41, 45])
def test_layernorm_bwd_dropout(dev, T, D):
    """Four wavefronts per 8-row generator group; 41 and 45 rows end inside the second half (rows r0 + 8 .. r0 + 11) of one."""
    for p in (0.0, 0.1, 0.5):
        for with_dres in (False, True):
            check_fused(dev, T, D, p, with_dres)


@gpu
@pytest.mark.parametrize("T", [4100, 8200, 16390])
def test_layernorm_bwd_dropout_fewer_wavefronts_per_group(dev, T):
    """4100 rows: two wavefronts per group; 8200: one; 16390: one, and 2052 groups for 2048 wavefronts (a second trip)."""
    for p in (0.0, 0.1):
        for with_dres in (False, True):
            check_fused(dev, T, 64, p, with_dres)


# ------------------------------------------------------------------------------------------------ canaries
def guarded(dev, rows, cols=None, dtype=torch.float32):
    """A [rows(, cols)] view into a sentinel-filled buffer: a guard row in front and behind ([rows, cols]), a spare word
    behind ([rows])."""
    if cols is None:
        buf = torch.full((rows + 1,), SENTINEL, dtype=torch.int32, device=dev)
        return buf, buf[:rows].view(dtype)
    buf = torch.full((rows + 2, cols), SENTINEL, dtype=torch.int32, device=dev)
    return buf, buf[1:rows + 1].view(dtype)


def assert_guards(bufs, case):
    torch.cuda.synchronize()
    for name, (buf, view, written) in bufs.items():
        b = buf.cpu().numpy()
        if b.ndim == 2:
            guard, body = np.concatenate([b[0], b[-1]]), b[1:-1]
        else:
            guard, body = b[-1:], b[:-1]
        assert (guard == SENTINEL).all(), f"{case}: guard of {name} overwritten"
        if written:
            assert not (body == SENTINEL).any(), f"{case}: {name} not written everywhere"


@gpu
def test_layernorm_kernels_write_their_outputs_and_nothing_else(dev):
    from protein_transformer_amd import kernels as K
    lib, ptr = K.lib(), K.ptr
    T, D, p = 37, 36, 0.1
    c, d = ln_case(T, D), ln_dev(T, D)

    def preloaded(t):
        buf = torch.full((t.numel() + 1,), SENTINEL, dtype=torch.int32, device=dev)
        buf[:t.numel()] = t.to(dev).view(torch.int32)
        return buf, buf[:t.numel()].view(t.dtype), False

    def fresh(*shape, dtype=torch.float32):
        return guarded(dev, *shape, dtype=dtype) + (True,)

    # forward
    o = dict(y=fresh(T, D), mean=fresh(T), rstd=fresh(T), rs=fresh(T, dtype=torch.int32))
    assert lib.ptamd_layernorm_fwd(ptr(d["x"]), ptr(d["gamma"]), ptr(d["beta"]), T, D, ptr(o["y"][1]), ptr(o["mean"][1]),
                                   ptr(o["rstd"][1]), ptr(o["rs"][1]), None, K.stream()) == 0
    assert_guards(o, "forward")
    check("layernorm_fwd", "y", o["y"][1], c["y32"], c["y"], c["u_y"], "canary")
    # unfused backward
    ws = torch.empty(lib.ptamd_layernorm_bwd_workspace_bytes(D), dtype=torch.uint8, device=dev)
    o = dict(dx=fresh(T, D), dg=preloaded(d["dg0"]), db=preloaded(d["db0"]))
    assert lib.ptamd_layernorm_bwd(ptr(d["dy"]), ptr(d["x"]), ptr(d["gamma"]), ptr(d["mean"]), ptr(d["rstd"]), ptr(d["dres"]), T, D,
                                   ptr(o["dx"][1]), ptr(o["dg"][1]), ptr(o["db"][1]), ptr(ws), ws.numel(), K.stream()) == 0
    assert_guards(o, "backward")
    check("layernorm_bwd", "dx", o["dx"][1], c["dx32"][True], c["dx"][True], c["u_dx"][True], "canary")
    check("layernorm_bwd", "dgamma", o["dg"][1], c["dg32"], c["dg"], c["u_dg"], "canary")
    # fused backward
    factor = torch.tensor([FACTOR], device=dev)
    preset = torch.full((4,), SCALE_PRESET, dtype=torch.int32)
    o = dict(dx=fresh(T, D), dr=fresh(T, D), dg=preloaded(d["dg0"]), db=preloaded(d["db0"]), rs=fresh(T, dtype=torch.int32),
             bs=fresh(T, dtype=torch.int32), rmin=preloaded(preset), bmin=preloaded(preset))
    assert lib.ptamd_layernorm_bwd_dropout(ptr(d["dy"]), ptr(d["x"]), ptr(d["gamma"]), ptr(d["mean"]), ptr(d["rstd"]), ptr(d["dres"]),
                                           T, D, p, SEED, STREAM, ptr(o["dx"][1]), ptr(o["dr"][1]), ptr(o["rs"][1]), ptr(factor),
                                           ptr(o["bs"][1]), ptr(o["rmin"][1]), ptr(o["bmin"][1]), None, ptr(o["dg"][1]),
                                           ptr(o["db"][1]), 1, 0, ptr(ws), ws.numel(), K.stream()) == 0
    assert_guards(o, "fused backward")
    check("layernorm_bwd_dropout", "dx", o["dx"][1], c["dx32"][True], c["dx"][True], c["u_dx"][True], "canary")
    check("layernorm_bwd_dropout", "dbeta", o["db"][1], c["db32"], c["db"], c["u_db"], "canary")
    assert np.array_equal(as_float(o["rmin"][1]), np.full(4, as_float(o["rs"][1]).min()))
    assert np.array_equal(as_float(o["bmin"][1]), np.full(4, as_float(o["bs"][1]).min()))


# ------------------------------------------------------------------------------------------------ deferred reductions
def run_sites(dev, sites, pending):
    """One LayerNorm backward per site into `pending`: even sites through the fused kernel, odd ones through the plain one."""
    from protein_transformer_amd import kernels as K
    outs = []
    for i, (c, d) in enumerate(sites):
        dg, db = d["dg0"].clone(), d["db0"].clone()
        if i % 2 == 0:
            K.layernorm_bwd_dropout(d["dy"], d["x"], d["gamma"], d["mean"], d["rstd"], dg, db, d["dres"], 0.1, SEED, STREAM, pending=pending)
        else:
            K.layernorm_bwd(d["dy"], d["x"], d["gamma"], d["mean"], d["rstd"], dg, db, dres=d["dres"], pending=pending)
        outs.append((dg, db))
    return outs


@gpu
def test_layernorm_bwd_reduce_of_sites_of_different_width(dev):
    """One reduce launch for D = 64, 260 and 1024: the grid is sized by the widest site, the blocks beyond a narrower one leave."""
    from protein_transformer_amd import kernels as K
    sites = [(ln_case(37, D), ln_dev(37, D)) for D in (64, 260, 1024)]
    pending = []
    outs = run_sites(dev, sites, pending)
    assert len(pending) == 3 and all(torch.equal(dg, d["dg0"]) and torch.equal(db, d["db0"]) for (dg, db), (_, d) in zip(outs, sites))
    K.layernorm_bwd_flush(pending)
    assert pending == []
    for (dg, db), (c, _) in zip(outs, sites):
        case = f"three sites, D={c['x'].shape[1]}"
        check("layernorm_bwd_reduce", "dgamma", dg, c["dg32"], c["dg"], c["u_dg"], case)
        check("layernorm_bwd_reduce", "dbeta", db, c["db32"], c["db"], c["u_db"], case)
    # widest first: the same kernels on the same rows, so the same bits
    pending = []
    rev = run_sites(dev, [sites[2], sites[1], sites[0]], pending)
    K.layernorm_bwd_flush(pending)
    for (dg, db), (dg_r, db_r) in zip(outs, (rev[2], rev[1], rev[0])):
        assert torch.equal(dg, dg_r) and torch.equal(db, db_r)


@gpu
def test_layernorm_bwd_reduce_of_more_sites_than_one_launch_takes(dev):
    """Eighteen pending sites: the seventeenth call flushes the first sixteen by itself, the flush finishes the rest."""
    from protein_transformer_amd import kernels as K
    T, D = 5, 36
    base = ln_case(T, D)
    sites = []
    for i in range(18):
        g = torch.Generator().manual_seed(100 + i)
        c = ln_refs(base["x"], base["dy"] * (1.0 + i), base["gamma"], base["beta"], base["dres"],
                    torch.randn(D, generator=g) + i, torch.randn(D, generator=g) - i)
        d = {k: c[k].to(dev) for k in ("x", "dy", "gamma", "beta", "dres", "dg0", "db0")}
        d["mean"], d["rstd"] = ln_dev(T, D)["mean"], ln_dev(T, D)["rstd"]
        sites.append((c, d))
    pending = []
    outs = run_sites(dev, sites, pending)
    assert len(pending) == 2
    K.layernorm_bwd_flush(pending)
    for i, ((dg, db), (c, _)) in enumerate(zip(outs, sites)):
        check("layernorm_bwd_reduce", "dgamma", dg, c["dg32"], c["dg"], c["u_dg"], f"site {i} of 18")
        check("layernorm_bwd_reduce", "dbeta", db, c["db32"], c["db"], c["u_db"], f"site {i} of 18")


# ------------------------------------------------------------------------------------------------ refusals
@gpu
@pytest.mark.parametrize("what,D,p,slabs,with_dropped", [("D above 1024", 1028, 0.1, 1, True), ("D no multiple of 4", 6, 0.1, 1, True),
                                                         ("slabs above D 512", 516, 0.1, 2, True), ("p > 0 without dropped", 64, 0.1, 1, False)])
def test_layernorm_bwd_dropout_refusals(dev, what, D, p, slabs, with_dropped):
    """Argument combinations ptamd_layernorm_bwd_dropout rejects on the host, before any launch: PTAMD_ERR_BAD_SHAPE, and
    nothing is written."""
    from protein_transformer_amd import kernels as K
    lib, ptr = K.lib(), K.ptr
    T = 5
    Dp = D + (-D) % 4
    dy = torch.zeros(slabs, T, Dp, device=dev)
    x, dres, gam = torch.zeros(T, Dp, device=dev), torch.zeros(T, Dp, device=dev), torch.ones(Dp, device=dev)
    mean, rstd = torch.zeros(T, device=dev), torch.ones(T, device=dev)
    outs = {k: torch.full(s, SENTINEL, dtype=torch.int32, device=dev)
            for k, s in dict(dx=(T, Dp), dr=(T, Dp), rs=(T,), bs=(T,), rmin=(4,), bmin=(4,), dg=(Dp,), db=(Dp,)).items()}
    ws = torch.full((lib.ptamd_layernorm_bwd_workspace_bytes(Dp) // 4,), SENTINEL, dtype=torch.int32, device=dev)
    factor = torch.tensor([FACTOR], device=dev)
    rc = lib.ptamd_layernorm_bwd_dropout(ptr(dy), ptr(x), ptr(gam), ptr(mean), ptr(rstd), ptr(dres), T, D, p, SEED, STREAM,
                                         ptr(outs["dx"]), ptr(outs["dr"]) if with_dropped else None, ptr(outs["rs"]), ptr(factor),
                                         ptr(outs["bs"]), ptr(outs["rmin"]), ptr(outs["bmin"]), None, ptr(outs["dg"]), ptr(outs["db"]),
                                         slabs, T * Dp, ptr(ws), ws.numel() * 4, K.stream())
    assert rc == BAD_SHAPE, what
    torch.cuda.synchronize()
    for k, t in outs.items():
        assert bool((t == SENTINEL).all()), (what, k)
    assert bool((ws == SENTINEL).all()), what


# ------------------------------------------------------------------------------------------------ embedding
@functools.lru_cache(maxsize=None)
def emb_case(B, L, D):
    from oracle.encoder import positional_table
    g = torch.Generator().manual_seed(31 * B * L + D)
    T = B * L
    used = torch.tensor([v for v in range(22) if v not in (3, 17)])
    seq = used[torch.randint(0, len(used), (T,), generator=g)]
    if T >= 50:                                                             # ids outside the vocabulary count as row 21
        seq[7], seq[T // 2], seq[T - 1] = -1, 22, 1000
    # |emb| sqrt(D) >= 1.5 > |pe|: x0, x0 + pe and their sums never cancel, an error relative to |out| means something
    emb = (torch.rand(22, D, generator=g) + 0.75) * torch.where(torch.rand(22, D, generator=g) < 0.5, -1.0, 1.0)
    return dict(seq=seq.view(B, L), emb=emb, pe=positional_table(L, D)[0].contiguous(), dout=torch.randn(T, D, generator=g),
                demb0=torch.randn(22, D, generator=g))


def embed_fwd_bound(c, B, p, seed, out):
    """First-order bound (in eps) of an fp32 evaluation of out = ks (x0 + ks keep1 (x0 + pe)) keep2: x0 = emb sqrt(D) carries
    two roundings (sqrt(D), the product) into both of its uses, ks three (1 - p, the division, its product), every sum its
    own.  |out| alone is not a unit an fp32 evaluation meets: fp32 PyTorch on the CPU is up to 4.7 |out| eps away."""
    D = c["emb"].shape[1]
    T = out.shape[0]
    x0 = f64(c["emb"])[R.embed_ids(c["seq"])] * np.sqrt(float(D))
    s = x0 + np.tile(f64(c["pe"]), (B, 1))
    if p == 0:
        return 4 * np.abs(x0) + np.abs(s) + np.abs(out)
    ks = R.keep_scale64(p)
    k1, k2 = R.embed_keep(T, D, p, seed, R.STREAM_EMB1), R.embed_keep(T, D, p, seed, R.STREAM_EMB2)
    inner = np.where(k1, s * ks, 0.0)
    return k2 * (2 * np.abs(x0) * ks * (1 + ks * k1) + k1 * np.abs(s) * ks * ks + 3 * np.abs(inner) * ks + np.abs(x0 + inner) * ks
                 + 3 * np.abs(out))


@gpu
@pytest.mark.parametrize("D", [4, 64, 252, 256, 260, 512])
@pytest.mark.parametrize("B,L", [(1, 1), (3, 50), (1, 4357), (7, 623)])
def test_embedding(dev, B, L, D):
    """4357 and 4361 tokens: 18 per chunk, i.e. for each of the two wavefronts one full round of 8 tokens and a clamped tail;
    D above 256: a second block of columns."""
    from protein_transformer_amd import kernels as K
    c = emb_case(B, L, D)
    T = B * L
    seq, emb, pe, dout = (c[k].to(dev) for k in ("seq", "emb", "pe", "dout"))
    ids = torch.from_numpy(R.embed_ids(c["seq"]))
    sq32 = torch.sqrt(torch.tensor(float(D)))
    x0 = c["emb"][ids] * sq32
    pe_t = c["pe"].repeat(B, 1)
    unused = np.setdiff1d(np.arange(22), ids.numpy())
    assert len(unused) >= 2
    for p in (0.0, 0.1):
        case = f"B={B} L={L} D={D} p={p}"
        seed = SEED + 5
        want = R.embed_fwd64(c["seq"], c["emb"], c["pe"], p, seed)
        out = K.embed_fwd(seq, emb, pe, p, seed)
        if p == 0:
            out32, w32 = x0 + (x0 + pe_t), torch.full((T, D), 2.0)
        else:
            k1, k2 = (torch.from_numpy(R.embed_keep(T, D, p, seed, s)) for s in (R.STREAM_EMB1, R.STREAM_EMB2))
            ks32 = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p))
            zero = torch.zeros(())
            out32 = torch.where(k2, (x0 + torch.where(k1, (x0 + pe_t) * ks32, zero)) * ks32, zero)
            w32 = torch.where(k2, ks32 * (1.0 + torch.where(k1, ks32, zero)), zero)
            assert np.array_equal(out.cpu().numpy() == 0, ~k2.numpy()), case      # exactly the restated pattern
        check("embed_fwd", "out", out, out32, want, EPS * embed_fwd_bound(c, B, p, seed, want), case, fixed=2.0)
        # backward, on top of what the table holds
        demb = c["demb0"].to(dev)
        K.embed_bwd(seq, dout, D, p, seed, demb)
        terms = R.embed_bwd_terms64(c["seq"], c["dout"], D, p, seed)
        unit = np.abs(f64(c["demb0"]))
        np.add.at(unit, ids.numpy(), np.abs(terms))
        demb32 = c["demb0"].clone().index_add_(0, ids, c["dout"] * w32 * sq32)
        check("embed_bwd", "demb", demb, demb32, R.embed_bwd64(c["seq"], c["dout"], D, p, seed, c["demb0"]), EPS * unit, case)
        assert np.array_equal(bits(demb)[unused], bits(c["demb0"])[unused]), case  # rows without a token: bit for bit


# ------------------------------------------------------------------------------------------------ column sums
@gpu
@pytest.mark.parametrize("N", [1, 255, 256, 257])
@pytest.mark.parametrize("T", [1, 3, 127, 128, 129, 517])
def test_colsum(dev, T, N):
    """T below 128: chunks without a row; 517 rows: 5 per chunk (the loop of four and its tail)."""
    from protein_transformer_amd import kernels as K
    g = torch.Generator().manual_seed(T * 1000 + N)
    x = torch.randn(T, N, generator=g) * torch.exp(torch.randn(T, 1, generator=g))
    out0 = torch.randn(N, generator=g)
    wide = torch.full((T, N + 9), 1e30)
    wide[:, 5:5 + N] = x
    wide_d = wide.to(dev)
    for name, xd in (("dense", x.to(dev)), ("slice", wide_d[:, 5:5 + N])):
        for acc in (True, False):
            out = out0.to(dev) if acc else torch.full((N,), float("nan"), device=dev)
            K.colsum(xd, out, accumulate=acc)
            before = np.abs(f64(out0)) if acc else 0.0
            check("colsum", "out", out, (out0 + x.sum(0)) if acc else x.sum(0), R.colsum64(x, out0 if acc else None),
                  EPS * (np.abs(f64(x)).sum(0) + before), f"T={T} N={N} {name} accumulate={acc}")


# ------------------------------------------------------------------------------------------------ elementwise backward
@gpu
@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_tanh_bwd(dev, n):
    from protein_transformer_amd import kernels as K
    g = torch.Generator().manual_seed(n)
    y = torch.tanh(torch.randn(n, generator=g) * 3)
    y[::7] = 1.0
    y[3::7] = -1.0
    y[5::7] = 0.0
    dy = torch.randn(n, generator=g)
    dx = K.tanh_bwd(dy.to(dev), y.to(dev))
    # two roundings behind an exact 1 - fl(y y) (or one, contracted): at most eps |dy| (2 - y^2)
    check("tanh_bwd", "dx", dx, dy * (1 - y * y), R.tanh_bwd64(dy, y), EPS * np.abs(f64(dy)) * (1 + f64(y) ** 2), f"n={n}", fixed=2.0)


@gpu
@pytest.mark.parametrize("n", [4, 1020, 1024, 1028])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_relu_dropout_bwd(dev, n, p):
    from protein_transformer_amd import kernels as K
    g = torch.Generator().manual_seed(n)
    y = torch.randn(n, generator=g)
    y[0], y[1] = 0.0, -0.0
    dy = torch.randn(n, generator=g)
    dx = K.relu_dropout_bwd(dy.to(dev), y.to(dev), p)
    ks = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
    want = np.where(y.numpy() > 0, dy.numpy() * ks, np.float32(0.0)).astype(np.float32)     # one fp32 multiplication: no tolerance
    assert np.array_equal(bits(dx), want.view(np.int32))


@gpu
@pytest.mark.parametrize("cols", [1, 255, 257])
@pytest.mark.parametrize("rows", [1, 5, 31, 33, 45])
def test_dropout_bwd(dev, rows, cols):
    from protein_transformer_amd import kernels as K
    lib, ptr = K.lib(), K.ptr
    dy = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows * 1000 + cols))
    dyd = dy.to(dev)
    for p in (0.1, 0.5):
        buf = torch.full((rows + 1, cols), SENTINEL, dtype=torch.int32, device=dev)
        assert lib.ptamd_dropout_bwd(ptr(dyd), rows, cols, p, SEED, STREAM, ptr(buf), K.stream()) == 0
        keep = dropout_mask_restated(rows, cols, p, SEED, STREAM)
        ks = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        want = np.where(keep, dy.numpy() * ks, np.float32(0.0)).astype(np.float32)
        got = buf.cpu().numpy()
        assert np.array_equal(got[:rows], want.view(np.int32)), (rows, cols, p)
        assert (got[rows] == SENTINEL).all(), (rows, cols, p)
        assert torch.equal(K.dropout_bwd(dyd, p, SEED, STREAM).view(torch.int32), buf[:rows])
