"""fp64 references of what csrc/elementwise.hip computes, in plain numpy on the CPU, written from the reference semantics
named at the top of that file (torch.nn.LayerNorm with eps 1e-5 and the biased variance, Embeddings * sqrt(D) with the
doubled positional add and its two dropouts, autograd of tanh), not from the kernels.  tests/test_gpu_elementwise.py
checks these functions against torch autograd in float64 on any machine and the kernels against them on the MI355X.

Only the dropout DECISIONS are restatements of device code (the counter hash of csrc/common.h, restated and tested in
tests/test_host_logic.py): a mask is part of the definition of the operation, the arithmetic around it is not.
"""
import numpy as np

from test_host_logic import dropout_mask_restated, rand4_restated

LN_EPS = 1e-5
STREAM_EMB1, STREAM_EMB2 = 0xE1, 0xE2
VOCAB_ROWS = 22


def f64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, dtype=np.float64)


def scale_of(amax):
    """The f16x2 row scale (csrc/common.h, pt_row_scale_bits): the power of two that takes the fp32 value amax into
    [2^14, 2^15); zeros get the largest finite power.  Same restatement as tests/test_gpu_scales.py."""
    amax = np.ascontiguousarray(amax, dtype=np.float32)
    e = (amax.view(np.uint32) >> 23).astype(np.int64)
    return np.ldexp(1.0, np.minimum(268 - e, 254) - 127)


def keep_scale64(p):
    """1 / (1 - p) of the probability the kernels are handed (p travels as a float)."""
    return 1.0 / (1.0 - float(np.float32(p)))


# ------------------------------------------------------------------------------------------------ LayerNorm
def ln_stats64(x):
    x = f64(x)
    mean = x.mean(axis=1)
    var = ((x - mean[:, None]) ** 2).mean(axis=1)             # biased
    return mean, 1.0 / np.sqrt(var + LN_EPS)


def ln_fwd64(x, gamma, beta):
    """y, mean, rstd of torch.nn.LayerNorm(D) on the rows of x [T, D]."""
    x, gamma, beta = f64(x), f64(gamma), f64(beta)
    mean, rstd = ln_stats64(x)
    y = (x - mean[:, None]) * rstd[:, None] * gamma[None, :] + beta[None, :]
    return y, mean, rstd


def ln_bwd64(dy, x, gamma, dres=None):
    """dx, dgamma, dbeta of y = xh * gamma + beta, xh = (x - mean) * rstd, with mean and rstd recomputed here in fp64.
    By hand: with g = dy * gamma and <.> the mean over the row,
        d xh = g,   dx = rstd * (g - <g> - xh <g xh>)          (the two projections: d mean and d rstd)
    plus dres, the gradient that went round the normalised sublayer through the residual add."""
    dy, x, gamma = f64(dy), f64(x), f64(gamma)
    mean, rstd = ln_stats64(x)
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma[None, :]
    m1 = g.mean(axis=1, keepdims=True)
    m2 = (g * xh).mean(axis=1, keepdims=True)
    dx = rstd[:, None] * (g - m1 - xh * m2)
    if dres is not None:
        dx = dx + f64(dres)
    return dx, (dy * xh).sum(axis=0), dy.sum(axis=0)


def dropped64(dx, p, seed, stream_id):
    """dx * mask / (1 - p) with the mask the GEMM epilogue of (seed, stream_id) drew (p == 0: dx)."""
    dx = f64(dx)
    if p <= 0:
        return dx.copy()
    keep = dropout_mask_restated(dx.shape[0], dx.shape[1], p, seed, stream_id)
    return np.where(keep, dx * keep_scale64(p), 0.0)


# ------------------------------------------------------------------------------------------------ embedding
def embed_ids(seq):
    ids = np.asarray(seq.detach().cpu().numpy() if hasattr(seq, "detach") else seq, dtype=np.int64).reshape(-1)
    return np.where((ids < 0) | (ids > 21), 21, ids)


def embed_keep(T, D, p, seed, stream):
    """Keep decisions [T, D] of one of the two embedding dropouts: word k of the generator call i = t (D / 4) + c / 4
    serves column c + k, and a value is kept iff its word >= uint32(p 2^32) - all 32 bits, unlike the 16-bit fields of
    the GEMM epilogue's mask."""
    thr = np.uint32(min(float(np.float32(p)) * 2.0 ** 32, 2.0 ** 32 - 1))
    i = np.arange(T * (D // 4), dtype=np.uint64)
    words = np.stack(rand4_restated(seed, i, stream), axis=1)              # [T D / 4, 4]
    return (words >= thr).reshape(T, D)


def embed_fwd64(seq, emb, pe, p=0.0, seed=0):
    """out [B L, D]: x0 = emb[id] sqrt(D) (ids outside 0 .. 21 are row 21), out = drop2(x0 + drop1(x0 + pe[pos]))."""
    emb, pe = f64(emb), f64(pe)
    B, L = seq.shape
    D = emb.shape[1]
    x0 = emb[embed_ids(seq)] * np.sqrt(float(D))
    pos = np.tile(np.arange(L), B)
    inner = x0 + pe[pos]
    if p <= 0:
        return x0 + inner
    ks = keep_scale64(p)
    k1, k2 = embed_keep(B * L, D, p, seed, STREAM_EMB1), embed_keep(B * L, D, p, seed, STREAM_EMB2)
    return np.where(k2, (x0 + np.where(k1, inner * ks, 0.0)) * ks, 0.0)


def embed_bwd_terms64(seq, dout, D, p=0.0, seed=0):
    """The per-token contributions [B L, D] to rows embed_ids(seq) of the table's gradient:
    d out / d x0 = ks (1 + ks keep1) keep2 (no dropout: 2), d x0 / d emb = sqrt(D)."""
    dout = f64(dout)
    T = dout.shape[0]
    if p <= 0:
        w = np.full((T, D), 2.0)
    else:
        ks = keep_scale64(p)
        k1, k2 = embed_keep(T, D, p, seed, STREAM_EMB1), embed_keep(T, D, p, seed, STREAM_EMB2)
        w = ks * (1.0 + ks * k1) * k2
    return dout * w * np.sqrt(float(D))


def embed_bwd64(seq, dout, D, p, seed, demb0):
    """demb0 [22, D] + the index_add of the terms above (rows that no token uses keep what they hold)."""
    out = f64(demb0).copy()
    np.add.at(out, embed_ids(seq), embed_bwd_terms64(seq, dout, D, p, seed))
    return out


# ------------------------------------------------------------------------------------------------ small kernels
def colsum64(x, out0=None):
    s = f64(x).sum(axis=0)
    return s if out0 is None else f64(out0) + s


def tanh_bwd64(dy, y):
    dy, y = f64(dy), f64(y)
    return dy * (1.0 - y * y)
