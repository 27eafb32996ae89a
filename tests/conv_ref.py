"""fp64 references of what csrc/conv.hip computes (include/ptamd.h, "conv-enc front end"), in plain numpy on the CPU, written
from the definition and not from the kernels: torch.nn.Conv1d(C, Co, k, padding=(k-1)/2) applied to token-major rows
x [T = B L, C] whose windows never leave a protein, its one-hot input and the doubled positional add behind it.
tests/test_conv_ref.py pins these functions against torch.nn.functional.conv1d and autograd in float64 on any machine;
tests/test_gpu_conv_edges.py holds the kernels to them on the MI355X.

Layouts (Cp = C rounded up to 4):
  col  [T, k, Cp]   col[b L + l, j, c] = x[b L + (l + j - pad), c]  where 0 <= l + j - pad < L and c < C, else 0
  W2   [Co, k, Cp]  W2[co, j, c] = W[co, c, j] where c < C, else 0                       (W [Co, C, k]: torch's Conv1d layout)
Every reduced quantity comes with the sum of the absolute values of its summands (as in tests/pae_head_ref.py): the scale its
rounding error is measured on.

Only the dropout DECISIONS of the positional add restate device code (`elementwise_ref.embed_keep`, the counter hash of
csrc/common.h tested in tests/test_host_logic.py): a mask is part of the definition of the operation.
"""
import numpy as np

from elementwise_ref import embed_keep, f64, keep_scale64

STREAM_POSADD = 0xE3


def pad4(c):
    return (c + 3) // 4 * 4


def window(L, k, j):
    """Output positions lo .. hi-1 of a protein of L residues whose window slot j looks at a residue of that protein (the source
    is l + j - pad), as a pair (lo, hi); lo >= hi: none."""
    pad = (k - 1) // 2
    return max(0, pad - j), min(L, L + pad - j)


# ------------------------------------------------------------------------------------------------ the four data movers
def im2col64(x, B, L, k):
    """x [B L, C] -> col [B L, k Cp]: a pure copy, so the result keeps the values (and, cast back, the bits) of x."""
    x = f64(x)
    C = x.shape[1]
    Cp, pad = pad4(C), (k - 1) // 2
    xb = x.reshape(B, L, C)
    col = np.zeros((B, L, k, Cp))
    for b in range(B):
        for l in range(L):
            for j in range(k):
                s = l + j - pad
                if 0 <= s < L:
                    col[b, l, j, :C] = xb[b, s]
    return col.reshape(B * L, k * Cp)


def col2im64(dcol, B, L, C, k):
    """dcol [B L, k Cp] -> (dx [B L, C], abs [B L, C]): the adjoint of im2col64, dx[b, s, c] = sum of dcol[b, l, j, c] over the
    (l, j) with l + j - pad = s; abs is the same sum over |dcol|.  Channels C .. Cp-1 of dcol are not looked at."""
    Cp, pad = pad4(C), (k - 1) // 2
    d = f64(dcol).reshape(B, L, k, Cp)
    dx, ab = np.zeros((B, L, C)), np.zeros((B, L, C))
    for b in range(B):
        for l in range(L):
            for j in range(k):
                s = l + j - pad
                if 0 <= s < L:
                    dx[b, s] += d[b, l, j, :C]
                    ab[b, s] += np.abs(d[b, l, j, :C])
    return dx.reshape(B * L, C), ab.reshape(B * L, C)


def col2im_terms(L, k):
    """Number of summands of every position of a protein of L residues under col2im: [L] ints (k in the interior)."""
    n = np.zeros(L, dtype=np.int64)
    for j in range(k):
        lo, hi = window(L, k, j)
        if lo < hi:
            n[lo + j - (k - 1) // 2:hi + j - (k - 1) // 2] += 1
    return n


def pack64(w):
    """W [Co, C, k] -> W2 [Co, k Cp]."""
    w = f64(w)
    Co, C, k = w.shape
    w2 = np.zeros((Co, k, pad4(C)))
    w2[:, :, :C] = w.transpose(0, 2, 1)
    return w2.reshape(Co, k * pad4(C))


def unpack_add64(dw2, dw):
    """dW2 [Co, k Cp], dW [Co, C, k] -> (dW + unpack(dW2), |dW| + |unpack(dW2)|); channels C .. Cp-1 of dW2 are not looked at."""
    dw = f64(dw)
    Co, C, k = dw.shape
    u = f64(dw2).reshape(Co, k, pad4(C))[:, :, :C].transpose(0, 2, 1)
    return dw + u, np.abs(dw) + np.abs(u)


def onehot64(seq, C):
    """ids [T] (any int64) -> x [T, Cp]: x[t, c] = 1 where c == seq[t] and 0 <= seq[t] < C; every other element 0, so the row of
    an id outside 0 .. C-1 and the columns C .. Cp-1 of every row are zero."""
    ids = np.asarray(seq, dtype=np.int64).reshape(-1)
    x = np.zeros((ids.size, pad4(C)))
    for t, a in enumerate(ids):
        if 0 <= a < C:
            x[t, a] = 1.0
    return x


# ------------------------------------------------------------------------------------------------ the positional add
def posenc_keep(T, D, p, seed):
    """Keep decisions [T, D] of the positional add's dropout (all True at p = 0)."""
    if p <= 0:
        return np.ones((T, D), dtype=bool)
    return embed_keep(T, D, p, seed, STREAM_POSADD)


def posenc_fwd64(x, pe, B, L, p=0.0, seed=0):
    """x [B L, D], pe [>= L, D] -> (y, keep): y = x + dropout(x + pe[l]), l = t mod L (convolutional_encoder.py:118-119 of the
    reference: `enc_output += positional_enc(enc_output)`, whose dropout covers the inner sum)."""
    x, pe = f64(x), f64(pe)
    T, D = x.shape
    assert T == B * L
    inner = x + pe[np.tile(np.arange(L), B)]
    keep = posenc_keep(T, D, p, seed)
    ks = keep_scale64(p) if p > 0 else 1.0
    return x + np.where(keep, inner * ks, 0.0), keep


def posenc_bwd64(dy, p=0.0, seed=0):
    """dy [T, D] -> (dx, keep): dx = dy (1 + keep / (1 - p))."""
    dy = f64(dy)
    keep = posenc_keep(dy.shape[0], dy.shape[1], p, seed)
    ks = keep_scale64(p) if p > 0 else 1.0
    return dy * (1.0 + np.where(keep, ks, 0.0)), keep


# ------------------------------------------------------------------------------------------------ the Conv1d
def conv1d64(x, w, bias, dy, B, L):
    """x [B L, C], W [Co, C, k], bias [Co], dy [B L, Co] -> dict of the forward and the three gradients of
    y[b, l, co] = bias[co] + sum_j sum_c W[co, c, j] x[b, l + j - pad, c] (zero outside the protein), by direct sums over
    zero-extended proteins:
      y, abs_y      [B L, Co]     abs_y includes |bias|
      dw, abs_dw    [Co, C, k]    dw[co, c, j] = sum_{b, l} dy[b, l, co] x[b, l + j - pad, c]
      db, abs_db    [Co]          db = sum_{b, l} dy
      dx, abs_dx    [B L, C]      dx[b, s, c] = sum_j sum_co dy[b, s - j + pad, co] W[co, c, j]
      dcol, abs_dcol [B L, k, C]  the inner sums over co of dx, at the OUTPUT position l they belong to (dy[b, l] W[:, c, j]):
                                  what the library's dcol = dy W2 holds before col2im, and the sum of |dy| |W| behind each."""
    x, w, bias, dy = f64(x), f64(w), f64(bias), f64(dy)
    Co, C, k = w.shape
    pad = (k - 1) // 2
    xe = np.zeros((B, L + 2 * pad, C))
    xe[:, pad:pad + L] = x.reshape(B, L, C)
    de = np.zeros((B, L + 2 * pad, Co))
    de[:, pad:pad + L] = dy.reshape(B, L, Co)
    d3 = dy.reshape(B, L, Co)
    y = np.broadcast_to(bias, (B, L, Co)).copy()
    ay = np.broadcast_to(np.abs(bias), (B, L, Co)).copy()
    dw, adw = np.zeros((Co, C, k)), np.zeros((Co, C, k))
    dx, adx = np.zeros((B, L, C)), np.zeros((B, L, C))
    dcol, adcol = np.zeros((B, L, k, C)), np.zeros((B, L, k, C))
    for j in range(k):
        xs = xe[:, j:j + L]                                                  # x[b, l + j - pad]
        y += xs @ w[:, :, j].T
        ay += np.abs(xs) @ np.abs(w[:, :, j]).T
        dw[:, :, j] = np.einsum("blo,blc->oc", d3, xs)
        adw[:, :, j] = np.einsum("blo,blc->oc", np.abs(d3), np.abs(xs))
        ds = de[:, 2 * pad - j:2 * pad - j + L]                              # dy[b, s - j + pad]
        dx += ds @ w[:, :, j]
        adx += np.abs(ds) @ np.abs(w[:, :, j])
        dcol[:, :, j] = d3 @ w[:, :, j]
        adcol[:, :, j] = np.abs(d3) @ np.abs(w[:, :, j])
    T = B * L
    return dict(y=y.reshape(T, Co), abs_y=ay.reshape(T, Co), dw=dw, abs_dw=adw, db=d3.sum(axis=(0, 1)),
                abs_db=np.abs(d3).sum(axis=(0, 1)), dx=dx.reshape(T, C), abs_dx=adx.reshape(T, C),
                dcol=dcol.reshape(T, k, C), abs_dcol=adcol.reshape(T, k, C))


# ------------------------------------------------------------------------------------------------ case tables
# Shared by tests/test_conv_ref.py (which checks on the CPU that they hit what they claim) and tests/test_gpu_conv_edges.py.
CHANNELS = (1, 2, 3, 4, 5, 7, 8, 22)              # every residue of C mod 4, below / at / above one float4, the vocabulary's 22
KERNELS = (1, 3, 11)
LENGTHS = (1, 2, 5, 6, 17)                        # 5 = (k - 1) / 2 at k = 11: below, at and above the half window
BATCHES = (1, 3)
# all seven kernels are flat grids of 256 threads with an `i >= n` guard: shapes whose count n lands on 255 / 256 / 257
IM2COL_EDGES = {255: (3, 5, 4, 17), 256: (1, 64, 16, 1), 257: (1, 257, 4, 1)}          # (B, L, C, k): n = B L k Cp / 4
COL2IM_EDGES = {255: (3, 5, 17, 3), 256: (1, 64, 4, 3), 257: (1, 257, 1, 3)}           # (B, L, C, k): n = B L C
PACK_SHAPES = [(Co, C, k) for Co in (1, 3) for C in (1, 5, 22) for k in KERNELS]
# (Co, C, k): unpack-add runs n = Co C k threads, pack n = Co k Cp - a multiple of 4, so its nearest counts are 252 / 256 / 260
UNPACK_EDGES = {255: (5, 17, 3), 256: (1, 256, 1), 257: (1, 257, 1)}
PACK_EDGES = {252: (1, 251, 1), 256: (1, 255, 1), 260: (1, 257, 1)}
ONEHOT_CLASSES = (1, 20, 22)
# (T, C): n = T Cp is a multiple of 4 as well: 252 / 256 / 260 are the counts next to the block edge
ONEHOT_EDGES = {252: (63, 1), 256: (64, 1), 260: (65, 1)}
POSENC_WIDTHS = (4, 8, 36)
# (B, L, D): n = B L D / 4.  The grid of widths runs at B = 3; 256 and 257 have no factor 3
POSENC_EDGES = {255: (3, 85, 4), 256: (2, 64, 8), 257: (1, 257, 4)}
POSENC_SEEDS = (5, 2 ** 40 + 5)
POSENC_PS = (0.0, 0.1, 0.5, 0.999)
CONV_SHAPES = [(3, 5, 22, 44, 11), (2, 1, 4, 4, 3), (2, 17, 44, 8, 7), (1, 65, 16, 12, 3)]     # (B, L, C, Co, k)


def out_of_range_ids(C):
    return [-1, C, C + 1, pad4(C), 2 ** 40, -2 ** 63]
