"""Plain fp64 reference of one ptamd_gemm call (the header text of include/ptamd.h) and the guard-band helpers of
tests/test_gpu_gemm_strides.py: operands and outputs embedded in larger buffers whose every other word is poison / sentinel.

Nothing here touches the GPU; tests/test_gemm_ref.py pins it against torch in fp64 and hand-built cases.
"""
import numpy as np
import torch

from test_host_logic import dropout_mask_restated

SENTINEL = 0x7FC5A5A5          # a quiet NaN with a payload: what output buffers, workspaces and their surroundings hold
NAN_POISON = float("nan")      # operand padding, first pass: any read of it that reaches the result shows as NaN
BIG_POISON = 1e30              # second pass: finite - a row-maximum pass that reads padding would shrink the row's scale


def fill_bits(fill):
    """int32 bit pattern of a fill value: an int is a bit pattern already, a float is converted to fp32."""
    if isinstance(fill, (int, np.integer)):
        return int(np.array(int(fill) & 0xFFFFFFFF, dtype=np.uint32).view(np.int32))
    return int(np.array(fill, dtype=np.float32).view(np.int32))


def embed(mat, ld, lead, trail, fill):
    """`mat` [rows, cols] (fp32, CPU) inside a 1-D fp32 buffer of lead + rows * ld + trail floats: row r starts at float
    lead + r * ld; every float outside the matrix's own [rows, cols] - lead, trail and the ld - cols padding of EVERY row -
    holds `fill` (a float, or an int bit pattern).  Returns (buffer, view of the matrix in it); the view's data pointer is
    what the kernel is given: lead % 4 == 0 keeps it 16-byte aligned, lead = 1 misaligns it by 4 bytes."""
    mat = torch.as_tensor(mat, dtype=torch.float32)
    rows, cols = mat.shape
    assert ld >= cols and lead >= 0 and trail >= 0
    buf = torch.empty(lead + rows * ld + trail, dtype=torch.float32)
    buf.view(torch.int32).fill_(fill_bits(fill))
    view = buf[lead:lead + rows * ld].view(rows, ld)[:, :cols]
    view.copy_(mat)
    return buf, view


def untouched(buf, view_rows, cols, ld, lead, fill):
    """None when every word of `buf` outside the [view_rows, cols] matrix embedded at `lead` with row stride `ld` still has
    the bit pattern of `fill`; else (flat offset, where, bits found) of the FIRST differing word, `where` = "lead", "trail"
    or (row, "padding", column)."""
    bits = torch.as_tensor(buf).detach().cpu().contiguous().view(-1).view(torch.int32).numpy()
    want = fill_bits(fill)
    inside = np.zeros(bits.size, dtype=bool)
    body = inside[lead:lead + view_rows * ld].reshape(view_rows, ld)
    body[:, :cols] = True
    bad = np.flatnonzero(~inside & (bits != want))
    if bad.size == 0:
        return None
    off = int(bad[0])
    if off < lead:
        where = "lead"
    elif off >= lead + view_rows * ld:
        where = "trail"
    else:
        where = ((off - lead) // ld, "padding", (off - lead) % ld)
    return off, where, hex(int(bits[off]) & 0xFFFFFFFF)


def gemm_ref(a, b, *, bias=None, relu=False, dropout=None, residual=None, gate=False, gate_scale=0.0, tanh=False,
             accum=None, colsum=None):
    """fp64 reference of one ptamd_gemm call on the LOGICAL operands a [M, K] and b [N, K] (whatever their storage):
        1. the product a b^T          2. + bias[N]            3. ReLU
        4. dropout = (p, seed, stream_id): keep ? v / (1 - p) : 0 with dropout_mask_restated(M, N, ...) - row, column and N,
           never a leading dimension
        5. + residual[M, N], or (gate) residual > 0 ? v * gate_scale : 0
        6. tanh                        7. + accum[M, N] (PTAMD_EPI_ACCUM: the old C)
        8. colsum[m] + sum_k a[m, k]   (k-major A: the column sums of the stored [K, M] matrix)
    Returns (C fp64 [M, N], bound scale sum_k |a||b| + 1 [M, N], colsum fp64 [M] or None, colsum scale [M] or None)."""
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    M, N = a.shape[0], b.shape[0]
    c = a @ b.T
    if bias is not None:
        c = c + np.asarray(bias, dtype=np.float64)[None, :]
    if relu:
        c = np.maximum(c, 0.0)
    if dropout is not None:
        p, seed, stream_id = dropout
        keep = dropout_mask_restated(M, N, p, seed, stream_id)
        c = np.where(keep, c * float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))), 0.0)
    if residual is not None:
        r = np.asarray(residual, dtype=np.float64)
        c = np.where(r > 0, c * float(np.float32(gate_scale)), 0.0) if gate else c + r
    else:
        assert not gate
    if tanh:
        c = torch.tanh(torch.from_numpy(np.ascontiguousarray(c))).numpy()
    if accum is not None:
        c = c + np.asarray(accum, dtype=np.float64)
    scale = np.abs(a) @ np.abs(b).T + 1.0
    cs = cs_scale = None
    if colsum is not None:
        cs = np.asarray(colsum, dtype=np.float64) + a.sum(1)
        cs_scale = np.abs(a).sum(1) + 1.0
    return c, scale, cs, cs_scale


def gate_mask_bits(y):
    """(y > 0) of an [M, N] matrix in the layout of ptamd_gate_mask_bytes (include/ptamd.h): uint64 entry
    ((cb * ceil(M / 32) + rb) * 16 + r), bit l = element (row 32 rb + (r & 3) + 8 (r >> 2) + 4 (l >> 5), column 32 cb + (l & 31));
    bits of rows / columns past the matrix are 0."""
    y = np.asarray(y)
    M, N = y.shape
    nrb, ncb = (M + 31) // 32, (N + 31) // 32
    pad = np.zeros((nrb * 32, ncb * 32), dtype=bool)
    pad[:M, :N] = y > 0
    blk = pad.reshape(nrb, 32, ncb, 32).transpose(2, 0, 1, 3)                       # [cb][rb][row][col]
    out = np.zeros((ncb, nrb, 16), dtype=np.uint64)
    for r in range(16):
        for half in (0, 1):
            row = (r & 3) + 8 * (r >> 2) + 4 * half
            shifted = blk[:, :, row, :].astype(np.uint64) << (np.arange(32, dtype=np.uint64) + np.uint64(32 * half))
            out[:, :, r] |= np.bitwise_or.reduce(shifted, axis=-1)
    return out.reshape(-1)


def row_scale_bits(x):
    """uint32 bits of the f16x2 scale of every row of x [rows, K] (csrc/gemm_split_kernel.h row_scale_bits): the power of two
    that takes the row's largest |x| into [2^14, 2^15); rows of zeros / subnormals get the largest finite power."""
    amax = np.abs(np.asarray(x, dtype=np.float32)).max(axis=1).astype(np.float32).view(np.uint32)
    return (np.minimum(268 - (amax >> 23).astype(np.int64), 254).astype(np.uint32) << np.uint32(23)).astype(np.uint32)


def effective_splits(K, split_k):
    """K slices ptamd_gemm makes of a reduction of length K asked to split `split_k` ways: whole 32-blocks, no empty slice."""
    kblocks = -(-K // 32)
    splits = max(1, min(int(split_k), kblocks))
    per = -(-kblocks // splits) * 32
    return -(-K // per)
