"""CPU tests of tests/conv_ref.py, the fp64 restatement the conv front-end kernels are held to in tests/test_gpu_conv_edges.py:
the restatement against torch.nn.functional.conv1d and autograd in float64, its parts against each other, and the case tables
of the MI355X tests against what they claim to hit."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R

SHAPES = R.CONV_SHAPES + [(2, 3, 5, 3, 11), (3, 6, 7, 2, 1), (1, 1, 1, 1, 1)]       # (B, L, C, Co, k)


def data(B, L, C, Co, k, seed=0):
    g = np.random.default_rng([seed, B, L, C, Co, k])
    return (g.standard_normal((B * L, C)), g.standard_normal((Co, C, k)), g.standard_normal(Co), g.standard_normal((B * L, Co)))


@pytest.mark.parametrize("B,L,C,Co,k", SHAPES)
def test_conv1d64_is_torch_conv1d(B, L, C, Co, k):
    x, w, b, dy = data(B, L, C, Co, k)
    tx, tw, tb = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (x, w, b))
    y = F.conv1d(tx.view(B, L, C).transpose(1, 2), tw, tb, padding=(k - 1) // 2).transpose(1, 2).reshape(B * L, Co)
    y.backward(torch.tensor(dy))
    r = R.conv1d64(x, w, b, dy, B, L)
    for name, want in (("y", y.detach()), ("dw", tw.grad), ("db", tb.grad), ("dx", tx.grad)):
        scale = r["abs_" + name] + 1.0
        assert (np.abs(r[name] - want.numpy()) <= 1e-14 * scale).all(), name
        assert (np.abs(r[name]) <= r["abs_" + name] * (1 + 1e-14)).all(), name          # |sum| <= sum | |


@pytest.mark.parametrize("B,L,C,Co,k", SHAPES)
def test_conv1d64_is_its_parts(B, L, C, Co, k):
    """The same four quantities through im2col64, pack64, col2im64 and unpack_add64, the way the library builds them."""
    x, w, b, dy = data(B, L, C, Co, k, seed=1)
    r = R.conv1d64(x, w, b, dy, B, L)
    Cp = R.pad4(C)
    col, w2 = R.im2col64(x, B, L, k), R.pack64(w)
    assert col.shape == (B * L, k * Cp) and w2.shape == (Co, k * Cp)
    assert np.abs(col @ w2.T + b - r["y"]).max() < 1e-12
    dw, adw = R.unpack_add64(dy.T @ col, np.zeros((Co, C, k)))
    assert np.abs(dw - r["dw"]).max() < 1e-12 and np.abs(adw - np.abs(r["dw"])).max() < 1e-12
    dcol = dy @ w2
    assert np.abs(dcol.reshape(B * L, k, Cp)[:, :, :C] - r["dcol"]).max() < 1e-12
    dx, adx = R.col2im64(dcol, B, L, C, k)
    assert np.abs(dx - r["dx"]).max() < 1e-12
    assert (adx <= r["abs_dx"] * (1 + 1e-12) + 1e-300).all()          # |sum over co| <= sum over co of | |, slot by slot
    assert np.abs(R.col2im64(np.abs(dy) @ np.abs(w2), B, L, C, k)[0] - r["abs_dx"]).max() < 1e-12


@pytest.mark.parametrize("B", R.BATCHES)
@pytest.mark.parametrize("k", R.KERNELS)
def test_im2col_col2im_adjoint_and_padding(B, k):
    """<col2im(d), x> == <d, im2col(x)>; padded channels and slots outside the protein are +0; NaN in the padded channels of dcol
    or the prior dW2 never reaches a result; the number of summands of col2im is what col2im_terms says."""
    for C in R.CHANNELS:
        for L in R.LENGTHS:
            g = np.random.default_rng([B, k, C, L])
            Cp, T = R.pad4(C), B * L
            x, d = g.standard_normal((T, C)), g.standard_normal((T, k, Cp))
            col = R.im2col64(x, B, L, k).reshape(B, L, k, Cp)
            assert not np.signbit(col[..., C:]).any() and (col[..., C:] == 0).all()
            for j in range(k):
                lo, hi = R.window(L, k, j)
                inside = np.zeros(L, dtype=bool)
                inside[lo:hi] = True
                assert (col[:, ~inside, j] == 0).all() and not np.signbit(col[:, ~inside, j]).any()
                if lo < hi:
                    assert np.array_equal(col[:, lo:hi, j, :C], x.reshape(B, L, C)[:, lo + j - (k - 1) // 2:hi + j - (k - 1) // 2])
            d[:, :, C:] = np.nan
            dx, ab = R.col2im64(d.reshape(T, k * Cp), B, L, C, k)
            assert np.isfinite(dx).all() and np.isfinite(ab).all()
            lhs, rhs = (dx * x).sum(), (np.nan_to_num(d).reshape(T, k * Cp) * col.reshape(T, k * Cp)).sum()
            assert abs(lhs - rhs) <= 1e-12 * (np.abs(dx * x).sum() + 1)
            ones, _ = R.col2im64(np.ones((T, k * Cp)), B, L, C, k)
            assert np.array_equal(ones, np.tile(R.col2im_terms(L, k), B)[:, None] * np.ones((1, C)))
            assert ones.max() <= min(k, L)


def test_pack_unpack_onehot():
    for Co, C, k in R.PACK_SHAPES:
        g = np.random.default_rng([Co, C, k])
        w, dw, Cp = g.standard_normal((Co, C, k)), g.standard_normal((Co, C, k)), R.pad4(C)
        w2 = R.pack64(w).reshape(Co, k, Cp)
        assert (w2[:, :, C:] == 0).all() and not np.signbit(w2[:, :, C:]).any()
        assert all(w2[co, j, c] == w[co, c, j] for co in range(Co) for j in range(k) for c in range(C))
        poisoned = w2.copy()
        poisoned[:, :, C:] = np.nan
        s, a = R.unpack_add64(poisoned.reshape(Co, k * Cp), dw)
        assert np.array_equal(s, dw + w) and np.array_equal(a, np.abs(dw) + np.abs(w))
    for C in R.ONEHOT_CLASSES:
        ids = list(range(C)) + [20] + R.out_of_range_ids(C)
        x = R.onehot64(ids, C)
        assert x.shape == (len(ids), R.pad4(C)) and (x[:, C:] == 0).all()
        valid = torch.tensor([i for i in ids if 0 <= i < C])
        assert np.array_equal(x[[0 <= i < C for i in ids], :C], F.one_hot(valid, C).numpy())
        assert (x[[not 0 <= i < C for i in ids]] == 0).all()
        assert all(not 0 <= i < C for i in R.out_of_range_ids(C))


@pytest.mark.parametrize("p", R.POSENC_PS)
def test_posenc64_is_autograd(p):
    """y = x + dropout(x + pe[l]) with the restated mask against torch autograd in float64 on the same mask."""
    B, L, D, seed = 3, 7, 8, R.POSENC_SEEDS[1]
    g = np.random.default_rng(3)
    x, pe, dy = g.standard_normal((B * L, D)), g.standard_normal((L + 3, D)), g.standard_normal((B * L, D))
    pe[L:] = np.nan
    y, keep = R.posenc_fwd64(x, pe, B, L, p, seed)
    dx, keep_b = R.posenc_bwd64(dy, p, seed)
    assert np.array_equal(keep, keep_b) and (keep.all() if p == 0 else True)
    tx = torch.tensor(x, requires_grad=True)
    mask = torch.tensor(keep / (1.0 - float(np.float32(p))))
    ty = tx + (tx + torch.tensor(pe[:L]).repeat(B, 1)) * mask
    ty.backward(torch.tensor(dy))
    assert np.abs(y - ty.detach().numpy()).max() < 1e-12 and np.abs(dx - tx.grad.numpy()).max() < 1e-12


# ------------------------------------------------------------------------------------------------ the case tables
def test_case_tables_hit_what_they_claim():
    assert {c % 4 for c in R.CHANNELS} == {0, 1, 2, 3} and 22 in R.CHANNELS and min(R.CHANNELS) == 1
    assert {C for C in R.CHANNELS if C < 4} and {C for C in R.CHANNELS if C > 4 and C % 4}      # a tail alone, a tail behind float4s
    half = (max(R.KERNELS) - 1) // 2
    assert any(L < half for L in R.LENGTHS) and half in R.LENGTHS and any(L > half for L in R.LENGTHS)
    assert 1 in R.LENGTHS and 1 in R.KERNELS and all(k % 2 for k in R.KERNELS)
    assert 1 in R.BATCHES and max(R.BATCHES) > 2                       # a protein with a neighbour on either side
    for n, (B, L, C, k) in R.IM2COL_EDGES.items():
        assert B * L * k * (R.pad4(C) // 4) == n and k % 2
    for n, (B, L, C, k) in R.COL2IM_EDGES.items():
        assert B * L * C == n and k % 2
    for n, (Co, C, k) in R.UNPACK_EDGES.items():
        assert Co * C * k == n
    for n, (Co, C, k) in R.PACK_EDGES.items():
        assert Co * k * R.pad4(C) == n
    for n, (T, C) in R.ONEHOT_EDGES.items():
        assert T * R.pad4(C) == n and C in R.ONEHOT_CLASSES
    for n, (B, L, D) in R.POSENC_EDGES.items():
        assert B * L * (D // 4) == n and D % 4 == 0
    for table in (R.IM2COL_EDGES, R.COL2IM_EDGES, R.UNPACK_EDGES, R.POSENC_EDGES):
        assert sorted(table) == [255, 256, 257]
    # counts that are multiples of 4 cannot be 255 or 257: the last full block, one float4 less and one more
    assert sorted(R.PACK_EDGES) == sorted(R.ONEHOT_EDGES) == [252, 256, 260]
    assert 22 in R.ONEHOT_CLASSES and R.pad4(22) == 24 and {22, 23} <= set(R.out_of_range_ids(22))    # ids in the padding columns
    assert R.POSENC_EDGES[255][0] == 3 and all(D % 4 == 0 for D in R.POSENC_WIDTHS)


def test_posenc_masks_tell_the_seeds_apart():
    """The two seeds differ only above bit 32 and give different masks at every width and edge shape; each mask keeps about
    1 - p of its elements; the stream is not one of the embedding's."""
    from elementwise_ref import STREAM_EMB1, STREAM_EMB2, embed_keep
    assert R.POSENC_SEEDS[0] == R.POSENC_SEEDS[1] & 0xffffffff
    for B, L, D in [(3, 7, D) for D in R.POSENC_WIDTHS] + list(R.POSENC_EDGES.values()):
        T = B * L
        for p in (0.1, 0.5):
            a, b = (R.posenc_keep(T, D, p, s) for s in R.POSENC_SEEDS)
            assert not np.array_equal(a, b)
            assert abs(a.mean() - (1 - p)) < 5 * np.sqrt(p * (1 - p) / a.size)
            for other in (STREAM_EMB1, STREAM_EMB2):
                assert not np.array_equal(a, embed_keep(T, D, p, R.POSENC_SEEDS[0], other))
    assert R.posenc_keep(255, 4, 0.999, 5).sum() < 10
