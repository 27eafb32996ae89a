"""CPU self-test of tests/gemm_ref.py: the fp64 reference of ptamd_gemm against torch in fp64, the guard-band helpers
against a hand-built 3 x 5 case."""
import numpy as np
import torch
import torch.nn.functional as F

import gemm_ref as R
from test_host_logic import dropout_mask_restated


def _operands(M=7, N=5, K=12, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g) + torch.arange(K) * 1e-3
    b = torch.randn(N, K, generator=g) + torch.arange(K) * 1e-3
    return a, b, torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)


def test_reference_is_linear_relu_tanh_in_fp64():
    a, b, bias, res, old = _operands()
    lin = F.linear(a.double(), b.double(), bias.double())
    c, scale, cs, _ = R.gemm_ref(a, b, bias=bias)
    assert np.array_equal(c, lin.numpy()) and cs is None
    assert np.array_equal(scale, (a.double().abs() @ b.double().abs().T + 1).numpy())
    c, *_ = R.gemm_ref(a, b, bias=bias, relu=True, residual=res, tanh=True, accum=old)
    want = torch.tanh(F.relu(lin) + res.double()) + old.double()              # ReLU, + residual, tanh, + old C: in that order
    assert np.array_equal(c, want.numpy())
    c, *_ = R.gemm_ref(a, b, residual=res, gate=True, gate_scale=1.25)
    want = torch.where(res.double() > 0, (a.double() @ b.double().T) * 1.25, torch.zeros(7, 5, dtype=torch.float64))
    assert np.array_equal(c, want.numpy())
    cs0 = torch.randn(7)
    _, _, cs, cs_scale = R.gemm_ref(a, b, colsum=cs0)
    assert np.array_equal(cs, (cs0.double() + a.double().sum(1)).numpy())
    assert np.array_equal(cs_scale, (a.double().abs().sum(1) + 1).numpy())


def test_reference_dropout_sits_between_relu_and_residual_and_counts_with_n():
    a, b, bias, res, _ = _operands(M=40, N=9, K=8, seed=1)
    p, seed, sid = 0.3, 77, 5
    keep = dropout_mask_restated(40, 9, p, seed, sid)
    assert 0 < keep.sum() < keep.size
    c, *_ = R.gemm_ref(a, b, bias=bias, relu=True, dropout=(p, seed, sid), residual=res)
    lin = F.relu(F.linear(a.double(), b.double(), bias.double())).numpy()
    ks = float(np.float32(1) / (np.float32(1) - np.float32(p)))
    assert np.array_equal(c, np.where(keep, lin * ks, 0.0) + res.double().numpy())
    assert np.array_equal(c[~keep], res.double().numpy()[~keep])              # a dropped element is the residual alone


def test_embed_and_untouched_on_a_hand_built_case():
    mat = torch.arange(15, dtype=torch.float32).view(3, 5) + 1
    buf, view = R.embed(mat, ld=8, lead=4, trail=2, fill=-7.0)
    want = [-7] * 4 + [1, 2, 3, 4, 5, -7, -7, -7, 6, 7, 8, 9, 10, -7, -7, -7, 11, 12, 13, 14, 15, -7, -7, -7] + [-7] * 2
    assert buf.tolist() == want
    assert view.shape == (3, 5) and view.stride() == (8, 1) and view.data_ptr() == buf.data_ptr() + 16
    assert torch.equal(view, mat)
    assert R.untouched(buf, 3, 5, 8, 4, -7.0) is None
    view[1, 2] = 99.0                                                          # the matrix itself is not compared
    assert R.untouched(buf, 3, 5, 8, 4, -7.0) is None
    # bit patterns, not values: a NaN sentinel equals itself, -0.0 differs from 0.0
    nb, nv = R.embed(mat, ld=5, lead=1, trail=3, fill=R.SENTINEL)
    assert nv.data_ptr() == nb.data_ptr() + 4 and torch.isnan(nb[0]) and torch.isnan(nb[-3:]).all()
    assert R.untouched(nb, 3, 5, 5, 1, R.SENTINEL) is None
    assert R.untouched(nb, 3, 5, 5, 1, float("nan")) == (0, "lead", hex(R.SENTINEL))   # another NaN is another pattern
    zb, _ = R.embed(mat, ld=6, lead=0, trail=0, fill=0.0)
    zb[5] = -0.0
    assert R.untouched(zb, 3, 5, 6, 0, 0.0) == (5, (0, "padding", 5), "0x80000000")


def test_untouched_fails_on_one_flipped_word_wherever_it_is():
    mat = torch.zeros(3, 5)
    for off, where in ((2, "lead"), (4 + 5, (0, "padding", 5)), (4 + 2 * 8 + 7, (2, "padding", 7)), (4 + 24 + 1, "trail")):
        buf, _ = R.embed(mat, ld=8, lead=4, trail=2, fill=R.SENTINEL)
        bits = buf.view(torch.int32)
        bits[off] ^= 1                                                        # one bit of one word
        got = R.untouched(buf, 3, 5, 8, 4, R.SENTINEL)
        assert got is not None and got[0] == off and got[1] == where, (off, got)
    buf, _ = R.embed(mat, ld=8, lead=4, trail=2, fill=R.SENTINEL)
    buf.view(torch.int32)[[9, 29]] = 0
    assert R.untouched(buf, 3, 5, 8, 4, R.SENTINEL)[0] == 9                   # the FIRST differing offset


def test_gate_mask_row_scales_and_splits_restated():
    y = np.zeros((33, 40), dtype=np.float32)
    y[0, 0] = y[5, 33] = y[32, 39] = 1.0
    y[1, 1] = -1.0
    m = R.gate_mask_bits(y)
    assert m.size == 2 * 2 * 16                                               # ptamd_gate_mask_bytes(33, 40) / 8
    want = np.zeros(64, dtype=np.uint64)
    want[(0 * 2 + 0) * 16 + 0] = 1                                            # (0, 0): block (0, 0), register 0, lane 0
    want[(1 * 2 + 0) * 16 + 1] = np.uint64(1) << np.uint64(32 + 1)            # (5, 33): cb 1, rb 0, r = 1, lane 32 + 1
    want[(1 * 2 + 1) * 16 + 0] = np.uint64(1) << np.uint64(7)                 # (32, 39): cb 1, rb 1, r = 0, lane 7
    assert np.array_equal(m, want)
    x = np.array([[1.0, -3.0], [0.0, 0.0], [2.0 ** 14, 1.0], [1e-30, 0.0]], dtype=np.float32)
    s = R.row_scale_bits(x).view(np.float32)
    assert s[0] == 2.0 ** 13 and s[2] == 1.0 and s[1] == np.float32(2.0 ** 127)
    top = np.abs(x).max(1)[[0, 2, 3]] * s[[0, 2, 3]].astype(np.float64)
    assert np.all((top >= 2.0 ** 14) & (top < 2.0 ** 15))
    assert [R.effective_splits(K, s) for K, s in ((36, 5), (32, 2), (100, 5), (100, 2), (68, 2), (17, 5))] == [2, 1, 4, 2, 2, 1]
