"""Head size 128: the f16x2 kernels of csrc/attention_f16x2.hip (`attn_*_f16x2_kernel<128, ...>`) and the exact-f32 ones of
csrc/attention.hip (`<128>`, which also serve bf16x3 requests) against dense fp64 attention.

The plan of head size 128 (attention_f16x2.hip `plan()`): the forward kernel at 8 wavefronts (W8) where 256-query
workgroups cover more than half of the CUs, else at 4 (W4); the backward pass always the dQ kernel + dK/dV kernel at 4
wavefronts; no K / V planes, no split-sweep slabs.  Each forward shape runs at the cheapest (B, H, L) the restated plan sends
there on this device, with ragged lengths 1, 31, 32, 33, a fully padded last tile and a full row.
"""
import functools
import os

import numpy as np
import pytest
import torch

from attn_dropout_ref import _attn_decisions_restated
from test_gpu_attention_plan import _seq, cdiv, delta_floats, device_cus, lengths, ref_lse
from test_gpu_kernels import assert_close, ref_attention, rnd

pytestmark = pytest.mark.gpu

DK = 128


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert "PTAMD_ATTN_FUSED" not in os.environ
    return torch.device("cuda:0")


def fwd_shape(B, L, H, cus):
    """attention_f16x2.hip plan() for head size 128: the forward workgroup shape."""
    return "W8" if cdiv(L, 256) * H * B * 2 > cus else "W4"


@functools.lru_cache(maxsize=None)
def pick_cases(cus):
    """forward shape -> (B, H, L): the cheapest candidate the restated plan sends there (at least 6 proteins)."""
    out = {}
    for _, L, H, B in sorted((B * H * L, L, H, B) for L in (33, 100, 129, 257, 300) for H in (1, 2, 4) for B in range(6, 400)):
        out.setdefault(fwd_shape(B, L, H, cus), (B, H, L))
    return out


def test_cases_cover_both_forward_shapes(dev):
    cases = pick_cases(device_cus())
    assert set(cases) == {"W8", "W4"}
    lens = {n for (B, H, L) in cases.values() for n in lengths(B, L)}
    assert {1, 31, 32, 33} <= lens


def _arith(name):
    from protein_transformer_amd import kernels as K
    return {"auto": K.GEMM_AUTO, "f16x2": K.GEMM_F16X2, "f32": K.GEMM_F32, "bf16x3": K.GEMM_BF16X3}[name]


@functools.lru_cache(maxsize=None)
def fp64_case(B, H, L):
    seq = _seq(B, L, seed=B + L)
    D = H * DK
    qkv = rnd((B * L, 3 * D), 20 + L, 1.5)
    dout = rnd((B * L, D), 21 + L)
    q64 = qkv.double().view(B, L, 3 * D).requires_grad_()
    key_ok = seq != 20
    out64, _ = ref_attention(q64, key_ok, H)
    out64.backward(dout.double().view(B, L, D))
    return seq, qkv, dout, out64.detach(), ref_lse(q64.detach(), key_ok, H), q64.grad.view(B * L, 3, D)


def _run(dev, B, H, L, arith, p=0.0, seed=0, sid=0, keep_bits=None, row_scales=False):
    from protein_transformer_amd import kernels as K
    seq, qkv, dout = fp64_case(B, H, L)[:3]
    seq, qkv, dout = seq.to(dev), qkv.to(dev), dout.to(dev)
    o, lse = K.attention_fwd(qkv, seq, H, p, seed, sid, arith=arith, keep_bits=keep_bits)
    rs = mn = None
    if row_scales:
        rs = torch.full((B * L,), 0x7F000000, dtype=torch.int32, device=dev)
        mn = torch.full((4,), 0x7F000000, dtype=torch.int32, device=dev)
    d = K.attention_bwd(qkv, seq, o, dout, lse, H, p, seed, sid, arith=arith, row_scale=rs, row_scale_min=mn, keep_bits=keep_bits)
    torch.cuda.synchronize()
    return o.cpu(), lse.cpu(), d.cpu(), rs, mn


@pytest.mark.parametrize("arith", ["auto", "f16x2", "f32", "bf16x3"])
@pytest.mark.parametrize("shape", ["W8", "W4"])
def test_dk128_vs_fp64(dev, shape, arith):
    """o, lse, dQ, dK, dV of each forward shape in each arithmetic against fp64: f16x2 with the bars of
    test_gpu_attention_plan.test_branch_vs_fp64, exact f32 (and bf16x3, which runs it: bit-identical) with those of
    test_gpu_kernels.test_attention_forward_backward."""
    from protein_transformer_amd import kernels as K
    B, H, L = pick_cases(device_cus())[shape]
    _, _, _, o64, lse64, d64 = fp64_case(B, H, L)
    D = H * DK
    o, lse, d, _, _ = _run(dev, B, H, L, _arith(arith))
    what = f"{shape} {arith}: {B} x {L}, {H} heads"
    assert torch.isfinite(o).all() and torch.isfinite(lse).all() and torch.isfinite(d).all(), what
    o = o.view(B, L, D)
    assert_close(o, o64, 1e-5, 2e-6, "fwd o " + what)
    assert_close(lse, lse64, 1e-6, 2e-6, "lse " + what)
    d = d.view(B * L, 3, D)
    atol = 2e-6 * max(1.0, d64.abs().max().item())
    if arith in ("auto", "f16x2"):
        for i, name in enumerate(("dQ", "dK", "dV")):
            a, r = d[:, i].double(), d64[:, i]
            assert_close(a, r, 1e-4, atol, f"{name} {what}")
            assert ((a - r).norm() / r.norm()).item() < 2e-6, f"{name} {what}"
    else:
        assert_close(d, d64, 1e-4, atol, "dqkv " + what)
        if arith == "bf16x3":
            o32, lse32, d32, _, _ = _run(dev, B, H, L, K.GEMM_F32)
            assert torch.equal(o, o32.view(B, L, D)) and torch.equal(lse, lse32), what
            assert torch.equal(d, d32.view(B * L, 3, D)), what


def test_f16x2_differs_from_f32(dev):
    """(the f16x2 kernels run at all: another rounding than the exact-f32 ones)"""
    from protein_transformer_amd import kernels as K
    B, H, L = pick_cases(device_cus())["W4"]
    assert not torch.equal(_run(dev, B, H, L, K.GEMM_AUTO)[0], _run(dev, B, H, L, K.GEMM_F32)[0])


@pytest.mark.parametrize("shape", ["W8", "W4"])
def test_dropout_decisions(dev, shape):
    """p = 0.25: the exported keep_bits are the generator's decisions; a backward pass that reads them equals one that draws
    them again, bit for bit; f16x2 and exact f32 apply the same decisions (both against fp64 with the restated mask)."""
    from protein_transformer_amd import kernels as K
    B, H, L = pick_cases(device_cus())[shape]
    p, seed, sid = 0.25, (77 << 32) | 991, 3
    n = K.lib().ptamd_attention_keep_bits_bytes(B, L, H) // 4
    buf = torch.full((n + 1024,), 0x13572468, dtype=torch.int32, device=dev)
    kb = buf[:n]
    o, lse, d_bits, _, _ = _run(dev, B, H, L, K.GEMM_AUTO, p, seed, sid, keep_bits=kb)
    words = _attn_decisions_restated(B, L, H, p, seed, sid)
    assert np.array_equal(kb.cpu().numpy().view(np.uint32).reshape(words.shape), words)
    assert bool((buf[n:] == 0x13572468).all())
    o2, _, d_gen, _, _ = _run(dev, B, H, L, K.GEMM_AUTO, p, seed, sid)
    assert torch.equal(o, o2) and torch.equal(d_bits, d_gen)
    # fp64 with the restated decisions: keep[b, h, q, key]
    seq, qkv, dout = fp64_case(B, H, L)[:3]
    lk = cdiv(L, 32) * 32
    bits = words.reshape(B * H, lk // 32, lk).astype(np.uint64)
    keep = ((bits[:, :, None, :] >> np.arange(32, dtype=np.uint64)[None, None, :, None]) & 1).reshape(B, H, lk, lk)[:, :, :L, :L]
    D = H * DK
    q64 = qkv.double().view(B, L, 3 * D).requires_grad_()
    out64, _ = ref_attention(q64, seq != 20, H, torch.tensor(keep, dtype=torch.float64), p)
    out64.backward(dout.double().view(B, L, D))
    d64 = q64.grad.view(B * L, 3 * D)
    atol = 2e-6 * max(1.0, d64.abs().max().item())
    o32, _, d32, _, _ = _run(dev, B, H, L, K.GEMM_F32, p, seed, sid)
    for name, oo, dd in (("f16x2", o, d_bits), ("f32", o32, d32)):
        assert_close(oo.view(B, L, D), out64.detach(), 1e-5, 2e-6, f"{shape} {name} o, dropout")
        assert_close(dd, d64, 1e-4, atol, f"{shape} {name} dqkv, dropout")


def test_row_scales(dev):
    """row_scale / row_scale_min from the dQ and dK/dV kernels: the f16x2 row scale of each dqkv row's maximum."""
    from test_gpu_scales import as_float, scale_of
    from protein_transformer_amd import kernels as K
    for shape in ("W8", "W4"):
        B, H, L = pick_cases(device_cus())[shape]
        _, _, d, rs, mn = _run(dev, B, H, L, K.GEMM_AUTO, 0.1, 5, 2, row_scales=True)
        want = scale_of(d.abs().amax(dim=1).numpy())
        assert np.array_equal(as_float(rs), want), shape
        assert np.array_equal(as_float(mn), np.full(4, want.min())), shape


def test_queries_match_the_dk128_plan(dev):
    """Workspace = delta only; the backward reads keep_bits in f16x2 arithmetic; no K / V planes - over a grid of shapes.
    Head sizes 96 and 256 are still refused."""
    from protein_transformer_amd import kernels as K
    lib = K.lib()
    bad = []
    for H in (1, 2, 4, 8, 16):
        for L in (1, 31, 32, 33, 100, 256, 257, 512, 1000):
            for B in (1, 2, 5, 16, 31, 32, 33, 64, 128, 257):
                ws = lib.ptamd_attention_workspace_bytes(B, L, H, DK)
                got = (ws, K.attention_bwd_reads_keep_bits(B, L, H, DK, K.GEMM_AUTO),
                       K.attention_bwd_reads_keep_bits(B, L, H, DK, K.GEMM_F32), K.attention_reads_kv_planes(B, L, H, DK, K.GEMM_AUTO))
                if got != (4 * delta_floats(B, L, H), True, False, False):
                    bad.append((B, L, H, got))
    assert not bad, bad[:8]
    assert K.attention_row_scales_available(128, K.GEMM_AUTO) and not K.attention_row_scales_available(128, K.GEMM_F32)
    B, L = 2, 40
    seq = torch.randint(0, 20, (B, L)).to(dev)
    for dk, H in ((96, 2), (256, 1)):
        qkv = rnd((B * L, 3 * H * dk), 3).to(dev)
        for arith in (K.GEMM_AUTO, K.GEMM_F32):
            with pytest.raises(Exception):
                K.attention_fwd(qkv, seq, H, 0.0, 0, 0, arith=arith)
