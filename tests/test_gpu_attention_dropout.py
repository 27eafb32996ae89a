"""Attention WITH dropout against dense fp64 attention whose mask comes from the numpy restatement of csrc/attn_dropout.h
(tests/attn_dropout_ref.py: `keep_mask`, kept probabilities times `scale(p)`) - never from a kernel:

  (a) every branch of the f16x2 plan (the shapes test_gpu_attention_plan.py derives from the device's CU count), head
      sizes 64 and 32, p = 0.1 and 0.25, with the exported keep_bits where the backward pass reads them;
  (b) odd lengths and proteins of one residue whose only key is dropped (an exactly zero output row) or kept (ks V);
  (c) the exact-f32 kernels (attention.hip: head sizes 8 and 16, 32 and 64 on request) and the three-term bf16 kernels
      (attention_split.hip) at their smallest shapes;
  (d) the three backward kinds of head size 64 forced (PTAMD_ATTN_FUSED) on one ragged shape of two 256-key blocks.

Bars: element-wise those the suite applies to dropout results (o 1e-5 / 5e-6, dQ | dK | dV 1e-4 / 5e-6 max(1, |ref|max), lse
1e-6 / 2e-6: tests/test_attn_dropout_ref.py shows that a mask wrong in any index breaks them ten-thousandfold) and, since
ks = 65536 / (65536 - thr16) differs from 1 / (1 - p) by 6.8e-6 at p = 0.1, which no element-wise bar sees, the relative L2
error per tensor at four times the largest figure measured per arithmetic (profiles/attention_dropout/NOTES.md).
"""
import functools
import os

import numpy as np
import pytest
import torch

import attn_dropout_ref as R
from test_gpu_attention_fused import fused
from test_gpu_attention_plan import BRANCHES, branches_of, case_inputs, device_cus, lengths, pick_cases, plan
from test_gpu_kernels import assert_close

pytestmark = pytest.mark.gpu

# relative L2 error against fp64, (o, the largest of dQ / dK / dV): four times the largest measured over the cases of this
# file (profiles/attention_dropout/NOTES.md: f16x2 1.37e-7 / 1.12e-6, exact f32 1.00e-7 / 8.97e-7, bf16x3 5.57e-8 / 6.79e-7).
# o's is the one that tells ks from 1 / (1 - p) (6.8e-6) and has to stay below R.KS_GAP_HALF = 3.4e-6; it does sixfold.
L2_LIMIT = {"f16x2": (5.5e-7, 4.5e-6), "f32": (4.0e-7, 3.6e-6), "bf16x3": (2.3e-7, 2.8e-6)}
GUARD, FILL = 4096, 0x13572468


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert "PTAMD_ATTN_FUSED" not in os.environ          # (the plan's own choice, except where a test forces a kind)
    assert all(o < R.KS_GAP_HALF + 1e-12 for o, _ in L2_LIMIT.values())
    return torch.device("cuda:0")


def _arith(name):
    from protein_transformer_amd import kernels as K
    return {"auto": K.GEMM_AUTO, "f32": K.GEMM_F32, "bf16x3": K.GEMM_BF16X3}[name]


@functools.lru_cache(maxsize=None)
def fp64(key, p, seed):
    """The reference of a case, built once: key = ("plan", dk, B, H, L, kv) or ("host", dk, B, H, L, lens, zero_padded_dout).
    -> (seq, qkv, qkv_in, planes, dout) on the device, keep [B, H, L, L], and fp64 o, lse, dqkv [T, 3, D]."""
    devc = torch.device("cuda:0")
    if key[0] == "plan":
        _, dk, B, H, L, kv = key
        seq, qkv, qkv_in, planes, dout = case_inputs(dk, B, H, L, kv)
    else:
        _, dk, B, H, L, lens, zero_padded = key
        seq, qkv, dout = R.host_inputs(dk, B, H, L, lens)
        if zero_padded:
            dout = dout * (seq != 20).reshape(B * L, 1)
        seq, qkv, dout = seq.to(devc), qkv.to(devc), dout.to(devc)
        qkv_in, planes = qkv, None
    keep = R.keep_mask(B, L, H, p, seed, R.SID)
    o64, lse64, d64 = R.reference(qkv.cpu(), dout.cpu(), seq.cpu() != 20, H, keep, R.scale(p))
    return (seq, qkv, qkv_in, planes, dout), keep, o64, lse64, d64


def check(what, family, o, lse, d, o64, lse64, d64):
    """o [B, L, D], lse [B, H, L], d [T, 3, D] of the device against fp64: finite, element-wise, norm-wise (printed)."""
    assert torch.isfinite(o).all() and torch.isfinite(lse).all() and torch.isfinite(d).all(), what
    l2 = [R.rel_l2(o, o64)] + [R.rel_l2(d[:, i], d64[:, i]) for i in range(3)]
    print(f"\nMEASURED {family:7s} {what}: relative L2 o {l2[0]:.2e} dQ {l2[1]:.2e} dK {l2[2]:.2e} dV {l2[3]:.2e}", end="")
    assert_close(o, o64, *R.O_BAR, "fwd o " + what)
    assert_close(lse, lse64, *R.LSE_BAR, "lse " + what)
    atol = R.D_ATOL * max(1.0, d64.abs().max().item())
    for i, name in enumerate(("dQ", "dK", "dV")):
        assert_close(d[:, i], d64[:, i], R.D_RTOL, atol, f"{name} {what}")
    lim_o, lim_d = L2_LIMIT[family]
    assert l2[0] < lim_o, f"o {what}: relative L2 {l2[0]:.3e}"
    assert max(l2[1:]) < lim_d, f"dQ / dK / dV {what}: relative L2 {l2[1:]}"


def check_single_key_rows(what, lens, H, dk, keep, ks, qkv, o, d, dkv_rows_too):
    """Proteins of one residue: every query (padded ones too) sees key 0 alone with probability 1 - dropped, its output row
    of that head is exactly +0.0 and so is its dQ row; kept, the output is ks V[key 0].  dkv_rows_too (dout zero at the padded
    queries): where the residue itself drops its key nothing reaches K and V, dK and dV of the head are exactly zero."""
    B, L = len(lens), o.shape[1]
    D = H * dk
    o, qkv, d = o.cpu(), qkv.cpu().view(B, L, 3, D), d.cpu().view(B, L, 3, D)
    n_drop = n_keep = n_own = 0
    for b in (b for b, n in enumerate(lens) if n == 1):
        for h in range(H):
            cols = slice(h * dk, (h + 1) * dk)
            kept = torch.as_tensor(keep[b, h, :, 0])
            rows = o[b, :, cols]
            assert bool((rows[~kept].contiguous().view(torch.int32) == 0).all()), f"{what}: protein {b} head {h}: o of dropped rows not +0.0"
            assert bool((d[b, :, 0, cols][~kept] == 0).all()), f"{what}: protein {b} head {h}: dQ of dropped rows not 0"
            want = (ks * qkv[b, 0, 2, cols].double()).expand(int(kept.sum()), dk)
            assert_close(rows[kept], want, *R.O_BAR, f"{what}: protein {b} head {h}: kept rows against ks V")
            n_drop, n_keep = n_drop + int((~kept).sum()), n_keep + int(kept.sum())
            if dkv_rows_too and not kept[0]:
                assert bool((d[b, 0, 1:, cols] == 0).all()), f"{what}: protein {b} head {h}: dK / dV of a dropped only key not 0"
                n_own += 1
    return n_drop, n_keep, n_own


def run(inputs, H, p, seed, arith, keep_bits=None, bwd_bits=None):
    from protein_transformer_amd import kernels as K
    seq, _, qkv_in, planes, dout = inputs
    B, L = seq.shape
    o, lse = K.attention_fwd(qkv_in, seq, H, p, seed, R.SID, arith=arith, keep_bits=keep_bits, kv=planes)
    d = K.attention_bwd(qkv_in, seq, o, dout, lse, H, p, seed, R.SID, arith=arith, keep_bits=bwd_bits, kv=planes)
    torch.cuda.synchronize()
    return o.view(B, L, -1).cpu(), lse.cpu(), d.view(B * L, 3, -1).cpu()


def lse_without_dropout(inputs, H, arith):
    from protein_transformer_amd import kernels as K
    seq, _, qkv_in, planes, _ = inputs
    return K.attention_fwd(qkv_in, seq, H, 0.0, 0, 0, arith=arith, kv=planes)[1].cpu()


@pytest.mark.parametrize("p", R.PS)
@pytest.mark.parametrize("branch", BRANCHES)
def test_branch_with_dropout_vs_fp64(dev, branch, p):
    """(a) o, lse, dQ, dK, dV of the case that runs `branch`; lse the bits of the call without dropout; where the backward
    pass reads keep_bits: the export changes no bit of o and lse, stays inside its buffer, holds the restatement's decisions
    for every protein's own queries and keys (include/ptamd.h says nothing about the words of padded ones), and the backward
    pass that reads the words gives the bits of the one that draws them."""
    from protein_transformer_amd import kernels as K
    cus = device_cus()
    dk, B, H, L, kv = pick_cases(cus)[branch]
    assert branch in branches_of(dk, plan(B, L, H, dk, cus), kv)
    what = f"{branch}: dk {dk}, {B} x {L}, {H} heads{', K/V planes' if kv else ''}, p {p}"
    inputs, keep, o64, lse64, d64 = fp64(("plan", dk, B, H, L, kv), p, R.SEED)
    o, lse, d = run(inputs, H, p, R.SEED, K.GEMM_AUTO)
    check(what, "f16x2", o, lse, d, o64, lse64, d64)
    assert torch.equal(lse, lse_without_dropout(inputs, H, K.GEMM_AUTO)), what
    lens = lengths(B, L)
    check_single_key_rows(what, lens, H, dk, keep, R.scale(p), inputs[1], o, d, False)
    if K.attention_bwd_reads_keep_bits(B, L, H, dk, K.GEMM_AUTO):
        n = K.lib().ptamd_attention_keep_bits_bytes(B, L, H) // 4
        buf = torch.full((n + GUARD,), FILL, dtype=torch.int32, device=dev)
        o2, lse2, d2 = run(inputs, H, p, R.SEED, K.GEMM_AUTO, keep_bits=buf[:n], bwd_bits=buf[:n])
        assert torch.equal(o, o2) and torch.equal(lse, lse2), what
        assert bool((buf[n:] == FILL).all()), what
        got = R.unpack_words(buf[:n].cpu().numpy().view(np.uint32), B, L, H)
        for b, m in enumerate(lens):
            bad = int((got[b, :, :m, :m] != keep[b, :, :m, :m]).sum())
            assert bad == 0, f"{what}: protein {b} (length {m}): {bad} exported decisions are not the restatement's"
        assert torch.equal(d, d2), what
    else:
        print("  (the backward pass reads no keep_bits)", end="")


@pytest.mark.parametrize("p", R.PS)
@pytest.mark.parametrize("dk", [64, 32])
def test_odd_lengths_and_single_keys(dev, dk, p):
    """(b) L = 97 with lengths 97, 95, 65, 63, 3, 1, 1, 1: the last key pair has one live key; three proteins of one residue.
    dout is zero at the padded queries here (the plan's cases have it everywhere), so that a residue that drops its only key
    leaves dK and dV of that (protein, head) exactly zero.  The seed was chosen on the CPU (test_attn_dropout_ref.py) to drop
    and to keep such a key for both p."""
    from protein_transformer_amd import kernels as K
    _, B, H, L, lens = R.ODD_CASES[dk]
    what = f"odd lengths: dk {dk}, {B} x {L}, {H} heads, p {p}"
    inputs, keep, o64, lse64, d64 = fp64(("host", dk, B, H, L, lens, True), p, R.ODD_SEED)
    o, lse, d = run(inputs, H, p, R.ODD_SEED, K.GEMM_AUTO)
    check(what, "f16x2", o, lse, d, o64, lse64, d64)
    assert torch.equal(lse, lse_without_dropout(inputs, H, K.GEMM_AUTO)), what
    n_drop, n_keep, n_own = check_single_key_rows(what, lens, H, dk, keep, R.scale(p), inputs[1], o, d, True)
    assert n_drop > 0 and n_keep > 0 and 0 < n_own < 3 * H, (n_drop, n_keep, n_own)


@pytest.mark.parametrize("p", R.PS)
@pytest.mark.parametrize("family,dk,B,H,L,lens", R.FAMILY_CASES, ids=[f"{c[0]}-dk{c[1]}" for c in R.FAMILY_CASES])
def test_other_arithmetic_families(dev, family, dk, B, H, L, lens, p):
    """(c) the exact-f32 and the three-term bf16 kernels draw the mask the header states and apply its scale."""
    what = f"{family}: dk {dk}, {B} x {L}, {H} heads, p {p}"
    inputs, keep, o64, lse64, d64 = fp64(("host", dk, B, H, L, lens, False), p, R.SEED)
    o, lse, d = run(inputs, H, p, R.SEED, _arith(family))
    check(what, family, o, lse, d, o64, lse64, d64)
    assert torch.equal(lse, lse_without_dropout(inputs, H, _arith(family))), what
    check_single_key_rows(what, lens, H, dk, keep, R.scale(p), inputs[1], o, d, False)


@pytest.mark.parametrize("p", R.PS)
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_forced_backward_kinds(dev, mode, p):
    """(d) PTAMD_ATTN_FUSED = 0 (two kernels), 1 (the unsplit sweep), 2 (the split sweep) on L = 257, lengths 257, 200, 1: two
    256-key blocks, the second with one key.  The plan picks one of the three per shape; all three against the same fp64."""
    from protein_transformer_amd import kernels as K
    dk, B, H, L, lens = R.FORCED_CASE
    what = f"PTAMD_ATTN_FUSED={mode}: dk {dk}, {B} x {L}, {H} heads, p {p}"
    inputs, keep, o64, lse64, d64 = fp64(("host", dk, B, H, L, lens, False), p, R.SEED)
    with fused(mode):
        o, lse, d = run(inputs, H, p, R.SEED, K.GEMM_AUTO)
    check(what, "f16x2", o, lse, d, o64, lse64, d64)
    check_single_key_rows(what, lens, H, dk, keep, R.scale(p), inputs[1], o, d, False)
