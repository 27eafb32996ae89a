"""Every branch of the f16x2 attention plan (csrc/attention_f16x2.hip: `plan(B, L, H, dk)`) against dense fp64 attention.

The plan picks the forward workgroup shape (W8 / W8_HALVES / W4_HALVES, the 2 x 4 `quarters` shape), the backward kind
(two kernels with their dK / dV shape, the one-sweep kernel, the sweep split per 256-key block and query range) and
whether the kernels read pre-split K / V, from (B, L, H, dk) and the CU count of the device.  Here:

  * `plan` restates it in Python; the restatement is pinned to the library over a grid of shapes through the queries the
    library exports (the split sweep's slabs in `ptamd_attention_workspace_bytes`, `ptamd_attention_reads_kv_planes`).
    Those pin split or not, nkb, qs and kv_planes (and W8 where kv_planes can be true) - NOT W8_HALVES against W4_HALVES,
    `quarters`, or the sweep against the two-kernel path for an unsplit head size 64: for those the branch named below is
    the restatement's claim, and a moved threshold there would go unnoticed here (the fp64 comparison still holds);
  * the test shapes are derived from the device's CU count: for every branch the cheapest (B, H, L) that the restated plan
    sends there (so they keep testing the same branches on another CU count or after a threshold edit);
  * every branch's forward output, log-sum-exp and dQ, dK, dV against fp64 (`ref_attention`), without dropout and without
    PTAMD_ATTN_FUSED: what the plan picks by itself.
"""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from attn_dropout_ref import ref_lse
from test_gpu_kernels import assert_close, ref_attention, rnd

pytestmark = pytest.mark.gpu

TR, FK = 32, 256          # rows of an LDS tile, keys of a block of the split sweep (attention_f16x2.hip)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert "PTAMD_ATTN_FUSED" not in os.environ          # (the plan's own choice, not a forced backward kind)
    return torch.device("cuda:0")


def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def cdiv(a, b):
    return -(-a // b)


def plan(B, L, H, dk, cus):
    """attention_f16x2.hip `plan()` in Python: forward shape, quarters, backward kind, dK / dV shape, nkb, qs, kv_planes."""
    bh = H * B
    if cdiv(L, 256) * bh * 2 > cus:
        shape = "W8"
    else:
        shape = "W8_HALVES" if cdiv(L, 128) * bh * 2 > cus else "W4_HALVES"
    quarters = dk == 64 and shape == "W4_HALVES" and L > 3 * TR
    bwd = ("sweep" if bh * 2 > cus else "split") if dk == 64 else "two"
    nkb, qs = cdiv(L, FK), 1
    if bwd == "split":
        wg, ntiles, q = bh * nkb, cdiv(L, TR), 1
        while 2 * q * wg <= cus and 2 * q <= ntiles:
            q *= 2
        per = cdiv(ntiles, q)
        qs = cdiv(ntiles, per)                   # ranges that are not empty
    kv_planes = (B > 0 and L > 0 and H > 0 and dk == 64 and L % 32 == 0 and shape == "W8" and
                 (bwd == "sweep" or (bwd == "split" and qs == 1)))
    return SimpleNamespace(shape=shape, quarters=quarters, bwd=bwd, dkv="W4" if shape == "W8_HALVES" else shape,
                           nkb=nkb, qs=qs, kv_planes=kv_planes)


def delta_floats(B, L, H):
    return (B * H * L + 3) // 4 * 4


def split_floats(B, L, H, pl):
    """Floats of the split sweep's slabs behind delta in the workspace (attention_f16x2.hip split_floats)."""
    if pl.bwd != "split":
        return 0
    T, D = B * L, H * 64
    return pl.nkb * T * D + (pl.qs * T * 2 * D if pl.qs > 1 else 0)


def branches_of(dk, pl, kv):
    """The branches a case (dk, plan, K / V given as planes) runs."""
    if kv:
        fwd = "fwd kv planes"
    else:
        fwd = "fwd quarters" if pl.quarters else "fwd " + pl.shape
    if pl.bwd == "two":
        bwd = "bwd two kernels, dK/dV " + pl.dkv
    elif pl.bwd == "sweep":
        bwd = "bwd sweep" + (", kv planes" if kv else "")
    else:
        bwd = "bwd split, qs > 1" if pl.qs > 1 else "bwd split, qs = 1" + (", kv planes" if kv else "")
    return {f"dk{dk} {fwd}", f"dk{dk} {bwd}"}


BRANCHES = ["dk64 fwd W8", "dk64 fwd W8_HALVES", "dk64 fwd W4_HALVES", "dk64 fwd quarters", "dk64 fwd kv planes",
            "dk64 bwd sweep", "dk64 bwd sweep, kv planes", "dk64 bwd split, qs = 1", "dk64 bwd split, qs = 1, kv planes",
            "dk64 bwd split, qs > 1",
            "dk32 fwd W8", "dk32 fwd W8_HALVES", "dk32 fwd W4_HALVES",
            "dk32 bwd two kernels, dK/dV W8", "dk32 bwd two kernels, dK/dV W4", "dk32 bwd two kernels, dK/dV W4_HALVES"]

# Candidate shapes: at least 6 proteins (the ragged lengths below), 2 - 8 heads; lengths with a ragged last 32-key tile,
# whole tiles (K / V planes need them), one / two 128- and 256-key blocks.  K / V planes with 8 heads (d_model 512, the
# model's QKV product).
CAND_L = (33, 64, 100, 129, 160, 257, 288, 300, 520)
CAND_H = (2, 4, 8)
CAND_B = range(6, 400)


def lengths(B, L):
    """Ragged lengths of a case: one full protein, 1, 31, 32, 33 and one whose last 32-key tile is entirely padding."""
    tail = max(1, 32 * (cdiv(L, 32) - 1) - 5)
    return [min(n, L) for n in [L, 1, 31, 32, 33, tail] + [L] * (B - 6)]


@functools.lru_cache(maxsize=None)
def pick_cases(cus):
    """branch -> (dk, B, H, L, kv): the cheapest candidate (B H L tokens x heads) the restated plan sends there."""
    cands = sorted(((B * H * L, L, H, B) for L in CAND_L for H in CAND_H for B in CAND_B))
    out = {}
    for dk in (64, 32):
        for _, L, H, B in cands:
            pl = plan(B, L, H, dk, cus)
            for kv in ((False, True) if pl.kv_planes and H == 8 else (False,)):
                for br in branches_of(dk, pl, kv):
                    out.setdefault(br, (dk, B, H, L, kv))
    return out


def test_restated_plan_matches_the_library(dev):
    """The restatement against the library's own queries over a grid of shapes (around the thresholds of this CU count too):
    the workspace beyond delta is the split sweep's slabs (pins backward == split, nkb and qs), the K / V plane query is
    `kv_planes` (pins the W8 forward shape where it matters)."""
    from protein_transformer_amd import _lib
    from protein_transformer_amd import kernels as K
    lib, cus = _lib.lib(), device_cus()
    Ls = (1, 2, 31, 32, 33, 63, 64, 96, 97, 100, 128, 129, 200, 255, 256, 257, 288, 300, 384, 511, 512, 513, 700, 1024, 1500)
    Bs = sorted(set(range(1, 41)) | {48, 64, 65, 96, 128, 129, 200, 256, 257} |
                {max(1, cus // d + e) for d in (2, 4, 8, 16, 32) for e in (-1, 0, 1)})
    bad, n = [], 0
    for dk in (8, 16, 32, 64):
        for H in (1, 2, 4, 8, 16):
            for L in Ls:
                for B in Bs:
                    pl = plan(B, L, H, dk, cus)
                    slabs = lib.ptamd_attention_workspace_bytes(B, L, H, dk) - 4 * delta_floats(B, L, H)
                    kvp = K.attention_reads_kv_planes(B, L, H, dk, K.GEMM_AUTO)
                    n += 1
                    if slabs != 4 * split_floats(B, L, H, pl) or kvp != pl.kv_planes:
                        bad.append((B, L, H, dk, slabs // 4, split_floats(B, L, H, pl), kvp, pl.kv_planes))
    assert not bad, f"{len(bad)} of {n} shapes: (B, L, H, dk, slab floats, restated, kv planes, restated) {bad[:8]}"


def test_cases_cover_every_branch(dev):
    """The shapes picked from this device's CU count run every branch of the plan, with ragged lengths 1, 31, 32, 33 and a
    fully padded trailing 32-key tile for both head sizes."""
    cus = device_cus()
    cases = pick_cases(cus)
    missing = [b for b in BRANCHES if b not in cases]
    assert not missing, f"no candidate shape reaches {missing} at {cus} CUs"
    assert set(cases) == set(BRANCHES), sorted(set(cases) - set(BRANCHES))
    for dk in (64, 32):
        mine = {c for b, c in cases.items() if b.startswith(f"dk{dk} ")}
        lens = {n for (_, B, _, L, _) in mine for n in lengths(B, L)}
        assert {1, 31, 32, 33} <= lens, dk
        assert any(n <= 32 * (cdiv(L, 32) - 1) for (_, B, _, L, _) in mine for n in lengths(B, L)), dk
    for b in BRANCHES:
        dk, B, H, L, kv = cases[b]
        assert b in branches_of(dk, plan(B, L, H, dk, cus), kv)
        print(f"{cus} CUs: {b:38s} <- dk {dk}, {B} x {L}, {H} heads{', K/V planes' if kv else ''}")


def _seq(B, L, seed):
    seq = torch.full((B, L), 20, dtype=torch.int64)
    for b, n in enumerate(lengths(B, L)):
        seq[b, :n] = torch.randint(0, 20, (n,), generator=torch.Generator().manual_seed(seed + b))
    return seq


def case_inputs(dk, B, H, L, kv):
    """-> (seq, qkv, qkv_in, planes, dout) on the device: the inputs the suite's f16x2 bars were set on (uniform +-1.5), or for
    K / V planes the QKV product of ptamd_gemm_hp (Gaussian projections of a similar size).  `qkv_in` is what the kernels are
    given (with planes: NaN in its K | V columns), `qkv` the full product the reference reads."""
    from protein_transformer_amd import kernels as K
    dev = torch.device("cuda:0")
    D, T = H * dk, B * L
    seq = _seq(B, L, seed=B + L).to(dev)
    planes = None
    if kv:
        g = torch.Generator().manual_seed(L)
        x = torch.randn(T, D, generator=g).to(dev)
        w = (torch.randn(3 * D, D, generator=g) / np.sqrt(D) * 0.8).to(dev)
        bias = (torch.randn(3 * D, generator=g) * 0.2).to(dev)
        a, bop = K.hp_split(x), K.hp_split(w)
        qkv = K.gemm_hp(a, bop, torch.empty(T, 3 * D, device=dev), bias=bias)
        planes = K.attention_kv_buffers(T, H, dev)
        qkv_in = K.gemm_hp(a, bop, torch.full((T, 3 * D), float("nan"), device=dev), bias=bias, kv=planes, kv_col0=D, kv_heads=H)
    else:
        qkv = rnd((T, 3 * D), 20 + L, 1.5).to(dev)
        qkv_in = qkv
    dout = rnd((T, D), 21 + L).to(dev)
    return seq, qkv, qkv_in, planes, dout


@functools.lru_cache(maxsize=None)
def run_case(dk, B, H, L, kv):
    """-> (o, lse, dqkv) of the device and their fp64 references, on `case_inputs`."""
    from protein_transformer_amd import kernels as K
    D, T = H * dk, B * L
    seq, qkv, qkv_in, planes, dout = case_inputs(dk, B, H, L, kv)
    o, lse = K.attention_fwd(qkv_in, seq, H, 0.0, 0, 0, arith=K.GEMM_AUTO, kv=planes)
    dqkv = K.attention_bwd(qkv_in, seq, o, dout, lse, H, 0.0, 0, 0, arith=K.GEMM_AUTO, kv=planes)
    torch.cuda.synchronize()
    q64 = qkv.double().cpu().view(B, L, 3 * D).requires_grad_()
    key_ok = seq.cpu() != 20
    out64, _ = ref_attention(q64, key_ok, H)
    out64.backward(dout.double().cpu().view(B, L, D))
    return (o.view(B, L, D).cpu(), lse.cpu(), dqkv.view(T, 3, D).cpu(),
            out64.detach(), ref_lse(q64.detach(), key_ok, H), q64.grad.view(T, 3, D))


@pytest.mark.parametrize("branch", BRANCHES)
def test_branch_vs_fp64(dev, branch):
    """Forward output, log-sum-exp, dQ, dK and dV of the case that runs `branch` against fp64 - the bars of the suite's f16x2
    attention tests (tests/test_gpu_kernels.py, tests/test_gpu_attention_fused.py)."""
    cus = device_cus()
    dk, B, H, L, kv = pick_cases(cus)[branch]
    assert branch in branches_of(dk, plan(B, L, H, dk, cus), kv)
    o, lse, d, o64, lse64, d64 = run_case(dk, B, H, L, kv)
    what = f"{branch}: dk {dk}, {B} x {L}, {H} heads{', K/V planes' if kv else ''}"
    assert torch.isfinite(o).all() and torch.isfinite(lse).all() and torch.isfinite(d).all(), what
    assert_close(o, o64, 1e-5, 2e-6, "fwd o " + what)
    assert_close(lse, lse64, 1e-6, 2e-6, "lse " + what)
    atol = 2e-6 * max(1.0, d64.abs().max().item())
    for i, name in enumerate(("dQ", "dK", "dV")):
        a, r = d[:, i].double(), d64[:, i]
        assert_close(a, r, 1e-4, atol, f"{name} {what}")
        assert ((a - r).norm() / r.norm()).item() < 2e-6, f"{name} {what}"
