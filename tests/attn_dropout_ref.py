"""Attention dropout restated in plain numpy / torch fp64, independent of every kernel: the generator of
csrc/attn_dropout.h (which key pair word, which half of it, which threshold, which scale) and dense fp64 attention that
applies such a mask.  tests/test_attn_dropout_ref.py checks this module on the CPU; the GPU tests
(test_gpu_attention_dropout.py, test_gpu_attention_fused.py, test_gpu_attention_dk128.py) hold the kernels against it.

Two formulations of the generator stand side by side on purpose: `_attn_decisions_restated` (64-bit integers masked to 32
bits, packed in the layout of `keep_bits`) and `decisions` (native 32-bit wrap-around, one bool per (query, key)); `word`
is the scalar transcription both are checked against.
"""
import numpy as np
import torch

C_Q, C_K, C_BH_LO, C_SID = 0x9E3779B1, 0x85EBCA77, 0xC2B2AE35, 0x27D4EB2F      # attn_dropout.h
M32 = 0xFFFFFFFF


def thr16(p):
    """make_attn_drop: the 16-bit threshold of drop probability p (a C float): a half of a word below it is dropped."""
    t = np.float32(p) * np.float32(65536.0) + np.float32(0.5)
    return 65535 if t >= np.float32(65535.0) else int(t)


def scale(p):
    """make_attn_drop: what the kept probabilities are multiplied by, 65536 / (65536 - thr16) - NOT 1 / (1 - p)."""
    return 65536.0 / (65536.0 - thr16(p))


def mix32_scalar(x):
    """pt_mix32 of csrc/common.h on a Python int."""
    x = (~x + (x << 15)) & M32
    x ^= x >> 12
    x = (x + (x << 2)) & M32
    x ^= x >> 4
    x = (x + (x << 3) + (x << 11)) & M32
    return x ^ (x >> 16)


def word(seed, sid, bh, q, key):
    """The 32-bit word of (query q, key pair key >> 1) of (protein, head) pair bh = b H + h: Python ints, line by line."""
    lo = (seed & M32) ^ ((bh * C_BH_LO) & M32)
    hi = ((seed >> 32) & M32) ^ ((sid * C_SID) & M32) ^ bh
    return mix32_scalar(((q * C_Q + lo) & M32) ^ (((key >> 1) * C_K + hi) & M32))


def keeps(seed, sid, bh, q, key, p):
    """One decision: the even key of a pair by the low 16 bits of the word, the odd key by the high 16 bits."""
    return ((word(seed, sid, bh, q, key) >> (16 * (key & 1))) & 0xFFFF) >= thr16(p)


def _mix32(x):
    """pt_mix32 on a uint32 array (numpy integer arrays wrap around silently)."""
    x = ~x + (x << np.uint32(15))
    x = x ^ (x >> np.uint32(12))
    x = x + (x << np.uint32(2))
    x = x ^ (x >> np.uint32(4))
    x = x + (x << np.uint32(3)) + (x << np.uint32(11))
    return x ^ (x >> np.uint32(16))


def decisions(bh, q, key, p, seed, sid, other_half=False):
    """keep[i, j, k] for the pairs bh[i], queries q[j] and keys key[k] (integer arrays; any values that fit 32 bits - the
    wrong-mask variants of the discriminating-power test pass shifted ones).  other_half: decide every key by the half of
    the word that belongs to its neighbour."""
    bh, q, key = (np.asarray(a, dtype=np.int64).astype(np.uint32) for a in (bh, q, key))
    lo = np.uint32(seed & M32) ^ (bh * np.uint32(C_BH_LO))
    hi = np.uint32((seed >> 32) & M32) ^ np.uint32((sid * C_SID) & M32) ^ bh
    qp = q[None, :] * np.uint32(C_Q) + lo[:, None]                                   # [pair, query]
    kp = (key >> np.uint32(1))[None, :] * np.uint32(C_K) + hi[:, None]               # [pair, key]
    w = _mix32(qp[:, :, None] ^ kp[:, None, :])
    odd = (key & np.uint32(1)) ^ np.uint32(1 if other_half else 0)
    return ((w >> (np.uint32(16) * odd)[None, None, :]) & np.uint32(0xFFFF)) >= np.uint32(thr16(p))


def keep_mask(B, L, H, p, seed, sid):
    """bool [B, H, L, L]: query q of head h of protein b keeps key k (padded queries and keys included: the generator knows
    no lengths)."""
    return decisions(np.arange(B * H), np.arange(L), np.arange(L), p, seed, sid).reshape(B, H, L, L)


def _attn_decisions_restated(B, L, H, p, seed, sid):
    """numpy restatement of csrc/attn_dropout.h (pt_mix32 of common.h on (query, key pair) words, 16-bit halves against a
    16-bit threshold) in the layout of ptamd_attention_fwd's keep_bits: word [(b, h)][q / 32][key], bit q % 32."""
    M = np.uint64(0xFFFFFFFF)
    u = lambda x: (x & M).astype(np.uint64)                          # noqa: E731
    sh = lambda n: np.uint64(n)                                      # noqa: E731

    def mix32(x):
        x = u(x)
        x = u((~x & M) + (x << sh(15)))
        x = x ^ (x >> sh(12))
        x = u(x + (x << sh(2)))
        x = x ^ (x >> sh(4))
        x = u(x + (x << sh(3)) + (x << sh(11)))
        return u(x ^ (x >> sh(16)))
    nt = (L + 31) // 32
    lk = nt * 32
    out = np.zeros((B * H, nt, lk), dtype=np.uint32)
    thr = thr16(p)
    idx = np.arange(lk, dtype=np.uint64)
    for bh in range(B * H):
        lo = np.uint64((seed & 0xFFFFFFFF) ^ ((bh * 0xC2B2AE35) & 0xFFFFFFFF))
        hi = np.uint64(((seed >> 32) & 0xFFFFFFFF) ^ ((sid * 0x27D4EB2F) & 0xFFFFFFFF) ^ bh)
        qp = u(idx * np.uint64(0x9E3779B1) + lo)
        kp = u((idx >> sh(1)) * np.uint64(0x85EBCA77) + hi)
        w = mix32(qp[:, None] ^ kp[None, :])                                                    # [q, key]
        keep = ((w >> (sh(16) * (idx & sh(1)))[None, :]) & np.uint64(0xFFFF)) >= thr
        for t in range(nt):
            out[bh, t] = (keep[32 * t:32 * t + 32].astype(np.uint64) << np.arange(32, dtype=np.uint64)[:, None]).sum(0).astype(np.uint32)
    return out


def unpack_words(words, B, L, H):
    """keep_bits words [(b, h)][q / 32][key] -> bool [B, H, L, L]."""
    nt = (L + 31) // 32
    w = np.asarray(words).astype(np.uint32).reshape(B * H, nt, 1, nt * 32)
    bits = (w >> np.arange(32, dtype=np.uint32)[None, None, :, None]) & np.uint32(1)
    return bits.reshape(B, H, nt * 32, nt * 32)[:, :, :L, :L].astype(bool)


def attention_ref(qkv64, key_ok, H, keep, ks):
    """Dense attention in fp64 (the reference's formulation, Attention.py:14-22, 55-68): qkv64 [B, L, 3 D] double (Q | K | V
    column blocks, head h at columns h dk ..), key_ok [B, L] bool, keep [B, H, L, L] (bool array / tensor, or None: no
    dropout), the kept probabilities times `ks` - pass scale(p), not 1 / (1 - p).  -> out [B, L, D]; differentiable."""
    B, L, D3 = qkv64.shape
    D = D3 // 3
    dk = D // H
    q, k, v = (t.reshape(B, L, H, dk).transpose(1, 2) for t in qkv64.split(D, dim=-1))
    s = (q @ k.transpose(-2, -1) / np.sqrt(dk)).masked_fill(~key_ok[:, None, None, :], -np.inf)
    pr = torch.softmax(s, dim=-1)
    if keep is not None:
        pr = pr * torch.as_tensor(np.asarray(keep), dtype=torch.float64) * ks
    return (pr @ v).transpose(1, 2).reshape(B, L, D)


def ref_lse(qkv64, key_ok, H):
    """The kernels' log-sum-exp convention: lse[b, h, q] = ln sum over the protein's keys of exp(q . k / sqrt(dk)) (natural
    log, scores already scaled; padded queries too), [B, H, L].  Dropout does not touch it."""
    B, L, D3 = qkv64.shape
    D = D3 // 3
    dk = D // H
    q, k = (t.reshape(B, L, H, dk).transpose(1, 2) for t in qkv64.split(D, dim=-1)[:2])
    s = (q @ k.transpose(-2, -1) / np.sqrt(dk)).masked_fill(~key_ok[:, None, None, :], -np.inf)
    return torch.logsumexp(s, dim=-1)


def reference(qkv, dout, key_ok, H, keep, ks):
    """fp32 inputs qkv [B L, 3 D], dout [B L, D] (torch, CPU) -> fp64 (o [B, L, D], lse [B, H, L], dqkv [B L, 3, D])."""
    B, L = key_ok.shape
    D = dout.shape[-1]
    q64 = qkv.double().view(B, L, 3 * D).requires_grad_()
    out = attention_ref(q64, key_ok, H, keep, ks)
    out.backward(dout.double().view(B, L, D))
    return out.detach(), ref_lse(q64.detach(), key_ok, H), q64.grad.view(B * L, 3, D)


# ---- the bars of test_gpu_attention_dropout.py, here so that the CPU test of their discriminating power uses the same
O_BAR = (1e-5, 5e-6)              # o: rtol, atol
LSE_BAR = (1e-6, 2e-6)
D_RTOL, D_ATOL = 1e-4, 5e-6       # dQ | dK | dV: atol = D_ATOL max(1, |reference dqkv|max)
KS_GAP_HALF = 3.4e-6              # half of scale(0.1) / (1 / 0.9) - 1 = 6.8e-6: no norm-wise limit on o may reach it


def excess(got, ref, rtol, atol):
    """max over the elements of |got - ref| / (atol + rtol |ref|): above 1, assert_close(got, ref, rtol, atol) fails."""
    got, ref = got.double(), ref.double()
    return ((got - ref).abs() / (atol + rtol * ref.abs())).max().item()


def rel_l2(got, ref):
    return ((got.double() - ref.double()).norm() / ref.double().norm()).item()


# ---- the cases of test_gpu_attention_dropout.py that do not depend on the device (the plan's branches are picked from its CU
# count by test_gpu_attention_plan.pick_cases); test_attn_dropout_ref.py checks the seeds and the bars on them without a GPU
SEED, SID = (77 << 32) | 991, 3
PS = (0.1, 0.25)
# lengths the plan test lacks: odd L, odd lengths (the last key pair has one live key), three proteins of one residue
ODD_LENS = (97, 95, 65, 63, 3, 1, 1, 1)
ODD_CASES = {64: (64, 8, 4, 97, ODD_LENS), 32: (32, 8, 4, 97, ODD_LENS)}                 # dk -> (dk, B, H, L, lens)
ODD_SEED = (77 << 32) | 992       # chosen on the CPU (test_single_key_proteins): SEED drops no single key at p = 0.1
# the exact-f32 kernels (head sizes 8 and 16 always; 32 and 64 on request) and the three-term bf16 kernels, smallest shapes
FAMILY_CASES = [("f32", 8, 3, 4, 100, (100, 37, 1)), ("f32", 16, 2, 2, 65, (65, 5)),
                ("f32", 32, 3, 2, 130, (130, 33, 1)), ("f32", 64, 3, 2, 130, (130, 33, 1)),
                ("bf16x3", 32, 3, 2, 130, (130, 33, 1)), ("bf16x3", 64, 3, 2, 130, (130, 33, 1))]
FORCED_CASE = (64, 3, 2, 257, (257, 200, 1))              # two 256-key blocks, ragged: every backward kind forced on it


def seq_of(lens, L, seed):
    seq = torch.full((len(lens), L), 20, dtype=torch.int64)
    for b, n in enumerate(lens):
        seq[b, :n] = torch.randint(0, 20, (n,), generator=torch.Generator().manual_seed(seed + b))
    return seq


def host_inputs(dk, B, H, L, lens):
    """(seq [B, L], qkv [B L, 3 D], dout [B L, D]) on the CPU: uniform +-1.5 / +-1 as in the plan test."""
    from test_gpu_kernels import rnd
    assert len(lens) == B and max(lens) <= L
    return seq_of(lens, L, B + L), rnd((B * L, 3 * H * dk), 20 + L, 1.5), rnd((B * L, H * dk), 21 + L)
