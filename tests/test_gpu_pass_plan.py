"""One model step per decision of the pass plan (protein_transformer_amd/models/encoder_only.py: `_PassPlan`) against the
fp64 oracle.

The plan takes every path decision of a training pass from the widths, the token count, the head size and the CU count:
the fused LayerNorm backward (`fuse`, d_model <= 1024) and with it the bound-derived f16x2 scales, ptamd_gemm_hp behind
the LayerNorms (`use_hp`, from HP_MIN_TOKENS tokens), the hp dX product of FFN layer 2 (`hp_dx`, d_ff a multiple of 32),
the row scales of dqkv from the attention kernels (`attn_row_scales`, head size 32 / 64), pre-split K / V (`kv_planes`),
bf16x3 for launch-bound AUTO steps, the side stream.  Every case reads the plan it actually got (a spy on
`_PassPlan.take_scales`), asserts the decisions it exists for - a threshold edit that moves it off its branch fails
here - and compares one forward + backward pass at dropout 0 (the AutoGuard-trusted second pass of the model) with
`oracle.encoder.encoder_forward` evaluated in fp64:
predictions max-abs 1e-5, every parameter gradient relative L2 1e-3 (the bars of tests/test_gpu_model.py).

The fp64 pass takes the ReLU decisions of FFN layer 1 from the device (its hidden activations f1 > 0), after checking that
the two disagree only on pre-activations within 1e-5 of the kink.  A pre-activation that close to 0 lands on either side
in fp32 - on the device and in plain fp32 PyTorch alike - and one such unit of one token moves the gradient of a LayerNorm
gain by 1e-3 (measured: d_model 256, 32 heads, 16 x 512, seed 0 - a pre-activation of 4.9e-9, fp32 CPU 1.05e-3 off fp64
on that gain like the device; with the decisions shared both sit at 1e-6).

The dropout-only decisions (`keep_bits`, `gate_mask`) cannot be compared with a dropout-free oracle: a dropout step with
each of them off must give the gradients of the step with both on, bit for bit.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_gpu_attention_plan import device_cus, plan as attn_plan

pytestmark = pytest.mark.gpu

PE = "encoder.positional_enc.pe"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture
def spy(monkeypatch):
    """Records the pass plans of the model steps that follow, and how often a LayerNorm forward / fused backward was handed
    unreduced K slices (kernels.PendingRows / kernels.Slabs)."""
    from protein_transformer_amd import kernels as K
    from protein_transformer_amd.models import encoder_only as enc
    seen = SimpleNamespace(plans=[], pending=0, slabs=0, relu=[])
    take, ln_fwd, ln_bwd = enc._PassPlan.take_scales, K.layernorm_fwd, K.layernorm_bwd_dropout
    linear_fwd, gemm_hp = K.linear_fwd, K.gemm_hp

    def take_spy(self, m, flat):
        seen.plans.append(self)
        return take(self, m, flat)

    def fwd_spy(x, *a, **kw):
        seen.pending += isinstance(x, K.PendingRows)
        return ln_fwd(x, *a, **kw)

    def bwd_spy(dy, *a, **kw):
        seen.slabs += isinstance(dy, K.Slabs)
        return ln_bwd(dy, *a, **kw)

    def relu_spy(fn):
        def call(*a, **kw):        # the ReLU outputs of FFN layer 1 (the only products with EPI_RELU), layer by layer
            out = fn(*a, **kw)
            if kw.get("flags", 0) & K.EPI_RELU:
                seen.relu.append(out)
            return out
        return call
    monkeypatch.setattr(enc._PassPlan, "take_scales", take_spy)
    monkeypatch.setattr(K, "linear_fwd", relu_spy(linear_fwd))
    monkeypatch.setattr(K, "gemm_hp", relu_spy(gemm_hp))
    monkeypatch.setattr(K, "layernorm_fwd", fwd_spy)
    monkeypatch.setattr(K, "layernorm_bwd_dropout", bwd_spy)
    return seen


def _step(dev, spy, nl, nh, D, dff, B, L, lens=None, gemm_mode=None, dropout=0.0, seed=0, **attrs):
    """One forward + backward pass of a model initialised like the reference (output layer off zero) on a loss linear in the
    predictions -> SimpleNamespace(plan, model, out, params, seq, w)."""
    from oracle import encoder as oenc
    from protein_transformer_amd.models.encoder_only import EncoderOnlyTransformer
    from protein_transformer_amd.protein.Sequence import VOCAB
    am = np.tanh(np.random.default_rng(seed).normal(0, 0.5, 24))
    params = oenc.init_params(nl, D, dff, L, am, seed=seed)
    params["output_projection.weight"].normal_(0, 0.8 / np.sqrt(D))
    m = EncoderOnlyTransformer(nl, nh, D, dff, L, VOCAB, am, True, dropout=dropout)
    m.load_state_dict(params)
    m.set_dropout(dropout)
    m = m.to(dev).train()
    m.gemm_mode = gemm_mode
    for k, v in attrs.items():
        setattr(m, k, v)
    g = torch.Generator().manual_seed(seed + 1)
    seq = torch.full((B, L), 20, dtype=torch.int64)
    for b, n in enumerate(lens or [L] * B):
        seq[b, :n] = torch.randint(0, 20, (n,), generator=g)
    w = torch.randn(B, L, 24, generator=g)
    n0 = len(spy.plans)
    # Until the AutoGuard's first measurement is honoured, every product of a pass with bound-derived scales runs in
    # bf16x3 and off its bounds: the first pass measures, `settle` honours it, the second pass (same weights, no optimizer
    # step in between) is the one checked - with every site and product of the plan trusted.
    for it in range(2):
        if it:
            m.auto_guard.settle()
            for k in ("_kv_plane_passes", "_attn_bits_passes", "_gate_mask_passes"):
                m.__dict__.pop(k, None)
            spy.relu.clear()
        m.zero_grad()
        out = m(seq.to(dev))
        (out * w.to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert len(spy.plans) == n0 + 2
    pl = spy.plans[-1]
    if pl.guard is not None:
        assert not pl.off.any() and not pl.wide.any(), (pl.off, pl.wide)
    assert len(spy.relu) == nl
    relu = [(f.view(B, L, dff) > 0).cpu() for f in spy.relu]
    return SimpleNamespace(plan=pl, model=m, out=out.detach().cpu(), params=params, seq=seq, w=w, relu=relu)


def _vs_oracle(r, nh, what):
    """Predictions and every parameter gradient of the step against the same step in fp64 (oracle.encoder)."""
    from oracle import encoder as oenc
    p64 = {k: v.double() for k, v in r.params.items()}
    leaf = {k: v.clone().requires_grad_() for k, v in p64.items() if k != PE}
    kinks = []

    def relu(u):            # FFN layer 1 of layer len(kinks): the device's decisions, which may differ only at the kink
        keep = r.relu[len(kinks)]
        off = keep != (u > 0)
        kinks.append((int(off.sum()), u.detach()[off].abs().max().item() if off.any() else 0.0))
        return u * keep.to(u.dtype)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(torch, "relu", relu)
        ref = oenc.encoder_forward({**leaf, PE: p64[PE]}, r.seq, nh)
    assert len(kinks) == len(r.relu) and all(m < 1e-5 for _, m in kinks), (what, kinks)
    (ref * r.w.double()).sum().backward()
    fwd = (r.out.double() - ref.detach()).abs().max().item()
    gmax = max(float(v.grad.abs().max()) for v in leaf.values())
    num = den = 0.0
    worst, bad = ("", 0.0), []
    for name, p in r.model.named_parameters():
        got, want = p.grad.detach().cpu().double(), leaf[name].grad
        num += float(((got - want) ** 2).sum())
        den += float((want ** 2).sum())
        if want.abs().max() > 1e-4 * gmax:
            e = ((got - want).norm() / want.norm()).item()
            worst = max(worst, (name, e), key=lambda t: t[1])
            if e >= 1e-3:
                bad.append((name, e))
        elif (got - want).abs().max() >= 1e-5 * gmax:
            bad.append((name, "abs", (got - want).abs().max().item() / gmax))
    print(f"{what}: predictions max-abs {fwd:.2e}, gradient rel-L2 {(num / den) ** 0.5:.2e}, worst tensor {worst[0]} {worst[1]:.2e}, "
          f"ReLU decisions at the kink (count, largest |u|) {kinks}")
    assert fwd < 1e-5, (what, fwd)
    assert not bad, (what, bad)


def _lens(B, L, *ragged):
    return [L] * (B - len(ragged)) + list(ragged)


def test_unfused_layernorm_backward_above_d1024(dev, spy):
    """d_model 1280 > 1024: the unfused LayerNorm backward, no bound-derived scales at all - every f16x2 product of the pass
    finds the row scales of its operands while it stages them - and the weight gradients on the side stream."""
    from protein_transformer_amd import kernels as K
    B, L = 8, 512
    r = _step(dev, spy, 2, 20, 1280, 2048, B, L, lens=_lens(B, L, 300, 33, 1), gemm_mode=K.GEMM_F16X2)
    pl = r.plan
    assert not pl.fuse and pl.scales is None and pl.arith == K.GEMM_F16X2
    assert not (pl.use_hp or pl.hp_dx or pl.top_scales or pl.attn_row_scales or pl.kv_planes)
    assert pl.side is not None
    _vs_oracle(r, 20, "d1280 unfused")


def test_head_size_32_two_kernel_attention_in_hp_pass(dev, spy):
    """Head size 32 at HP_MIN_TOKENS tokens: hp products, the two-kernel f16x2 attention backward leaving the row scales of
    dqkv behind, no K / V planes (head size 64 only)."""
    from protein_transformer_amd import kernels as K
    from protein_transformer_amd.models.encoder_only import HP_MIN_TOKENS
    B, L, H = 8, 512, 16
    r = _step(dev, spy, 2, H, 512, 1024, B, L, lens=_lens(B, L, 257, 33, 1))
    pl = r.plan
    assert B * L >= HP_MIN_TOKENS and pl.arith == K.GEMM_AUTO and pl.attn_arith == K.GEMM_AUTO
    assert pl.fuse and pl.use_hp and pl.hp_qkv and pl.hp_dx and pl.top_scales
    assert pl.attn_row_scales and not pl.kv_planes
    assert attn_plan(B, L, H, 32, device_cus()).bwd == "two"
    _vs_oracle(r, H, "d512 dk32")


@pytest.mark.parametrize("nh", [16, 32])
def test_head_sizes_16_and_8_exact_attention_in_hp_pass(dev, spy, nh):
    """Head size 16 / 8 inside an f16x2 pass on hp products: the exact-f32 generic attention kernels, the row scales of dqkv
    from a pass over it (`attn_row_scales` False)."""
    from protein_transformer_amd import kernels as K
    B, L, D = 16, 512, 256
    r = _step(dev, spy, 1, nh, D, 1024, B, L, lens=_lens(B, L, 100, 33, 1))
    pl = r.plan
    assert pl.arith == K.GEMM_AUTO and pl.scales is not None and pl.use_hp and pl.hp_qkv
    assert not K.attention_row_scales_available(D // nh, pl.attn_arith) and not pl.attn_row_scales and not pl.kv_planes
    _vs_oracle(r, nh, f"d256 dk{D // nh}")


def test_dff_not_a_multiple_of_32(dev, spy):
    """d_ff 1000: hp products in front of the FFN, but dX of FFN layer 2 on the staging GEMM (`hp_dx` False through
    d_ff % 32 alone), and the separate scale launches (the one-pass preparation cannot panel 1000 columns)."""
    B, L, dff = 8, 512, 1000
    r = _step(dev, spy, 2, 8, 512, dff, B, L, lens=_lens(B, L, 411, 33))
    pl = r.plan
    assert dff % 32 and r.model.hp_dx and "hp_2t" in pl.scales[0]
    assert pl.fuse and pl.use_hp and not pl.hp_dx
    # W1's hp planes have a scale array of 1024 padded rows: the padding must not land on the column scales behind it
    for i in range(2):
        w1 = r.model.flat_parameters()[0][r.model._layout[f"encoder.enc_layers.{i}.pwff.layer1.weight"][0]:][:dff * 512]
        amax = w1.view(dff, 512).abs().amax(0).cpu().numpy()
        want = np.ldexp(1.0, np.minimum(268 - (amax.view(np.uint32) >> 23).astype(np.int64), 254) - 127).astype(np.float32)
        assert np.array_equal(pl.scales[i]["cs_1"].view(torch.float32).cpu().numpy(), want), i
    _vs_oracle(r, 8, "d512 dff1000")


def test_length_not_a_multiple_of_32(dev, spy):
    """9 x 500 (ragged, lengths 1 and 33): hp QKV product, but fp32 K / V (`kv_planes` False through L & 31 alone)."""
    from protein_transformer_amd import kernels as K
    B, L = 9, 500
    r = _step(dev, spy, 2, 8, 512, 1024, B, L, lens=_lens(B, L, 250, 33, 1))
    pl = r.plan
    assert L & 31 and r.model.kv_planes and pl.hp_qkv and not pl.kv_planes
    assert not K.attention_reads_kv_planes(B, L, 8, 64, pl.attn_arith)
    _vs_oracle(r, 8, "9 x 500")


def test_kv_planes(dev, spy):
    """d_model 512, 8 heads x 512: the fewest proteins (at this CU count) with at least HP_MIN_TOKENS tokens for which the
    attention plan reads pre-split K / V - the QKV product writes them, both attention kernels read them."""
    from protein_transformer_amd.models.encoder_only import HP_MIN_TOKENS
    L, H, cus = 512, 8, device_cus()
    B = next(b for b in range(1, 1024) if b * L >= HP_MIN_TOKENS and attn_plan(b, L, H, 64, cus).kv_planes)
    r = _step(dev, spy, 2, H, 512, 1024, B, L, lens=_lens(B, L, 480, 300, 33))
    assert r.plan.kv_planes and r.model.__dict__.get("_kv_plane_passes", 0) == 2
    _vs_oracle(r, H, f"{B} x 512 on K/V planes")


def test_auto_below_the_f16x2_threshold(dev, spy):
    """AUTO on a step of fewer than AUTO_F16X2_MIN_WORK tokens x d_model: the whole step in bf16x3, no scales."""
    from protein_transformer_amd import kernels as K
    from protein_transformer_amd.models.encoder_only import AUTO_F16X2_MIN_WORK
    assert K.get_gemm_mode() == K.GEMM_AUTO
    B, L, D = 4, 256, 256
    r = _step(dev, spy, 1, 8, D, 512, B, L, lens=_lens(B, L, 33, 1))
    assert B * L * D < AUTO_F16X2_MIN_WORK
    assert r.plan.arith == K.GEMM_BF16X3 and r.plan.scales is None and not r.plan.use_hp
    _vs_oracle(r, 8, "auto below threshold")


def test_few_tokens_no_hp_and_deferred_slabs(dev, spy):
    """2560 tokens (< HP_MIN_TOKENS) in f16x2: the staging GEMM behind the LayerNorms on bound-derived scales, and at d_model
    512 the split FFN-2 / dX products hand their K slices to the LayerNorm kernels unreduced."""
    from protein_transformer_amd import kernels as K
    from protein_transformer_amd.models.encoder_only import HP_MIN_TOKENS
    B, L, D, dff = 5, 512, 512, 2048
    r = _step(dev, spy, 2, 8, D, dff, B, L, lens=_lens(B, L, 200, 33))
    pl = r.plan
    assert B * L < HP_MIN_TOKENS and pl.arith == K.GEMM_AUTO and pl.scales is not None and pl.fuse and not pl.use_hp
    assert K.pick_split_k_rows(B * L, D, dff) > 1
    assert spy.pending >= 1 and spy.slabs >= 1
    _vs_oracle(r, 8, "2560 tokens, d512")


def test_split_k_at_d768_is_reduced_before_the_layernorm(dev, spy):
    """d_model 768 with few tokens: the FFN-2 product and the dX product of FFN layer 1 are split over K into slices the
    LayerNorm kernels could sum, but those take D <= 512 only - the slices are reduced first (kernels.linear_fwd /
    linear_bwd_input: N / K <= 512)."""
    from protein_transformer_amd import kernels as K
    B, L, D, dff = 4, 512, 768, 2048
    r = _step(dev, spy, 2, 12, D, dff, B, L, lens=_lens(B, L, 129, 33))
    pl = r.plan
    assert pl.arith == K.GEMM_AUTO and pl.scales is not None and pl.fuse and not pl.use_hp
    sk = K.pick_split_k_rows(B * L, D, dff)              # ([T, dff] x [dff, D] both ways)
    assert sk > 1 and 2 <= K.effective_splits(dff, sk) <= 4          # only the width keeps the slices from the LayerNorm
    assert spy.pending == 0 and spy.slabs == 0
    _vs_oracle(r, 12, "2048 tokens, d768")


def test_dropout_decisions_read_equal_drawn(dev, spy):
    """Dropout 0.1: the attention decisions handed from the forward to the backward kernels (`keep_bits`) and the 1-bit FFN
    gate (`gate_mask`) against the same step drawing / reading them again - the same predictions and gradients, bit for
    bit."""
    B, L = 8, 512
    res = {}
    for name, attrs in (("both", {}), ("no keep bits", dict(keep_attn_bits=False)), ("no gate mask", dict(ffn_gate_mask=False))):
        r = _step(dev, spy, 2, 8, 512, 1024, B, L, lens=_lens(B, L, 300, 33), dropout=0.1, seed=4, **attrs)
        pl, m = r.plan, r.model
        assert pl.use_hp and pl.pa > 0 and pl.p > 0
        assert pl.keep_bits == (name != "no keep bits") and pl.gate_mask == (name != "no gate mask")
        assert m.__dict__.get("_attn_bits_passes", 0) == (2 if pl.keep_bits else 0)
        assert m.__dict__.get("_gate_mask_passes", 0) == (2 if pl.gate_mask else 0)
        res[name] = (r.out, m.flat_parameters()[1].detach().clone())
    for name in ("no keep bits", "no gate mask"):
        assert torch.equal(res[name][0], res["both"][0]), name
        assert torch.equal(res[name][1], res["both"][1]), name
