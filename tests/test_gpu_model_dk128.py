"""Models with 128-wide attention heads on the device: one dropout-free pass against the fp64 oracle (the method and bars of
tests/test_gpu_pass_plan.py), short training runs with dropout, and the `train.py` CLI at `-dm 256 -nh 2`."""
import sys
import types

import numpy as np
import pytest
import torch

from test_gpu_pass_plan import _lens, _step, _vs_oracle, spy  # noqa: F401  (spy: the fixture)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _assert_dk128_plan(pl, K, hp):
    assert pl.attn_arith == K.GEMM_AUTO and pl.use_hp == hp and not pl.kv_planes
    # (row scales of dqkv are wanted where the pass has f16x2 scales; then the dk 128 kernels deliver them)
    assert pl.attn_row_scales == (pl.scales is not None)
    if hp:
        assert pl.attn_row_scales


def test_enc_only_d512_4_heads_hp_pass(dev, spy):
    """d_model 512, 4 heads at HP_MIN_TOKENS tokens: hp products, the f16x2 dk 128 kernels leaving the row scales of dqkv
    behind, no K / V planes."""
    from protein_transformer_amd import kernels as K
    from protein_transformer_amd.models.encoder_only import HP_MIN_TOKENS
    B, L, H = 8, 512, 4
    r = _step(dev, spy, 2, H, 512, 1024, B, L, lens=_lens(B, L, 257, 33, 1))
    assert B * L >= HP_MIN_TOKENS
    _assert_dk128_plan(r.plan, K, True)
    assert r.plan.fuse
    _vs_oracle(r, H, "d512 dk128")


def test_enc_only_d256_2_heads(dev, spy):
    from protein_transformer_amd import kernels as K
    B, L, H = 6, 200, 2
    r = _step(dev, spy, 2, H, 256, 512, B, L, lens=_lens(B, L, 100, 33, 1))
    _assert_dk128_plan(r.plan, K, False)
    _vs_oracle(r, H, "d256 dk128")


def test_conv_enc_d256_2_heads(dev, spy, monkeypatch):
    """conv-enc shares the encoder of enc-only: the same pass with two convolutions in front (the oracle's conv stack)."""
    from protein_transformer_amd import kernels as K
    from protein_transformer_amd.models import encoder_only as enc
    from protein_transformer_amd.models.convolutional_encoder import ConvEncoderOnlyTransformer
    B, L, H, D = 6, 160, 2, 256
    convs = {}

    def conv_model(nl, nh, dm, dff, msl, vocab, am, tanh, dropout=0.1):
        m = ConvEncoderOnlyTransformer(nl, nh, dm, dff, msl, vocab, am, tanh, [3, 5], [1, 1], True, True, dropout=dropout)
        g = torch.Generator().manual_seed(7)
        for k, v in m.state_dict().items():
            if "conv_layers" in k:
                fan = v[0].numel() if v.dim() > 1 else 10.0
                convs[k] = torch.randn(v.shape, generator=g) / np.sqrt(fan)
        return m
    load = enc._TransformerBase.load_state_dict

    def load_with_convs(self, sd, *a, **kw):
        sd.update(convs)                     # (the same dict the oracle pass reads: r.params)
        return load(self, sd, *a, **kw)
    monkeypatch.setattr(enc, "EncoderOnlyTransformer", conv_model)
    monkeypatch.setattr(enc._TransformerBase, "load_state_dict", load_with_convs)
    r = _step(dev, spy, 1, H, D, 512, B, L, lens=_lens(B, L, 90, 33, 1))
    assert isinstance(r.model, ConvEncoderOnlyTransformer) and any("conv_layers" in k for k in r.params)
    _assert_dk128_plan(r.plan, K, False)
    _vs_oracle(r, H, "conv-enc d256 dk128")


@pytest.mark.parametrize("opt", ["sgd", "adam"])
@pytest.mark.parametrize("model", ["enc-only", "conv-enc"])
def test_ten_steps_with_dropout(dev, model, opt):
    """Ten training steps at dropout 0.1 with an evaluation pass in the middle: finite, and the loss falls."""
    from oracle import geometry, encoder as oenc
    from protein_transformer_amd import synthetic
    from protein_transformer_amd.models.convolutional_encoder import ConvEncoderOnlyTransformer
    from protein_transformer_amd.models.encoder_only import EncoderOnlyTransformer
    from protein_transformer_amd.optim import FusedAdam, FusedSGD
    from protein_transformer_amd.protein.Sequence import VOCAB
    from protein_transformer_amd.train import train_step
    lens = [64, 50, 33, 64]
    build_cpu = lambda ang, seq: torch.stack([                                  # noqa: E731
        torch.cat([geometry.generate_coords(ang[b, :n], seq[b, :n]), torch.zeros((seq.shape[1] - n) * 14, 3)])
        for b, n in enumerate(lens)])
    batch = synthetic.make_batch(lens, L_pad=64, seed=3, build_coords=build_cpu, frac_missing=0.05)
    am = synthetic.angle_means(batch["true_ang"])
    if model == "enc-only":
        m = EncoderOnlyTransformer(2, 4, 512, 1024, 64, VOCAB, am, True, dropout=0.1)
        m.load_state_dict(oenc.init_params(2, 512, 1024, 64, am, seed=2))
    else:
        m = ConvEncoderOnlyTransformer(2, 2, 256, 512, 64, VOCAB, am, True, [3], [1], True, True, dropout=0.1)
    m = m.to(dev).train()
    opt_ = FusedSGD(m, lr=1e-2, weight_decay=10e-3) if opt == "sgd" else FusedAdam(m, betas=(0.9, 0.98), eps=1e-9, lr=1e-3)
    args = types.SimpleNamespace(loss="drmsd", combined_drmsd_weight=0.5, backbone_loss=False, clip=1.0)
    seq, ang, crd = (batch[k].to(dev) for k in ("seq", "true_ang", "true_crd"))
    losses = []
    for it in range(10):
        losses.append(float(train_step(m, opt_, args, seq, ang, crd)["drmsd-full"]))
        if it == 4:
            m.eval()
            with torch.no_grad():
                pred = m(seq)
            assert torch.isfinite(pred).all()
            m.train()
    assert all(np.isfinite(losses)), losses
    assert losses[-1] < losses[0], losses


def test_train_cli_dm256_nh2(dev, tmp_path, monkeypatch):
    """`train.py --synthetic ... -dm 256 -nh 2`: one short epoch, log rows and the checkpoint."""
    import csv
    import os
    from protein_transformer_amd import train as TR
    monkeypatch.setattr(TR, "START_EPOCH", 0)
    monkeypatch.setattr(sys, "argv", ["train", "--synthetic", "4,24,2", "--name", "h128", "-dm", "256", "-nl", "1", "-nh", "2",
                                      "-dih", "512", "-l", "drmsd", "-b", "4", "--max_seq_len", "24", "--train_only",
                                      "--log_dir", str(tmp_path / "logs"), "--chkpt_dir", str(tmp_path / "ck"), "-opt", "adam",
                                      "-e", "1"])
    TR.main()
    rows = list(csv.reader(open(tmp_path / "logs" / "h128.train")))
    epochs = [r for r in rows[1:] if r[7] == "epoch"]
    assert len(epochs) == 1 and np.isfinite(float(epochs[0][0]))
    assert os.path.exists(tmp_path / "ck" / "h128_best.chkpt")
    ck = torch.load(tmp_path / "ck" / "h128_best.chkpt", map_location="cpu", weights_only=False)
    assert ck is not None
