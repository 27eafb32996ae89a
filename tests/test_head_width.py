"""Head widths the model accepts (protein_transformer_amd/models/encoder_only.py): d_model / n_head in {8, 16, 32, 64, 128}.
128-wide heads (`-dm 512 -nh 4`, `-dm 256 -nh 2`, `-dm 1024 -nh 8`) build for enc-only and conv-enc; 256-wide ones do not."""
import numpy as np
import pytest

from protein_transformer_amd.models.convolutional_encoder import ConvEncoderOnlyTransformer
from protein_transformer_amd.models.encoder_only import EncoderOnlyTransformer
from protein_transformer_amd.protein.Sequence import VOCAB

AM = np.zeros(24)


@pytest.mark.parametrize("dm,nh", [(512, 4), (256, 2), (1024, 8), (768, 6)])
def test_enc_only_builds_with_128_wide_heads(dm, nh):
    m = EncoderOnlyTransformer(1, nh, dm, 2 * dm, 64, VOCAB, AM, True)
    assert m.nhead == nh and m.dlayer // nh == 128


def test_conv_enc_builds_with_128_wide_heads():
    m = ConvEncoderOnlyTransformer(1, 2, 256, 512, 64, VOCAB, AM, True, [3], [1], True, True)
    assert m.dlayer // m.nhead == 128


@pytest.mark.parametrize("dm,nh", [(256, 1), (768, 8)])
def test_other_head_widths_still_raise(dm, nh):
    with pytest.raises(ValueError, match=r"\{8, 16, 32, 64, 128\}"):
        EncoderOnlyTransformer(1, nh, dm, 2 * dm, 64, VOCAB, AM, True)
