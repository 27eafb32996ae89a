"""What ptamd_attention_fwd / ptamd_attention_bwd refuse before any launch (csrc/attention.hip and the plan checks of
csrc/attention_f16x2.hip), as one table next to the dispatch: every call below returns its code from the host.  One shape,
1 x 33 tokens, 2 heads (of 64 unless a case says otherwise), every buffer of the size the library asks for; the valid call of
the same shape returns PTAMD_OK in each arithmetic family.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

B, L, H, DK = 1, 33, 2, 64
OK, BAD_SHAPE, WORKSPACE, ALIGN = 0, -1, -3, -5     # include/ptamd.h
F32, BF16X3, F16X2, AUTO = 0, 1, 3, 4               # PTAMD_GEMM_*


@pytest.fixture(scope="module")
def bufs():
    from protein_transformer_amd import kernels as K
    from protein_transformer_amd._lib import lib
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    D = H * DK
    g = torch.Generator().manual_seed(3)
    planes, inv = K.attention_kv_buffers(B * L, H, dev)
    ws_bytes = lib().ptamd_attention_workspace_bytes(B, L, H, DK)
    return dict(
        qkv=torch.randn(B * L + 1, 3 * D, generator=g).to(dev),     # (a spare row: the pointer 4 bytes on stays inside)
        seq=torch.randint(0, 20, (B, L), generator=g).to(dev),
        out=torch.randn(B * L, D, generator=g).to(dev), dout=torch.randn(B * L, D, generator=g).to(dev),
        lse=torch.zeros(B, H, L, device=dev), dqkv=torch.empty(B * L, 3 * D, device=dev),
        keep_bits=K.attention_keep_bits(B, L, H, dev), kv_planes=planes.zero_(), kv_inv=inv.zero_(),
        row_scale=torch.full((B * L,), 0x7F000000, dtype=torch.int32, device=dev),
        row_min=torch.full((4,), 0x7F000000, dtype=torch.int32, device=dev),
        ws=torch.empty(ws_bytes, dtype=torch.uint8, device=dev), ws_bytes=ws_bytes)


def call(bufs, which, dk=DK, p=0.0, arith=AUTO, qkv_offset=0, ws_short=0, **given):
    """ptamd_attention_fwd / _bwd on the module's buffers; `given`: the optional pointers to pass (name=True)."""
    from protein_transformer_amd._lib import lib, ptr, stream
    opt = lambda name: ptr(bufs[name]) if given.get(name) else None      # noqa: E731
    qkv = C.c_void_p(bufs["qkv"].data_ptr() + qkv_offset)
    if which == "fwd":
        return lib().ptamd_attention_fwd(qkv, ptr(bufs["seq"]), B, L, H, dk, p, 7, 1, arith, ptr(bufs["out"]), ptr(bufs["lse"]),
                                         opt("keep_bits"), opt("kv_planes"), opt("kv_inv"), stream())
    return lib().ptamd_attention_bwd(qkv, ptr(bufs["seq"]), ptr(bufs["out"]), ptr(bufs["dout"]), ptr(bufs["lse"]), B, L, H, dk, p,
                                     7, 1, arith, ptr(bufs["dqkv"]), opt("row_scale"), opt("row_min"), opt("keep_bits"),
                                     opt("kv_planes"), opt("kv_inv"), ptr(bufs["ws"]), bufs["ws_bytes"] - ws_short, stream())


BOTH = ("fwd", "bwd")
REFUSALS = [(name, which, kw, code) for name, passes, kw, code in [
    # the forward kernels' decisions exist in f16x2 arithmetic only
    ("keep_bits at head size 16", ("fwd",), dict(dk=16, keep_bits=True), BAD_SHAPE),
    ("keep_bits under F32", ("fwd",), dict(arith=F32, keep_bits=True), BAD_SHAPE),
    # pre-split K / V: both buffers, f16x2 arithmetic, a shape whose plan reads them (whole 32-token tiles: not L = 33)
    ("kv_planes without kv_inv", BOTH, dict(kv_planes=True), BAD_SHAPE),
    ("kv_planes under BF16X3", BOTH, dict(arith=BF16X3, kv_planes=True, kv_inv=True), BAD_SHAPE),
    ("kv_planes where the plan reads none", BOTH, dict(kv_planes=True, kv_inv=True), BAD_SHAPE),
    ("kv_planes where the plan reads none, F16X2", BOTH, dict(arith=F16X2, kv_planes=True, kv_inv=True), BAD_SHAPE),
    # the by-products and inputs of the f16x2 backward kernels under another arithmetic
    ("row_scale under F32", ("bwd",), dict(arith=F32, row_scale=True, row_min=True), BAD_SHAPE),
    ("keep_bits under F32", ("bwd",), dict(arith=F32, keep_bits=True), BAD_SHAPE),
    ("kv_planes under F32", ("bwd",), dict(arith=F32, kv_planes=True, kv_inv=True), BAD_SHAPE),
    ("workspace one byte short", ("bwd",), dict(ws_short=1), WORKSPACE),
    ("arith above the enum", BOTH, dict(arith=5), BAD_SHAPE),
    ("arith below the enum", BOTH, dict(arith=-1), BAD_SHAPE),
    ("p = 1", BOTH, dict(p=1.0), BAD_SHAPE),
    ("head size 48", BOTH, dict(dk=48), BAD_SHAPE),
    ("qkv 4 bytes off", BOTH, dict(qkv_offset=4), ALIGN),
] for which in passes]


@pytest.mark.parametrize("name,which,kw,code", REFUSALS, ids=[f"{w}: {n}" for n, w, _, _ in REFUSALS])
def test_refused_before_any_launch(bufs, name, which, kw, code):
    assert call(bufs, which, **kw) == code


@pytest.mark.parametrize("arith", [F32, BF16X3, AUTO], ids=["f32", "bf16x3", "auto"])
def test_valid_call_of_the_same_shape(bufs, arith):
    assert call(bufs, "fwd", arith=arith) == OK
    assert call(bufs, "bwd", arith=arith) == OK
    torch.cuda.synchronize()
    assert torch.isfinite(bufs["out"]).all() and torch.isfinite(bufs["dqkv"]).all()
