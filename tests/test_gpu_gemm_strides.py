"""MI355X tests of the ADDRESSING of the GEMM family (ptamd_gemm, ptamd_gemm_group, ptamd_gemm_hp and the ptamd_hp_split*
writers): every leading dimension padded and padded differently, operands surrounded by poison (NaN, then a finite 1e30),
outputs and workspaces surrounded by a sentinel bit pattern (tests/gemm_ref.py).

Every product is checked three ways:
  (a) each element of C[:M, :N] against the fp64 reference with the bound every arithmetic of the project meets,
      |err| < 2e-6 (sum_k |a||b| + 1) (tests/test_gpu_kernels.py::test_gemm_randomised); a NaN fails it;
  (b) not one word outside the matrices changed: C, the residual, colsum, the operands and the workspace;
  (c) the SAME BITS as the same call on tight, unpadded copies of the operands - the k order of an element does not depend
      on a leading dimension.

Which tile height a shape lands on (csrc/gemm_split_kernel.h `launch`, csrc/gemm.hip), for the M values below - none of
the shapes here has more than 3 N tiles x 5 K splits, so with one workgroup per CU every candidate height needs one round:
  F32 (and every arithmetic at K < 16)   128 x 128 tiles: M = 127 / 128 / 129 is the tile edge, 255 / 256 / 257 / 260 the second;
  BF16X3, K-contiguous A                 M <= 128: one 256-row tile; M > 128: 128-row tiles (3 rounds2 < 5 rounds4), so
                                         129, 255 / 256 / 257 and 260 sit at the edges of the first, second and third tile;
  F16X2 (AUTO with K-contiguous A)       M <= 128: one 256-row tile; M > 128: 64-row tiles (4 rounds1 < 6 rounds2);
                                         K < 32 is demoted to BF16X3 and follows its rule;
  BF16X3_FULL, and every k-major A       256-row tiles always: 255 / 256 / 257 / 260 is the edge;
  ptamd_gemm_group                       256-row tiles (k-major x k-major only).
31 / 32 / 33 and 63 / 64 / 65 are the edges of the 32 x 32 MFMA blocks and of a consumer wavefront's share of a tile.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import gemm_ref as R
from test_host_logic import dropout_mask_restated

pytestmark = pytest.mark.gpu

F32, BF16X3, BF16X3_FULL, F16X2, AUTO = 0, 1, 2, 3, 4
EPI_RELU, EPI_TANH, EPI_ACCUM, EPI_GATE, EPI_SLABS = 1, 2, 4, 8, 16
ERR_BAD_SHAPE, ERR_ALIGN = -1, -5
BOUND = 2e-6
# (arithmetic, scales given: None = found by the pass over the operands, 1 / 0 = a_scale / b_scale at that stride)
ARITHS = [("F32", F32, None), ("BF16X3", BF16X3, None), ("BF16X3_FULL", BF16X3_FULL, None), ("F16X2", F16X2, None),
          ("F16X2-scales1", F16X2, 1), ("F16X2-scales0", F16X2, 0), ("AUTO", AUTO, None)]
ARITH_IDS = [a[0] for a in ARITHS]
LAYOUTS = [(False, False), (False, True), (True, False), (True, True)]      # (a_kmajor, b_kmajor)
POISONS = [R.NAN_POISON, R.BIG_POISON]
RATIOS = {}                       # arithmetic -> largest err / (sum |a||b| + 1) seen by check (a)
CALLS = [0]                       # ptamd_gemm calls made by run()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    for name in sorted(RATIOS):
        print(f"\n[gemm strides] largest err / (sum|a||b| + 1), {name}: {RATIOS[name]:.3e} (bound {BOUND:.0e})", end="")
    print(f"\n[gemm strides] ptamd_gemm calls checked: {CALLS[0]}")


def lib():
    from protein_transformer_amd._lib import lib as _lib
    return _lib()


def stream():
    from protein_transformer_amd import kernels as K_
    return K_.stream()


# ------------------------------------------------------------------------------------------------------------ one call
class Spec:
    """One ptamd_gemm call on LOGICAL operands: a [M, K], b [N, K] (CPU fp32) and its epilogue."""

    def __init__(self, a, b, *, a_km=False, b_km=False, arith=F32, scales=None, bias=None, residual=None, flags=0, dropout=None,
                 split_k=1, colsum0=None, c0=None, gate_scale=0.0, use_mask=False):
        self.a, self.b, self.a_km, self.b_km, self.arith, self.scales = a, b, a_km, b_km, arith, scales
        self.bias, self.residual, self.flags, self.dropout, self.split_k = bias, residual, flags, dropout, split_k
        self.colsum0, self.c0, self.gate_scale, self.use_mask = colsum0, c0, gate_scale, use_mask
        self.M, self.K, self.N = a.shape[0], a.shape[1], b.shape[0]

    def reference(self):
        return R.gemm_ref(self.a, self.b, bias=self.bias, relu=bool(self.flags & EPI_RELU), dropout=self.dropout,
                          residual=self.residual, gate=bool(self.flags & EPI_GATE), gate_scale=self.gate_scale,
                          tanh=bool(self.flags & EPI_TANH), accum=self.c0 if self.flags & EPI_ACCUM else None, colsum=self.colsum0)


class Layout:
    """Paddings (floats beyond the row extent) and leads (floats in front of the matrix) of one call."""

    def __init__(self, pa=4, pb=12, pc=8, pr=20, c_lead=4, r_lead=8, poison=R.NAN_POISON, ldc=None):
        self.pa, self.pb, self.pc, self.pr, self.c_lead, self.r_lead, self.poison, self.ldc = pa, pb, pc, pr, c_lead, r_lead, poison, ldc


TIGHT = Layout(0, 0, 0, 0, 0, 0)
WS_LEAD = 64                      # floats of sentinel in front of / behind the carved workspace (256 bytes: keeps it aligned)


def sentinel_matrix(rows, cols):
    m = torch.empty(rows, cols, dtype=torch.float32)
    m.view(torch.int32).fill_(R.fill_bits(R.SENTINEL))
    return m


class Prepared:
    """Device buffers + ptamd_gemm_args of one Spec in one Layout; collect() brings everything back and checks the guards."""

    def __init__(self, dev, s, lay):
        from protein_transformer_amd._lib import GemmArgs
        self.s, self.lay, self.guards, self.keep = s, lay, [], []
        M, N, K = s.M, s.N, s.K
        As, Bs = (s.a.t() if s.a_km else s.a), (s.b.t() if s.b_km else s.b)
        self.lda, self.ldb = As.shape[1] + lay.pa, Bs.shape[1] + lay.pb
        self.ldc = lay.ldc if lay.ldc is not None else N + lay.pc
        self.ldr = N + lay.pr
        A = self.put(dev, "A", As, self.lda, 8, 12, lay.poison)
        B = self.put(dev, "B", Bs, self.ldb, 4, 16, lay.poison)
        cmat = s.c0 if (s.flags & EPI_ACCUM) else sentinel_matrix(M, N)
        self.Cd = self.put(dev, "C", cmat, self.ldc, lay.c_lead, 16, R.SENTINEL, out=True)
        res = None
        if s.residual is not None and not s.use_mask:
            res = self.put(dev, "residual", s.residual, self.ldr, lay.r_lead, 8, lay.poison)
        mask = None
        if s.use_mask:
            mask = torch.from_numpy(R.gate_mask_bits(s.residual.numpy()).view(np.int64)).to(dev)
            self.keep.append(mask)
        bias = self.put(dev, "bias", s.bias.view(1, -1), N, 4, 4, lay.poison) if s.bias is not None else None
        self.csd = self.put(dev, "colsum", s.colsum0.view(1, -1), M, 4, 4, R.SENTINEL, out=True) if s.colsum0 is not None else None
        self.ws_bytes = int(lib().ptamd_gemm_workspace_bytes(M, N, s.split_k))      # exactly what the library asks for
        assert self.ws_bytes % 4 == 0
        self.wsbuf = torch.full((2 * WS_LEAD + self.ws_bytes // 4,), R.fill_bits(R.SENTINEL), dtype=torch.int32, device=dev)
        ws = self.wsbuf[WS_LEAD:WS_LEAD + self.ws_bytes // 4]
        sa = sb = None
        self.sa_stride = self.sb_stride = 1
        if s.scales is not None:
            ra, rb = R.row_scale_bits(s.a.numpy()), R.row_scale_bits(s.b.numpy())
            if s.scales == 0:           # ONE scale per operand - that of its largest row - in four copies
                ra, rb = np.full(4, ra.min(), dtype=np.uint32), np.full(4, rb.min(), dtype=np.uint32)
            sa, sb = (torch.from_numpy(x.view(np.int32).copy()).to(dev) for x in (ra, rb))
            self.keep += [sa, sb]
            self.sa_stride = self.sb_stride = s.scales
        p, seed, sid = s.dropout if s.dropout is not None else (0.0, 0, 0)
        P = lambda t: t.data_ptr() if t is not None else None                     # noqa: E731
        self.args = GemmArgs(M=M, N=N, K=K, A=A.data_ptr(), lda=self.lda, a_kmajor=int(s.a_km), B=B.data_ptr(), ldb=self.ldb,
                             b_kmajor=int(s.b_km), C=self.Cd.data_ptr(), ldc=self.ldc, bias=P(bias), residual=P(res), ldr=self.ldr,
                             flags=s.flags, dropout_p=float(p), seed=int(seed), stream_id=int(sid), split_k=int(s.split_k),
                             workspace=ws.data_ptr(), workspace_bytes=self.ws_bytes, colsum=P(self.csd), gate_scale=float(s.gate_scale),
                             arith=int(s.arith), reserved_cus=0, a_scale=P(sa), a_scale_stride=self.sa_stride, b_scale=P(sb),
                             b_scale_stride=self.sb_stride, gate_mask=P(mask))

    def put(self, dev, name, mat, ld, lead, trail, fill, out=False):
        buf, _ = R.embed(mat, ld, lead, trail, fill)
        d = buf.to(dev)
        self.guards.append((name, d, mat.shape[0], mat.shape[1], ld, lead, fill))
        return d[lead:]

    def collect(self, what):
        torch.cuda.synchronize()
        for name, d, rows, cols, ld, lead, fill in self.guards:
            bad = R.untouched(d, rows, cols, ld, lead, fill)
            assert bad is None, f"{what}: a word outside {name} [{rows}, {cols}] (ld {ld}, lead {lead}) changed: (offset, where, bits) = {bad}"
        bad = R.untouched(self.wsbuf, 1, self.ws_bytes // 4, self.ws_bytes // 4, WS_LEAD, R.SENTINEL)
        assert bad is None, (f"{what}: a word outside the workspace of ptamd_gemm_workspace_bytes = {self.ws_bytes} bytes changed: "
                             f"(offset in floats incl. {WS_LEAD} lead, where, bits) = {bad}")
        s = self.s
        self.C = self.Cd[:s.M * self.ldc].view(s.M, self.ldc)[:, :s.N].cpu().numpy()
        self.colsum = self.csd[:s.M].cpu().numpy() if self.csd is not None else None
        self.ws = self.wsbuf[WS_LEAD:WS_LEAD + self.ws_bytes // 4].cpu().numpy().view(np.float32)
        return self


def run(dev, s, lay, what):
    p = Prepared(dev, s, lay)
    rc = lib().ptamd_gemm(C.byref(p.args), stream())
    assert rc == 0, f"{what}: ptamd_gemm refused a valid call with {rc}"
    CALLS[0] += 1
    return p.collect(what)


def where_is(m, n):
    return (f"element ({m}, {n}): 32 x 32 block ({m // 32}, {n // 32}) at ({m % 32}, {n % 32}); row {m % 128} of 128-row tile "
            f"{m // 128}, row {m % 256} of 256-row tile {m // 256}, column {n % 128} of N tile {n // 128}")


def check_bound(got, ref, scale, what, name):
    """(a): every element, NaN included, within the project's bound; the message names the worst element and its tile position."""
    ratio = np.abs(got.astype(np.float64) - ref) / scale
    ok = ratio < BOUND                                            # (NaN compares false)
    if not ok.all():
        bad = np.argwhere(~ok)
        m, n = (int(v) for v in bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {ok.size} elements miss |err| < {BOUND} (sum|a||b| + 1); first: got {got[m, n]!r}, "
                             f"fp64 {ref[m, n]!r}, ratio {ratio[m, n]:.3e} at {where_is(m, n)}")
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(ratio.max()))


def same_bits(x, y, what):
    xb, yb = np.ascontiguousarray(x).view(np.int32), np.ascontiguousarray(y).view(np.int32)
    if not np.array_equal(xb, yb):
        bad = np.argwhere(xb != yb)
        m, n = (int(v) for v in bad[0]) if xb.ndim == 2 else (int(bad[0][0]), 0)
        raise AssertionError(f"{what}: {len(bad)} of {xb.size} words differ; first: {x[tuple(bad[0])]!r} against {y[tuple(bad[0])]!r} "
                             f"at {where_is(m, n)}")


def check_product(dev, s, lay, what, name, tight=None):
    """(a) + (b) + (c) for one padded call; returns (padded run, tight run) - the tight one can be handed to the next layout."""
    got = run(dev, s, lay, what)
    ref, scale, cs_ref, cs_scale = s.reference()
    check_bound(got.C, ref, scale, what, name)
    if cs_ref is not None:
        check_bound(got.colsum[None, :], cs_ref[None, :], cs_scale[None, :], what + " colsum", name + " colsum")
    if tight is None:
        tight = run(dev, s, TIGHT, what + " (tight copies)")
    same_bits(got.C, tight.C, what + ": padded against tight copies")
    if got.colsum is not None:
        same_bits(got.colsum, tight.colsum, what + ": colsum, padded against tight copies")
    return got, tight


def operands(M, N, K, seed):
    """Asymmetric operands from a seeded generator; + arange * 1e-3 so that a transposed or shifted read is not accidentally right."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g) + torch.arange(K) * 1e-3
    b = torch.randn(N, K, generator=g) * 0.5 + torch.arange(N)[:, None] * 1e-3
    return a, b, g


def pairwise(Ms, Ns, Ks):
    """Every (M, K), (M, N) and (N, K) pair at least once (needs len(Ms), len(Ks) >= len(Ns)), not the full product."""
    assert len(Ms) >= len(Ns) and len(Ks) >= len(Ns)
    return [(m, Ns[(i + j) % len(Ns)], k) for i, m in enumerate(Ms) for j, k in enumerate(Ks)]


M_EDGES = [1, 4, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 260]
N_EDGES = [4, 124, 128, 132, 260]
K_EDGES = [4, 12,                        # the F32 fallback below 16
           16, 20, 28,                   # BF16X3 below one 32-stage; F16X2 demoted below 32
           32, 36, 44, 48, 52, 68, 100]  # the tail stage with kskip 4, 8, 12 (bf16x3: 16-k stages; f16x2: 32-k stages)


def shapes_of(a_km, b_km):
    Ms = sorted({(m + 3) // 4 * 4 for m in M_EDGES}) if a_km else M_EDGES                 # k-major A: M % 4 == 0
    Ns = N_EDGES if b_km else N_EDGES + [1, 5, 129]                                        # K-contiguous B: the scalar epilogue
    Ks = K_EDGES + [17, 33, 50] if (a_km and b_km) else K_EDGES                            # no K-contiguous row: any K
    return pairwise(Ms, Ns, Ks)


# ------------------------------------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("a_km,b_km", LAYOUTS, ids=["nn", "nk", "kn", "kk"])
@pytest.mark.parametrize("name,arith,scales", ARITHS, ids=ARITH_IDS)
def test_padded_strides_at_the_tile_edges(dev, name, arith, scales, a_km, b_km):
    """All four layouts x every arithmetic over the pairwise sweep of the tile-edge shapes, every leading dimension padded
    differently (lda = extent + 4, ldb + 12, ldc + 8), NaN poison then 1e30; one case per (layout, arithmetic) with ldc = 4096,
    where a stride mistake lands in another row instead of in padding."""
    cases = shapes_of(a_km, b_km) + [(132, 132, 36, 4096)]
    for i, case in enumerate(cases):
        M, N, K = case[:3]
        a, b, _ = operands(M, N, K, 1000 + i)
        s = Spec(a, b, a_km=a_km, b_km=b_km, arith=arith, scales=scales)
        tight = None
        for poison in POISONS:
            lay = Layout(poison=poison, ldc=case[3] if len(case) > 3 else None)
            what = f"{name} a_kmajor={int(a_km)} b_kmajor={int(b_km)} M={M} N={N} K={K} ldc={lay.ldc or N + lay.pc} poison={poison}"
            _, tight = check_product(dev, s, lay, what, name, tight)


# ------------------------------------------------------------------------------------------------------------ epilogues
def epilogue_spec(kind, a, b, g, **kw):
    M, N = a.shape[0], b.shape[0]
    bias, res, c0 = torch.randn(N, generator=g), torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    if kind == "plain":
        return Spec(a, b, **kw)
    if kind == "accum":
        return Spec(a, b, flags=EPI_ACCUM, c0=c0, **kw)
    if kind == "full":
        return Spec(a, b, bias=bias, residual=res, c0=c0, flags=EPI_RELU | EPI_TANH | EPI_ACCUM, **kw)
    if kind == "gate":
        return Spec(a, b, residual=res, flags=EPI_GATE, gate_scale=1.25, **kw)
    raise ValueError(kind)


def narrower(s, n):
    """The same call on the first n columns (B K-contiguous): an element does not depend on how many columns follow it."""
    cut = lambda t: t[:, :n].contiguous() if t is not None else None                # noqa: E731
    return Spec(s.a, s.b[:n].contiguous(), a_km=s.a_km, b_km=False, arith=s.arith, scales=s.scales,
                bias=s.bias[:n].contiguous() if s.bias is not None else None, residual=cut(s.residual), flags=s.flags,
                c0=cut(s.c0), gate_scale=s.gate_scale)


@pytest.mark.parametrize("b_km", [False, True], ids=["nn", "nk"])
@pytest.mark.parametrize("name,arith", [("F32", F32), ("BF16X3", BF16X3), ("BF16X3_FULL", BF16X3_FULL), ("F16X2", F16X2), ("AUTO", AUTO)])
def test_float4_and_scalar_epilogues_give_the_same_bits(dev, name, arith, b_km):
    """The float4 epilogue and the scalar one, forced each of the four ways build_params knows (N % 4, ldc % 4, C misaligned by
    4 bytes, ldr % 4 or a misaligned residual), on the same operands with padded ldc / ldr and guard bands: (a), (b), (c) each,
    and the SAME BITS among all of them.  (Both epilogues transpose the same accumulators through the same LDS scratch and apply
    the same fp32 operations in the same order - tile_epilogue_vec<VEC> of csrc/gemm_common.h differs in the width of its global
    accesses only - so nothing stands in the way of bit equality; it is asserted, not merely bounded.)"""
    for M, N, K in ((129, 132, 52), (260, 260, 36)):
        for kind in ("plain", "accum", "full", "gate"):
            a, b, g = operands(M, N, K, 7 * M + K)
            s = epilogue_spec(kind, a, b, g, b_km=b_km, arith=arith)
            variants = [("float4", Layout()), ("ldc % 4 = 1", Layout(pc=9)), ("C misaligned by 4 bytes", Layout(c_lead=1))]
            if s.residual is not None:
                variants += [("ldr % 4 = 1", Layout(pr=21)), ("residual misaligned by 4 bytes", Layout(r_lead=1))]
            base = tight = None
            for vname, lay in variants:
                what = f"{name} b_kmajor={int(b_km)} M={M} N={N} K={K} {kind} epilogue, {vname}"
                got, tight = check_product(dev, s, lay, what, name, tight)
                if base is None:
                    base = got
                else:
                    same_bits(got.C, base.C, what + ": scalar epilogue against the float4 epilogue")
            if not b_km:                                                             # N % 4 != 0: the first N - 3 columns alone
                sn = narrower(s, N - 3)
                what = f"{name} M={M} N={N - 3} K={K} {kind} epilogue, N % 4 = 1"
                got, _ = check_product(dev, sn, Layout(), what, name)
                same_bits(got.C, base.C[:, :N - 3], what + ": scalar epilogue against the float4 epilogue of the wider product")


@pytest.mark.parametrize("name,arith", [("F32", F32), ("BF16X3", BF16X3), ("F16X2", F16X2)])
def test_dropout_counter_uses_n_not_ldc(dev, name, arith):
    """Dropout with ldc != N, in the float4 and the scalar epilogue and in the split-K reduction: the kept set is exactly
    dropout_mask_restated(M, N, p, seed, stream_id) - the counter is built from row, column and N, never from a leading dimension."""
    p, seed, sid = 0.3, 0x1234567890AB, 5
    for M, N, K, split in ((260, 132, 36, 1), (65, 124, 32, 1), (129, 132, 100, 2)):
        a, b, g = operands(M, N, K, M + N)
        bias = torch.randn(N, generator=g)
        s = Spec(a, b, arith=arith, bias=bias, dropout=(p, seed, sid), split_k=split)
        want = dropout_mask_restated(M, N, p, seed, sid)
        for vname, lay in (("float4, ldc = N + 8", Layout()), ("scalar, ldc = N + 9", Layout(pc=9)), ("ldc = 4096", Layout(ldc=4096))):
            what = f"{name} M={M} N={N} K={K} split_k={split} dropout, {vname}"
            got, _ = check_product(dev, s, lay, what, name)
            kept = got.C != 0
            if not np.array_equal(kept, want):
                m, n = (int(v) for v in np.argwhere(kept != want)[0])
                raise AssertionError(f"{what}: the kept set is not dropout_mask_restated({M}, {N}, ...): {int((kept != want).sum())} "
                                     f"elements differ (is the counter built from ldc = {got.ldc} instead of N = {N}?); first at {where_is(m, n)}")


@pytest.mark.parametrize("b_km", [False, True], ids=["nn", "nk"])
@pytest.mark.parametrize("name,arith", [("F16X2", F16X2), ("AUTO", AUTO)])
def test_gate_from_padded_activation_and_from_one_bit_mask(dev, name, arith, b_km):
    """PTAMD_EPI_GATE from the fp32 activation with a padded ldr, and from the 1-bit mask (its 32 x 32 blocks are indexed with
    ceil(M / 32), never with a padded width) with a padded ldc that is a multiple of 4: (a), (b), (c) each, and the same bits."""
    for M, N, K in ((129, 132, 36), (33, 260, 68), (260, 124, 100)):
        a, b, g = operands(M, N, K, 3 * M + N)
        f1 = torch.relu(torch.randn(M, N, generator=g))                             # the saved ReLU output: about half zeros
        what = f"{name} b_kmajor={int(b_km)} M={M} N={N} K={K} gate"
        kw = dict(b_km=b_km, arith=arith, residual=f1, flags=EPI_GATE, gate_scale=1.0 / 0.9)
        by_act, _ = check_product(dev, Spec(a, b, **kw), Layout(), what + " from the activation (ldr = N + 20)", name)
        for ldc in (N + 8, 4096):
            by_mask, _ = check_product(dev, Spec(a, b, use_mask=True, **kw), Layout(ldc=ldc), what + f" from the 1-bit mask (ldc = {ldc})", name)
            same_bits(by_mask.C, by_act.C, what + f": 1-bit mask (ldc = {ldc}) against the fp32 activation")


@pytest.mark.parametrize("a_km,b_km", LAYOUTS, ids=["nn", "nk", "kn", "kk"])
@pytest.mark.parametrize("name,arith,scales", ARITHS, ids=ARITH_IDS)
def test_split_k_and_colsum_with_padded_strides(dev, name, arith, scales, a_km, b_km):
    """split_k in {2, 5} - more splits than K has 32-blocks, so the clamp is exercised (K = 36: 2 slices; K = 100: 4; K = 32:
    one, the unsplit kernel) - through the float4 reduction (plain / accumulate), the general one (bias + ReLU + residual) and
    the general one forced by ldc % 4; with k-major A the fused column sums from a padded lda, split and unsplit.  N = 260 is
    three N tiles: two of them share the column-sum work of a split."""
    for M, N, K in ((132, 260, 100), (36, 124, 36), (260, 132, 32), (64, 128, 68)):
        for split in (1, 2, 5):
            if split == 1 and not a_km:
                continue                                                            # (the sweep above)
            for kind, lay in (("accum", Layout()), ("full", Layout()), ("plain", Layout(pc=9))):
                a, b, g = operands(M, N, K, M + K + split)
                cs0 = torch.randn(M, generator=g) if a_km else None
                s = epilogue_spec(kind, a, b, g, a_km=a_km, b_km=b_km, arith=arith, scales=scales, split_k=split, colsum0=cs0)
                what = (f"{name} a_kmajor={int(a_km)} b_kmajor={int(b_km)} M={M} N={N} K={K} split_k={split} "
                        f"(effective {R.effective_splits(K, split)}) {kind} ldc={N + lay.pc} colsum={a_km}")
                check_product(dev, s, lay, what, name)


@pytest.mark.parametrize("b_km", [False, True], ids=["nn", "nk"])
@pytest.mark.parametrize("name,arith", [("F32", F32), ("BF16X3", BF16X3), ("F16X2", F16X2), ("AUTO", AUTO)])
def test_slabs_stay_in_the_workspace(dev, name, arith, b_km):
    """PTAMD_EPI_SLABS: C stays entirely sentinel, the workspace holds [splits][M][N] whose slab-order fp64 sum meets the
    bound, the bytes past ptamd_gemm_workspace_bytes stay untouched (collect()), same bits as on tight copies; with an
    effective split of 1 the flag is ignored and C is written."""
    for M, N, K, split in ((129, 132, 100, 2), (129, 132, 100, 5), (260, 124, 68, 5), (33, 260, 36, 5), (65, 128, 32, 2)):
        a, b, _ = operands(M, N, K, M + K)
        s = Spec(a, b, b_km=b_km, arith=arith, split_k=split, flags=EPI_SLABS)
        n = R.effective_splits(K, split)
        what = f"{name} b_kmajor={int(b_km)} M={M} N={N} K={K} split_k={split} (effective {n}) slabs"
        ref, scale, _, _ = s.reference()
        got, tight = run(dev, s, Layout(), what), run(dev, s, TIGHT, what + " (tight copies)")
        if n == 1:
            check_bound(got.C, ref, scale, what + ": one slice, C written", name)
            same_bits(got.C, tight.C, what)
            continue
        assert np.array_equal(got.C.view(np.int32), sentinel_matrix(M, N).numpy().view(np.int32)), what + ": C was written"
        slabs = got.ws[:n * M * N].reshape(n, M, N)
        total = np.zeros((M, N))
        for k in range(n):
            total = total + slabs[k].astype(np.float64)
        check_bound(total, ref, scale, what + ": slab-order sum", name)
        same_bits(slabs.reshape(n * M, N), tight.ws[:n * M * N].reshape(n * M, N), what + ": slabs, padded against tight copies")


@pytest.mark.parametrize("split", [1, 2, 5])
@pytest.mark.parametrize("a_km,b_km", LAYOUTS, ids=["nn", "nk", "kn", "kk"])
def test_workspace_of_exactly_the_documented_size(dev, a_km, b_km, split):
    """F16X2 with no scales given - the row-scale pass writes round4(M) + round4(N) scales BEHIND the slabs and column-sum slabs -
    on a workspace of exactly ptamd_gemm_workspace_bytes(M, N, split_k) carved from a sentinel buffer: lead and trail stay
    sentinel (collect() asserts it for every call of this file; here the shapes put every part of the workspace to use)."""
    for M, N, K in ((260, 132, 100), (36, 260, 68), (132, 4, 36)):
        a, b, g = operands(M, N, K, M + N + split)
        cs0 = torch.randn(M, generator=g) if a_km else None
        s = Spec(a, b, a_km=a_km, b_km=b_km, arith=F16X2, split_k=split, colsum0=cs0)
        for poison in POISONS:
            check_product(dev, s, Layout(poison=poison), f"F16X2 a_kmajor={int(a_km)} b_kmajor={int(b_km)} M={M} N={N} K={K} "
                          f"split_k={split} own workspace, poison={poison}", "F16X2")


# ------------------------------------------------------------------------------------------------------------ the group
@pytest.mark.parametrize("with_colsum", [True, False], ids=["colsum", "no-colsum"])
@pytest.mark.parametrize("n", [2, 4])
def test_group_members_with_their_own_padded_strides(dev, n, with_colsum):
    """ptamd_gemm_group on members of different M, N, K, each with its own padded lda / ldb / ldc, guard-banded C, colsum and
    workspace: bit for bit what ptamd_gemm gives member by member (the header's promise), (a) and (b) for every member."""
    from protein_transformer_amd._lib import GemmArgs
    members = [(132, 260, 100, 2, 0), (36, 4, 68, 5, 1), (260, 128, 50, 2, 0), (4, 132, 33, 2, 1)][:n]
    specs, lays = [], []
    for j, (M, N, K, split, sc) in enumerate(members):
        a, b, g = operands(M, N, K, 50 + j)
        specs.append(Spec(a, b, a_km=True, b_km=True, arith=F16X2, scales=sc, split_k=split, flags=EPI_ACCUM,
                          c0=torch.randn(M, N, generator=g), colsum0=torch.randn(M, generator=g) if with_colsum else None))
        lays.append(Layout(pa=4 + 8 * j, pb=12 + 4 * j, pc=8 + 4 * j))
    prepared = [Prepared(dev, s, lay) for s, lay in zip(specs, lays)]
    rc = lib().ptamd_gemm_group((GemmArgs * n)(*[p.args for p in prepared]), n, stream())
    assert rc == 0, f"ptamd_gemm_group refused {n} valid members with {rc}"
    for j, (p, s, lay) in enumerate(zip(prepared, specs, lays)):
        what = f"group member {j} of {n}: M={s.M} N={s.N} K={s.K} split_k={s.split_k} lda={p.lda} ldb={p.ldb} ldc={p.ldc}"
        p.collect(what)
        ref, scale, cs_ref, cs_scale = s.reference()
        check_bound(p.C, ref, scale, what, "F16X2 group")
        alone = run(dev, s, lay, what + " (ptamd_gemm alone)")
        same_bits(p.C, alone.C, what + ": group against ptamd_gemm")
        if with_colsum:
            check_bound(p.colsum[None, :], cs_ref[None, :], cs_scale[None, :], what + " colsum", "F16X2 group colsum")
            same_bits(p.colsum, alone.colsum, what + ": colsum, group against ptamd_gemm")


# ------------------------------------------------------------------------------------------------------------ hp format
def carved_operand(dev, rows, K):
    """HpOperand whose planes and scales are carved from sentinel buffers; returns (operand, check) - check() asserts that
    nothing outside ptamd_hp_bytes / ptamd_hp_padded_rows was written."""
    from protein_transformer_amd import kernels as K_
    nb, ns = int(lib().ptamd_hp_bytes(rows, K)), int(lib().ptamd_hp_padded_rows(rows))
    assert nb % 4 == 0
    pbuf = torch.full((2 * WS_LEAD + nb // 4,), R.fill_bits(R.SENTINEL), dtype=torch.int32, device=dev)
    sbuf = torch.full((8 + ns,), R.fill_bits(R.SENTINEL), dtype=torch.int32, device=dev)
    op = K_.hp_view(pbuf[WS_LEAD:WS_LEAD + nb // 4].view(torch.uint8), sbuf[4:4 + ns].view(torch.float32), rows, K)

    def check(what):
        for name, buf, cols, lead in (("planes", pbuf, nb // 4, WS_LEAD), ("scales", sbuf, ns, 4)):
            bad = R.untouched(buf, 1, cols, cols, lead, R.SENTINEL)
            assert bad is None, f"{what}: a word outside the {name} changed: {bad}"
    return op, check


def device_view(dev, mat, ld, lead, trail, fill):
    buf, _ = R.embed(mat, ld, lead, trail, fill)
    d = buf.to(dev)
    return d, d[lead:lead + mat.shape[0] * ld].view(mat.shape[0], ld)[:, :mat.shape[1]]


HP_SHAPES = [(rows, K) for rows in (31, 32, 33, 65) for K in (16, 36, 100)]


@pytest.mark.parametrize("poison", POISONS, ids=["nan", "1e30"])
def test_hp_writers_with_a_padded_ld(dev, poison):
    """ptamd_hp_split (both orientations, ld > the row), ptamd_hp_split_rows and ptamd_hp_split_cols from matrices whose row
    padding, lead and trail are poison: planes and scales identical, byte for byte, to the tight call; the source untouched;
    nothing written outside ptamd_hp_bytes / ptamd_hp_padded_rows."""
    from protein_transformer_amd import kernels as K_
    row_jobs, col_jobs = [], []
    for i, (rows, K) in enumerate(HP_SHAPES):
        g = torch.Generator().manual_seed(i)
        x = torch.randn(rows, K, generator=g) * torch.exp(torch.randn(rows, 1, generator=g) * 2) + torch.arange(K) * 1e-3
        what = f"rows={rows} K={K} poison={poison}"
        tight = K_.hp_split(x.to(dev))
        for transposed, src, ld, lead in ((False, x, K + 12, 4), (True, x.t().contiguous(), rows + 7, 1)):
            buf, view = device_view(dev, src, ld, lead, 9, poison)
            op, check = carved_operand(dev, rows, K)
            K_.hp_split(view, transposed=transposed, out=op)
            torch.cuda.synchronize()
            w = f"ptamd_hp_split transposed={int(transposed)} ld={ld} {what}"
            check(w)
            assert R.untouched(buf, src.shape[0], src.shape[1], ld, lead, poison) is None, w + ": the source changed"
            assert torch.equal(op.planes, tight.planes), w + ": planes differ from the tight call"
            assert torch.equal(op.scale.view(torch.int32), tight.scale.view(torch.int32)), w + ": scales differ from the tight call"
        rbuf, rview = device_view(dev, x, K + 4 + 4 * (i % 3), 8, 4, poison)
        rop, rcheck = carved_operand(dev, rows, K)
        row_jobs.append((rview, rop, rcheck, tight, f"ptamd_hp_split_rows job {i} ld={rview.stride(0)} {what}"))
        cbuf, cview = device_view(dev, x.t().contiguous(), rows + 9 + i, 1, 5, poison)
        cop, ccheck = carved_operand(dev, rows, K)
        cop.scale.copy_(tight.scale)                                   # the operand rows' scales are GIVEN to this writer
        col_jobs.append((cview, cop, ccheck, tight, f"ptamd_hp_split_cols job {i} ld={cview.stride(0)} {what}"))
    K_.hp_split_rows([j[0] for j in row_jobs], [j[1] for j in row_jobs])                    # all twelve in ONE launch each
    K_.hp_split_cols([j[0] for j in col_jobs], [j[1].scale for j in col_jobs], [j[1] for j in col_jobs])
    torch.cuda.synchronize()
    for view, op, check, tight, w in row_jobs + col_jobs:
        check(w)
        assert torch.equal(op.planes, tight.planes), w + ": planes differ from ptamd_hp_split on the tight matrix"
        assert torch.equal(op.scale.view(torch.int32), tight.scale.view(torch.int32)), w + ": scales differ"


@pytest.mark.parametrize("poison", POISONS, ids=["nan", "1e30"])
def test_gemm_hp_with_padded_ldc_and_ldr(dev, poison):
    """ptamd_gemm_hp with padded ldc and ldr (float4 and scalar epilogue, unsplit and split): (a) per element, guard bands on C
    and the residual, same bits as the tight call; gate_mask_out writes nothing past ptamd_gate_mask_bytes."""
    from protein_transformer_amd import kernels as K_
    for M, N, K, split in ((129, 132, 36, 1), (33, 260, 100, 2), (260, 124, 16, 1), (65, 128, 100, 5)):
        a, b, g = operands(M, N, K, M + N + K)
        bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
        A, B = K_.hp_split(a.to(dev)), K_.hp_split(b.to(dev))
        drop = (0.2, 99, 4)
        ref, scale, _, _ = R.gemm_ref(a, b, bias=bias, relu=True, dropout=drop, residual=res)
        outs = []
        for vname, pc, pr, c_lead in (("tight", 0, 0, 0), ("float4 ldc = N + 8, ldr = N + 20", 8, 20, 4), ("scalar ldc = N + 9", 9, 20, 4),
                                      ("scalar ldr = N + 21", 8, 21, 4), ("C misaligned", 8, 20, 1)):
            what = f"gemm_hp M={M} N={N} K={K} split_k={split} {vname} poison={poison}"
            cbuf, cview = device_view(dev, sentinel_matrix(M, N), N + pc, c_lead, 16, R.SENTINEL)
            rbuf, rview = device_view(dev, res, N + pr, 8, 8, poison)
            K_.gemm_hp(A, B, cview, bias=bias.to(dev), residual=rview, ldr=N + pr, flags=EPI_RELU, dropout_p=drop[0], seed=drop[1],
                       stream_id=drop[2], split_k=split)
            torch.cuda.synchronize()
            bad = R.untouched(cbuf, M, N, N + pc, c_lead, R.SENTINEL)
            assert bad is None, f"{what}: a word outside C changed: {bad}"
            assert R.untouched(rbuf, M, N, N + pr, 8, poison) is None, what + ": the residual changed"
            got = cview.cpu().numpy()
            check_bound(got, ref, scale, what, "gemm_hp")
            outs.append(got)
            same_bits(got, outs[0], what + ": against the tight call")
        # the 1-bit gate of the product's output, carved from a sentinel buffer
        n64 = int(lib().ptamd_gate_mask_bytes(M, N)) // 8
        mbuf = torch.full((2 * (8 + n64 + 8),), R.fill_bits(R.SENTINEL), dtype=torch.int32, device=dev)
        cbuf, cview = device_view(dev, sentinel_matrix(M, N), N + 8, 4, 16, R.SENTINEL)
        what = f"gemm_hp M={M} N={N} K={K} gate_mask_out"
        K_.gemm_hp(A, B, cview, bias=bias.to(dev), flags=EPI_RELU, gate_mask_out=mbuf.view(torch.int64)[8:8 + n64])
        torch.cuda.synchronize()
        bad = R.untouched(mbuf, 1, 2 * n64, 2 * n64, 16, R.SENTINEL)
        assert bad is None, f"{what}: a word outside ptamd_gate_mask_bytes = {8 * n64} bytes changed: {bad}"
        assert R.untouched(cbuf, M, N, N + 8, 4, R.SENTINEL) is None, what + ": a word outside C changed"
        y = cview.cpu().numpy()
        inside = R.gate_mask_bits(np.ones((M, N), dtype=np.float32))
        mask = mbuf.view(torch.int64)[8:8 + n64].cpu().numpy().view(np.uint64)
        assert np.array_equal(mask & inside, R.gate_mask_bits(y)), what + ": the mask is not (C > 0) in the documented layout"


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_are_host_side_and_leave_the_outputs_alone(dev):
    """lda % 4 / ldb % 4: PTAMD_ERR_BAD_SHAPE; a misaligned A or B: PTAMD_ERR_ALIGN; a leading dimension SMALLER than the row it
    strides (lda against K or M, ldb against K or N, ldc and ldr against N; 0 included; `ld` of the hp split entry points):
    PTAMD_ERR_BAD_SHAPE from ptamd_gemm, ptamd_gemm_group, ptamd_gemm_hp, ptamd_hp_split, ptamd_hp_split_rows and
    ptamd_hp_split_cols.  Nothing is launched: C, colsum, the workspace, planes and scales stay sentinel.  (Every buffer is a
    real allocation large enough for the valid call.)"""
    from protein_transformer_amd import kernels as K_
    from protein_transformer_amd._lib import GemmArgs, GemmHpArgs, HpSplitJob
    M, N, K = 36, 132, 68
    a, b, g = operands(M, N, K, 1)
    res, cs0 = torch.randn(M, N, generator=g), torch.randn(M, generator=g)

    def refused(s, want, what, group=False, **override):
        p = Prepared(dev, s, Layout())
        for k, v in override.items():
            v = getattr(p.args, k[:-4]) + 4 if k.endswith("_off") else v          # X_off: the pointer X moved by 4 bytes
            setattr(p.args, k[:-4] if k.endswith("_off") else k, v)
        rc = lib().ptamd_gemm_group((GemmArgs * 1)(p.args), 1, stream()) if group else lib().ptamd_gemm(C.byref(p.args), stream())
        assert rc == want, f"{what}: {override} gave {rc}, expected {want}"
        p.collect(what)
        assert np.all(p.C.view(np.int32) == R.fill_bits(R.SENTINEL)), what + ": C was written"
        assert np.all(p.ws.view(np.int32) == R.fill_bits(R.SENTINEL)), what + ": the workspace was written"
        if p.colsum is not None:
            assert np.array_equal(p.colsum, s.colsum0.numpy()), what + ": colsum was written"

    for a_km, b_km in LAYOUTS:
        for arith in (F32, BF16X3, F16X2, AUTO):
            s = Spec(a, b, a_km=a_km, b_km=b_km, arith=arith, residual=res, colsum0=cs0 if a_km else None)
            what = f"ptamd_gemm a_kmajor={int(a_km)} b_kmajor={int(b_km)} arith={arith}"
            ext_a, ext_b = (M if a_km else K), (N if b_km else K)
            refused(s, ERR_BAD_SHAPE, what, lda=ext_a + 2)
            refused(s, ERR_BAD_SHAPE, what, ldb=ext_b + 6)
            refused(s, ERR_ALIGN, what, A_off=1)
            refused(s, ERR_ALIGN, what, B_off=1)
            for short in (dict(lda=ext_a - 4), dict(lda=0), dict(ldb=ext_b - 4), dict(ldb=0), dict(ldc=N - 1), dict(ldc=N - 4),
                          dict(ldc=0), dict(ldr=N - 4), dict(ldr=0)):
                refused(s, ERR_BAD_SHAPE, what, **short)
    sg = Spec(a, b, a_km=True, b_km=True, arith=F16X2, scales=0, split_k=2, flags=EPI_ACCUM, c0=sentinel_matrix(M, N), colsum0=cs0)
    p = Prepared(dev, sg, Layout())
    assert lib().ptamd_gemm_group((GemmArgs * 1)(p.args), 1, stream()) == 0          # the member itself is a valid one
    p.collect("ptamd_gemm_group, valid member")
    for short in (dict(lda=M - 4), dict(lda=0), dict(ldb=N - 4), dict(ldb=0), dict(ldc=N - 4), dict(ldc=0)):
        refused(sg, ERR_BAD_SHAPE, "ptamd_gemm_group", group=True, **short)
    refused(sg, ERR_BAD_SHAPE, "ptamd_gemm_group", group=True, lda=M + 2)
    refused(sg, ERR_ALIGN, "ptamd_gemm_group", group=True, A_off=1)

    # ptamd_gemm_hp: ldc / ldr against N
    A, B = K_.hp_split(a.to(dev)), K_.hp_split(b.to(dev))
    cbuf, cview = device_view(dev, sentinel_matrix(M, N), N + 8, 4, 16, R.SENTINEL)
    rbuf, rview = device_view(dev, res, N + 20, 8, 8, R.NAN_POISON)
    for ldc, ldr in ((N - 4, N + 20), (0, N + 20), (N + 8, N - 4), (N + 8, 0)):
        args = GemmHpArgs(M=M, N=N, K=K, A=A.planes.data_ptr(), A_scale=A.scale.data_ptr(), B=B.planes.data_ptr(),
                          B_scale=B.scale.data_ptr(), C=cview.data_ptr(), ldc=ldc, bias=None, residual=rview.data_ptr(), ldr=ldr,
                          flags=0, dropout_p=0.0, seed=0, stream_id=0, split_k=1, workspace=None, workspace_bytes=0, gate_scale=0.0,
                          reserved_cus=0, gate_mask=None, gate_mask_out=None, kv_planes=None, kv_inv=None, kv_col0=0, kv_heads=0)
        assert lib().ptamd_gemm_hp(C.byref(args), stream()) == ERR_BAD_SHAPE, f"ptamd_gemm_hp ldc={ldc} ldr={ldr}"
    torch.cuda.synchronize()
    assert torch.equal(cbuf.view(torch.int32), torch.full_like(cbuf.view(torch.int32), R.fill_bits(R.SENTINEL))), "ptamd_gemm_hp wrote C"

    # the writers of the format: ld against the row of x
    rows = 33
    x = torch.randn(rows, K).to(dev)
    xt = x.t().contiguous()
    op, check = carved_operand(dev, rows, K)
    pl, sc = op.planes.data_ptr(), op.scale.data_ptr()
    for ld in (K - 4, 0):
        assert lib().ptamd_hp_split(K_.ptr(x), ld, rows, K, 0, pl, sc, stream()) == ERR_BAD_SHAPE, f"ptamd_hp_split ld={ld}"
        job = (HpSplitJob * 1)(HpSplitJob(x=x.data_ptr(), ld=ld, rows=rows, K=K, planes=pl, scale=sc))
        assert lib().ptamd_hp_split_rows(job, 1, stream()) == ERR_BAD_SHAPE, f"ptamd_hp_split_rows ld={ld}"
    for ld in (rows - 1, 0):
        assert lib().ptamd_hp_split(K_.ptr(xt), ld, rows, K, 1, pl, sc, stream()) == ERR_BAD_SHAPE, f"ptamd_hp_split transposed ld={ld}"
        job = (HpSplitJob * 1)(HpSplitJob(x=xt.data_ptr(), ld=ld, rows=rows, K=K, planes=pl, scale=sc))
        assert lib().ptamd_hp_split_cols(job, 1, stream()) == ERR_BAD_SHAPE, f"ptamd_hp_split_cols ld={ld}"
    torch.cuda.synchronize()
    check("refused hp writers")
    assert (op.planes.view(torch.int32) == R.fill_bits(R.SENTINEL)).all() and (op.scale.view(torch.int32) == R.fill_bits(R.SENTINEL)).all()
