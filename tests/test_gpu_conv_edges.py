"""MI355X tests of the seven kernels of csrc/conv.hip (im2col, col2im, weight pack, weight unpack-add, one-hot, the positional
add and its adjoint) through the C ABI, element by element against the fp64 restatement tests/conv_ref.py, at their edges:
every residue of C mod 4 passed UNPADDED, k = 1 / 3 / 11, proteins shorter than, as long as and longer than the half window,
one protein and three, row strides wider than the row, thread counts on either side of a 256-thread block, ids outside the
vocabulary, dropout masks from the restated generator (stream 0xE3), and the Conv1d that kernels.conv1d_fwd / _bwd build from
them.  tests/test_conv_ref.py checks on any machine that the restatement is torch's Conv1d and that the case tables hit what
they claim.

Every buffer a kernel writes sits between guard bands of a sentinel bit pattern (a NaN) and is pre-filled with it; every input
sits between such bands too and is compared with what was uploaded after the call; the spare columns of a padded stride, the
rows in front of row 0 and behind row T-1 of x, the padded channels of dcol and dW2 and the rows of pe from L on hold NaN: a
window that leaves its buffer, a lane that reads a spare column or a store out of its row shows.

BARS (none measured):
  copies (im2col, pack, one-hot) and single fp32 operations (unpack-add, the positional add at p = 0, dropped elements): the bits;
  col2im: |err| <= (k - 1) 2^-24 sum_j |term_j|, k - 1 sequential fp32 adds to first order; exact at k = 1;
  positional add, kept elements: 4 x 2^-24 (|x| + |x + pe| / (1 - p)) forward, 3 x 2^-24 |dy| (1 + 1 / (1 - p)) backward: one
    rounding each of 1 / (1 - p), the inner add, the product and the outer add (backward: 1 / (1 - p), 1 + it, the product), each at
    most 2^-24 of an intermediate no larger than that scale, whether or not the compiler contracts the multiply-add;
  the composite Conv1d: the bound every arithmetic of the project meets in tests/test_gpu_gemm_strides.py,
    2e-6 (sum of |summands| + 1), per element; for dx the sum of that bound over the window slots of the element plus the col2im
    bound.  The largest ratios measured are printed and recorded in profiles/conv/NOTES.md."""
import numpy as np
import pytest
import torch

import conv_ref as R
from test_gpu_plddt import SENT, Guarded

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
BOUND = 2e-6                      # tests/test_gpu_gemm_strides.py: |err| < BOUND (sum |a||b| + 1) for every arithmetic
ERR_BAD_SHAPE = -1
ROWS = 6                          # NaN rows in front of and behind x: more than the largest half window
RATIOS = {}                       # (quantity, mode) -> largest |err| / bar of the composite Conv1d


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    yield torch.device("cuda:0")
    for q, mode in sorted(RATIOS):
        print(f"\n[conv edges] largest |err| / bar, {q}, {mode}: {RATIOS[q, mode]:.3e}", end="")
    print()


def lib():
    from protein_transformer_amd._lib import lib as _lib
    return _lib()


def stream():
    from protein_transformer_amd import kernels as K_
    return K_.stream()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def same_bits(got, want, what):
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.shape == w.shape, what
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        i = int(bad[0])
        raise AssertionError(f"{what}: {bad.size} of {g.size} words differ; first at flat index {i}: "
                             f"{np.asarray(got).reshape(-1)[i]!r} against {np.asarray(want).reshape(-1)[i]!r}")


def upload(dev, host):
    return Guarded(dev, host.size).set(host)


def unchanged(g, host, what):
    same_bits(g.collect(), host, what + ": an input was written")


def normal(g, shape):
    return g.standard_normal(shape).astype(np.float32)


def within(got, ref, bar, what):
    """Every element within its bar of the fp64 reference (a NaN fails); returns the largest |err| / bar where the bar is not 0
    (a bar of 0 asks for the exact value)."""
    got, err = np.asarray(got, np.float64), np.abs(np.asarray(got, np.float64) - ref)
    ok = err <= bar
    if not ok.all():
        i = tuple(int(v) for v in np.argwhere(~ok)[0])
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.size} elements miss their bar; first at {i}: got {got[i]!r}, "
                             f"fp64 {ref[i]!r}, |err| {err[i]:.3e}, bar {np.broadcast_to(bar, err.shape)[i]:.3e}")
    pos = np.broadcast_to(bar, err.shape) > 0
    return float((err[pos] / np.broadcast_to(bar, err.shape)[pos]).max()) if pos.any() else 0.0


# ------------------------------------------------------------------------------------------------ im2col
def im2col_case(dev, B, L, C, k, ldx):
    what = f"im2col B {B} L {L} C {C} k {k} ldx {ldx}"
    T, Cp = B * L, R.pad4(C)
    x = normal(np.random.default_rng([1, B, L, C, k]), (T, C))
    host = np.full((T + 2 * ROWS, ldx), np.nan, np.float32)
    host[ROWS:ROWS + T, :C] = x
    gx, gcol = upload(dev, host), Guarded(dev, T * k * Cp)
    rc = lib().ptamd_im2col1d(gx.ptr(ROWS * ldx), ldx, B, L, C, k, gcol.ptr(), stream())
    assert rc == 0, (what, rc)
    col = gcol.collect().reshape(B, L, k, Cp)
    unchanged(gx, host, what)
    assert np.isfinite(col).all(), f"{what}: col holds a NaN (a spare column, a guard row or an unwritten element)"
    assert (bits(col[..., C:]) == 0).all(), f"{what}: a padded channel is not +0"
    for j in range(k):
        lo, hi = R.window(L, k, j)
        outside = np.ones(L, dtype=bool)
        outside[lo:hi] = False
        assert (bits(col[:, outside, j]) == 0).all(), f"{what}: slot {j} outside the protein is not +0"
    same_bits(col, R.im2col64(x, B, L, k), what)


@pytest.mark.parametrize("C", R.CHANNELS)
def test_im2col_unpadded_channels(dev, C):
    for k in R.KERNELS:
        for L in R.LENGTHS:
            for B in R.BATCHES:
                for ldx in (R.pad4(C), R.pad4(C) + 8):
                    im2col_case(dev, B, L, C, k, ldx)


@pytest.mark.parametrize("n", sorted(R.IM2COL_EDGES))
def test_im2col_thread_count_edge(dev, n):
    B, L, C, k = R.IM2COL_EDGES[n]
    for ldx in (R.pad4(C), R.pad4(C) + 8):
        im2col_case(dev, B, L, C, k, ldx)


# ------------------------------------------------------------------------------------------------ col2im
def col2im_case(dev, B, L, C, k, lddx):
    what = f"col2im B {B} L {L} C {C} k {k} lddx {lddx}"
    T, Cp = B * L, R.pad4(C)
    d = normal(np.random.default_rng([2, B, L, C, k]), (T, k, Cp))
    d[:, :, C:] = np.nan                                           # never read
    gd, gdx = upload(dev, d), Guarded(dev, T * lddx)
    rc = lib().ptamd_col2im1d(gd.ptr(), B, L, C, k, gdx.ptr(), lddx, stream())
    assert rc == 0, (what, rc)
    dx = gdx.collect().reshape(T, lddx)
    unchanged(gd, d, what)
    assert (bits(dx[:, C:]) == SENT).all(), f"{what}: a column of dx beyond C was written"
    ref, ab = R.col2im64(d.reshape(T, k * Cp), B, L, C, k)
    if k == 1:
        same_bits(dx[:, :C], ref, what)
    within(dx[:, :C], ref, (k - 1) * EPS * ab, what)
    assert (bits(dx[:, :C])[ab == 0] == 0).all(), f"{what}: an element without a summand is not +0"


@pytest.mark.parametrize("C", R.CHANNELS)
def test_col2im_unpadded_channels(dev, C):
    for k in R.KERNELS:
        for L in R.LENGTHS:
            for B in R.BATCHES:
                for lddx in (C, R.pad4(C), R.pad4(C) + 8):
                    col2im_case(dev, B, L, C, k, lddx)


@pytest.mark.parametrize("n", sorted(R.COL2IM_EDGES))
def test_col2im_element_count_edge(dev, n):
    B, L, C, k = R.COL2IM_EDGES[n]
    for lddx in (R.pad4(C), R.pad4(C) + 8):
        col2im_case(dev, B, L, C, k, lddx)


# ------------------------------------------------------------------------------------------------ pack / unpack-add
@pytest.mark.parametrize("Co,C,k", R.PACK_SHAPES + list(R.PACK_EDGES.values()) + list(R.UNPACK_EDGES.values()))
def test_weight_pack_unpack_add(dev, Co, C, k):
    what = f"Co {Co} C {C} k {k}"
    g = np.random.default_rng([3, Co, C, k])
    Cp = R.pad4(C)
    w = normal(g, (Co, C, k))
    gw, gw2 = upload(dev, w), Guarded(dev, Co * k * Cp)
    rc = lib().ptamd_conv_weight_pack(gw.ptr(), Co, C, k, gw2.ptr(), stream())
    assert rc == 0, ("pack " + what, rc)
    w2 = gw2.collect().reshape(Co, k, Cp)
    unchanged(gw, w, "pack " + what)
    assert (bits(w2[:, :, C:]) == 0).all(), f"pack {what}: a padded channel is not +0"
    same_bits(w2, R.pack64(w), "pack " + what)

    dw2 = normal(g, (Co, k, Cp))
    dw2[:, :, C:] = np.nan                                         # never read
    dw0 = normal(g, (Co, C, k))
    gdw2, gdw = upload(dev, dw2), upload(dev, dw0)
    u = np.ascontiguousarray(dw2[:, :, :C].transpose(0, 2, 1))
    want = dw0
    for call in (1, 2):                                            # it accumulates: one fp32 add per call
        rc = lib().ptamd_conv_weight_unpack_add(gdw2.ptr(), Co, C, k, gdw.ptr(), stream())
        assert rc == 0, ("unpack-add " + what, rc)
        want = want + u
        assert want.dtype == np.float32
        same_bits(gdw.collect(), want, f"unpack-add {what}, call {call}")
    unchanged(gdw2, dw2, "unpack-add " + what)
    ref, ab = R.unpack_add64(dw2.reshape(Co, k * Cp), dw0)
    assert (np.abs((dw0 + u).astype(np.float64) - ref) <= EPS * ab).all()                   # the fp32 add is the fp64 sum, rounded


# ------------------------------------------------------------------------------------------------ one-hot
def onehot_case(dev, ids, C):
    what = f"one-hot C {C}, {len(ids)} ids"
    T, Cp = len(ids), R.pad4(C)
    host = np.asarray(ids, dtype=np.int64)
    seq = torch.from_numpy(host.copy()).to(dev)
    gx = Guarded(dev, T * Cp)
    rc = lib().ptamd_onehot(seq.data_ptr(), T, C, gx.ptr(), stream())
    assert rc == 0, (what, rc)
    x = gx.collect().reshape(T, Cp)
    assert np.array_equal(seq.cpu().numpy(), host), what + ": an input was written"
    return x, R.onehot64(host, C), what


@pytest.mark.parametrize("C", R.ONEHOT_CLASSES)
def test_onehot_out_of_range_ids_give_zero_rows(dev, C):
    ids = list(range(C)) + [20] + R.out_of_range_ids(C)
    x, ref, what = onehot_case(dev, ids, C)
    out = np.array([not 0 <= i < C for i in ids])
    assert (bits(x[out]) == 0).all(), f"{what}: ids {sorted({ids[t] for t in np.flatnonzero((bits(x) != 0).any(axis=1) & out)})} " \
                                      f"outside 0 .. {C - 1} do not give a row of +0"
    same_bits(x, ref, what)


@pytest.mark.parametrize("C", R.ONEHOT_CLASSES)
def test_onehot_padding_columns_are_zero_for_every_id(dev, C):
    """Columns C .. Cp-1 are +0 whatever the id: an id that names a padding column (22 and 23 at the vocabulary's 22) included."""
    ids = list(range(-2, R.pad4(C) + 3)) + [20] + R.out_of_range_ids(C)
    x, _, what = onehot_case(dev, ids, C)
    hit = sorted({ids[t] for t in np.flatnonzero((bits(x[:, C:]) != 0).any(axis=1))})
    assert not hit, f"{what}: ids {hit} write into the padding columns {C} .. {R.pad4(C) - 1}"


@pytest.mark.parametrize("n", sorted(R.ONEHOT_EDGES))
def test_onehot_thread_count_edge(dev, n):
    T, C = R.ONEHOT_EDGES[n]
    pool = list(range(C)) + R.out_of_range_ids(C)
    x, ref, what = onehot_case(dev, [pool[t % len(pool)] for t in range(T)], C)
    same_bits(x, ref, what)


# ------------------------------------------------------------------------------------------------ positional add
def posenc_case(dev, B, L, D, worst=None):
    T = B * L
    g = np.random.default_rng([4, B, L, D])
    x, pe, dy = normal(g, (T, D)), np.full((L + 3, D), np.nan, np.float32), normal(g, (T, D))
    pe[:L] = normal(g, (L, D))
    pos = np.tile(np.arange(L), B)
    third = (np.arange(T * D) % 3 == 0).reshape(T, D)
    x[third] = -pe[pos][third]                     # x + pe = 0: a kept element equals a dropped one, only the generator tells
    gx, gpe, gdy = upload(dev, x), upload(dev, pe), upload(dev, dy)
    masks = {}
    for p in R.POSENC_PS:
        for seed in R.POSENC_SEEDS:
            what = f"posenc B {B} L {L} D {D} p {p} seed {seed}"
            gy, gdx = Guarded(dev, T * D), Guarded(dev, T * D)
            rc = lib().ptamd_posenc_add_fwd(gx.ptr(), gpe.ptr(), B, L, D, p, seed, gy.ptr(), stream())
            assert rc == 0, (what, rc)
            rc = lib().ptamd_posenc_add_bwd(gdy.ptr(), T * D, p, seed, gdx.ptr(), stream())
            assert rc == 0, (what, rc)
            y, dx = gy.collect().reshape(T, D), gdx.collect().reshape(T, D)
            ref, keep = R.posenc_fwd64(x, pe, B, L, p, seed)
            dref, keep_b = R.posenc_bwd64(dy, p, seed)
            assert np.array_equal(keep, keep_b)
            assert np.isfinite(y).all() and np.isfinite(dx).all(), what
            if p == 0:
                same_bits(y, x + (x + pe[pos]), what + " forward")
                same_bits(dx, np.float32(2) * dy, what + " backward")
                continue
            masks[p, seed] = keep
            same_bits(y[~keep], x[~keep], what + ": a dropped element of y is not x")
            same_bits(dx[~keep], dy[~keep], what + ": a dropped element of dx is not dy")
            ks = 1.0 / (1.0 - float(np.float32(p)))
            inner = np.abs(np.float64(x) + np.float64(pe[pos]))
            within(y[keep], ref[keep], (4 * EPS * (np.abs(np.float64(x)) + inner * ks))[keep], what + " forward, kept")
            within(dx[keep], dref[keep], (3 * EPS * np.abs(np.float64(dy)) * (1 + ks))[keep], what + " backward, kept")
            # the backward mask read off the result: dy (1 + ks) != dy wherever dy != 0
            assert np.array_equal((dx != dy) | (dy == 0), keep | (dy == 0)), what + ": the backward mask is not the generator's"
            live = ~third                                           # x + pe != 0: the forward mask shows too
            assert np.array_equal((y != x)[live], keep[live]), what + ": the forward mask is not the generator's"
    for p in (0.1, 0.5):
        assert not np.array_equal(masks[p, R.POSENC_SEEDS[0]], masks[p, R.POSENC_SEEDS[1]])
    unchanged(gx, x, "posenc x")
    unchanged(gpe, pe, "posenc pe")
    unchanged(gdy, dy, "posenc dy")


@pytest.mark.parametrize("D", R.POSENC_WIDTHS)
def test_posenc_add_masks_and_arithmetic(dev, D):
    posenc_case(dev, 3, 7, D)


@pytest.mark.parametrize("n", sorted(R.POSENC_EDGES))
def test_posenc_add_thread_count_edge(dev, n):
    posenc_case(dev, *R.POSENC_EDGES[n])


# ------------------------------------------------------------------------------------------------ the Conv1d built from them
@pytest.mark.parametrize("mode", ["f32", "auto"])
@pytest.mark.parametrize("B,L,C,Co,k", R.CONV_SHAPES)
def test_conv1d_per_element(dev, B, L, C, Co, k, mode):
    """kernels.conv1d_fwd / _bwd against conv1d64, every element on its own sum of absolute summands."""
    from protein_transformer_amd import kernels as K
    arith = K.GEMM_F32 if mode == "f32" else K.GEMM_AUTO
    what = f"conv1d B {B} L {L} C {C} Co {Co} k {k} {mode}"
    g = np.random.default_rng([5, B, L, C, Co, k])
    T, Cp = B * L, R.pad4(C)
    x, dy = normal(g, (T, C)), normal(g, (T, Co))
    w, b = (normal(g, (Co, C, k)) / np.float32(np.sqrt(C * k))).astype(np.float32), normal(g, (Co,))
    dw0, db0 = normal(g, (Co, C, k)), normal(g, (Co,))
    r = R.conv1d64(x, w, b, dy, B, L)
    xp = np.zeros((T, Cp), np.float32)
    xp[:, :C] = x
    up = lambda a: torch.from_numpy(a.copy()).to(dev)                                  # noqa: E731
    xd, dyd, wd, bd = up(xp), up(dy), up(w), up(b)
    y, w2 = K.conv1d_fwd(xd, B, L, C, wd, bd, k, arith=arith)
    ratio = {"y": within(y.cpu().numpy(), r["y"], BOUND * (r["abs_y"] + 1), what + " y")}
    # dx: each dcol term carries the GEMM bound of its own sum over co, col2im adds them in k - 1 fp32 adds
    gemm_part, _ = R.col2im64(np.pad(BOUND * (r["abs_dcol"] + 1), ((0, 0), (0, 0), (0, Cp - C))).reshape(T, k * Cp), B, L, C, k)
    _, terms = R.col2im64(np.pad(r["dcol"], ((0, 0), (0, 0), (0, Cp - C))).reshape(T, k * Cp), B, L, C, k)
    for need_dx in (True, False):
        dw, db = up(dw0), up(db0)
        dx = K.conv1d_bwd(dyd, xd, B, L, C, w2, k, dw, db, need_dx=need_dx, arith=arith)
        # the increments, on top of random prior contents: the prior is one more summand of the element
        ratio["dw"] = within(dw.cpu().numpy() - np.float64(dw0), r["dw"], BOUND * (r["abs_dw"] + np.abs(dw0) + 1), what + " dW")
        ratio["db"] = within(db.cpu().numpy() - np.float64(db0), r["db"], BOUND * (r["abs_db"] + np.abs(db0) + 1), what + " db")
        if need_dx:
            dxh = dx.cpu().numpy()
            assert dxh.shape == (T, Cp) and np.isfinite(dxh).all()
            ratio["dx"] = within(dxh[:, :C], r["dx"], gemm_part + (k - 1) * EPS * terms, what + " dx")
        else:
            assert dx is None
    assert np.array_equal(xd.cpu().numpy(), xp) and np.array_equal(dyd.cpu().numpy(), dy)
    assert np.array_equal(wd.cpu().numpy(), w) and np.array_equal(bd.cpu().numpy(), b)
    for q, v in ratio.items():
        RATIOS[q, mode] = max(RATIOS.get((q, mode), 0.0), v)
        print(f"[conv edges] {what}: largest |err| / bar, {q}: {v:.3e}")
        assert v <= 1.0


# ------------------------------------------------------------------------------------------------ bad arguments
VALID = dict(B=2, L=3, C=5, k=3, ld=8, Co=2, T=6, D=8, n=48)
# (entry point, the arguments that differ from VALID, refused only since the checks of ldx / lddx / NULL were added)
BAD = [(e, {a: v}, False) for e, names in (("im2col", "BLCk"), ("col2im", "BLCk"), ("pack", ("Co", "C", "k")),
                                           ("unpack_add", ("Co", "C", "k")), ("onehot", "TC"), ("posenc_fwd", "BLD"),
                                           ("posenc_bwd", "n")) for a in names for v in (0, -1)]
BAD += [("im2col", dict(k=2), False), ("col2im", dict(k=4), False), ("im2col", dict(ld=6), False), ("im2col", dict(ld=10), False),
        ("posenc_fwd", dict(D=6), False), ("posenc_bwd", dict(n=46), False), ("posenc_bwd", dict(n=2), False)]
BAD += [("im2col", dict(ld=4), True), ("im2col", dict(ld=0), True), ("im2col", dict(ld=-8), True),
        ("col2im", dict(ld=4), True), ("col2im", dict(ld=0), True), ("col2im", dict(ld=-8), True),
        ("im2col", dict(null="x"), True), ("im2col", dict(null="col"), True),
        ("col2im", dict(null="dcol"), True), ("col2im", dict(null="dx"), True)]


def bad_id(case):
    e, over, new = case
    return f"{e}-{'-'.join(f'{a}_{v}' for a, v in over.items())}{'-new' if new else ''}"


@pytest.mark.parametrize("case", BAD, ids=bad_id)
def test_bad_arguments_are_refused(dev, case):
    """PTAMD_ERR_BAD_SHAPE and nothing written.  The buffers are those of the VALID call, so a kernel that were launched with the
    refused stride or count would stay inside them."""
    entry, over, _ = case
    a = dict(VALID, **over)
    null = a.pop("null", None)
    v = VALID
    T, Cp = v["B"] * v["L"], R.pad4(v["C"])
    g = np.random.default_rng(6)
    P = lambda buf, name: None if name == null else buf.ptr()                          # noqa: E731
    if entry == "im2col":
        src = normal(g, (T + 2 * ROWS, v["ld"]))
        ins, outs = [(upload(dev, src), src)], [Guarded(dev, T * v["k"] * Cp)]
        rc = lib().ptamd_im2col1d(None if null == "x" else ins[0][0].ptr(ROWS * v["ld"]), a["ld"], a["B"], a["L"], a["C"], a["k"],
                                  P(outs[0], "col"), stream())
    elif entry == "col2im":
        src = normal(g, (T, v["k"] * Cp))
        ins, outs = [(upload(dev, src), src)], [Guarded(dev, T * v["ld"])]
        rc = lib().ptamd_col2im1d(P(ins[0][0], "dcol"), a["B"], a["L"], a["C"], a["k"], P(outs[0], "dx"), a["ld"], stream())
    elif entry == "pack":
        src = normal(g, (v["Co"], v["C"], v["k"]))
        ins, outs = [(upload(dev, src), src)], [Guarded(dev, v["Co"] * v["k"] * Cp)]
        rc = lib().ptamd_conv_weight_pack(ins[0][0].ptr(), a["Co"], a["C"], a["k"], outs[0].ptr(), stream())
    elif entry == "unpack_add":
        src = normal(g, (v["Co"], v["k"] * Cp))
        ins, outs = [(upload(dev, src), src)], [Guarded(dev, v["Co"] * v["C"] * v["k"])]
        rc = lib().ptamd_conv_weight_unpack_add(ins[0][0].ptr(), a["Co"], a["C"], a["k"], outs[0].ptr(), stream())
    elif entry == "onehot":
        seq = torch.arange(v["T"], dtype=torch.int64).to(dev)
        ins, outs = [], [Guarded(dev, v["T"] * Cp)]
        rc = lib().ptamd_onehot(seq.data_ptr(), a["T"], a["C"], outs[0].ptr(), stream())
    elif entry == "posenc_fwd":
        src, pe = normal(g, (T, v["D"])), normal(g, (v["L"], v["D"]))
        ins, outs = [(upload(dev, src), src), (upload(dev, pe), pe)], [Guarded(dev, T * v["D"])]
        rc = lib().ptamd_posenc_add_fwd(ins[0][0].ptr(), ins[1][0].ptr(), a["B"], a["L"], a["D"], 0.1, 5, outs[0].ptr(), stream())
    else:
        src = normal(g, (v["n"],))
        ins, outs = [(upload(dev, src), src)], [Guarded(dev, v["n"])]
        rc = lib().ptamd_posenc_add_bwd(ins[0][0].ptr(), a["n"], 0.1, 5, outs[0].ptr(), stream())
    torch.cuda.synchronize()
    assert rc == ERR_BAD_SHAPE, f"{bad_id(case)}: returned {rc}, not PTAMD_ERR_BAD_SHAPE"
    for o in outs:
        assert o.untouched(), f"{bad_id(case)}: an output was written"
    for buf, host in ins:
        unchanged(buf, host, bad_id(case))
