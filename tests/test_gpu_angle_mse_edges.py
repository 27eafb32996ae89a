"""MI355X tests of csrc/angle_mse.hip alone - `mse_sums`, `mse_grad`, `mse_over_angles` and the two C entry points - PER ROW and PER
ELEMENT against the fp64 restatement tests/metric_ref.py, at the edges of its index arithmetic.

Forward: 128 blocks x 256 threads stride over the rows, so a thread takes a second row only from row 32768 on; the backward is one
thread per row in blocks of 256.  T in {1, 255, 256, 257, 32767, 32768, 32769, 32768 + 257}; in every run ONE heavy row
(|p - t| = 8 on every element against <= 0.5 elsewhere) sits at row 0, 255, 256, T - 1, 32767 or 32768: it is >= 1e-3 of every
sum it is in (asserted), so a dropped or doubled row moves a sum by a hundred times the bar.

Rows (tests/metric_ref.py ROW_CLASSES, every class in every case from T = 255 on, asserted; T = 1 runs each class alone):
ordinary; all-zero truth (padding); backbone all zero; side chain all zero; some NaN; all 24 NaN (selected, contributes
nothing); backbone zero except one NaN (the NaN selects the row for the backbone slice); a row of -0.0 (padding);
and a row whose only non-zero truth element is the DENORMAL 1e-40 in a side-chain column.  The reference selects that row for the
full and the side-chain slice.  THE KERNEL SELECTS IT TOO: the library is built without flush-to-zero (no -ffast-math, no
-fgpu-flush-denormals-to-zero; gfx950 runs fp32 denormals at full rate), `tv != 0.f` is a v_cmp that sees the denormal, and the
three exact counts of every case below hold with such rows in them (MI355X run of this file).

Bars:
  * the three counts exactly; the three sums at relative 1e-5 against fp64 (the bar of test_mse_over_angles_golden); two runs and the
    [B, L, 24] / [1, B L, 24] views give the same bits;
  * gradient: a masked element is exactly 0 (accumulating: exactly the old value); every other element within 4 * 2^-24 relative
    of the fp64 value - four fp32 roundings: coef as passed, the division by the count, the difference, the product - and, when
    accumulating, one more half-ulp of the result; the count is the device-side sums[1], from `mse_sums` and as a hand-set larger
    global count (data parallelism);
  * no selected element: sums and counts 0, gradient exactly 0 without a NaN (the kernel divides by the zero count and selects
    the quotient nowhere), `mse_over_angles` NaN - as torch's mse_loss of an empty selection.
"""
import functools

import numpy as np
import pytest
import torch

import metric_ref as R

pytestmark = pytest.mark.gpu

T_EDGES = [1, 255, 256, 257, 32767, 32768, 32769, 32768 + 257]
SUM_REL = 1e-5
EPS32 = 2.0 ** -24
W_DEFAULT = 0.5                                                  # train.py --combined_drmsd_weight
COEFS = [1.0, (1 - W_DEFAULT) / 0.01]                            # -l mse; -l combined (losses.combine_drmsd_mse)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def base_case(T):
    """the case of a T without a heavy row, checked once; read-only for the tests"""
    pred, true, classes = R.make_mse_case(T, None, seed=1000 + T)
    R.check_row_classes(true, classes)
    if T >= 255:
        assert set(classes) == set(R.ROW_CLASSES)
    return pred, true, classes


def heavy_rows(T):
    return sorted({r for r in (0, 255, 256, T - 1, 32767, 32768) if 0 <= r < T})


def dt(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def check_forward(got, pred, true, tag):
    sums, counts = R.mse_sums_ref(pred, true)
    got = got.astype(np.float64)
    assert (got[1], got[3], got[5]) == counts, (tag, got, counts)
    for k in range(3):
        rel = abs(got[2 * k] - sums[2 * k]) / sums[2 * k] if sums[2 * k] else abs(got[2 * k])
        assert rel <= SUM_REL, (tag, k, got[2 * k], sums[2 * k])
    return sums, counts


# --------------------------------------------------------------------------- forward
@pytest.mark.parametrize("T", T_EDGES)
def test_forward_sums_and_counts_with_a_heavy_row_at_every_edge(dev, T):
    from protein_transformer_amd.losses import mse_sums
    pred0, true0, classes0 = base_case(T)
    for row in heavy_rows(T):
        pred, true, classes = R.set_heavy_row(pred0, true0, classes0, row, seed=T)
        p, t = dt(pred, dev)[None], dt(true, dev)[None]
        got = mse_sums(p, t)
        again = mse_sums(p, t)
        assert torch.equal(got, again), (T, row)
        sums, counts = check_forward(got.cpu().numpy(), pred, true, (T, row))
        heavy = R.HEAVY ** 2 * 0.999
        assert 24 * heavy >= 1e-3 * sums[0] and 12 * heavy >= 1e-3 * sums[2] and 12 * heavy >= 1e-3 * sums[4], (T, row)
        print(f"MEASURED forward T = {T} heavy row {row}: relative error of the sums "
              + " ".join(f"{abs(float(got[2 * k]) - sums[2 * k]) / sums[2 * k]:.1e}" for k in range(3)))


@pytest.mark.parametrize("cls", list(R.ROW_CLASSES))
def test_forward_single_row_of_every_class(dev, cls):
    """T = 1: one thread of one block has a row; 32767 threads have none"""
    from protein_transformer_amd.losses import mse_sums
    rng = np.random.default_rng(5)
    true = R.make_truth_rows(cls, 1, rng).astype(np.float32)
    R.check_row_classes(true, [cls])
    pred = (np.nan_to_num(true.astype(np.float64), nan=0.3) + rng.uniform(-0.5, 0.5, (1, 24))).astype(np.float32)
    got = mse_sums(dt(pred, dev)[None], dt(true, dev)[None]).cpu().numpy()
    _, counts = check_forward(got, pred, true, cls)
    full, bb, sc, n_bb, n_sc = R.ROW_CLASSES[cls]
    assert counts == ((n_bb + n_sc) * full, n_bb * bb, n_sc * sc)


def test_forward_ragged_batch_equals_the_flattened_call(dev):
    from protein_transformer_amd.losses import mse_sums
    B, L = 25, 1321                                              # 25 * 1321 = 32768 + 257
    pred, true, classes = base_case(B * L)
    pred, true = pred.copy().reshape(B, L, 24), true.copy().reshape(B, L, 24)
    lens = np.random.default_rng(6).integers(1, L + 1, B)
    lens[0], lens[-1] = L, 1
    for b, n in enumerate(lens):                                 # rows behind a protein's end: zero truth, whatever the prediction
        true[b, n:] = 0.0
    p, t = dt(pred, dev), dt(true, dev)
    got = mse_sums(p, t)
    flat = mse_sums(p.reshape(1, B * L, 24), t.reshape(1, B * L, 24))
    assert torch.equal(got, flat)
    check_forward(got.cpu().numpy(), pred, true, "ragged")


# --------------------------------------------------------------------------- backward, per element
def check_grad(got, old, pred, true, coef, count, tag):
    ref = R.mse_grad_ref(pred, true, coef, count)
    masked = ~R.mse_masks(true)["full"].reshape(ref.shape)
    assert not np.isnan(got).any(), tag
    if old is None:
        assert np.all(got[masked] == 0), tag
        total, slack = ref, 0.0
    else:
        assert np.array_equal(got[masked], old[masked]), tag
        total = old.astype(np.float64) + ref
        slack = EPS32 * np.abs(total)
    err = np.abs(got.astype(np.float64) - total)
    bar = 4 * EPS32 * np.abs(ref) + slack
    live = ~masked
    assert live.any(), tag
    worst = float((err[live] / np.maximum(bar[live], 1e-300)).max())
    assert np.all(err[live] <= bar[live]), (tag, worst)
    return worst


@pytest.mark.parametrize("T", T_EDGES)
def test_backward_per_element(dev, T):
    from protein_transformer_amd.losses import mse_grad, mse_sums
    pred, true, classes = base_case(T) if T > 1 else R.make_mse_case(1, 0, seed=1)
    p, t = dt(pred, dev)[None], dt(true, dev)[None]
    sums = mse_sums(p, t)
    local = float(sums[1])
    assert local == R.mse_sums_ref(pred, true)[1][0] > 0
    world = sums.clone()
    world[1] = local + 12345.0                                   # the count of a global batch, as LossReport hands it over
    old = np.random.default_rng(T).normal(0, 1e-3, (1, T, 24)).astype(np.float32)
    old[0, :, 3] *= 1e3                                          # an accumulator far above, at, and (columns 4..) below the gradient
    old[0, :, 4:8] *= 1e-3
    worst = {"fresh": 0.0, "acc": 0.0}
    for coef in COEFS:
        for s in (sums, world):
            count = float(s[1])
            tag = (T, coef, count)
            g = mse_grad(p, t, s, coef=coef).cpu().numpy()
            worst["fresh"] = max(worst["fresh"], check_grad(g, None, pred[None], true[None], coef, count, tag + ("fresh",)))
            acc = dt(old.copy(), dev)
            out = mse_grad(p, t, s, coef=coef, accumulate_into=acc)
            assert out.data_ptr() == acc.data_ptr()
            got = acc.cpu().numpy()
            worst["acc"] = max(worst["acc"], check_grad(got, old, pred[None], true[None], coef, count, tag + ("acc",)))
    print(f"MEASURED backward T = {T}: worst error / bar {worst['fresh']:.3f} (fresh), {worst['acc']:.3f} (accumulating)")


# --------------------------------------------------------------------------- nothing selected
@pytest.mark.parametrize("kind", ["padding", "all_nan"])
def test_no_selected_element(dev, kind):
    from protein_transformer_amd.losses import mse_grad, mse_over_angles, mse_sums
    rng = np.random.default_rng(8)
    T = 300
    true = np.zeros((T, 24), np.float32)
    true[1::2] = -0.0
    if kind == "all_nan":
        true[[0, 255, 256, 299]] = np.nan                        # selected rows, no element
    pred = rng.normal(size=(T, 24)).astype(np.float32)
    p, t = dt(pred, dev)[None], dt(true, dev)[None]
    sums = mse_sums(p, t)
    assert np.array_equal(sums.cpu().numpy(), np.zeros(6, np.float32))
    assert R.mse_sums_ref(pred, true)[1] == (0, 0, 0)
    g = mse_grad(p, t, sums, coef=50.0).cpu().numpy()
    assert g.shape == (1, T, 24) and np.all(g == 0)
    old = rng.normal(size=(1, T, 24)).astype(np.float32)
    acc = dt(old.copy(), dev)
    mse_grad(p, t, sums, coef=50.0, accumulate_into=acc)
    assert np.array_equal(acc.cpu().numpy(), old)
    for kw in ({}, {"bb_only": True}, {"sc_only": True}):
        assert np.isnan(mse_over_angles(p, t, **kw).item())
    pg = p.clone().requires_grad_()
    mse_over_angles(pg, t).backward()
    assert np.all(pg.grad.cpu().numpy() == 0)


# --------------------------------------------------------------------------- the C entry points
def test_entry_points_refuse_and_accept(dev):
    from protein_transformer_amd import _lib
    lib = _lib.lib()
    T = 257
    pred, true, _ = base_case(T)
    N = T * 24
    pbuf, tbuf = torch.zeros(N + 4, device=dev), torch.zeros(N + 4, device=dev)
    pbuf[:N], tbuf[:N] = dt(pred, dev).reshape(-1), dt(true, dev).reshape(-1)
    pbuf[1:N + 1], p_al = pbuf[:N].clone(), pbuf[:N].clone()     # the same data 4 bytes further on, and an aligned copy
    tbuf[1:N + 1], t_al = tbuf[:N].clone(), tbuf[:N].clone()
    p_off, t_off = pbuf[1:N + 1], tbuf[1:N + 1]
    assert p_off.data_ptr() % 16 == 4 and t_off.data_ptr() % 16 == 4 and p_al.data_ptr() % 16 == 0 and t_al.data_ptr() % 16 == 0
    need = lib.ptamd_mse_angles_workspace_bytes()
    assert need == 128 * 6 * 8
    ws = torch.zeros(need, dtype=torch.uint8, device=dev)
    sentinel = torch.full((6,), 7.0, device=dev)
    fwd = lambda p, t, n, out, w, wb: lib.ptamd_mse_angles_fwd(_lib.ptr(p), _lib.ptr(t), n, _lib.ptr(out), _lib.ptr(w), wb,   # noqa: E731
                                                               _lib.stream())
    out = sentinel.clone()
    assert fwd(p_off, t_al, T, out, ws, need) == -5               # PTAMD_ERR_ALIGN
    assert fwd(p_al, t_off, T, out, ws, need) == -5
    assert fwd(p_al, t_al, T, out, ws, need - 1) == -3            # PTAMD_ERR_WORKSPACE
    assert fwd(p_al, t_al, T, out, None, need) == -3
    assert fwd(p_al, t_al, 0, out, ws, need) == -1                # PTAMD_ERR_BAD_SHAPE
    assert fwd(p_al, t_al, -5, out, ws, need) == -1
    torch.cuda.synchronize()
    assert torch.equal(out, sentinel)                             # nothing was launched
    assert fwd(p_al, t_al, T, out, ws, need) == 0
    check_forward(out.cpu().numpy(), pred, true, "ctypes")
    # backward: T = 0 refused, unaligned pointers accepted with the aligned call's bits
    bwd = lambda p, t, n, d, acc: lib.ptamd_mse_angles_bwd(_lib.ptr(p), _lib.ptr(t), n, _lib.ptr(out), 50.0, acc, _lib.ptr(d),   # noqa: E731
                                                           _lib.stream())
    d_al = torch.full((N,), 7.0, device=dev)
    assert bwd(p_al, t_al, 0, d_al, 0) == -1 and bwd(p_al, t_al, -1, d_al, 0) == -1
    torch.cuda.synchronize()
    assert bool((d_al == 7.0).all())
    dbuf = torch.full((N + 4,), 7.0, device=dev)
    assert bwd(p_al, t_al, T, d_al, 0) == 0 and bwd(p_off, t_off, T, dbuf[1:N + 1], 0) == 0
    assert torch.equal(d_al, dbuf[1:N + 1])
    assert float(dbuf[0]) == 7.0 and bool((dbuf[N + 1:] == 7.0).all())   # and not a word beside the T rows
    check_grad(d_al.cpu().numpy().reshape(T, 24), None, pred, true, 50.0, float(out[1]), "ctypes")


# --------------------------------------------------------------------------- autograd
def test_autograd_matches_fp64_autograd_of_the_oracle(dev):
    from oracle import losses as olosses
    from protein_transformer_amd.losses import mse_over_angles
    T = 257
    pred, true, _ = R.make_mse_case(T, 256, seed=3)
    p64 = torch.from_numpy(pred).double()[None].requires_grad_()
    t64 = torch.from_numpy(true).double()[None]
    want = olosses.mse_over_angles(p64, t64)
    want.backward()
    p = dt(pred, dev)[None].requires_grad_()
    got = mse_over_angles(p, dt(true, dev)[None])
    assert abs(got.item() - want.item()) <= SUM_REL * want.item()
    got.backward()
    g, ref = p.grad.cpu().numpy(), p64.grad.numpy()
    masked = ~R.mse_masks(true)["full"].reshape(ref.shape)
    assert np.all(ref[masked] == 0) and np.all(g[masked] == 0)
    assert np.all(np.abs(g - ref) <= 4 * EPS32 * np.abs(ref))
    for kw in ({"bb_only": True}, {"sc_only": True}):
        q = dt(pred, dev)[None].requires_grad_()
        loss = mse_over_angles(q, dt(true, dev)[None], **kw)
        sums, _ = R.mse_sums_ref(pred, true)
        k = 1 if "bb_only" in kw else 2
        assert abs(loss.item() - sums[2 * k] / sums[2 * k + 1]) <= SUM_REL * sums[2 * k] / sums[2 * k + 1]
        with pytest.raises(NotImplementedError):
            loss.backward()
