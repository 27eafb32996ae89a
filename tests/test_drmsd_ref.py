"""Pins tests/drmsd_ref.py, the fp64 restatement that tests/test_gpu_drmsd_edges.py holds csrc/drmsd.hip against.  CPU only.

  * against `oracle.batched.drmsd_direct` in fp64 with torch autograd, on drawn proteins with absent atoms and padding and on
    the inputs of the golden vectors g3_drmsd and g4_drmsd_work: 1e-12 relative (two fp64 evaluations of one formula);
  * against the numbers stored in those golden files, which the reference computed in fp32: at the precision the oracle's own
    golden test holds them to (tests/test_oracle_golden.py: 2e-6 for g3, 2e-5 for g4);
  * the backbone call (spr = 3) against entries 2, 3, 5 of the full call;
  * the blockwise evaluation against a plain double loop, and the two per-atom arrays against their definitions.
"""
import numpy as np
import pytest
import torch
from pytest import approx

import drmsd_ref
from oracle import batched

REL = 1e-12


def draw(rng, n_res, L, frac_missing=0.2, sigma=8.0, near=None):
    true = rng.normal(0, sigma, (L * 14, 3)).astype(np.float32)
    pred = (rng.normal(0, sigma, (L * 14, 3)) if near is None else true + rng.normal(0, near, (L * 14, 3))).astype(np.float32)
    seq = np.full(L, 20, np.int64)
    seq[:n_res] = rng.integers(0, 20, n_res)
    gone = rng.random(L * 14) < frac_missing
    true[gone, rng.integers(0, 3, L * 14)[gone]] = np.nan                 # one NaN coordinate is enough
    return pred, true, seq


def autograd64(pred, true, seq, spr=14):
    """(D, n, d(D/n)/d pred) of the oracle's direct formula in fp64 on the atoms `drmsd_ref.present_slots` names."""
    ps, ts, _ = drmsd_ref.present_slots(true, seq, spr)
    p = torch.tensor(np.asarray(pred, np.float64).reshape(-1, 3)).requires_grad_()
    t = torch.tensor(np.asarray(true, np.float64).reshape(-1, 3))
    d = batched.drmsd_direct(p[torch.as_tensor(ps)], t[torch.as_tensor(ts)])
    (d / len(ps)).backward()
    return d.item(), len(ps), p.grad.numpy()


def rel_err(a, b):
    return np.linalg.norm(np.asarray(a) - np.asarray(b)) / np.linalg.norm(b)


@pytest.mark.parametrize("n_res,L,block", [(2, 4, 256), (9, 9, 4), (23, 32, 64), (40, 48, 256), (75, 80, 100)])
def test_reference_vs_oracle_autograd(n_res, L, block):
    rng = np.random.default_rng(100 + n_res)
    for near in (None, 0.5):
        pred, true, seq = draw(rng, n_res, L, near=near)
        r = drmsd_ref.drmsd_reference(pred, true, seq, block=block)
        D, n, g = autograd64(pred, true, seq)
        assert r["stats"][4] == n and r["stats"][0] == approx(D, rel=REL) and r["stats"][1] == approx(D / n, rel=REL)
        assert rel_err(r["grad"], g) < REL
        assert np.array_equal(r["grad"] == 0, g == 0)                     # absent and padded slots: exact zeros in both
        assert np.all(r["grad"][n_res * 14:] == 0) and np.count_nonzero(r["grad"]) == 3 * n
        # the backbone numbers of the full call are the backbone call's, which is the oracle's formula over N, CA, C
        bb_pred = pred.reshape(L, 14, 3)[:, :3].reshape(-1, 3)
        rb = drmsd_ref.drmsd_reference(bb_pred, true, seq, spr=3, block=block)
        Db, nb, gb = autograd64(bb_pred, true, seq, spr=3)
        assert rb["stats"][5] == nb == r["stats"][5]
        assert rb["stats"][2] == approx(Db, rel=REL) and rb["stats"][3] == approx(Db / nb, rel=REL)
        assert r["stats"][2] == approx(rb["stats"][2], rel=REL) and r["stats"][3] == approx(rb["stats"][3], rel=REL)
        assert tuple(rb["stats"][[0, 1, 4]]) == tuple(rb["stats"][[2, 3, 5]])          # the mirror
        assert rb["grad"].shape == (L * 3, 3) and rel_err(rb["grad"], gb) < REL
        assert tuple(r["stats"][6:]) == tuple(rb["stats"][6:]) == (0.0, 0.0)


def test_blockwise_equals_the_double_loop_and_the_per_atom_arrays_their_definitions():
    rng = np.random.default_rng(7)
    pred, true, seq = draw(rng, 6, 8)
    for spr in (14, 3):
        p = pred if spr == 14 else pred.reshape(8, 14, 3)[:, :3].reshape(-1, 3)
        r = drmsd_ref.drmsd_reference(p, true, seq, spr=spr, block=5)
        stats, grad = drmsd_ref.drmsd_loops(p, true, seq, spr=spr)
        assert np.allclose(r["stats"], stats, rtol=REL, atol=0) and rel_err(r["grad"], grad) < REL
        ps, ts, _ = drmsd_ref.present_slots(true, seq, spr)
        x, t, n = p[ps].astype(np.float64), true[ts].astype(np.float64), len(ps)
        d = np.sqrt(((x[:, None] - x[None]) ** 2).sum(-1))
        tau = np.sqrt(((t[:, None] - t[None]) ** 2).sum(-1))
        scale = 1.0 / (n * (n * (n - 1) / 2) * stats[0])
        off = ~np.eye(n, dtype=bool)
        assert r["scale"] == approx(scale, rel=REL)
        assert np.allclose(r["unit"], 2.0 ** -24 * scale * ((d + tau) * off).sum(1), rtol=REL, atol=0)
        e, iu = d - tau, np.triu_indices(n, 1)
        lever = (np.abs(e) * (d + tau))[iu].sum() / (e * e)[iu].sum()
        assert np.allclose(r["stat_unit"][:2], 2.0 ** -24 * np.array([lever + 1, lever + 2]), rtol=REL, atol=0)
        if spr == 3:
            assert np.array_equal(r["stat_unit"][:2], r["stat_unit"][2:])
        move = scale * np.abs(d - tau)
        for i in range(n):
            mine = move[i][off[i]]
            at_least = (mine >= r["pairmove_p10"][i] * (1 - REL)).sum()
            assert at_least >= 0.9 * (n - 1) and (mine <= r["pairmove_p10"][i] * (1 + REL)).any()


def test_degenerate_proteins():
    rng = np.random.default_rng(9)
    pred, true, seq = draw(rng, 3, 5, frac_missing=0.0)
    for keep, (n_bb, n) in (((), (0, 0)), ((1,), (1, 1)), ((5,), (0, 1)), ((0, 15), (2, 2)), ((2, 9), (1, 2)), ((0, 1, 31), (2, 3))):
        t = np.full_like(true, np.nan)
        t[list(keep)] = true[list(keep)]
        t[3 * 14:] = true[3 * 14:]                                        # padded residues hold finite numbers
        r = drmsd_ref.drmsd_reference(pred, t, seq)
        assert (r["stats"][5], r["stats"][4]) == (n_bb, n)
        assert np.isnan(r["stats"][:2]).all() == (n < 2) and np.isnan(r["stats"][2:4]).all() == (n_bb < 2)
        assert np.isfinite(r["stats"][:2]).all() == (n >= 2) and np.isfinite(r["stats"][2:4]).all() == (n_bb >= 2)
        assert np.isfinite(r["grad"]).all() and (np.count_nonzero(r["grad"]) == 3 * n if n >= 2 else not r["grad"].any())
    same = drmsd_ref.drmsd_reference(true[:, :], true, seq)              # prediction == truth: D = 0, sqrt'(0) * 0
    assert tuple(same["stats"][:4]) == (0.0, 0.0, 0.0, 0.0) and np.isnan(same["grad"][:3 * 14]).all()
    assert not same["grad"][3 * 14:].any()


def test_reference_vs_golden_g3(golden):
    g = golden("g3_drmsd")
    assert int(g["n"]) > 0
    for k in range(int(g["n"])):
        a, b = np.asarray(g[f"a{k}"], np.float64), np.asarray(g[f"b{k}"], np.float64)
        n = len(a)
        # a bare point set as one protein: every slot present, n a multiple of 14 or not - pad the slot arrays with absent atoms
        L = -(-n // 14)
        pred, true = np.zeros((L * 14, 3)), np.full((L * 14, 3), np.nan)
        pred[:n], true[:n] = a, b
        r = drmsd_ref.drmsd_reference(pred, true, np.zeros(L, np.int64))
        direct = batched.drmsd_direct(torch.tensor(a), torch.tensor(b)).item()
        assert r["stats"][4] == n and r["stats"][0] == approx(direct, rel=REL)
        assert r["stats"][0] == approx(float(g[f"drmsd{k}"]), rel=2e-6)               # the stored value is fp32 arithmetic


def test_reference_vs_golden_g4(golden):
    g = golden("g4_drmsd_work")
    ang, seq, true = torch.tensor(g["pred_ang"]), torch.tensor(g["seq"]), g["true_crd"]
    crd = batched.generate_coords_batched(ang.double(), seq, torch.float64).numpy()
    stats64, _, _ = batched.batch_loss_and_grads(ang, seq, torch.tensor(true), torch.float64)
    for b in range(4):
        r = drmsd_ref.drmsd_reference(crd[b], true[b], g["seq"][b])
        assert np.allclose(r["stats"][:4], np.asarray(stats64[b][:4], np.float64), rtol=REL, atol=0)
        assert np.allclose(r["stats"][:4], g[f"vals{b}"], rtol=2e-5, atol=0)           # stored: the reference's fp32 chain
        D, n, grad = autograd64(crd[b], true[b], g["seq"][b])
        assert r["stats"][4] == n and rel_err(r["grad"], grad) < REL
        bb = crd[b].reshape(-1, 14, 3)[:, :3].reshape(-1, 3)
        rb = drmsd_ref.drmsd_reference(bb, true[b], g["seq"][b], spr=3)
        assert np.allclose(rb["stats"][[2, 3, 5]], r["stats"][[2, 3, 5]], rtol=REL, atol=0)


# ---------------------------------------------------------------- the layout restatement and the chunk-width witness
@pytest.fixture(scope="module")
def built_lib():
    from protein_transformer_amd import _lib, build
    build.build()                       # hipcc cross-compiles gfx950 without a GPU
    return _lib.lib()


def test_layout_restatement_is_the_librarys_byte_count(built_lib):
    lib = built_lib
    for B, L in ((1, 1), (5, 96), (27, 96), (18, 448), (12, 512), (13, 512), (213, 512), (214, 512), (32, 512), (32, 1500)):
        for spr, fn in ((14, lib.ptamd_drmsd_workspace_bytes_budget), (3, lib.ptamd_drmsd_bb_workspace_bytes_budget)):
            one = drmsd_ref.layout(B, L, 0, spr)
            budgets = (0, one["per_strip"], one["per_strip"] - 1, 4 * one["per_strip"] + 7, 1 << 20, 100 << 20)
            for budget in budgets:
                assert fn(B, L, budget) == drmsd_ref.layout(B, L, budget, spr)["total"], (B, L, spr, budget)


def test_b13_and_b12_at_512_take_different_chunk_widths(built_lib):
    """tri_layout: 8-tile chunks from strips (chunks + 1) / 2 B >= 2560 work items on, 4-tile chunks below.  With one width the
    workspace would be proportional to B."""
    lib = built_lib
    assert drmsd_ref.tri_layout(512 * 14, 13)["chunk_tiles"] == 8 and drmsd_ref.tri_layout(512 * 14, 12)["chunk_tiles"] == 4
    assert 28 * 15 // 2 * 13 == 2730 and 28 * 15 // 2 * 12 == 2520
    assert lib.ptamd_drmsd_workspace_bytes(13, 512) * 12 != lib.ptamd_drmsd_workspace_bytes(12, 512) * 13
    # the backbone instantiation (3 L atoms: 6 strips, 3 chunks of 8 tiles) flips between B = 213 and 214
    assert drmsd_ref.tri_layout(512 * 3, 214)["chunk_tiles"] == 8 and drmsd_ref.tri_layout(512 * 3, 213)["chunk_tiles"] == 4
    assert lib.ptamd_drmsd_bb_workspace_bytes(214, 512) * 213 != lib.ptamd_drmsd_bb_workspace_bytes(213, 512) * 214
