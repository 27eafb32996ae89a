"""CPU checks of tests/attn_dropout_ref.py, the kernel-independent restatement of attention dropout: the layout of the mask,
what the seed words and the stream id do to it, the kept fraction, the single-key proteins the GPU test relies on, and the
discriminating power of the bars of tests/test_gpu_attention_dropout.py (a wrong mask or a wrong scale of the kept
probabilities must break them by a wide margin, or they could not tell it from rounding)."""
import numpy as np
import pytest

import attn_dropout_ref as R
from test_gpu_attention_plan import lengths, pick_cases

CUS = 256                 # the CU count the plan's shapes are derived for here (MI355X); the GPU test uses the device's own


def test_threshold_and_scale():
    """make_attn_drop: t = p 65536 + 0.5 in fp32, clamped at 65535; ks = 65536 / (65536 - thr16).  At p = 0.25 the quantised
    probability is p itself, at the production p = 0.1 it is not: ks is 6.8e-6 above 1 / (1 - p)."""
    assert R.thr16(0.0) == 0 and R.thr16(0.25) == 16384 and R.thr16(0.1) == 6554 and R.thr16(0.2) == 13107
    assert R.thr16(1.0) == 65535 and R.thr16(0.99999) == 65535
    assert R.scale(0.25) == 1 / 0.75 and R.scale(0.0) == 1.0
    gap = R.scale(0.1) / (1 / 0.9) - 1
    assert 6.7e-6 < gap < 6.9e-6 and gap / 2 <= R.KS_GAP_HALF < gap / 2 + 1e-7


@pytest.mark.parametrize("B,L,H,p", [(2, 70, 3, 0.1), (1, 33, 1, 0.25), (3, 97, 2, 0.1)])
def test_mask_layout(B, L, H, p):
    """The packed words (64-bit formulation), `keep_mask` (32-bit formulation) and the scalar transcription agree; the even
    key of a pair is decided by the low half of the pair's word and the odd key by the high half."""
    seed, sid = R.SEED, R.SID
    words = R._attn_decisions_restated(B, L, H, p, seed, sid)
    keep = R.keep_mask(B, L, H, p, seed, sid)
    assert keep.shape == (B, H, L, L) and keep.dtype == bool
    assert np.array_equal(R.unpack_words(words, B, L, H), keep)
    nt = (L + 31) // 32
    assert words.shape == (B * H, nt, nt * 32)
    rng = np.random.default_rng(L)
    thr = R.thr16(p)
    for _ in range(200):
        b, h, q, k = (int(rng.integers(0, n)) for n in (B, H, L, L))
        w = R.word(seed, sid, b * H + h, q, k)
        assert w == R.word(seed, sid, b * H + h, q, k ^ 1)                           # one word per key pair
        half = (w & 0xFFFF) if k % 2 == 0 else (w >> 16)
        assert bool(keep[b, h, q, k]) == (half >= thr) == R.keeps(seed, sid, b * H + h, q, k, p)
        assert bool((int(words[b * H + h, q // 32, k]) >> (q % 32)) & 1) == bool(keep[b, h, q, k])
    # the halves are not interchangeable: deciding every key by its neighbour's half gives the mask with the keys of each pair
    # swapped (and another mask than the right one)
    other = R.decisions(np.arange(B * H), np.arange(L), np.arange(L), p, seed, sid, other_half=True).reshape(B, H, L, L)
    ev = L // 2 * 2
    assert np.array_equal(other[..., 0:ev:2], keep[..., 1:ev:2]) and np.array_equal(other[..., 1:ev:2], keep[..., 0:ev:2])
    assert not np.array_equal(other, keep)


def test_seed_and_stream_id():
    """The mask changes with the low seed word, the high seed word, the stream id and the (protein, head) pair; two
    (seed, sid) that differ only above bit 32 of the seed give different masks."""
    B, L, H, p = 2, 64, 2, 0.25
    base = R.keep_mask(B, L, H, p, R.SEED, R.SID)
    differs = lambda m: 0.2 < (m != base).mean() < 0.6               # noqa: E731  (independent masks: 2 p (1 - p) = 0.375)
    assert differs(R.keep_mask(B, L, H, p, R.SEED ^ 1, R.SID))                       # low word
    assert differs(R.keep_mask(B, L, H, p, R.SEED ^ (1 << 32), R.SID))               # high word
    assert differs(R.keep_mask(B, L, H, p, R.SEED ^ (1 << 63), R.SID))               # its top bit
    assert differs(R.keep_mask(B, L, H, p, R.SEED & 0xFFFFFFFF, R.SID))              # only the bits above 32 differ
    assert differs(R.keep_mask(B, L, H, p, R.SEED, R.SID + 1))
    pairs = base.reshape(B * H, L, L)
    for i in range(B * H):
        for j in range(i):
            assert 0.2 < (pairs[i] != pairs[j]).mean() < 0.6, (i, j)
    # (`decisions` takes any pair index - what the bh + 1 variant of test_discriminating_power relies on)
    assert np.array_equal(R.decisions([1], np.arange(L), np.arange(L), p, R.SEED, R.SID)[0], pairs[1])


@pytest.mark.parametrize("p", R.PS)
def test_kept_fraction(p):
    """Within a binomial 5 sigma of 1 - thr16 / 65536 at 4 x 2 x 200 x 200 = 320000 decisions."""
    keep = R.keep_mask(4, 200, 2, p, R.SEED, R.SID)
    want = 1 - R.thr16(p) / 65536
    sigma = np.sqrt(want * (1 - want) / keep.size)
    print(f"p {p}: kept {keep.mean():.6f}, expected {want:.6f}, sigma {sigma:.2e}")
    assert abs(keep.mean() - want) < 5 * sigma


def plan_shapes():
    return sorted({(dk, B, H, L, tuple(lengths(B, L))) for (dk, B, H, L, _) in pick_cases(CUS).values()})


def test_single_key_proteins():
    """The zero-row assertions of the GPU test are not vacuous: in the odd-length cases, for both p, the proteins of one
    residue have a (protein, head) whose residue drops its only key and one whose residue keeps it (seed R.ODD_SEED, chosen
    here); over all queries of those proteins (the padded ones attend to the same single key) both happen as well - also in
    the plan's cases with the seed the issue fixed, whose protein 1 has one residue."""
    for dk, (_, B, H, L, lens) in R.ODD_CASES.items():
        ones = [b for b, n in enumerate(lens) if n == 1]
        assert len(ones) == 3
        for p in R.PS:
            keep = R.keep_mask(B, L, H, p, R.ODD_SEED, R.SID)
            own = keep[ones, :, 0, 0]
            assert own.any() and not own.all(), (dk, p, own)
            rows = keep[ones, :, :, 0]
            assert rows.any() and not rows.all()
    for dk, B, H, L, lens in plan_shapes():
        assert lens[1] == 1
        for p in R.PS:
            rows = R.keep_mask(B, L, H, p, R.SEED, R.SID)[1, :, :, 0]
            assert rows.any() and not rows.all(), (dk, B, H, L, p)


def wrong_masks(B, L, H, p, seed, sid):
    bh, i = np.arange(B * H), np.arange(L)
    d = lambda *a, **k: R.decisions(*a, p, seed, sid, **k).reshape(B, H, L, L)       # noqa: E731
    return {"keys shifted by one": d(bh, i, i + 1), "keys shifted by one pair": d(bh, i, i + 2),
            "queries shifted by one": d(bh, i + 1, i), "queries shifted by 32": d(bh, i + 32, i),
            "bh + 1": d(bh + 1, i, i), "the other half of each word": d(bh, i, i, other_half=True)}


FAMILIES = ([("plan", *c, R.SEED) for c in plan_shapes()] + [("odd lengths", *c, R.ODD_SEED) for c in R.ODD_CASES.values()] +
            [("arithmetic families", *c[1:], R.SEED) for c in R.FAMILY_CASES if c[0] == "f32"] + [("forced backward", *R.FORCED_CASE, R.SEED)])


def test_discriminating_power():
    """On every shape of the GPU test (the plan's at 256 CUs), fp64 with the right mask against fp64 with a wrong one, held to
    the GPU test's own bars; the margin is the factor by which the bar is exceeded.

      wrong version                          caught by
      keys shifted by one / by one pair      element-wise o (rtol 1e-5, atol 5e-6) and element-wise dQ, dK, dV
      queries shifted by one / by 32         the same
      bh + 1                                 the same
      the other half of each word            the same
      1 / (1 - p) for ks at p = 0.1          NOT element-wise (everything moves by 6.8e-6 relative, inside rtol 1e-5): only
                                             by the norm-wise limit on o, which no arithmetic's limit may exceed 3.4e-6
                                             (R.KS_GAP_HALF) for; the same figure of dQ, dK, dV moves by 6.8e-6 too
    """
    margins, missed = {}, []
    for family, dk, B, H, L, lens, seed in FAMILIES:
        seq, qkv, dout = R.host_inputs(dk, B, H, L, lens)
        key_ok = seq != 20
        for p in R.PS:
            right = R.keep_mask(B, L, H, p, seed, R.SID)
            o, _, d = R.reference(qkv, dout, key_ok, H, right, R.scale(p))
            atol = R.D_ATOL * max(1.0, d.abs().max().item())
            for name, keep in wrong_masks(B, L, H, p, seed, R.SID).items():
                assert (keep != right).any(), name
                ow, _, dw = R.reference(qkv, dout, key_ok, H, keep, R.scale(p))
                mo = R.excess(ow, o, *R.O_BAR)
                md = [R.excess(dw[:, i], d[:, i], R.D_RTOL, atol) for i in range(3)]
                print(f"{family} dk {dk} {B} x {L} x {H} p {p}: {name:28s} o x{mo:9.1f}   dQ x{md[0]:9.1f} dK x{md[1]:9.1f} dV x{md[2]:9.1f}")
                if not (mo > 1 and max(md) > 1):
                    missed.append((family, dk, B, H, L, p, name, mo, md))
                margins[name] = min(margins.get(name, np.inf), mo, max(md))
            if p == 0.1:
                ow, _, dw = R.reference(qkv, dout, key_ok, H, right, 1 / (1 - p))
                assert R.excess(ow, o, *R.O_BAR) < 1 and all(R.excess(dw[:, i], d[:, i], R.D_RTOL, atol) < 1 for i in range(3))
                m = [R.rel_l2(ow, o) / R.KS_GAP_HALF] + [R.rel_l2(dw[:, i], d[:, i]) / R.KS_GAP_HALF for i in range(3)]
                print(f"{family} dk {dk} {B} x {L} x {H} p {p}: 1 / (1 - p) for ks: element-wise inside the bars; relative L2 over "
                      f"3.4e-6: o x{m[0]:.3f} dQ x{m[1]:.3f} dK x{m[2]:.3f} dV x{m[3]:.3f}")
                if not m[0] > 1.99:
                    missed.append((family, dk, B, H, L, p, "ks", m))
                margins["1 / (1 - p) for ks"] = min(margins.get("1 / (1 - p) for ks", np.inf), m[0])
    for name, m in margins.items():
        print(f"smallest margin, {name:28s} x{m:.3f}")
    assert not missed, missed
    assert len(margins) == 7 and min(m for n, m in margins.items() if n != "1 / (1 - p) for ks") > 10
