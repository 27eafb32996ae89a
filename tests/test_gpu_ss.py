"""Secondary-structure agreement on the device (csrc/dssp.hip) against tests/ss_ref.py on the same fp32 inputs.

Bars.  Everything the kernel returns is an integer, or a ratio of two of its integers rounded once to fp32, so everything is
compared EXACTLY: the bond bits of both structures, the states, the confusion counts, the scores.  The condition is the one
tests/test_ss_ref.py shows on the CPU for every fixture used here: no candidate pair's fp64 energy lies within ss_ref.BAND
(2e-3 kcal/mol, derived there from fp32 rounding at coordinates within +-64 A) of the threshold -0.5."""
import numpy as np
import pytest
import torch

import ss_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def run(pred, true, seq):
    """numpy batch -> (score [B,3], confusion [B,3,3], states [B,L,2], hb [B,2,L,L] bool) as numpy."""
    from protein_transformer_amd.eval_metrics import ss_batch
    score, conf, states, bits = ss_batch(torch.from_numpy(pred).to(DEV), torch.from_numpy(true).to(DEV),
                                         torch.from_numpy(seq).to(DEV), hbonds=True)
    torch.cuda.synchronize()
    B, L = seq.shape
    words = bits.cpu().numpy().view(np.uint64)
    hb = np.stack([np.stack([R.unpack_bits(words[b, s], L) for s in (0, 1)]) for b in range(B)])
    return score.cpu().numpy(), conf.cpu().numpy(), states.cpu().numpy(), hb


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check_protein(name, got, b, pred, true, seq):
    """Protein b of the batch result `got` against the reference of (pred, true, seq), rows possibly padded beyond len(seq)."""
    score, conf, states, hb = (x[b] for x in got)
    L = len(seq)
    ref = R.reference(pred, true, seq)
    assert not hb[:, L:].any() and not hb[:, :, L:].any() and (states[L:] == -1).all(), name          # nothing in the padding
    for s, which in enumerate(("pred", "true")):
        if ref["bad"] and s == 0:                # (the bond bits of a prediction that is not finite are unspecified)
            continue
        diff = np.argwhere(hb[s, :L, :L] != ref["hb"][s])
        assert diff.size == 0, (name, which, diff[:8].tolist())
        # the reference's pattern logic applied to the kernel's OWN bits
        own = R.states_from_bits(hb[s, :L, :L], ref["present"])
        assert np.array_equal(states[:L, s], own), (name, which)
    assert np.array_equal(states[:L], ref["states"]), (name, states[:L].T, ref["states"].T)
    assert np.array_equal(conf, R.confusion_of(states[:L], ref["present"], ref["bad"])) and np.array_equal(conf, ref["confusion"]), name
    want = R.scores_of(conf, ref["bad"])
    assert same_bits(np.nan_to_num(score, nan=-1.0), np.nan_to_num(want, nan=-1.0)), (name, score, want)
    assert np.array_equal(np.isnan(score), np.isnan(ref["score"])), (name, score, ref["score"])
    return ref


@pytest.fixture(scope="module")
def fixtures_run():
    items = list(R.cases().items())
    batch = R.batch_of([v for _, v in items])
    return items, batch, run(*batch)


def test_bits_states_counts_scores_on_every_fixture(fixtures_run):
    items, batch, got = fixtures_run
    for b, (name, (pred, true, seq)) in enumerate(items):
        ref = check_protein(name, got, b, pred, true, seq)
        print(name, "score", got[0][b], "bonds", int(ref["hb"][0].sum()), int(ref["hb"][1].sum()))
    by = {name: got[2][b][:len(v[2]), 1] for b, (name, v) in enumerate(items)}
    assert (by["helix"][1:-1] == R.ST_H).all() and (by["anti"] == R.ST_E).sum() == 12 and (by["par"] == R.ST_E).sum() == 12
    names = [n for n, _ in items]
    assert np.isnan(got[0][names.index("helix")][2]) and np.isnan(got[0][names.index("anti")][1])     # no true E / no true H


def test_determinism_and_batch_independence(fixtures_run):
    """Two runs give the same bits; a protein alone, in a row cut to its own length, and at another batch position padded
    further, gives what it gave in the batch."""
    items, batch, got = fixtures_run
    again = run(*batch)
    for a, b in zip(got, again):
        assert same_bits(a, b)
    for b in (1, 3):
        name, (pred, true, seq) = items[b]
        L = len(seq)
        alone = run(pred[None], true[None], seq[None])
        moved = run(*R.batch_of([items[0][1], items[2][1], (pred, true, seq)], L_pad=70))
        for k in (alone, moved):
            at = 0 if k is alone else 2
            assert same_bits(np.nan_to_num(k[0][at], nan=-1.0), np.nan_to_num(got[0][b], nan=-1.0)), name
            assert np.array_equal(k[1][at], got[1][b]) and np.array_equal(k[2][at][:L], got[2][b][:L]), name
            assert np.array_equal(k[3][at][:, :L, :L], got[3][b][:, :L, :L]), name


def test_tile_edges():
    """L = 63, 64, 65, 128, 129 in one batch, rows padded to 129: three tiles per row, bonds across residue 64 in both
    directions and across residue 128."""
    cases = R.edge_cases()
    got = run(*R.batch_of(list(cases.values())))
    up = down = far = 0
    for b, (L, (pred, true, seq)) in enumerate(cases.items()):
        ref = check_protein(f"edge{L}", got, b, pred, true, seq)
        i, j = np.nonzero(got[3][b][1])
        up, down, far = up + ((i < 64) & (j >= 64)).sum(), down + ((j < 64) & (i >= 64)).sum(), far + ((i < 128) & (j >= 128)).sum()
        assert (ref["states"][:, 1] == R.ST_E).sum() >= 12 and (ref["states"][:, 1] == R.ST_H).sum() >= 14
    assert up > 0 and down > 0 and far > 0


def test_edges_of_the_definition():
    """A chain break, a fully padded row, a one-residue protein, a NaN prediction, poison in absent slots and in the padding."""
    ht, hs = R.helix_case(24)
    hp = R.noised(ht, 22)
    broken = ht.copy()
    broken[10 * R.NUM_SLOTS + R.SLOT_C, 1] = np.nan                  # one backbone atom of residue 10 missing in the truth
    nanpred = hp.copy()
    nanpred[5 * R.NUM_SLOTS + R.SLOT_O, 2] = np.nan                  # a present residue without a usable prediction
    infpred = hp.copy()
    infpred[7 * R.NUM_SLOTS + R.SLOT_N, 0] = np.inf
    one = (hp[:R.NUM_SLOTS], ht[:R.NUM_SLOTS], hs[:1])
    empty = (np.zeros((3 * R.NUM_SLOTS, 3), np.float32), np.zeros((3 * R.NUM_SLOTS, 3), np.float32), np.full(3, R.PAD_ID, np.int64))
    items = [(hp, broken, hs), (hp, ht, hs), (nanpred, ht, hs), empty, one, (infpred, ht, hs), (hp, ht, hs)]
    pred, true, seq = R.batch_of(items, L_pad=30)
    got = run(pred, true, seq)
    for b, (p, t, s) in enumerate(items):
        check_protein(f"edge/{b}", got, b, p, t, s)
    score, conf, states, hb = got
    # the break: residue 10 is absent from BOTH structures, residue 11 has no H (no donor), no turn spans the break
    assert (states[0][10] == -1).all() and not hb[0][:, 10].any() and not hb[0][:, :, 10].any() and not hb[0][:, :, 11].any()
    # (the bond 8 -> 12 exists on both sides of the break - 12 has an H - but is no turn: every turn that could put residue 9
    # in a helix spans residue 10)
    assert hb[0][1, 8, 12] and hb[1][1, 8, 12] and states[1][9, 1] == R.ST_H and states[0][9, 1] != R.ST_H
    assert (states[1][1:23, 1] == R.ST_H).all() and conf[0].sum() == 23 and conf[1].sum() == 24
    # NaN / infinite prediction on a present residue: NaN scores, no counts, no predicted string; the neighbours are untouched
    for b in (2, 5):
        assert np.isnan(score[b]).all() and not conf[b].any() and (states[b][:, 0] == -1).all()
        assert np.array_equal(states[b][:24, 1], states[1][:24, 1]) and np.array_equal(hb[b][1], hb[1][1])
    assert same_bits(score[1], score[6]) and np.array_equal(conf[1], conf[6]) and np.array_equal(hb[1], hb[6])
    # a fully padded row and a one-residue protein
    assert np.isnan(score[3]).all() and not conf[3].any() and (states[3] == -1).all() and not hb[3].any()
    assert score[4][0] == 1.0 and np.isnan(score[4][1:]).all() and conf[4].tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, 1]]
    # poison: in the absent residue of the truth's row, in every pad residue, in the side chains - no bit moves
    pred2, true2 = pred.copy(), true.copy()
    pad = np.repeat(seq == R.PAD_ID, R.NUM_SLOTS, axis=1)
    pred2[pad], true2[pad] = np.nan, 1e30
    pred2[0, 10 * R.NUM_SLOTS:11 * R.NUM_SLOTS] = np.inf
    true2[0, 10 * R.NUM_SLOTS + 4:11 * R.NUM_SLOTS] = -1e30
    side = np.tile(np.arange(R.NUM_SLOTS) >= 4, seq.shape[1])
    pred2[:, side] = np.nan
    again = run(pred2, true2, seq)
    for a, b in zip(got, again):
        assert same_bits(a, b)


def test_workspace_guard_band_and_null_outputs():
    """A poisoned workspace between guard bands, poisoned outputs between guard bands: every output element is written, nothing
    beyond; with `hbonds` NULL the bits live in the workspace and the results are the same; `states` may be NULL too."""
    from protein_transformer_amd import _lib
    lib = _lib.lib()
    cases = R.edge_cases()
    pred, true, seq = (torch.from_numpy(a).to(DEV) for a in R.batch_of([cases[65], cases[63], R.cases()["anti"]]))
    B, L = seq.shape
    W = (L + 63) // 64
    need = lib.ptamd_ss_workspace_bytes(B, L)
    G = 64
    results = []
    for fill, with_states, with_bits in ((0x00, True, True), (0xFF, True, False), (0x5A, False, True), (0xA5, False, False)):
        ws = torch.full((need + 512,), fill, dtype=torch.uint8, device=DEV)
        score = torch.full((G + B * 3 + G,), 777.0, dtype=torch.float32, device=DEV)
        conf = torch.full((G + B * 9 + G,), -777, dtype=torch.int32, device=DEV)
        states = torch.full((G + B * L * 2 + G,), 77, dtype=torch.int8, device=DEV)
        bits = torch.full((G + B * 2 * L * W + G,), 0x7777777777777777, dtype=torch.int64, device=DEV)
        rc = lib.ptamd_ss(_lib.ptr(pred), _lib.ptr(true), _lib.ptr(seq), B, L, _lib.ptr(score[G:]), _lib.ptr(conf[G:]),
                          _lib.ptr(states[G:]) if with_states else None, _lib.ptr(bits[G:]) if with_bits else None,
                          _lib.ptr(ws[256:]), need, _lib.stream())
        assert rc == 0
        torch.cuda.synchronize()
        for t, n, poison, used in ((score, B * 3, 777.0, True), (conf, B * 9, -777, True), (states, B * L * 2, 77, with_states),
                                   (bits, B * 2 * L * W, 0x7777777777777777, with_bits)):
            assert (t[:G] == poison).all() and (t[G + n:] == poison).all()           # nothing in front, nothing behind
            body = t[G:G + n]
            assert (body == poison).all() if not used else not (body == poison).any()
        assert (ws[:256] == fill).all() and (ws[256 + need:] == fill).all()          # the workspace's bounds are respected
        results.append((score[G:G + B * 3].cpu().numpy(), conf[G:G + B * 9].cpu().numpy()))
    for r in results[1:]:
        assert same_bits(r[0], results[0][0]) and np.array_equal(r[1], results[0][1])
    assert np.array_equal(results[0][1].reshape(B, 3, 3)[0], R.reference(*cases[65])["confusion"])
    assert lib.ptamd_ss(_lib.ptr(pred), _lib.ptr(true), _lib.ptr(seq), B, L, _lib.ptr(score), _lib.ptr(conf), None, None,
                        _lib.ptr(ws[256:]), need - 1, _lib.stream()) == -3


def test_get_losses_reports_the_three_scores(monkeypatch):
    """`--eval_ss` through get_losses(eval_mode=True): the three keys are the finite means of ss_batch on the coordinates it built;
    without the flag the dictionary is, key for key and bit for bit, the one of before and the kernel is never called; training
    steps never carry the keys."""
    from test_gpu_clash_train import _setup
    from protein_transformer_amd import eval_metrics, train
    from protein_transformer_amd.eval_metrics import ss_batch
    from protein_transformer_amd.losses import angles_forward, finite_mean
    from protein_transformer_amd.protein.Structure import nerf_forward
    calls = []               # (get_losses reaches the kernel through the record of eval_metrics.EVAL_METRICS, which calls this name)
    monkeypatch.setattr(eval_metrics, "ss_batch", lambda *a, **k: calls.append(1) or ss_batch(*a, **k))
    model, _, args, batch = _setup("drmsd")
    seq, ang, crd = (t.to(DEV) for t in batch)
    model.eval()
    kw = dict(do_backwards=False, eval_mode=True, return_rmsd=True)
    with torch.no_grad():
        pred = model(seq, ang)
        plain = train.get_losses(args, pred, ang, crd, seq, **kw)
        args.eval_ss = False
        off = train.get_losses(args, pred, ang, crd, seq, **kw)
        assert not calls
        args.eval_ss = True
        on = train.get_losses(args, pred, ang, crd, seq, **kw)
        assert len(calls) == 1
        steps = train.get_losses(args, pred, ang, crd, seq, do_backwards=False)
        assert len(calls) == 1                                        # a training step launches nothing
        args.backbone_loss = True
        bb = train.get_losses(args, pred, ang, crd, seq, **kw)
        built, _ = nerf_forward(angles_forward(pred.detach().float().contiguous().view(*seq.shape, -1)), seq)
        score = ss_batch(built, crd, seq)[0].cpu().numpy()
    keys = ["ss-q3", "ss-h", "ss-e"]
    assert list(off) == list(plain) and not any(k in plain for k in keys)
    assert list(on) == list(plain) + keys and list(steps) == list(plain)
    for k in plain:
        a, b, c = (np.float64(d[k]) for d in (plain, off, on))
        assert a.tobytes() == b.tobytes() == c.tobytes(), k
    assert np.isfinite(score[:, 0]).all()
    for j, k in enumerate(keys):
        want = finite_mean(score[:, j])
        assert (np.isnan(on[k]) and np.isnan(want)) or on[k] == want, (k, on[k], score[:, j])
        assert (np.isnan(bb[k]) and np.isnan(want)) or bb[k] == want, k
