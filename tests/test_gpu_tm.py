"""TM-score and GDT on the device (csrc/tmscore.hip) against tests/tm_ref.py on the same fp32 inputs.

Bars.
  counts   exactly the reference's.  Every case has min_margin >= 1e-9 A and min_rank >= 1e-3 (tests/test_tm_ref.py checks that on
           the CPU): no distance of any visited superposition lies within 1e-9 A of a threshold, while the two fp64 routes
           (quaternion + Jacobi here, SVD there) differ by ~1e-13 A - a correct kernel makes the reference's decisions.
  score    |kernel - reference| <= 2^-22.  A score is a mean of N terms in [0,1] (or a ratio of small integers) formed in fp64
           and rounded ONCE to fp32: half an fp32 ulp at 1 is 2^-24; the bar is four ulps at 1.
  xform    a proper rotation: |R^T R - I| <= 1e-6 (fp32 storage of entries <= 1: 6e-8 each), det > 0.
  re-score applying xform to the prediction and scoring in numpy fp64 gives tm within 1e-5: R is stored in fp32 (6e-8 relative),
           which moves a point at 1e3 A from the origin by up to ~1e-4 A, and |dTM/dd| <= 1/d0 per residue with d0 >= 0.5.
The printed figures are the measured errors (profiles/tm/NOTES.md records them)."""
import numpy as np
import pytest
import torch

import tm_ref as T

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCORE_BAR = 2.0 ** -22
POISON_F, POISON_I = 777.0, -777


def run(pred, true, seq):
    """numpy batch -> (score [B,3], counts [B,6], xform [B,3,4]) as numpy."""
    from protein_transformer_amd.eval_metrics import tm_batch
    out = tm_batch(torch.from_numpy(pred).to(DEV), torch.from_numpy(true).to(DEV), torch.from_numpy(seq).to(DEV))
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def check_protein(name, score, counts, xform, pred, true, seq, ref):
    assert np.array_equal(counts, ref["counts"]), (name, counts, ref["counts"])
    err = np.abs(score.astype(np.float64) - ref["score"]).max()
    R, t = xform[:, :3].astype(np.float64), xform[:, 3].astype(np.float64)
    ortho = np.abs(R.T @ R - np.eye(3)).max()
    p, q = T.ca_pairs(pred, true, seq)
    again = T.tm_of(T.distances(R, t, p, q), T.d0_of(len(p)))
    print(f"{name}: N {counts[0]}  score err {err:.2e}  |RtR - I| {ortho:.2e}  det {np.linalg.det(R):+.7f}  "
          f"re-scored tm err {abs(again - ref['score'][0]):.2e}  (margin {ref['min_margin']:.1e}, rank {ref['min_rank']:.1e})")
    assert err <= SCORE_BAR, (name, score, ref["score"])
    assert ortho <= 1e-6 and np.linalg.det(R) > 0, (name, R)
    assert abs(again - ref["score"][0]) <= 1e-5, (name, again, ref["score"][0])


@pytest.mark.parametrize("name", list(T.GPU_CASES))
def test_against_the_reference(name):
    pred, true, seq, ref = T.case_with_reference(name)
    score, counts, xform = run(pred[None], true[None], seq[None])
    check_protein(name, score[0], counts[0], xform[0], pred, true, seq, ref)
    if name == "rigid1e3":
        assert np.all(np.abs(score[0] - 1.0) <= SCORE_BAR) and np.all(counts[0] == counts[0][0])
    again = run(pred[None], true[None], seq[None])                       # two calls: the same bits
    for a, b in zip((score, counts, xform), again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), name


def test_ragged_batch():
    """B = 3: 65 residues, 20 residues, all padding - a protein's result does not depend on the batch around it."""
    names = ("walk65", "walk20")
    cases = [T.case_with_reference(n)[:3] for n in names]
    empty = (np.zeros((4 * T.NUM_SLOTS, 3), np.float32), np.zeros((4 * T.NUM_SLOTS, 3), np.float32), np.full(4, T.PAD_ID, np.int64))
    pred, true, seq = T.stack(cases + [empty])
    score, counts, xform = run(pred, true, seq)
    for b, n in enumerate(names):
        ref = T.case_with_reference(n)[3]
        check_protein(f"ragged/{n}", score[b], counts[b], xform[b], pred[b], true[b], seq[b], ref)
        alone = run(*(a[None] for a in T.case_with_reference(n)[:3]))
        assert np.array_equal(score[b].view(np.int32), alone[0][0].view(np.int32)) and np.array_equal(counts[b], alone[1][0])
        assert np.array_equal(xform[b].view(np.int32), alone[2][0].view(np.int32))
    assert np.isnan(score[2]).all() and np.array_equal(counts[2], [0] * 6) and np.isnan(xform[2]).all()


def test_unscorable_proteins_are_nan():
    """N = 2, and a NaN (an infinite) prediction on a present C-alpha: NaN scores, counts {N,0,0,0,0,0}, NaN transform - and the
    protein beside them is untouched."""
    good = T.case_with_reference("walk9")
    two = T.noisy_chain(2, 5)
    nanp = tuple(a.copy() for a in T.case_with_reference("walk8")[:3])
    nanp[0][3 * T.NUM_SLOTS + T.CA_SLOT, 1] = np.nan
    infp = tuple(a.copy() for a in T.case_with_reference("walk8")[:3])
    infp[0][0 * T.NUM_SLOTS + T.CA_SLOT, 2] = np.inf
    pred, true, seq = T.stack([two, nanp, good[:3], infp])
    score, counts, xform = run(pred, true, seq)
    for b, n in ((0, 2), (1, 8), (3, 8)):
        assert T.tm_ref(pred[b], true[b], seq[b])["counts"].tolist() == [n, 0, 0, 0, 0, 0]          # the reference says the same
        assert np.isnan(score[b]).all() and counts[b].tolist() == [n, 0, 0, 0, 0, 0] and np.isnan(xform[b]).all(), b
    check_protein("beside NaN", score[2], counts[2], xform[2], pred[2], true[2], seq[2], good[3])
    # what the prediction holds anywhere but on a present C-alpha decides nothing
    pred2 = pred[2:3].copy()
    slots = pred2.reshape(1, -1, T.NUM_SLOTS, 3)
    slots[:, :, :T.CA_SLOT], slots[:, :, T.CA_SLOT + 1:] = np.nan, np.inf
    got = run(pred2, true[2:3], seq[2:3])
    assert np.array_equal(got[1][0], counts[2]) and np.array_equal(got[0][0].view(np.int32), score[2].view(np.int32))


def test_every_output_is_written_and_nothing_else():
    """Poisoned workspace, poisoned outputs with guard bands: every output element is written, nothing beyond them is, and the
    poison in the workspace changes no bit.  Also the NULL xform form."""
    from protein_transformer_amd import _lib
    lib = _lib.lib()
    cases = [T.case_with_reference(n)[:3] for n in ("walk64", "walk5")] + [T.noisy_chain(2, 5)]
    pred, true, seq = (torch.from_numpy(a).to(DEV) for a in T.stack(cases))
    B, L = seq.shape
    need = lib.ptamd_tm_workspace_bytes(B, L)
    G = 64                                                                           # guard elements on both sides
    results = []
    for fill, with_xform in ((0x00, True), (0xFF, True), (0x5A, False)):
        ws = torch.full((need + 512,), fill, dtype=torch.uint8, device=DEV)
        score = torch.full((G + B * 3 + G,), POISON_F, dtype=torch.float32, device=DEV)
        counts = torch.full((G + B * 6 + G,), POISON_I, dtype=torch.int32, device=DEV)
        xform = torch.full((G + B * 12 + G,), POISON_F, dtype=torch.float32, device=DEV)
        rc = lib.ptamd_tm_score(_lib.ptr(pred), _lib.ptr(true), _lib.ptr(seq), B, L, _lib.ptr(score[G:]), _lib.ptr(counts[G:]),
                                _lib.ptr(xform[G:]) if with_xform else None, _lib.ptr(ws[256:]), need, _lib.stream())
        assert rc == 0
        torch.cuda.synchronize()
        for t, n, poison in ((score, B * 3, POISON_F), (counts, B * 6, POISON_I), (xform, B * 12, POISON_F)):
            assert (t[:G] == poison).all() and (t[G + n:] == poison).all()           # nothing in front, nothing behind
            body = t[G:G + n]
            if t is xform and not with_xform:
                assert (body == poison).all()
            else:
                assert not (body == poison).any()                                    # (NaN != poison: a NaN output counts as written)
        assert (ws[:256] == fill).all() and (ws[256 + need:] == fill).all()          # the workspace's bounds are respected
        results.append((score[G:G + B * 3].cpu().numpy(), counts[G:G + B * 6].cpu().numpy(), xform[G:G + B * 12].cpu().numpy()))
    for r in results[1:]:
        assert np.array_equal(r[0].view(np.int32), results[0][0].view(np.int32)) and np.array_equal(r[1], results[0][1])
    assert np.array_equal(results[1][2].view(np.int32), results[0][2].view(np.int32))
    assert np.array_equal(results[0][1].reshape(B, 6)[0], T.case_with_reference("walk64")[3]["counts"])
    assert np.isnan(results[0][0].reshape(B, 3)[2]).all() and results[0][1].reshape(B, 6)[2].tolist() == [2, 0, 0, 0, 0, 0]


def test_get_losses_reports_the_three_scores():
    """`--eval_tm` through get_losses(eval_mode=True): the three keys are the finite means of tm_batch on the coordinates it built;
    without the flag the dictionary is, key for key and bit for bit, the one of before; training steps never carry the keys."""
    from test_gpu_clash_train import _setup
    from protein_transformer_amd.eval_metrics import batch_tm, tm_batch
    from protein_transformer_amd.losses import angles_forward
    from protein_transformer_amd.protein.Structure import nerf_forward
    from protein_transformer_amd.train import get_losses
    model, _, args, batch = _setup("drmsd")
    seq, ang, crd = (t.to(DEV) for t in batch)
    model.eval()
    kw = dict(do_backwards=False, eval_mode=True, return_rmsd=True)
    with torch.no_grad():
        pred = model(seq, ang)
        plain = get_losses(args, pred, ang, crd, seq, **kw)
        args.eval_tm = False
        off = get_losses(args, pred, ang, crd, seq, **kw)
        args.eval_tm = True
        on = get_losses(args, pred, ang, crd, seq, **kw)
        train = get_losses(args, pred, ang, crd, seq, do_backwards=False)
        built, _ = nerf_forward(angles_forward(pred.detach().float().contiguous().view(*seq.shape, -1)), seq)
        score = tm_batch(built, crd, seq)[0].cpu().numpy().astype(np.float64)
        means = batch_tm(pred, crd, seq)
    assert list(off) == list(plain) and not any(k in plain for k in ("tm-ca", "gdt-ts", "gdt-ha"))
    assert list(on) == list(plain) + ["tm-ca", "gdt-ts", "gdt-ha"] and list(train) == [k for k in plain]
    for k in plain:
        a, b, c = (np.float64(d[k]) for d in (plain, off, on))
        assert a.tobytes() == b.tobytes() == c.tobytes(), k
    assert np.isfinite(score).all() and (score > 0).all() and (score <= 1).all()
    for j, k in enumerate(("tm-ca", "gdt-ts", "gdt-ha")):
        assert on[k] == score[:, j].mean() and abs(means[j] - on[k]) <= 1e-12, (k, on[k], score[:, j])
