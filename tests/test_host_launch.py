"""CPU-only tests of the host launch layer (protein_transformer_amd/kernels.py): the pure plan of the one-pass weight
preparation, the deferred-reduce rule and the job-array launcher.  No device, no library."""
import numpy as np
import pytest

from protein_transformer_amd import kernels as K
from protein_transformer_amd._lib import FILL_JOB_CAP, FillJob, WprepBound, WprepSeg

RB, PF = 32, 4 * 4096                 # csrc/wprep.hip: RB, 4 * PLAIN_F4 (what the two ptamd_wprep_* getters return)
CASES = {"d64_f128": (64, 128), "d64_f1024": (64, 1024), "d512_f2048": (512, 2048)}       # (d_model, d_ff); 2 layers each


def encoder_description(D, F, nlayers=2):
    """(numel, segs, groups, nstats) as EncoderOnlyTransformer._build_prep describes its weights, with integers for the views:
    scales are indices into the int32 pool in the order `_step_scales` takes them, planes are made-up addresses, the flat
    buffer holds an embedding, the layers' parameters in module order and an output projection."""
    Fp = -(-F // 128) * 128
    segs, groups, pos, o = [], [], 24 * D, 0
    plane = iter(range(0x7F0000000000, 0x7F8000000000, 1 << 28))

    def take(n):
        nonlocal o
        o += n
        return o - n

    def put(n):
        nonlocal pos
        pos += n
        return pos - n
    for i in range(nlayers):
        rs_qkv, cs_qkv, rs_o, cs_o, rs_1, cs_1, rs_2, cs_2 = (take(n) for n in (3 * D, D, D, D, Fp, D, D, F))
        att, f1, h1, h2, _dqkv = (take(4) for _ in range(5))
        wqkv, bqkv, wo, _bo, g0, b0 = put(3 * D * D), put(3 * D), put(D * D), put(D), put(D), put(D)
        w1, b1, w2, _b2, g1, be1 = put(F * D), put(F), put(D * F), put(D), put(D), put(D)
        r = lambda k, i=i: 9 * i + k                                                                   # noqa: E731
        segs += [dict(offset=wqkv, rows=3 * D, cols=D, row_scale=rs_qkv, col_scale=cs_qkv, stats=r(0), stats_row0=2 * D,
                      row_planes=next(plane)),
                 dict(offset=bqkv + 2 * D, rows=1, cols=D, stats=r(7)),
                 dict(offset=wo, rows=D, cols=D, row_scale=rs_o, col_scale=cs_o),
                 dict(offset=w1, rows=F, cols=D, row_scale=rs_1, col_scale=cs_1, stats=r(1), row_planes=next(plane)),
                 dict(offset=b1, rows=1, cols=F, stats=r(8)),
                 dict(offset=w2, rows=D, cols=F, row_scale=rs_2, col_scale=cs_2, stats=r(2), colnorm=True, col_planes=next(plane)),
                 dict(offset=g0, rows=1, cols=D, stats=r(3)), dict(offset=b0, rows=1, cols=D, stats=r(4)),
                 dict(offset=g1, rows=1, cols=D, stats=r(5)), dict(offset=be1, rows=1, cols=D, stats=r(6))]
        sq = D ** 0.5
        groups.append([dict(ln_gamma=r(3), ln_beta=r(4), w=r(0), w_index=0, bias=r(7), sqrt_d=sq, post_scale=1.0 / 0.9, out_scale=att),
                       dict(ln_gamma=r(5), ln_beta=r(6), w=r(1), w_index=0, bias=r(8), sqrt_d=sq, post_scale=1.0 / 0.9, out_scale=f1),
                       dict(w=r(2), w_index=1, post_scale=1.0 / 0.9, out_value=4 * i + 2),
                       dict(ln_gamma=r(3), ln_beta=r(4), w=-1, w_index=0, sqrt_d=sq, out_scale=h1),
                       dict(ln_gamma=r(5), ln_beta=r(6), w=-1, w_index=0, sqrt_d=sq, out_scale=h2)])
    return pos + 24 * D + 24, segs, groups, 9 * nlayers


def uploaded(p):
    """The tables of a plan as WeightsPrep.__init__ uploads them (the padding of empty tables included)."""
    return dict(segs=np.frombuffer(bytes((WprepSeg * len(p["segs"]))(*p["segs"])), dtype=np.uint8),
                blocks_a=np.asarray(p["blocks_a"], dtype=np.int32).reshape(-1, 2),
                plain=np.asarray(p["plain"] if p["plain"] else [(0, 0)], dtype=np.int64).reshape(-1, 2),
                blocks_b=np.asarray(p["blocks_b"], dtype=np.int32).reshape(-1, 4),
                bounds=np.frombuffer(bytes((WprepBound * max(len(p["bounds"]), 1))(*p["bounds"])), dtype=np.uint8),
                groups=np.asarray(p["groups"], dtype=np.int32).reshape(-1, 4),
                colnorm=np.asarray(p["colnorm"] if p["colnorm"] else [0], dtype=np.int32),
                counts=np.asarray([len(p["segs"]), len(p["blocks_a"]), p["n_matrix_blocks"], len(p["plain"]), len(p["blocks_b"]),
                                   len(p["bounds"]), max(p["ncolmax"], 1), max(p["ncolsq"], 2)], dtype=np.int64))


@pytest.mark.parametrize("case", sorted(CASES))
def test_wprep_plan_of_the_encoder(case):
    D, F = CASES[case]
    numel, segs, groups, _ = encoder_description(D, F)
    p = K.wprep_plan(numel, segs, groups, RB, PF)
    table, plain, blocks_a = p["segs"], p["plain"], p["blocks_a"]
    # blocks_a: every row block of every panel once, the matrices first, then every block of every plain range once
    # (entries that kernel B alone reads - a panelled matrix as a whole, kinds 3 and 1 of blocks_b - are not in blocks_a)
    whole = {k for kind, k, _, _ in p["blocks_b"] if kind in (1, 3)}
    panels = [k for k in range(len(table)) if k not in whole]
    assert len(table) == 2 * (10 + (-(-F // 512) - 1) * 2 + 1) and len(whole) == 2
    assert blocks_a[:p["n_matrix_blocks"]] == [(k, b) for k in panels for b in range(-(-table[k].rows // RB))]
    assert blocks_a[p["n_matrix_blocks"]:] == [(-(j + 1), b) for j, (_, n) in enumerate(plain) for b in range(-(-n // PF))]
    # the plain ranges and the segments of the description tile [0, numel) exactly once; so do the plain ranges and the panels
    cover = sorted(plain + [(s["offset"], s["rows"] * s["cols"]) for s in segs])
    assert cover[0][0] == 0 and all(a + n == b for (a, n), (b, _) in zip(cover, cover[1:] + [(numel, 0)]))
    covered = np.zeros(numel, dtype=np.int8)
    for first, n in plain:
        covered[first:first + n] += 1
    for k in panels:
        t = table[k]
        rows = t.offset + np.arange(t.rows)[:, None] * t.ld + np.arange(t.cols)[None, :]
        np.add.at(covered, rows.ravel(), 1)
    assert (covered == 1).all()
    # pool of maxima: the columns of the four matrices of a layer (+ the rows of W2 where it is panelled); colsq: W2's
    # columns per row block
    assert p["ncolmax"] == 2 * (3 * D + F + (D if F > 512 else 0))
    assert p["ncolsq"] == 2 * -(-D // RB) * F
    assert len(p["bounds"]) == 10 and p["groups"] == [(0, 5, 0, -(-F // 512)), (5, 5, -(-F // 512), -(-F // 512))]
    assert all(table[k].colsq_index >= 0 for k in p["colnorm"])


def test_wprep_plan_golden(golden):
    """Byte for byte the tables WeightsPrep.__init__ built and uploaded before the plan was split off.  golden/wprep_plan.npz
    holds the t_* tensors and counts of that constructor (commit 0e25cc2) for the three descriptions above, run on CPU tensors
    (views of an int32 / a float pool at the indices above, objects with the addresses above as planes) with the two block
    sizes of csrc/wprep.hip in place of the library's getters: profiles/host_launch/NOTES.md."""
    g = golden("wprep_plan")
    for case, (D, F) in CASES.items():
        numel, segs, groups, _ = encoder_description(D, F)
        for name, got in uploaded(K.wprep_plan(numel, segs, groups, RB, PF)).items():
            want = g[f"{case}.{name}"]
            assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), (case, name)


@pytest.mark.parametrize("seg,job,message", [
    (dict(offset=0, rows=8, cols=6), None, "segment (offset 0, 8 x 6) is not representable"),
    (dict(offset=2, rows=8, cols=8), None, "segment (offset 2, 8 x 8) is not representable"),
    (dict(offset=0, rows=8, cols=768), None, "segment (offset 0, 8 x 768) is not representable"),
    (dict(offset=0, rows=16, cols=64, row_planes=4096), None, "planes need rows and cols that are multiples of 32"),
    (dict(offset=0, rows=32, cols=64, col_planes=4096), None, "col_planes need col_scale"),
    (dict(offset=0, rows=32, cols=64, col_scale=0, colnorm=True), None, "colnorm needs a statistics record and col_scale"),
    (dict(offset=0, rows=32, cols=1024, stats=0, stats_row0=16), None,
     "a matrix wider than 512 columns cannot have row planes or a statistics sub-range"),
    (dict(offset=0, rows=32, cols=1024, row_planes=4096), None,
     "a matrix wider than 512 columns cannot have row planes or a statistics sub-range"),
    (dict(offset=0, rows=32, cols=1024, stats=0), dict(w=0, w_index=0, out_scale=0),
     "a bound job reads the row norm of a matrix wider than 512 columns, which the pass does not compute"),
    (dict(offset=0, rows=32, cols=1024, stats=0), dict(w=1, w_index=1, ln_beta=0, out_scale=0),
     "a bound job reads the row norm of a matrix wider than 512 columns, which the pass does not compute"),
    (dict(offset=0, rows=32, cols=64), (), "at least one bounds group (it also resets the statistics)")])
def test_wprep_plan_refusals(seg, job, message):
    groups = [] if job == () else [[job or dict(w=0, w_index=2, out_scale=0)]]
    with pytest.raises(ValueError) as e:
        K.wprep_plan(1 << 16, [seg], groups, RB, PF)
    assert str(e.value) == "ptamd_weights_prep: " + message
    # overlapping segments are not representable either
    with pytest.raises(ValueError, match="is not representable"):
        K.wprep_plan(1 << 16, [dict(offset=0, rows=8, cols=8), dict(offset=32, rows=8, cols=8)], [[dict(w=0, w_index=2)]], RB, PF)


F32, X3, X3F, F16, AUTO = K.GEMM_F32, K.GEMM_BF16X3, K.GEMM_BF16X3_FULL, K.GEMM_F16X2, K.GEMM_AUTO


def test_deferred_reduce_rule(monkeypatch):
    """kernels.deferred_slabs, the one rule of linear_fwd (FFN-2 forward: N = d_model columns, reduction d_ff) and
    linear_bwd_input (the dX of FFN-1 and QKV: d_model columns, reduction d_ff / 3 d_model).  The expected numbers are written
    out from the conditions both call sites carried before: split > 1, columns % 4 == 0, columns <= 512, 2 ... 4 slices of
    whole 32-blocks, not the f32 arithmetic."""
    monkeypatch.setattr(K, "DEFER_REDUCE", True)
    monkeypatch.setattr(K, "SPLIT_K_ROWS", True)
    D, F = 512, 2048
    #         tokens  cols  reduction  split  slabs
    shapes = [(2048, D, F, 4, 4), (4096, D, F, 2, 2), (8192, D, F, 1, 0),                  # FFN-2 forward / dX of FFN-1
              (2048, D, 3 * D, 3, 3), (4096, D, 3 * D, 2, 2), (8192, D, 3 * D, 1, 0),      # dX of QKV
              (2048, D, 1023, 1, 0), (2048, D, 1024, 2, 2)]                                # a reduction just under 1024 is not cut
    for tokens, cols, red, split, slabs in shapes:
        assert K.pick_split_k_rows(tokens, cols, red) == split, (tokens, cols, red)
        for arith in (None, X3, X3F, F16, AUTO):
            assert K.deferred_slabs(cols, red, split, arith) == slabs, (tokens, cols, red, arith)
        assert K.deferred_slabs(cols, red, split, F32) == 0
    #        cols  reduction  split  arith  slabs
    edges = [(512, 2048, 1, AUTO, 0), (512, 2048, 2, AUTO, 2), (512, 2048, 4, AUTO, 4), (512, 2048, 5, AUTO, 0),
             (512, 2048, 3, AUTO, 3),                       # 64 blocks in 3 slices of 22, 22, 20
             (510, 2048, 4, AUTO, 0), (516, 2048, 4, AUTO, 0), (508, 2048, 4, AUTO, 4), (4, 2048, 4, F16, 4),
             (512, 1023, 2, AUTO, 2), (512, 1023, 4, X3, 4), (512, 96, 8, AUTO, 3), (512, 100, 3, AUTO, 2), (512, 32, 4, AUTO, 0),
             (512, 2048, 4, F32, 0)]
    for cols, red, split, arith, slabs in edges:
        assert K.deferred_slabs(cols, red, split, arith) == slabs, (cols, red, split, arith)
    monkeypatch.setattr(K, "_DEFAULT_ARITH", F32)          # the default arithmetic counts where the call names none
    assert K.deferred_slabs(512, 2048, 4, None) == 0 and K.deferred_slabs(512, 2048, 4, AUTO) == 4
    monkeypatch.setattr(K, "DEFER_REDUCE", False)          # the knob is read at call time
    assert K.deferred_slabs(512, 2048, 4, AUTO) == 0


@pytest.mark.parametrize("n,chunks", [(0, []), (1, [1]), (FILL_JOB_CAP - 1, [7]), (FILL_JOB_CAP, [8]), (FILL_JOB_CAP + 1, [8, 1]),
                                      (2 * FILL_JOB_CAP, [8, 8]), (2 * FILL_JOB_CAP + 3, [8, 8, 3])])
def test_job_array_launcher_chunks(monkeypatch, n, chunks):
    monkeypatch.setattr(K, "stream", lambda: "the stream")
    calls = []

    def fake(arr, count, stream):
        assert stream == "the stream" and len(arr) == count and isinstance(arr[0], FillJob)
        calls.append([(j.dst, j.n, j.value) for j in arr])
        return 0
    jobs = [FillJob(dst=4096 + 16 * k, n=k, value=100 + k) for k in range(n)]
    K._launch_jobs(FillJob, FILL_JOB_CAP, fake, "fake", iter(jobs))
    assert [len(c) for c in calls] == chunks
    assert [j for c in calls for j in c] == [(4096 + 16 * k, k, 100 + k) for k in range(n)]      # every job once, in order


def test_job_array_launcher_raises_through_check(monkeypatch):
    monkeypatch.setattr(K, "stream", lambda: None)
    calls = []

    def fake(arr, count, stream):
        calls.append(count)
        return -1 if len(calls) == 2 else 0
    with pytest.raises(RuntimeError, match="libptamd fake: bad shape"):
        K._launch_jobs(FillJob, 2, fake, "fake", [FillJob(dst=0, n=k, value=0) for k in range(6)])
    assert calls == [2, 2]                                  # nothing is launched behind a refused chunk
