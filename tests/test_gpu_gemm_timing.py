"""The timing records bench.py reads: every launcher of the GEMM family with kernels.GEMM_TIMING set appends one
(flops, start event, end event, nprod, label) and one GEMM_BYTES entry, takes two events from GEMM_EVENT_POOL and computes
the same bits as without timing.  Labels and byte formulas are those bench.py's tables were built on."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def timed(K, call):
    """(result without timing, result with timing, the record, the bytes entry, events used)."""
    assert K.GEMM_TIMING is None
    plain = call()
    pool = [torch.cuda.Event(enable_timing=True) for _ in range(6)]
    saved = K.GEMM_TIMING, K.GEMM_EVENT_POOL, K.GEMM_BYTES
    K.GEMM_TIMING, K.GEMM_EVENT_POOL, K.GEMM_BYTES = [], list(pool), []
    try:
        got = call()
        torch.cuda.synchronize()
        records, nbytes, left = K.GEMM_TIMING, K.GEMM_BYTES, K.GEMM_EVENT_POOL
    finally:
        K.GEMM_TIMING, K.GEMM_EVENT_POOL, K.GEMM_BYTES = saved
    assert len(records) == 1 and len(records[0]) == 5 and len(nbytes) == 1
    assert left == pool[:4]                                    # two events, popped from the end of the pool
    flops, e0, e1, nprod, label = records[0]
    assert (e0, e1) == (pool[5], pool[4]) and e0.elapsed_time(e1) >= 0.0       # both recorded, around the launch
    return plain, got, (flops, nprod, label), nbytes[0]


def test_linear_fwd_record(dev):
    from protein_transformer_amd import kernels as K
    g = torch.Generator().manual_seed(3)
    x, w, b = (torch.randn(*s, generator=g).to(dev) for s in ((64, 64), (64, 64), (64,)))
    r = torch.randn(64, 64, generator=g).to(dev)
    for arith, nprod in ((K.GEMM_F32, 1), (K.GEMM_BF16X3, 6), (K.GEMM_AUTO, 3)):     # gemm.hip: ptamd_gemm_products
        for kw, extra in ((dict(), 1), (dict(residual=r, ldr=64), 2)):
            plain, got, rec, nbytes = timed(K, lambda: K.linear_fwd(x, w, b, arith=arith, **kw))
            assert torch.equal(plain, got)
            assert rec == (2.0 * 64 * 64 * 64, nprod, f"ptamd_gemm fwd (staging kernel, A_KMAJOR=0 B_KMAJOR=0 NPROD={nprod})")
            assert nbytes == 4 * (64 * 64 + 64 * 64 + 64 * 64 * extra)
    # the other two kinds of the same launcher: dX (B k-major) and dW (both, accumulating)
    plain, got, rec, nbytes = timed(K, lambda: K.linear_bwd_input(x, w, arith=K.GEMM_F32))
    assert torch.equal(plain, got) and nbytes == 4 * 3 * 64 * 64
    assert rec == (2.0 * 64 ** 3, 1, "ptamd_gemm dX (staging kernel, A_KMAJOR=0 B_KMAJOR=1 NPROD=1)")
    dw = torch.zeros(64, 64, device=dev)
    _, _, rec, nbytes = timed(K, lambda: K.linear_bwd_weight(x, w, dw, arith=K.GEMM_F32))
    assert rec == (2.0 * 64 ** 3, 1, "ptamd_gemm dW (staging kernel, A_KMAJOR=1 B_KMAJOR=1 NPROD=1)") and nbytes == 4 * 4 * 64 * 64


def test_gemm_hp_record(dev):
    from protein_transformer_amd import kernels as K
    g = torch.Generator().manual_seed(4)
    a, b = K.hp_split(torch.randn(32, 32, generator=g).to(dev)), K.hp_split(torch.randn(32, 32, generator=g).to(dev))
    plain, got, rec, nbytes = timed(K, lambda: K.gemm_hp(a, b, torch.empty(32, 32, device=dev)))
    assert torch.equal(plain, got)
    assert rec == (2.0 * 32 * 32 * 32, 3, "ptamd_gemm_hp (LDS-DMA kernel gemm_hp3_kernel, NPROD=3)")
    assert nbytes == 4 * (32 * 32 + 32 * 32 + 32 * 32)


def test_weight_gradient_group_record(dev):
    from protein_transformer_amd import kernels as K
    T, N, Kd = 2048, 64, 64
    g = torch.Generator().manual_seed(5)
    members = []
    for _ in range(2):
        dy, x = torch.randn(T, N, generator=g).to(dev), torch.randn(T, Kd, generator=g).to(dev)
        uni, st = torch.zeros(2, 4, dtype=torch.int32, device=dev), torch.zeros(2, 4, device=dev)
        K.weight_scales([dict(w=dy, stats=st[0], rows_only=True), dict(w=x, stats=st[1], rows_only=True)])
        K.bound_scales([dict(w=st[0], w_index=2, out_scale=uni[0]), dict(w=st[1], w_index=2, out_scale=uni[1])])
        members.append((dy, x, torch.randn(N, Kd, generator=g).to(dev), torch.randn(N, generator=g).to(dev), uni[0], uni[1]))

    def call():
        jobs = [(dy, x, dw.clone(), db.clone(), sy, sx) for dy, x, dw, db, sy, sx in members]
        K.linear_bwd_weight_group(jobs, 2)
        return torch.cat([t.reshape(-1) for j in jobs for t in j[2:4]])
    plain, got, rec, nbytes = timed(K, call)
    assert torch.equal(plain, got)
    assert rec == (2 * 2.0 * N * Kd * T, 3, "ptamd_gemm_group dW (staging kernel on a group + one split-K reduce, NPROD=3)")
    assert nbytes == 2 * 4 * (N * T + Kd * T + 2 * N * Kd)
