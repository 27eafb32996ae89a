"""The kernels on the compacted 64-atom tiles of csrc/atom_tiles.h - the lDDT metric (csrc/lddt.hip), the smooth-lDDT loss
(csrc/slddt.hip), the clash term (csrc/clash.hip), the last two through the shared sweep of csrc/pair_sweep.h, and FAPE
(csrc/fape.hip) - called through the C ABI on a workspace this file owns, on the cases of tests/atom_tiles_cases.py (strip and
chunk edges, the box cull, rows of one strip that disagree about a column tile, the shares of the compaction, and for FAPE the
grid of 63, 64, 65 frames by 511, 512, 513 atoms in rows of 65, 128 and 129 residues).

Every (case, kernel) runs under three states of the workspace: filled with 0x00, filled with 0xFF (NaN as a float, -1 as an
int: a `kept` flag nobody wrote reads true, a partial nobody wrote is NaN), and `stale` - as left by a call, immediately
before, on other proteins of the same B and L (`Case.stale_batch`).  The workspace is handed over at offset 256 of a buffer 512
bytes longer; every output has 64 poisoned elements in front and behind.  Asserted: the three runs give the same bits; all
guard bands are intact; no output element keeps its poison; the Python wrapper, called right after a larger batch went through
its cached workspace, returns the same bits; a forward-only call (NULL dcrd) returns the same statistics; and against fp64
  * npairs, nclash, nclamped and the lDDT counts exactly;
  * the loss to 1e-5 / tau (slddt, the bar of tests/test_gpu_slddt.py), 1e-5 (clash, the bar of tests/test_gpu_clash.py:
    a term carries a few fp32 ulps of a distance below 3.6 A, the sum is divided by the atom count) and 1e-5 (FAPE, the
    VALUE_BAR of tests/test_gpu_fape.py, derived there for lever arms up to 64 A, which `fape_clamp` asserts);
  * the gradient PER ATOM: err_i <= K scale_i + floor_i (tests/atom_tiles_cases.py), and exactly +0.0 on every slot without
    an atom.

Measured on an MI355X, worst (err_i - floor_i) / scale_i over the atoms of a case (every test prints it; the full table is in
profiles/atom_tiles/NOTES.md): slddt 7.656e-6 (shares-147; the other cases 1.8e-6 ... 4.6e-6), clash 6.321e-5
(shares-147-clash; shares-74-clash 3.2e-5, counts-clash 1.15e-5, hairpin-clash 6.3e-6, box-cull-clash 1.3e-6); K = 8 x the worst
of a kernel = 6.12e-5 and 5.06e-4; fape 2.538e-6 (fape-grid-128; grid-129 2.53e-6, grid-65 1.76e-6, shares-74-fape 1.34e-6,
shares-147-fape 7.4e-7), K = 2.03e-5.  The slddt and clash ratios grow with the distance of the atoms from the origin (the share cases are chains
280 and 560 A long against clash distances of ~2 A): the column side of the sweep forms x_j S_j - V_j."""
import numpy as np
import pytest
import torch

import atom_tiles_cases as atc
from test_gpu_lddt import scores_of

pytestmark = pytest.mark.gpu

GUARD = 64                 # elements in front of and behind every output
POISON = 0xCD              # outputs and guard bands (never the workspace: its entries are read as indices)
STATES = ("zeros", "ones", "stale")


class Guarded:
    """A device tensor of `shape` inside a poisoned buffer, 64 elements of guard band on either side."""

    def __init__(self, shape, dtype, dev):
        self.isz = torch.empty(0, dtype=dtype).element_size()
        n = int(np.prod(shape))
        self.raw = torch.full(((n + 2 * GUARD) * self.isz,), POISON, dtype=torch.uint8, device=dev)
        self.inner = self.raw[GUARD * self.isz:(GUARD + n) * self.isz]
        self.t = self.inner.view(dtype).view(*shape)

    def guards_intact(self):
        g = GUARD * self.isz
        return bool((self.raw[:g] == POISON).all()) and bool((self.raw[-g:] == POISON).all())

    def poisoned(self):
        """bool per element: all its bytes are still the poison"""
        return (self.inner.view(-1, self.isz) == POISON).all(1).cpu().numpy().reshape(tuple(self.t.shape))


SPEC = {   # kernel -> (name, shape as a function of B and L, dtype) of every output, in the ABI's order
    "slddt": [("stats", lambda B, L: (B, 2), torch.float32), ("npairs", lambda B, L: (B,), torch.int64),
              ("dcrd", lambda B, L: (B, L * atc.SLOTS, 3), torch.float32)],
    "clash": [("stats", lambda B, L: (B, 2), torch.float32), ("npairs", lambda B, L: (B,), torch.int64),
              ("dcrd", lambda B, L: (B, L * atc.SLOTS, 3), torch.float32)],
    "fape": [("stats", lambda B, L: (B, 2), torch.float32), ("npairs", lambda B, L: (B,), torch.int64),
             ("nclamped", lambda B, L: (B,), torch.int64), ("dcrd", lambda B, L: (B, L * atc.SLOTS, 3), torch.float32)],
    "lddt": [("counts", lambda B, L: (B, L, 2, 5), torch.int32), ("per_res", lambda B, L: (B, L, 2), torch.float32),
             ("score", lambda B, L: (B, 2), torch.float32)],
}


def call_abi(kernel, pred, true, seq, cutoff, ws, nbytes, outs, grad=True):
    from protein_transformer_amd import _lib
    lib, P = _lib.lib(), _lib.ptr
    B, L = seq.shape
    if kernel == "slddt":
        rc = lib.ptamd_slddt_fwd_bwd(P(pred), P(true), P(seq), B, L, float(cutoff), atc.TAU, P(outs["stats"]), P(outs["npairs"]),
                                     P(outs["dcrd"]) if grad else None, P(ws), nbytes, _lib.stream())
    elif kernel == "clash":
        rc = lib.ptamd_clash_fwd_bwd(P(pred), P(seq), B, L, atc.clash_ref.TOLERANCE, 1.0, 0, P(outs["stats"]), P(outs["npairs"]),
                                     P(outs["dcrd"]) if grad else None, P(ws), nbytes, _lib.stream())
    elif kernel == "fape":                                            # (`cutoff` is the clamp)
        rc = lib.ptamd_fape_fwd_bwd(P(pred), P(true), P(seq), B, L, float(cutoff), P(outs["stats"]), P(outs["npairs"]),
                                    P(outs["nclamped"]), P(outs["dcrd"]) if grad else None, P(ws), nbytes, _lib.stream())
    else:
        rc = lib.ptamd_lddt(P(pred), P(true), P(seq), B, L, float(cutoff), P(outs["counts"]), P(outs["per_res"]), P(outs["score"]),
                            P(ws), nbytes, _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc


def workspace_bytes(kernel, B, L):
    from protein_transformer_amd import _lib
    return getattr(_lib.lib(), f"ptamd_{kernel}_workspace_bytes")(B, L)


def to_dev(c, dev, batch=None):
    pred, true, seq = batch if batch is not None else (c.pred, c.true, c.seq)
    return (torch.from_numpy(np.array(pred)).to(dev), None if true is None else torch.from_numpy(np.array(true)).to(dev),
            torch.from_numpy(np.array(seq)).to(dev))


def threshold(kernel, c):
    """The cutoff of the case, or for FAPE its clamp."""
    return atc.fape_clamp(c.name) if kernel == "fape" else c.cutoff


def run_state(kernel, c, state, dev, grad=True):
    """One call on a workspace in `state` -> name -> numpy array of every output, after the guard and poison checks."""
    B, L = c.B, c.L
    nbytes = workspace_bytes(kernel, B, L)
    assert nbytes > 0
    whole = torch.full((nbytes + 512,), POISON, dtype=torch.uint8, device=dev)
    ws = whole[256:256 + nbytes]
    assert ws.data_ptr() % 16 == 0
    ws.fill_(0xFF if state == "ones" else 0x00)
    if state == "stale":
        batch = to_dev(c, dev, c.stale_batch(np.random.default_rng(7)))
        scrap = {name: torch.empty(shape(B, L), dtype=dtype, device=dev) for name, shape, dtype in SPEC[kernel]}
        call_abi(kernel, *batch, threshold(kernel, c), ws, nbytes, scrap)
    outs = {name: Guarded(shape(B, L), dtype, dev) for name, shape, dtype in SPEC[kernel]}
    call_abi(kernel, *to_dev(c, dev), threshold(kernel, c), ws, nbytes, {k: g.t for k, g in outs.items()}, grad=grad)
    assert bool((whole[:256] == POISON).all()) and bool((whole[256 + nbytes:] == POISON).all()), "workspace guard band"
    for name, g in outs.items():
        assert g.guards_intact(), name
        if name == "dcrd" and not grad:
            assert g.poisoned().all()                                  # not an output of a forward-only call
        else:
            assert not g.poisoned().any(), (name, state)
    return {name: g.t.cpu().numpy().copy() for name, g in outs.items()}


def run_wrapper(kernel, c, dev):
    """The Python wrapper on the case, right after a batch one row and three residues larger went through its cached workspace."""
    from protein_transformer_amd.eval_metrics import lddt_batch
    from protein_transformer_amd.losses import clash_forward_backward, fape_forward_backward, slddt_forward_backward
    rng = np.random.default_rng(9)
    Bb, Lb = c.B + 1, c.L + 3
    big_crd = torch.from_numpy(rng.normal(0, 9.0, (Bb, Lb * atc.SLOTS, 3)).astype(np.float32)).to(dev)
    big_seq = torch.from_numpy(rng.integers(0, 20, (Bb, Lb))).to(dev)
    pred, true, seq = to_dev(c, dev)
    if kernel == "slddt":
        slddt_forward_backward(big_crd + 1.0, big_crd, big_seq, cutoff=c.cutoff, temperature=atc.TAU)
        out = slddt_forward_backward(pred, true, seq, cutoff=c.cutoff, temperature=atc.TAU)
        names = ("stats", "npairs", "dcrd")
    elif kernel == "fape":
        fape_forward_backward(big_crd + 1.0, big_crd, big_seq, clamp=threshold(kernel, c))
        out = fape_forward_backward(pred, true, seq, clamp=threshold(kernel, c))
        names = ("stats", "npairs", "nclamped", "dcrd")
    elif kernel == "clash":
        clash_forward_backward(big_crd, big_seq)
        out = clash_forward_backward(pred, seq)
        names = ("stats", "npairs", "dcrd")
    else:
        lddt_batch(big_crd + 1.0, big_crd, big_seq, c.cutoff)
        out = lddt_batch(pred, true, seq, c.cutoff)
        names = ("score", "per_res", "counts")
    torch.cuda.synchronize()
    return {n: o.cpu().numpy() for n, o in zip(names, out)}


def same_bits(a, b):
    return all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a)


def check_against_fp64(kernel, c, got):
    refs = atc.reference(c, kernel)
    worst = 0.0
    for b, ref in enumerate(refs):
        if kernel == "lddt":
            assert np.array_equal(got["counts"][b], ref["counts"]), b
            want_res, want = scores_of(ref["counts"]), scores_of(ref["counts"].sum(0))
            for g, w in ((got["per_res"][b], want_res), (got["score"][b], want)):
                assert np.array_equal(np.isnan(g), np.isnan(w)) and np.allclose(g[~np.isnan(w)], w[~np.isnan(w)], rtol=0, atol=1e-6)
            continue
        stats, n, dcrd = got["stats"][b], int(got["npairs"][b]), got["dcrd"][b]
        assert n == ref["npairs"], (b, n, ref["npairs"])
        absent = np.setdiff1d(np.arange(dcrd.shape[0]), c.present(b))
        assert not dcrd[absent].view(np.uint32).any(), b               # exactly +0.0 on slots without an atom
        if kernel == "fape":
            assert int(got["nclamped"][b]) == ref["nclamped"], b
            if n:
                assert stats[1] == pytest.approx(ref["nclamped"] / n, rel=1e-6)
        if kernel in ("slddt", "fape") and n == 0:
            assert np.isnan(stats).all() and not dcrd.view(np.uint32).any()
            continue
        if kernel == "clash" and ref["atoms"] == 0:
            assert np.isnan(stats[0]) and stats[1] == 0 and not dcrd.view(np.uint32).any()
            continue
        bar = 1e-5 / atc.TAU if kernel == "slddt" else 1e-5
        assert abs(stats[0] - ref["loss"]) <= bar, (b, stats[0], ref["loss"])
        if kernel == "slddt":
            assert abs(stats[1] - (1 - ref["loss"])) <= bar
        elif kernel == "clash":
            assert stats[1] == ref["atoms"]
        ratio, x = atc.worst_ratio(dcrd, ref), atc.excess(dcrd, ref, kernel)
        worst = max(worst, ratio)
        print(f"{c.name}[{b}] {kernel}: n {n}, |loss - ref| {abs(stats[0] - ref['loss']):.2e}, worst (err - floor) / scale "
              f"{ratio:.3e}, {x:.3f} x the bar")
        assert np.isfinite(dcrd).all() and x <= 1.0, (b, x)
    return worst


@pytest.mark.parametrize("name,kernel", atc.RUNS)
def test_poisoned_workspaces_at_the_tile_and_box_edges(name, kernel):
    dev = torch.device("cuda:0")
    c = atc.case(name)
    runs = {state: run_state(kernel, c, state, dev) for state in STATES}
    for state in STATES[1:]:
        assert same_bits(runs["zeros"], runs[state]), state
    wrapped = run_wrapper(kernel, c, dev)
    assert same_bits({k: runs["zeros"][k] for k in wrapped}, wrapped)
    if kernel != "lddt":
        fwd = run_state(kernel, c, "ones", dev, grad=False)
        ints = [k for k in fwd if k != "dcrd"]
        assert same_bits({k: runs["zeros"][k] for k in ints}, {k: fwd[k] for k in ints})
    worst = check_against_fp64(kernel, c, runs["zeros"])
    print(f"{name} {kernel}: worst ratio of the case {worst:.3e}")


def test_clash_accumulates_only_into_the_slots_of_atoms():
    """accumulate = 1 on a 0xFF workspace: slots without an atom keep what they held, bit for bit; the others hold
    fma(weight, g, held) with g the gradient of the plain call."""
    from protein_transformer_amd import _lib
    dev = torch.device("cuda:0")
    c = atc.case("counts-clash")
    plain = run_state("clash", c, "zeros", dev)["dcrd"]
    B, L = c.B, c.L
    nbytes = workspace_bytes("clash", B, L)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)
    held = np.random.default_rng(3).normal(0, 1e-3, plain.shape).astype(np.float32)
    dcrd = torch.from_numpy(held).to(dev)
    stats, n = torch.empty(B, 2, device=dev), torch.empty(B, dtype=torch.int64, device=dev)
    pred, _, seq = to_dev(c, dev)
    P = _lib.ptr
    rc = _lib.lib().ptamd_clash_fwd_bwd(P(pred), P(seq), B, L, atc.clash_ref.TOLERANCE, 0.5, 1, P(stats), P(n), P(dcrd), P(ws), nbytes,
                                        _lib.stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = dcrd.cpu().numpy()
    for b in range(B):
        have = np.zeros(L * atc.SLOTS, bool)
        have[c.present(b)] = True
        assert np.array_equal(got[b, ~have].view(np.uint32), held[b, ~have].view(np.uint32))
        want = (0.5 * plain[b, have].astype(np.float64) + held[b, have]).astype(np.float32)      # (one rounding: an fma)
        assert np.array_equal(got[b, have], want)
