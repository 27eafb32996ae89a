"""MI355X tests of csrc/wprep.hip (ptamd_weights_prep, ptamd_sgd_step_prep, ptamd_adam_step_prep) driven directly through
`kernels.WeightsPrep` on ONE hand-built plan whose segments sit on the kernel's edges, against numpy / fp64 references:

  * every row / column scale is `scale_of` of the exact maximum, every statistics record and every weight-derived bound
    matches fp64, the row planes are the bits of the numpy restatement of `store4_split`, the planes of the transposes
    reconstruct the weights inside the format's error model; nothing outside what the plan owns is written;
  * the fused SGD / Adam steps update every element of the buffer exactly once (fp64, element by element), with the bits of
    the plain optimizer kernels, and leave behind what a pass over the NEW weights gives;
  * the two alternating copies of the maxima / statistics are reset: weights that SHRINK between calls get smaller maxima;
  * what the builder and the library refuse, and that a refusal changes nothing.

The host references use no device code; `make_case` and `host_reference` run without a GPU.
"""
import math

import numpy as np
import pytest
import torch

from test_gpu_gemm_hp import unpack
from test_gpu_kernels import assert_close
from test_gpu_scales import scale_of

pytestmark = pytest.mark.gpu

SEED = 7
PAD = 64                         # sentinel floats on either side of w / g / m / v
FSENT, VSENT, ISENT, BSENT = -12345.0, -777.0, 0x5A5A5A5A, 0xA5
IPAD, VPAD, BPAD, GUARD = 8, 4, 256, 3
NSTATS = 10                      # records 0 .. 8 are fed by segments, 9 by none
f32 = lambda x: float(np.float32(x))                                                  # noqa: E731
PS_A, PS_B = f32(1.0 / 0.9), f32(1.0 / 0.75)     # post_scale values (fp32 numbers: the kernel and the reference see the same input)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------------------------- the plan and its weights
class Case:
    pass


def make_case():
    """The layout (host side only), the weights with their planted cases, two gradients.  From csrc/wprep.hip: 32 rows per
    workgroup (RB, read back), 8 per wavefront, 256 columns per register vector, 512 per panel, 16384 floats per plain
    workgroup (PF, read back), 256 rows per type-3 block of kernel B."""
    from protein_transformer_amd._lib import lib
    RB, PF = lib().ptamd_wprep_rows_per_block(), lib().ptamd_wprep_plain_floats_per_block()
    c = Case()
    c.RB, c.PF = RB, PF
    S = lambda name, rows, cols, **kw: dict(name=name, rows=rows, cols=cols, **kw)   # noqa: E731
    spec = [
        S("qkv", 3 * RB, 64, rs=True, cs=True, stats=0, stats_row0=2 * RB, row_planes=True),     # statistics over a sub-range of rows
        4,                                                                                       # a 4-float plain range
        S("ragged", RB + 13, 36, rs=True, cs=True, stats=1, colnorm=True),     # last block: 13 rows = wavefront 0 full, 1 with 5, 2 and 3 idle
        S("twovec", RB + 1, 260, rs=True, cs=True, stats=2),                   # 4 floats into the second vector; one row alone in its block
        S("bias64", 1, 64, stats=5),                                           # offset: a multiple of 4, not of 16
        PF + 8,                                                                # two plain workgroups
        S("full", 2 * RB, 512, rs=True, cs=True, stats=3, row_planes=True, col_planes=True, colnorm=True),
        S("w2", 2 * RB, 1024, rs=True, cs=True, stats=4, colnorm=True, col_planes=True),         # two panels, one record
        S("tall", 9 * RB + 12, 1024, rs=True, cs=True),                        # two type-3 blocks (256 + 44 rows), ragged last 32-row block
        S("bias1024", 1, 1024, stats=6),                                       # b_1 at d_ff above 512
        S("gamma", 1, 64, stats=7),
        S("beta", 1, 64, stats=8),
        7,                                                                     # tail: numel % 4 == 3
    ]
    pos, c.segs, c.plain = 0, {}, []
    for s in spec:
        if isinstance(s, int):
            c.plain.append((pos, s))
            pos += s
        else:
            s["offset"] = pos
            c.segs[s["name"]] = s
            pos += s["rows"] * s["cols"]
    c.numel = pos
    assert c.numel % 4 == 3 and c.numel < 500000
    assert c.segs["bias64"]["offset"] % 16 == 12 and all(s["offset"] % 4 == 0 for s in c.segs.values())
    assert c.plain[1][1] > PF and c.segs["tall"]["rows"] > 256 and c.segs["tall"]["rows"] % RB
    # `ints`: every scale array and every out_scale quadruple, GUARD sentinel entries in front of each and behind the last
    c.ints_at, o = {}, GUARD
    for s in c.segs.values():
        for kind, n in (("rs", s["rows"]), ("cs", s["cols"])):
            if s.get(kind):
                c.ints_at[(s["name"], kind)] = (o, n)
                o += n + GUARD
    for name in ("att", "h1", "f1", "one"):
        c.ints_at[(name, "out")] = (o, 4)
        o += 4 + GUARD
    c.n_ints = o
    c.ints_owned = np.zeros(c.n_ints + 2 * IPAD, bool)
    for o, n in c.ints_at.values():
        c.ints_owned[IPAD + o:IPAD + o + n] = True
    c.values_at = {"dz_w2": 1, "f1": 3, "dz_full": 5, "dz_ragged": 7}
    c.n_values = 9
    c.values_owned = np.zeros(c.n_values + 2 * VPAD, bool)
    c.values_owned[[VPAD + k for k in c.values_at.values()]] = True
    R = {n: s["stats"] for n, s in c.segs.items() if s.get("stats") is not None}
    # every form models/encoder_only.py:_build_prep uses: LayerNorm + w_index 0 + bias -> out_scale; w_index 1 on the panelled
    # colnorm record -> out_value; w = -1 (with and without a LayerNorm)
    c.groups = [
        [dict(ln_gamma=R["gamma"], ln_beta=R["beta"], w=R["qkv"], w_index=0, bias=R["bias64"], sqrt_d=8.0, post_scale=PS_A, out_scale="att"),
         dict(w=R["w2"], w_index=1, post_scale=PS_A, out_value="dz_w2"),
         dict(ln_gamma=R["gamma"], ln_beta=R["beta"], w=-1, w_index=0, sqrt_d=8.0, out_scale="h1")],
        [dict(ln_gamma=R["gamma"], ln_beta=R["beta"], w=R["twovec"], w_index=0, bias=R["bias1024"], sqrt_d=8.0, post_scale=PS_B,
              out_scale="f1", out_value="f1"),
         dict(w=R["full"], w_index=1, out_value="dz_full"),
         dict(w=R["ragged"], w_index=1, post_scale=PS_B, out_value="dz_ragged"),
         dict(w=-1, w_index=0, post_scale=PS_A, out_scale="one")]]
    c.colnorm_read = {j["w"] for grp in c.groups for j in grp if j["w_index"] == 1}

    # ---- weights: rows and columns of magnitudes that span many binades, then the planted cases
    rng = np.random.default_rng(SEED)
    w = (rng.standard_normal(c.numel) * np.exp(rng.standard_normal(c.numel))).astype(np.float32)
    mat = lambda name: w[c.segs[name]["offset"]:][:c.segs[name]["rows"] * c.segs[name]["cols"]].reshape(c.segs[name]["rows"], -1)   # noqa: E731
    for name, s in c.segs.items():
        if s["rows"] > 1:
            m = mat(name)
            m *= np.exp(1.5 * rng.standard_normal((s["rows"], 1))).astype(np.float32)
            m *= np.exp(1.5 * rng.standard_normal((1, s["cols"]))).astype(np.float32)
    mat("gamma")[:] = np.abs(1.0 + 0.3 * rng.standard_normal(64))
    mat("beta")[:] = 0.3 * rng.standard_normal(64)
    last = lambda m, r: m.__setitem__((r, -1), 4 * np.abs(m[r]).max())                             # noqa: E731  (a row whose maximum is its last element)
    m = mat("qkv")
    m[70], m[:, 5], m[3, 9] = 0, 0, 1e-40               # zero row (inside the statistics range), zero column, a subnormal
    last(m, 80)
    m = mat("ragged")
    m[33], m[:, 35] = 0, 0
    m[40, 7] = 8 * np.abs(m[:, 7]).max()                # a column whose maximum lies in the ragged last row block
    last(m, 44)
    m = mat("twovec")
    m[5] = 0
    m[5, 100] = 3e-41                                   # a row whose only entry is subnormal
    m[32, 258] = 4 * np.abs(m[32]).max()                # the lone row of the last block: maximum in the second vector
    m[:, 259] = 0
    m = mat("full")
    m[17], m[:, 300] = 0, 0
    last(m, 63)
    m = mat("w2")
    m[0:8, 512:] *= 2.0 ** 10                           # maximum in the second panel only ...
    m[8:16, :512] *= 2.0 ** 10                          # ... and in the first only
    m[20], m[:, 700], m[30, 600] = 0, 0, 1e-40
    last(m, 63)
    m = mat("tall")
    for r in (100, 280, 295):                           # (first / second type-3 block, ragged 32-row block)
        m[r, 512:] *= 2.0 ** 12
    m[296, :512] *= 2.0 ** 12
    m[257] = 0
    m[299, 900] = 16 * np.abs(m[:, 900]).max()
    c.w = w
    c.mat = lambda name, buf: buf[c.segs[name]["offset"]:][:c.segs[name]["rows"] * c.segs[name]["cols"]].reshape(c.segs[name]["rows"], -1)
    c.g = (0.01 * rng.standard_normal(c.numel) * np.exp(rng.standard_normal(c.numel))).astype(np.float32)
    c.g_same = np.where(w < 0, -np.abs(c.g), np.abs(c.g)).astype(np.float32)      # same sign as w: Adam's g' = coef g + wd w never cancels
    return c


@pytest.fixture(scope="module")
def case():
    return make_case()


def host_reference(c, w):
    """({(segment, "rs" / "cs"): scales as fp64}, statistics records [NSTATS, 4] in fp64) of the weights `w` (fp32, host)."""
    scales, stats = {}, np.zeros((NSTATS, 4))
    for name, s in c.segs.items():
        m = c.mat(name, w)
        if s.get("rs"):
            scales[(name, "rs")] = scale_of(np.abs(m).max(1))
        if s.get("cs"):
            scales[(name, "cs")] = scale_of(np.abs(m).max(0))
        k = s.get("stats")
        if k is not None:
            sub = m[s.get("stats_row0", 0):].astype(np.float64)
            # ([0] of a matrix wider than 512 columns is not computed: include/ptamd.h)
            stats[k, 0] = 0.0 if s["cols"] > 512 else np.sqrt((sub ** 2).sum(1)).max()
            stats[k, 2] = np.abs(sub).max()
            if s.get("colnorm") and k in c.colnorm_read:
                stats[k, 1] = np.sqrt((m.astype(np.float64) ** 2).sum(0)).max()
    return scales, stats


def bound64(j, st):
    """ptamd_bound_scales' formula (include/ptamd.h) in fp64 on statistics records `st`."""
    x = 1.0
    if j.get("ln_gamma") is not None:
        x = st[j["ln_gamma"], 2] * j["sqrt_d"] + (st[j["ln_beta"], 0] if j.get("ln_beta") is not None else 0.0)
    v = x * st[j["w"], j["w_index"]] if j["w"] >= 0 else x
    if j.get("bias") is not None:
        v += st[j["bias"], 2]
    return v * j.get("post_scale", 1.0)


def off_power_of_two(v):
    """Relative distance of v > 0 from the nearest power of two."""
    return abs(v / 2.0 ** round(math.log2(v)) - 1.0)


def bounds_of(c, st):
    out = [bound64(j, st) for grp in c.groups for j in grp]
    # precondition (on reference values alone): no bound within 1e-4 of a power of two, so that the fp32 rounding of the
    # kernel's bound cannot move its scale and the comparison of scales below is exact
    assert all(b > 0 and off_power_of_two(b) >= 1e-4 for b in out), out
    return out


# ----------------------------------------------------------------------------------------------- the plan on the device
class Plan:
    def __init__(self, c, dev, w):
        from protein_transformer_amd import kernels as K
        self.c, self.dev = c, dev
        self.big, self.view = {}, {}
        for name, init in (("w", w), ("g", np.zeros_like(w)), ("m", np.zeros_like(w)), ("v", np.zeros_like(w))):
            big = torch.full((c.numel + 2 * PAD,), FSENT, dtype=torch.float32, device=dev)
            big[PAD:PAD + c.numel] = torch.from_numpy(init).to(dev)
            self.big[name], self.view[name] = big, big[PAD:PAD + c.numel]
        self.w, self.g, self.m, self.v = (self.view[k] for k in "wgmv")
        self.ints_big = torch.full((c.n_ints + 2 * IPAD,), ISENT, dtype=torch.int32, device=dev)
        self.ints = self.ints_big[IPAD:IPAD + c.n_ints]
        self.values_big = torch.full((c.n_values + 2 * VPAD,), VSENT, dtype=torch.float32, device=dev)
        self.values = self.values_big[VPAD:VPAD + c.n_values]
        self.planes_big, self.planes = {}, {}
        iv = lambda key: self.ints[c.ints_at[key][0]:][:c.ints_at[key][1]]                     # noqa: E731
        self.iv = iv
        segs = []
        for name, s in c.segs.items():
            d = dict(offset=s["offset"], rows=s["rows"], cols=s["cols"], stats_row0=s.get("stats_row0", 0), stats=s.get("stats"),
                     row_scale=iv((name, "rs")) if s.get("rs") else None, col_scale=iv((name, "cs")) if s.get("cs") else None,
                     colnorm=bool(s.get("colnorm")))
            for kind, (r, k) in (("row_planes", (s["rows"], s["cols"])), ("col_planes", (s["cols"], s["rows"]))):
                if s.get(kind):
                    n = K.lib().ptamd_hp_bytes(r, k)
                    big = torch.full((n + 2 * BPAD,), BSENT, dtype=torch.uint8, device=dev)
                    self.planes_big[(name, kind)], self.planes[(name, kind)] = big, big[BPAD:BPAD + n]
                    d[kind] = self.planes[(name, kind)]
            segs.append(d)
        groups = []
        for grp in c.groups:
            jobs = []
            for j in grp:
                j = dict(j)
                if "out_scale" in j:
                    j["out_scale"] = iv((j["out_scale"], "out"))
                if "out_value" in j:
                    k = c.values_at[j["out_value"]]
                    j["out_value"] = self.values[k:k + 1]
                jobs.append(j)
            groups.append(jobs)
        self.wp = K.WeightsPrep(c.numel, segs, groups, self.ints, self.values, NSTATS)

    def host_w(self):
        return self.w.cpu().numpy()

    def scribble(self, byte):
        """Everything a call has to write is overwritten (the sentinels around it stay)."""
        self.ints.fill_(ISENT)
        self.values.fill_(VSENT)
        for p in self.planes.values():
            p.fill_(byte)

    def check_padding(self):
        for name, big in self.big.items():
            assert bool((big[:PAD] == FSENT).all()) and bool((big[PAD + self.c.numel:] == FSENT).all()), name
        for key, big in self.planes_big.items():
            assert bool((big[:BPAD] == BSENT).all()) and bool((big[-BPAD:] == BSENT).all()), key

    def check(self, w, planes=True, what=""):
        """Everything a call leaves behind against the references for the weights `w` (fp32, host)."""
        from protein_transformer_amd import kernels as K
        c = self.c
        torch.cuda.synchronize()
        ints, vals = self.ints_big.cpu().numpy(), self.values_big.cpu().numpy()
        st = self.wp.last_stats().cpu().numpy().astype(np.float64)
        assert np.all(ints[~c.ints_owned] == ISENT) and np.all(vals[~c.values_owned] == VSENT), what
        self.check_padding()
        scales, stats = host_reference(c, w)
        got_scale = lambda key: ints[IPAD + c.ints_at[key][0]:][:c.ints_at[key][1]].view(np.float32).astype(np.float64)   # noqa: E731
        for key, want in scales.items():
            # bit-exact: maxima have no summation order
            assert np.array_equal(got_scale(key), want), (what, key, int((got_scale(key) != want).sum()))
        for k in range(NSTATS):
            assert abs(st[k, 0] - stats[k, 0]) <= 1e-5 * stats[k, 0], (what, k, st[k], stats[k])       # tests/test_gpu_scales.py::test_weight_scales_vs_numpy
            assert abs(st[k, 1] - stats[k, 1]) <= 2.0 ** -23 * stats[k, 1], (what, k, st[k], stats[k])  # fp64 sum: fp32 square root and cast
            assert st[k, 2] == stats[k, 2] and st[k, 3] == 0.0, (what, k, st[k], stats[k])             # a maximum: exact
        bounds_of(c, stats)                                   # (the same precondition on the host's own statistics)
        want_b = iter(bounds_of(c, st))
        for grp in c.groups:
            for j in grp:
                b = next(want_b)
                if "out_value" in j:
                    got = float(vals[VPAD + c.values_at[j["out_value"]]])
                    assert abs(got - b) <= 4 * 2.0 ** -24 * b, (what, j, got, b)                        # four fp32 roundings of non-negative terms
                if "out_scale" in j:
                    assert np.array_equal(got_scale((j["out_scale"], "out")), np.full(4, scale_of(np.float32(b)))), (what, j, b)
        if not planes:
            return
        for (name, kind), buf in self.planes.items():
            m = c.mat(name, w)
            if kind == "row_planes":
                op = K.hp_view(buf, self.iv((name, "rs")), m.shape[0], m.shape[1])
                x, amax, s = m, np.abs(m).max(1), scales[(name, "rs")]
            else:
                op = K.hp_view(buf, self.iv((name, "cs")), m.shape[1], m.shape[0])
                x, amax, s = np.ascontiguousarray(m.T), np.abs(m).max(0), scales[(name, "cs")]
            back, pl, scale = unpack(op, self.dev)
            assert np.array_equal(scale, s)
            a = x * s.astype(np.float32)[:, None]              # exact: s is a power of two
            hi = a.astype(np.float16)
            assert np.array_equal(pl[0], hi.astype(np.float64)), (what, name, kind, "hi")
            if kind == "row_planes":                           # store4_split: lo = float16(a - float32(hi)), bit for bit
                lo = (a - hi.astype(np.float32)).astype(np.float16)
                assert np.array_equal(pl[1], lo.astype(np.float64)), (what, name, kind, "lo")
            # the format's error model (tests/test_gpu_gemm_hp.py::test_hp_split_roundtrip)
            x64 = x.astype(np.float64)
            assert np.all(np.abs(back - x64) <= 2.0 ** -22 * np.abs(x64) + 2.0 ** -39 * amax[:, None]), (what, name, kind)
            zero = amax == 0
            assert np.all(s[zero] == 2.0 ** 127) and np.all(pl[:, zero] == 0)     # rows of zeros: largest finite power of two, zero planes


# ----------------------------------------------------------------------------------------------- 1. the pass
def test_prepare_against_fp64(dev, case):
    """ptamd_weights_prep against the host references, with planes; then without, on scribbled outputs: the scales and bounds
    are written again, no plane byte is."""
    P = Plan(case, dev, case.w)
    assert float(np.abs(case.mat("qkv", case.w)[70]).max()) == 0 and float(np.abs(case.mat("w2", case.w)[:, 700]).max()) == 0
    P.wp.prepare(P.w, with_planes=True)
    P.check(case.w, planes=True, what="with planes")
    assert np.array_equal(P.host_w().view(np.uint32), case.w.view(np.uint32))         # the pass does not write the weights
    P.scribble(0x3C)
    P.wp.prepare(P.w, with_planes=False)
    P.check(case.w, planes=False, what="without planes")                             # scales and bounds are written ...
    assert all(bool((p == 0x3C).all()) for p in P.planes.values())                   # ... the planes are not touched


# ----------------------------------------------------------------------------------------------- 2. the fused steps
def clip_coef32(sq, max_norm):
    """optim_update.h's clip_coef in the same fp32 operations (division and square root are correctly rounded on both sides)."""
    if max_norm <= 0:
        return 1.0
    c = np.float32(max_norm) / (np.sqrt(np.float32(sq)) + np.float32(1e-6))
    return float(min(c, np.float32(1.0)))


@pytest.mark.parametrize("max_norm", [1.0, 0.0], ids=["clip", "noclip"])
@pytest.mark.parametrize("zero_grad", [False, True], ids=["keepgrad", "zerograd"])
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_fused_step_against_fp64_and_the_plain_kernels(dev, case, optimizer, zero_grad, max_norm):
    """ptamd_sgd_step_prep (one step) / ptamd_adam_step_prep (three, so that the bias correction moves): (a) the update of
    every element of the buffer against fp64 from the same inputs and the device's squared norm, (b) the bits of the plain
    optimizer kernels on copies, (c) scales, statistics, bounds and planes of the weights the step wrote."""
    from protein_transformer_amd import kernels as K
    adam = optimizer == "adam"
    lr, wd, b1, b2, eps = f32(1e-3 if adam else 1e-2), f32(0.01), f32(0.9), f32(0.98), f32(1e-9)
    g0 = case.g_same if adam else case.g
    assert not adam or bool(np.all(case.w.astype(np.float64) * g0 >= 0))             # precondition: same-signed Adam inputs
    P = Plan(case, dev, case.w)
    P.wp.prepare(P.w)
    w2, m2, v2 = P.w.clone(), P.m.clone(), P.v.clone()                               # the plain kernels' copies
    p64, m64, v64 = case.w.astype(np.float64), np.zeros(case.numel), np.zeros(case.numel)
    sq = torch.zeros(1, device=dev)
    for step in range(1, 4 if adam else 2):
        gi = g0 * np.float32(step)
        P.g.copy_(torch.from_numpy(gi))
        g2 = P.g.clone()
        K.grad_sqnorm(P.g, sq)
        g64 = gi.astype(np.float64)
        assert math.sqrt(float(sq)) == pytest.approx(math.sqrt(float((g64 ** 2).sum())), rel=1e-5)   # tests/test_gpu_kernels.py::test_clip_and_sgd_adam
        coef = clip_coef32(float(sq), max_norm)
        assert (coef < 1.0) == (max_norm > 0)                                        # "clip" clips, "noclip" has coefficient exactly 1
        if adam:
            P.wp.adam_step(P.w, P.g, P.m, P.v, sq, max_norm, lr, b1, b2, eps, wd, step, zero_grad=zero_grad)
            K.adam_step(w2, g2, m2, v2, sq, max_norm, lr, b1, b2, eps, wd, step, zero_grad=zero_grad)
            gr = coef * g64 + wd * p64
            m64 = b1 * m64 + (1 - b1) * gr
            v64 = b2 * v64 + (1 - b2) * gr * gr
            p64 = p64 - (lr / (1 - b1 ** step)) * m64 / (np.sqrt(v64) / math.sqrt(1 - b2 ** step) + eps)
        else:
            P.wp.sgd_step(P.w, P.g, sq, max_norm, lr, wd, zero_grad=zero_grad)
            K.sgd_step(w2, g2, sq, max_norm, lr, wd, zero_grad=zero_grad)
            # three fp32 roundings (wd p, two fmas) of terms of these sizes
            tol = 4 * 2.0 ** -24 * (np.abs(p64) + lr * (np.abs(coef * g64) + np.abs(wd * p64)))
            p64 = p64 - lr * (coef * g64 + wd * p64)
        torch.cuda.synchronize()
        # (b) the bits of the plain kernels (optim_update.h), at every segment shape, plain range and the 3-element tail
        assert torch.equal(P.w, w2) and torch.equal(P.m, m2) and torch.equal(P.v, v2) and torch.equal(P.g, g2), step
        got_g = P.g.cpu().numpy()
        if zero_grad:
            assert not got_g.any()
        else:
            assert np.array_equal(got_g.view(np.uint32), gi.view(np.uint32))
        w_now = P.host_w()
        if not adam:                                                                 # (a) element by element over the whole buffer
            err = np.abs(w_now.astype(np.float64) - p64)
            assert np.all(err <= tol), (int((err > tol).sum()), int(np.argmax(err - tol)))
            assert not P.m.any() and not P.v.any()
        # (c) what the step left behind, for the weights it wrote
        P.check(w_now, planes=True, what=f"{optimizer} step {step}")
    if adam:                                                                         # (a), test_clip_and_sgd_adam's tolerances
        assert_close(P.w, torch.from_numpy(p64), 1e-5, 1e-6, "adam")
        assert_close(P.m, torch.from_numpy(m64), 1e-4, 1e-9, "adam m")
        assert_close(P.v, torch.from_numpy(v64), 1e-4, 1e-12, "adam v")


# ----------------------------------------------------------------------------------------------- 3. stale maxima
def test_shrinking_weights_get_smaller_maxima(dev, case):
    """atomicMax of the same weights is idempotent, so only weights that SHRINK between calls show a copy of the maxima /
    statistics that kernel B of the call before did not reset."""
    from protein_transformer_amd import kernels as K
    c = case
    P = Plan(c, dev, c.w)
    seg = lambda name: P.w[c.segs[name]["offset"]:][:c.segs[name]["rows"] * c.segs[name]["cols"]]   # noqa: E731
    parities = [P.wp.parity]
    P.wp.prepare(P.w)
    P.check(c.w, what="call 1")
    P.w.mul_(2.0 ** -3)
    parities.append(P.wp.parity)
    P.wp.prepare(P.w)
    w = P.host_w()
    assert np.abs(w).max() == np.abs(c.w).max() / 8
    P.check(w, what="call 2 (everything 2^-3)")
    seg("w2").mul_(2.0 ** -5)
    seg("bias64").mul_(2.0 ** 4)
    P.g.copy_(torch.from_numpy(c.g))
    sq = torch.zeros(1, device=dev)
    K.grad_sqnorm(P.g, sq)
    before = P.w.clone()
    parities.append(P.wp.parity)
    P.wp.sgd_step(P.w, P.g, sq, 1.0, 0.0, 0.0)           # lr 0, wd 0: the bookkeeping alone
    assert torch.equal(P.w, before)
    w = P.host_w()
    P.check(w, what="call 3 (fused step; w2 2^-5, bias64 2^4)")
    for k in (4, 5):
        parities.append(P.wp.parity)
        P.wp.prepare(P.w)
        P.check(w, what=f"call {k}")
    assert parities == [0, 1, 0, 1, 0]


# ----------------------------------------------------------------------------------------------- 4. refusals
def test_builder_refusals(dev):
    from protein_transformer_amd import kernels as K
    ints = torch.zeros(8192, dtype=torch.int32, device=dev)
    values = torch.zeros(8, dtype=torch.float32, device=dev)
    planes = torch.zeros(1 << 18, dtype=torch.uint8, device=dev)
    job = dict(w=-1, w_index=0, out_scale=ints[0:4])
    rs, cs = ints[16:16 + 64], ints[2048:2048 + 1024]

    def build(segs, groups=None, numel=1 << 17):
        return K.WeightsPrep(numel, segs, [[job]] if groups is None else groups, ints, values, 4)
    S = lambda **kw: dict(dict(offset=0, rows=32, cols=64), **kw)                    # noqa: E731
    bad = [
        [S(cols=6)],                                                                 # cols % 4
        [S(offset=2)],                                                               # offset % 4
        [S(), S(offset=1024)],                                                       # overlapping segments
        [S(cols=768)],                                                               # above 512, no multiple of 512
        [S(rows=48, row_scale=rs, row_planes=planes)],                               # planes: rows % 32
        [S(cols=36, col_scale=cs, col_planes=planes)],                               # planes: cols % 32
        [S(col_planes=planes)],                                                      # col_planes without col_scale
        [S(col_scale=cs, colnorm=True)],                                             # colnorm without a record
        [S(stats=0, colnorm=True)],                                                  # colnorm without col_scale
        [S(cols=1024, row_scale=rs, row_planes=planes)],                             # a wide matrix with row planes
        [S(cols=1024, stats=0, stats_row0=16)],                                      # ... with a statistics sub-range
    ]
    for segs in bad:
        with pytest.raises(ValueError):
            build(segs)
    with pytest.raises(ValueError):
        build([S()], groups=[])                                                      # no groups
    # entry [0] of a record that only panels feed is not computed: neither w_index 0 nor ln_beta may read it
    wide = [S(cols=1024, stats=0, col_scale=cs, colnorm=True), S(offset=32768, rows=1, stats=1)]
    with pytest.raises(ValueError):
        build(wide, groups=[[dict(w=0, w_index=0, out_value=values[0:1])]])
    with pytest.raises(ValueError):
        build(wide, groups=[[dict(ln_gamma=1, ln_beta=0, w=-1, w_index=0, sqrt_d=8.0, out_value=values[0:1])]])
    # its [1] and [2] are; and a record that whole rows feed as well has its [0]
    build(wide, groups=[[dict(w=0, w_index=1, bias=0, out_value=values[0:1]), dict(w=1, w_index=0, out_value=values[1:2])]])
    build(wide + [S(offset=32768 + 64, stats=0)], groups=[[dict(w=0, w_index=0, out_value=values[0:1])]])


def test_library_refusals_change_nothing(dev, case):
    c = case
    P = Plan(c, dev, c.w)
    P.g.copy_(torch.from_numpy(c.g))
    P.wp.prepare(P.w)
    sq = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    state = lambda: ([b.clone() for b in P.big.values()] + [P.ints_big.clone(), P.values_big.clone(), P.wp.stats.clone(),     # noqa: E731
                                                            P.wp.colmax.clone()] + [b.clone() for b in P.planes_big.values()])
    before, parity = state(), P.wp.parity
    g_odd = P.big["g"][PAD + 1:PAD + 1 + c.numel]                                    # 4 bytes off a 16-byte boundary
    assert g_odd.data_ptr() % 16 == 4 and P.g.data_ptr() % 16 == 0
    hyper = (1.0, 1e-3, 0.9, 0.98, 1e-9, 0.01)
    refused = [
        lambda: P.wp.sgd_step(P.w[:-4], P.g[:-4], sq, 1.0, 1e-2, 0.01),              # n != numel
        lambda: P.wp.adam_step(P.w[:-4], P.g[:-4], P.m[:-4], P.v[:-4], sq, *hyper, 1),
        lambda: P.wp.adam_step(P.w, P.g, P.m, P.v, sq, *hyper, 0),                   # step <= 0
        lambda: P.wp.adam_step(P.w, P.g, P.m, P.v, sq, *hyper, -1),
        lambda: P.wp.sgd_step(P.w, g_odd, sq, 1.0, 1e-2, 0.01),                      # g not 16-byte aligned
        lambda: P.wp.adam_step(P.w, g_odd, P.m, P.v, sq, *hyper, 1),
    ]
    for k, call in enumerate(refused):
        with pytest.raises(RuntimeError):
            call()
        assert P.wp.parity == parity, k
    for bad_parity in (2, -1):                                                       # a parity outside {0, 1}
        P.wp.parity = bad_parity
        with pytest.raises(RuntimeError):
            P.wp.prepare(P.w)
        with pytest.raises(RuntimeError):
            P.wp.sgd_step(P.w, P.g, sq, 1.0, 1e-2, 0.01)
        assert P.wp.parity == bad_parity
    P.wp.parity = parity
    torch.cuda.synchronize()
    for a, b in zip(state(), before):
        assert torch.equal(a, b)
    P.wp.prepare(P.w)                                                                # ... and the plan still works
    P.check(c.w, what="after the refusals")


# ----------------------------------------------------------------------------------------------- d_model 1024
def test_d_model_1024_trains_on_the_separate_launches(dev):
    """`-dm 1024` raised ValueError in its first forward pass: `_step_scales` built the one-pass plan although W_qkv's
    statistics sub-range and the row planes of W_qkv / W_1 cannot be panelled.  Such a model takes the separate launches, as
    d_model 768 does.  (Two proteins of 64 residues are below the size at which GEMM_AUTO picks the f16x2 arithmetic, whose
    bookkeeping this is about: the arithmetic is set.)"""
    import types
    from protein_transformer_amd import kernels as K, synthetic
    from protein_transformer_amd.models.encoder_only import EncoderOnlyTransformer
    from protein_transformer_amd.optim import FusedSGD
    from protein_transformer_amd.protein.Sequence import VOCAB
    from protein_transformer_amd.protein.Structure import nerf_forward
    from protein_transformer_amd.train import train_step
    build = lambda ang, seq: nerf_forward(ang.to(dev), seq.to(dev))[0]  # noqa: E731
    batch = synthetic.make_batch([64, 64], L_pad=64, seed=4, build_coords=build)
    data = tuple(batch[k].to(dev) for k in ("seq", "true_ang", "true_crd"))
    args = types.SimpleNamespace(loss="drmsd", combined_drmsd_weight=0.5, backbone_loss=False, clip=1.0)
    flats = []
    for prep in (True, False):
        torch.manual_seed(4)
        m = EncoderOnlyTransformer(1, 16, 1024, 2048, 64, VOCAB, synthetic.angle_means(batch["true_ang"]), True, dropout=0.1).to(dev).train()
        assert m.weights_prep is True                                                # the default
        m.gemm_mode = K.GEMM_F16X2
        if not prep:
            m.weights_prep = False
        opt = FusedSGD(m, lr=1e-2, weight_decay=10e-3)
        for _ in range(2):
            losses = train_step(m, opt, args, *data)
        assert np.isfinite(float(losses["drmsd-full"]))
        caches = m.__dict__.get("_scale_caches", {})
        assert caches and all(c["prep"] is None for c in caches.values())
        flats.append(m.flat_parameters()[0].clone())
    assert torch.isfinite(flats[0]).all() and torch.equal(flats[0], flats[1])
