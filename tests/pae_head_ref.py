"""fp64 numpy restatement of the pair sweep of the PAE head (include/ptamd.h, `ptamd_pae_head_fwd` / `ptamd_pae_head_bwd`) and of
the whole head (protein_transformer_amd/confidence.py, class PaeHead: LayerNorm -> Linear(d -> 2H) -> that sweep) with every
gradient, for tests/test_pae_head_ref.py (CPU) and the MI355X tests tests/test_gpu_pae_head.py and tests/test_gpu_pae_fit.py.

Everything is fp64 on the fp32 inputs except the bin of a target, which is DEFINED in fp32: floorf(target * bins_per_angstrom) with
one fp32 multiply, as `plddt_ref.bin_index`."""
import numpy as np

from plddt_ref import LN_EPS, f64

NAMES = ("ln.gamma", "ln.beta", "w1", "b1", "w2", "b2")


def present(seq):
    seq = np.asarray(seq)
    return (seq >= 0) & (seq < 20)


def bin_index(target, nbins, bpa):
    """target [...] -> (finite bool, bin int; 0 where not finite): min(nbins - 1, max(0, floorf(t * bpa))), one fp32 multiply."""
    t = np.asarray(target, np.float32)
    finite = np.isfinite(t)
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor(np.where(finite, t, np.float32(0)) * np.float32(bpa))
    assert f.dtype == np.float32
    return finite, np.clip(f.astype(np.float64), 0, nbins - 1).astype(np.int64)


def d0_of(n):
    return 1.24 * np.cbrt(max(int(n), 19) - 15.0) - 1.8


def centres(nbins, bpa):
    return (np.arange(nbins) + 0.5) / float(np.float32(bpa))


def tm_weights(nbins, bpa, n):
    return 1.0 / (1.0 + (centres(nbins, bpa) / d0_of(n)) ** 2)


def pair_head(uv, w2, b2, seq, target=None, bpa=2.0, coef=1.0):
    """uv [B, L, 2H] (the used columns), w2 [nbins, H], b2 [nbins], seq [B, L], target [B, L, L] fp32 or None -> dict(pae [B,L,L],
    stats [B,2]) and, with a target, sums [2], counted [B,L,L], bin, the gradients duv [B,L,2H], dw2, db2 of coef x (mean CE) and
    `abs_duv`, `abs_dw2`, `abs_db2`: the sums of the absolute values of their summands (|w2[k,h] g_ijk| under the relu mask for
    duv, |g_ijk z_ijh| for dw2, |g_ijk| for db2), the scale a reduced gradient's error is measured on."""
    uv, w2, b2 = f64(uv), f64(w2), f64(b2)
    B, L, H2 = uv.shape
    H, nbins = H2 // 2, w2.shape[0]
    u, v = uv[:, :, :H], uv[:, :, H:]
    pre = u[:, :, None, :] + v[:, None, :, :]                                   # [B, L(i), L(j), H]
    z = np.maximum(pre, 0.0)
    x = z @ w2.T + b2
    d = x - x.max(axis=-1, keepdims=True)
    e = np.exp(d)
    s = e.sum(axis=-1)
    p = e / s[..., None]
    pres = present(seq)
    defined = pres[:, :, None] & pres[:, None, :]
    c = centres(nbins, bpa)
    pae = np.where(defined, p @ c, np.nan)
    stats = np.full((B, 2), np.nan)
    for b in range(B):
        n = int(pres[b].sum())
        if n:
            stats[b, 0] = pae[b][defined[b]].sum() / (n * n)
            term = np.where(defined[b], p[b] @ tm_weights(nbins, bpa, n), 0.0)
            stats[b, 1] = (term.sum(axis=1) / n)[pres[b]].max()
    out = dict(pae=pae, stats=stats, defined=defined, p=p, z=z)
    if target is None:
        return out
    finite, bins = bin_index(target, nbins, bpa)
    counted = defined & finite
    onehot = np.arange(nbins)[None, None, None, :] == bins[..., None]
    others = np.where(onehot, 0.0, e).sum(axis=-1)
    d_bin = np.take_along_axis(d, bins[..., None], axis=-1)[..., 0]
    ce = np.where(d_bin == 0.0, np.log1p(others), np.log(s) - d_bin)
    n = int(counted.sum())
    out.update(counted=counted, bin=bins, ce=np.where(counted, ce, np.nan),
               sums=np.array([ce[counted].sum() / n if n else np.nan, float(n)]))
    g = np.zeros_like(p)
    if n:
        pm = np.where(onehot, (-others / s)[..., None], p)                        # p - onehot without the cancellation
        g = np.where(counted[..., None], coef / n * pm, 0.0)
    mask = pre > 0.0
    dz = (g @ w2) * mask
    adz = (np.abs(g) @ np.abs(w2)) * mask
    out.update(g=g, db2=g.sum(axis=(0, 1, 2)), abs_db2=np.abs(g).sum(axis=(0, 1, 2)),
               dw2=np.einsum("bijk,bijh->kh", g, z), abs_dw2=np.einsum("bijk,bijh->kh", np.abs(g), z),
               duv=np.concatenate([dz.sum(axis=2), dz.sum(axis=1)], axis=-1),
               abs_duv=np.concatenate([adz.sum(axis=2), adz.sum(axis=1)], axis=-1))
    return out


# ---------------------------------------------------------------------- the head
def head_uv(params, x):
    """params: ln.gamma, ln.beta [d], w1 [2H, d], b1 [2H] (w2, b2 are not read); x [T, d] -> dict(xh, rstd, y, uv [T, 2H])."""
    P = {k: f64(v) for k, v in params.items()}
    x = f64(x)
    mean = x.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(axis=1, keepdims=True) + LN_EPS)
    xh = (x - mean) * rstd
    y = xh * P["ln.gamma"][None, :] + P["ln.beta"][None, :]
    return dict(xh=xh, rstd=rstd, y=y, uv=y @ P["w1"].T + P["b1"][None, :])


def head_forward(params, x, seq, target=None, bpa=2.0, coef=1.0):
    B, L = np.shape(seq)
    a = head_uv(params, x)
    r = pair_head(a["uv"].reshape(B, L, -1), params["w2"], params["b2"], seq, target, bpa, coef)
    r.update(a)
    return r


def head_loss(params, x, seq, target, bpa=2.0):
    return float(head_forward(params, x, seq, target, bpa)["sums"][0])


def head_grads(params, x, seq, target, bpa=2.0, coef=1.0):
    """{name: d(coef x mean CE)/d(parameter)}, by hand."""
    P = {k: f64(v) for k, v in params.items()}
    r = head_forward(P, x, seq, target, bpa, coef)
    duv = r["duv"].reshape(-1, r["duv"].shape[-1])
    g = {"w2": r["dw2"], "b2": r["db2"], "w1": duv.T @ r["y"], "b1": duv.sum(axis=0)}
    dy = duv @ P["w1"]
    g["ln.gamma"], g["ln.beta"] = (dy * r["xh"]).sum(axis=0), dy.sum(axis=0)
    return g


# ---------------------------------------------------------------------- inputs of the device tests
def grid_uv(rng, B, L, H):
    """uv [B, L, 2H] fp32, multiples of 2^-8 in [-4, 4] with exact zeros and u_i = -v_j cases: u + v is exact in fp32 (and in
    fp64), so relu and its derivative at 0 take the same side in the kernel and here."""
    uv = (rng.integers(-1024, 1025, (B, L, 2 * H)) / 256.0).astype(np.float32)
    uv[rng.random(uv.shape) < 0.05] = 0.0
    for b in range(B):                                                            # v_j = -u_i on some (i, j, h)
        for _ in range(max(1, L // 2)):
            i, j, h = rng.integers(0, L), rng.integers(0, L), rng.integers(0, H)
            uv[b, j, H + h] = -uv[b, i, h]
    return uv
