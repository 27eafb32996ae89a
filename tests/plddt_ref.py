"""fp64 numpy restatement of the binned-lDDT loss (include/ptamd.h, `ptamd_plddt_fwd` / `ptamd_plddt_bwd`) and of the whole
confidence head (protein_transformer_amd/confidence.py: LayerNorm -> Linear -> ReLU -> Linear -> that loss) with every gradient, for
tests/test_plddt_ref.py (CPU) and the MI355X tests tests/test_gpu_plddt.py and tests/test_gpu_confidence.py.

Everything is fp64 on the fp32 inputs except the bin of a target, which is DEFINED in fp32: floorf(target * nbins) with one fp32
multiply - a target one ulp under an edge k / nbins may round up onto it, and the definition says which bin that is."""
import numpy as np

LN_EPS = 1e-5                                        # torch.nn.LayerNorm's, as csrc/elementwise.hip
NAMES = ("ln.gamma", "ln.beta", "w1", "b1", "w2", "b2")


def bin_index(target, nbins):
    """target [T] -> (counted bool [T], bin int [T]; 0 where the row does not count): min(nbins - 1, max(0, floorf(t * nbins)))
    with the product rounded to fp32 once."""
    t = np.asarray(target, np.float32)
    counted = np.isfinite(t)
    with np.errstate(over="ignore", invalid="ignore"):
        f = np.floor(np.where(counted, t, np.float32(0)) * np.float32(nbins))
    assert f.dtype == np.float32
    return counted, np.clip(f.astype(np.float64), 0, nbins - 1).astype(np.int64)


def softmax64(logits):
    x = np.asarray(logits, np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def log_softmax64(logits):
    x = np.asarray(logits, np.float64)
    d = x - x.max(axis=1, keepdims=True)
    return d - np.log(np.exp(d).sum(axis=1, keepdims=True))


def plddt64(logits):
    """logits [T, nbins] -> 100 sum_k p_k (k + 0.5) / nbins."""
    nbins = np.shape(logits)[1]
    return 100.0 * (softmax64(logits) * ((np.arange(nbins) + 0.5) / nbins)[None, :]).sum(axis=1)


def bin_loss(logits, target=None):
    """logits [T, nbins] (the used columns only), target [T] fp32 or None -> dict(plddt [T], ce [T] (NaN where the row does not
    count), sums [2] = {mean ce or NaN, count}, counted, bin).  -log p_bin is taken from the log-softmax, and where the bin holds
    the row's maximum from log1p of the other lanes' sum: exact to fp64 also for a loss of 1e-30."""
    x = np.asarray(logits, np.float64)
    T, nbins = x.shape
    out = {"plddt": plddt64(x)}
    if target is None:
        return out
    counted, b = bin_index(target, nbins)
    rows = np.arange(T)
    d = x - x.max(axis=1, keepdims=True)
    e = np.exp(d)
    e_wo = e.copy()
    e_wo[rows, b] = 0.0
    others = e_wo.sum(axis=1)
    ce = np.where(d[rows, b] == 0.0, np.log1p(others), np.log(e.sum(axis=1)) - d[rows, b])
    ce = np.where(counted, ce, np.nan)
    n = int(counted.sum())
    out.update(ce=ce, counted=counted, bin=b, others=others, esum=e.sum(axis=1), e=e,
               sums=np.array([ce[counted].sum() / n if n else np.nan, float(n)]))
    return out


def bin_loss_grad(logits, target, coef=1.0):
    """d(coef x mean ce)/d(logits) [T, nbins]: coef / n (p - onehot) on counted rows, 0 elsewhere and when n = 0.  p_bin - 1 is
    -(sum of the others) / (sum of all), without the cancellation."""
    r = bin_loss(logits, target)
    T, nbins = np.shape(logits)
    n = int(r["counted"].sum())
    g = np.zeros((T, nbins))
    if n == 0:
        return g
    p = r["e"] / r["esum"][:, None]
    rows = np.arange(T)
    p[rows, r["bin"]] = -r["others"] / r["esum"]
    g[r["counted"]] = coef / n * p[r["counted"]]
    return g


# ---------------------------------------------------------------------- the head
def f64(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.float64)


def head_logits(params, x):
    """params {name: array}: ln.gamma, ln.beta [d], w1 [h, d], b1 [h], w2 [nbins, h], b2 [nbins]; x [T, d] -> dict of the
    activations: xh, rstd, y (LayerNorm), h (ReLU(y w1^T + b1)), logits."""
    P = {k: f64(v) for k, v in params.items()}
    x = f64(x)
    mean = x.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(axis=1, keepdims=True) + LN_EPS)
    xh = (x - mean) * rstd
    y = xh * P["ln.gamma"][None, :] + P["ln.beta"][None, :]
    z = y @ P["w1"].T + P["b1"][None, :]
    h = np.maximum(z, 0.0)
    return dict(xh=xh, rstd=rstd, y=y, z=z, h=h, logits=h @ P["w2"].T + P["b2"][None, :])


def head_loss(params, x, target):
    """The mean cross-entropy over the counted rows (NaN when there is none)."""
    return float(bin_loss(head_logits(params, x)["logits"], target)["sums"][0])


def head_grads(params, x, target, coef=1.0):
    """{name: d(coef x mean ce)/d(parameter)}, by hand, plus "dlogits"."""
    P = {k: f64(v) for k, v in params.items()}
    a = head_logits(P, x)
    dl = bin_loss_grad(a["logits"], target, coef)
    g = {"dlogits": dl, "w2": dl.T @ a["h"], "b2": dl.sum(axis=0)}
    dz = (dl @ P["w2"]) * (a["z"] > 0)
    g["w1"], g["b1"] = dz.T @ a["y"], dz.sum(axis=0)
    dy = dz @ P["w1"]
    g["ln.gamma"], g["ln.beta"] = (dy * a["xh"]).sum(axis=0), dy.sum(axis=0)
    return g
