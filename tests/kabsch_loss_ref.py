"""The yardstick of the superposition loss (csrc/kabsch_loss.hip, `train.py -l kabsch`): the definition of include/ptamd.h
(`ptamd_kabsch_loss_fwd_bwd`) restated in plain numpy fp64, and the cases of tests/test_gpu_kabsch_loss.py.  TEST INFRASTRUCTURE
ONLY: the product never imports it.  Pinned by tests/test_kabsch_loss_ref.py without a GPU.

The rotation comes from an SVD with the determinant correction (Kabsch 1978) - a route that shares nothing with the kernel's, which
is Horn's quaternion eigenvector (csrc/tm_rotation.h).  `horn_rotation` carries that header's arithmetic over to Python, so that
the two routes can be held against each other on the very inputs the GPU test uses."""
import functools

import numpy as np

PAD, SLOTS = 20, 14


def present_slots(true, seq):
    """true [L*14,3], seq [L] -> bool [L*14]: the residue is not PAD and no true coordinate of the atom is NaN."""
    true, seq = np.asarray(true), np.asarray(seq)
    assert true.shape == (len(seq) * SLOTS, 3)
    return np.repeat(seq != PAD, SLOTS) & ~np.isnan(true).any(1)


def svd_rotation(a, b):
    """a, b [n,3] centred fp64 -> the proper rotation R (det = +1, column vectors: R a_k lies on b_k) that minimises
    sum |R a_k - b_k|^2."""
    u, _, vt = np.linalg.svd(a.T @ b)                             # S = sum a b^T = U diag(s) V^T;  R = V diag(1, 1, d) U^T
    d = 1.0 if np.linalg.det(u) * np.linalg.det(vt) >= 0 else -1.0
    return vt.T @ np.diag([1.0, 1.0, d]) @ u.T


def kabsch_loss_reference(pred, true, seq):
    """One protein, whatever the arrays hold read as fp64 -> dict(loss, n, grad [L*14,3], R, rg, slots): loss = sqrt(sum |r_k|^2 /
    n) with r_k = R (a_k - abar) - (b_k - bbar), grad = R^T r_k / (n loss) at the present slots and exactly zero elsewhere; rg, the
    RMS distance of the present true atoms from their mean, is the protein's length scale.  n < 3, or a non-finite coordinate on a
    present atom: loss NaN, gradient zero.  loss == 0: gradient zero, nothing divided."""
    pred, true = np.asarray(pred, np.float64).reshape(-1, 3), np.asarray(true, np.float64).reshape(-1, 3)
    m = present_slots(true, seq)
    a, b, n = pred[m], true[m], int(m.sum())
    out = dict(loss=float("nan"), n=n, grad=np.zeros_like(pred), R=None, rg=float("nan"), slots=np.nonzero(m)[0])
    if n < 3 or not (np.isfinite(a).all() and np.isfinite(b).all()):
        return out
    ac, bc = a - a.mean(0), b - b.mean(0)
    R = svd_rotation(ac, bc)
    r = ac @ R.T - bc
    loss = float(np.sqrt((r * r).sum() / n))
    if loss > 0:
        out["grad"][m] = (r @ R) / (n * loss)
    out.update(loss=loss, R=R, rg=float(np.sqrt((bc * bc).sum() / n)))
    return out


def horn_rotation(a, b):
    """tm_rotation::solve of csrc/tm_rotation.h, statement for statement, on the moments of the centred a, b [n,3] fp64: Horn's
    symmetric 4x4 matrix, cyclic Jacobi with the rotations accumulated, the eigenvector of the largest eigenvalue as a unit
    quaternion -> R (column vectors)."""
    S = a.T @ b
    A = np.empty((4, 4))
    A[0, 0] = S[0, 0] + S[1, 1] + S[2, 2]
    A[1, 1] = S[0, 0] - S[1, 1] - S[2, 2]
    A[2, 2] = -S[0, 0] + S[1, 1] - S[2, 2]
    A[3, 3] = -S[0, 0] - S[1, 1] + S[2, 2]
    A[0, 1] = A[1, 0] = S[1, 2] - S[2, 1]
    A[0, 2] = A[2, 0] = S[2, 0] - S[0, 2]
    A[0, 3] = A[3, 0] = S[0, 1] - S[1, 0]
    A[1, 2] = A[2, 1] = S[0, 1] + S[1, 0]
    A[1, 3] = A[3, 1] = S[2, 0] + S[0, 2]
    A[2, 3] = A[3, 2] = S[1, 2] + S[2, 1]
    V = np.eye(4)
    for _ in range(30):
        off = sum(abs(A[i, j]) for i in range(4) for j in range(i + 1, 4))
        if off <= 1e-20 * sum(abs(A[i, i]) for i in range(4)):
            break
        for p in range(3):
            for q in range(p + 1, 4):
                apq = A[p, q]
                if apq == 0.0:
                    continue
                theta = (A[q, q] - A[p, p]) / (2.0 * apq)
                t = (1.0 if theta >= 0.0 else -1.0) / (abs(theta) + np.sqrt(theta * theta + 1.0))
                c = 1.0 / np.sqrt(t * t + 1.0)
                s = t * c
                A[p, p] -= t * apq
                A[q, q] += t * apq
                A[p, q] = A[q, p] = 0.0
                for r in range(4):
                    if r != p and r != q:
                        arp, arq = A[r, p], A[r, q]
                        A[r, p] = A[p, r] = c * arp - s * arq
                        A[r, q] = A[q, r] = s * arp + c * arq
                    vrp, vrq = V[r, p], V[r, q]
                    V[r, p] = c * vrp - s * vrq
                    V[r, q] = s * vrp + c * vrq
    k = 0
    tie = 64.0 * 2.220446049250313e-16 * sum(abs(A[i, i]) for i in range(4))
    for j in range(1, 4):                                          # the first of eigenvalues that are equal to Jacobi's rounding
        if A[j, j] > A[k, k] + tie:
            k = j
    qw, qx, qy, qz = V[:, k] / np.linalg.norm(V[:, k])
    return np.array([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qw * qz), 2 * (qx * qz + qw * qy)],
                     [2 * (qx * qy + qw * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qw * qx)],
                     [2 * (qx * qz - qw * qy), 2 * (qy * qz + qw * qx), 1 - 2 * (qx * qx + qy * qy)]])


# ----------------------------------------------------------------------------- cases
def rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def chain(n_res, rng):
    """A chiral all-atom cloud of n_res residues, [n_res*14,3] fp64: a random walk of residue centres (3.8 A steps) with the 14
    slots of a residue scattered 1.5 A around its centre."""
    steps = rng.normal(size=(n_res, 3))
    centres = np.cumsum(3.8 * steps / np.linalg.norm(steps, axis=1, keepdims=True), 0)
    return (centres[:, None, :] + rng.normal(0, 1.5, (n_res, SLOTS, 3))).reshape(-1, 3)


def row(pred, true, L, rng):
    """pred, true [n_res*14,3] -> (pred [L*14,3] fp32, true [L*14,3] fp32, seq [L]): the protein in a row of L residues; the pad
    residues carry zeros in the truth (as collate pads) and finite garbage in the prediction."""
    n_res = len(true) // SLOTS
    assert len(pred) == len(true) == n_res * SLOTS and n_res <= L
    p = rng.normal(0, 50, (L * SLOTS, 3)).astype(np.float32)
    t = np.zeros((L * SLOTS, 3), np.float32)
    p[:len(pred)], t[:len(true)] = pred, true
    seq = np.full(L, PAD, np.int64)
    seq[:n_res] = rng.integers(0, 20, n_res)
    return p, t, seq


def moved(x, rng, shift=3.0):
    """a rigid motion of x, in fp64"""
    return x @ rotation(rng).T + rng.normal(0, shift, 3)


def only(true, keep):
    """`true` with every slot but `keep` absent"""
    out = np.full_like(true, np.nan)
    out[list(keep)] = true[list(keep)]
    return out


@functools.lru_cache(maxsize=None)
def proteins(L):
    """name -> (pred, true, seq), rows of L residues: every edge of the issue that fits into L residues.  Deterministic."""
    rng = np.random.default_rng(1000 + L)
    out = {}

    def add(name, pred, true):
        out[name] = row(pred, true, L, rng)

    t = chain(L, rng)                                             # a full row, NaN truth at the first slot, the last one and others
    holes = np.unique(np.concatenate([[0, L * SLOTS - 1], rng.choice(L * SLOTS, max(1, L * SLOTS // 9), replace=False)]))
    if L == 1:
        holes = np.array([0, SLOTS - 1])
    th = t.copy()
    th[holes] = np.nan
    add("noisy", moved(t, rng) + rng.normal(0, 0.5, t.shape), th)
    add("three", moved(t, rng) + rng.normal(0, 0.5, t.shape), only(t, (1, 5, L * SLOTS - 2)))
    add("two", moved(t, rng) + rng.normal(0, 0.5, t.shape), only(t, (2, L * SLOTS - 1)))
    add("none", moved(t, rng), only(t, ()))
    add("mirror", t * np.array([1.0, 1.0, -1.0]), th)
    if L >= 5:
        s = chain(L - 2, rng)                                     # shorter than the row
        sh = s.copy()
        sh[rng.choice(len(s), len(s) // 7, replace=False)] = np.nan
        add("short", moved(s, rng) + rng.normal(0, 1.0, s.shape), sh)
        copy = s.astype(np.float32).astype(np.float64)             # the truth as the kernel reads it
        add("rigid", moved(copy, rng), sh)                        # ... rotated and shifted in fp64, rounded to fp32 once
        garbage = np.where(np.isnan(sh), rng.normal(0, 50, s.shape), copy)          # what absent slots predict is never read
        add("copy", garbage, np.where(np.isnan(sh), np.nan, copy))
        add("far", moved(s, rng) + rng.normal(0, 0.5, s.shape) + 1e3, sh)
    if L >= 19:
        bad = int(np.nonzero(~np.isnan(th).any(1))[0][7])         # a present atom of "noisy"
        base = out["noisy"]
        for name, value in (("nan-pred", np.nan), ("inf-pred", np.inf)):
            p = base[0].copy()
            p[bad, 1] = value
            out[name] = (p, base[1], base[2])
        t2 = base[1].copy()
        t2[bad] = np.nan                                          # the same atom made absent: the NaN is never read
        p2 = out["nan-pred"][0]
        out["nan-pred-absent"] = (p2, t2, base[2])
        p3 = base[0].copy()
        p3[bad] = 7.0
        out["finite-pred-absent"] = (p3, t2, base[2])             # ... and gives the bits of any finite value there
    return out


UNUSABLE = ("nan-pred", "inf-pred")
LENGTHS = (1, 5, 19, 37)


def batch(L, names=None):
    """(names, pred [B,L*14,3], true, seq [B,L]) of `proteins(L)`, in their order or the given one."""
    ps = proteins(L)
    names = list(ps) if names is None else list(names)
    return names, *(np.stack([ps[n][k] for n in names]) for k in range(3))


@functools.lru_cache(maxsize=None)
def reference(L, name):
    return kabsch_loss_reference(*proteins(L)[name])
