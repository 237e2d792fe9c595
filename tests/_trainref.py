"""The head-training step (csrc/head_train.hip; contract: include/pigeon_hip.h) restated in float64 / np.longdouble with math.fsum
sums, and the bounds the kernels are held to.  numpy only: no torch device, no GPU.  tests/test_trainref_cpu.py pins every function
here (the reference's recorded loss, a finite difference, torch.optim.AdamW) and shows that the comparisons reject the mistakes they
are for; tests/test_gpu_head_train.py holds the kernels to them.

  targets_smooth   y_c = exp(-(d_c - min d) / tau) with d from _georef.haversine_truth (longdouble), plus the relative error the
                   kernel's fp64 y_c may carry: its distances are within 16 U of the truth (_georef.U, the bound tests/test_gpu_geo.py
                   holds pg_haversine_matrix to), so the exponent t = (d - dmin) / tau moves by (16 U_c + 16 U_min) / tau, the
                   subtraction and the division add 2 eps t, exp one ulp:  rel_y = (16 U_c + 16 U_min) / tau + (t + 4) eps.
  targets_onehot   y_c = (c == label), exact.
  row_truth        from the fp32 logits l:  S = sum y, m = max l, e = exp(l - m), Z = sum e, T = sum y l,
                   loss = S (m + log Z) - T,  g = (S e / Z - y) grad_scale.  Bounds, with eps = 2^-52 and n = ceil(C / 256) + 8 additions
                   on the path of any summand (thread-strided, six butterfly levels, two levels of waves):
                     rel_e = (|l - m| + 4) eps           the difference of two fp32 values in fp64, then exp
                     rel_S = max rel_y + n eps,  rel_Z = max rel_e + n eps                     (all terms non-negative)
                     err_T = sum |y l| (max rel_y + (n + 1) eps)
                     loss:  |S (m + log Z)| (rel_S + 3 eps) + S (rel_Z + eps) + err_T + eps |loss|
                     g:     grad_scale (p (rel_S + rel_e + rel_Z + 3 eps) + y rel_y + eps |p - y|) + 2^-24 |g| + 2^-149,  p = S e / Z
                   -- the last two terms are the rounding of the result to fp32, which dominates everywhere.
  adamw_truth      torch.optim.AdamW's default update in float64 with the TRUE scalars:
                     w1 = w (1 - lr wd);  m' = b1 m + (1 - b1) d;  v' = b2 v + (1 - b2) d^2;
                     w' = w1 - (lr / (1 - b1^t)) m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
                   The kernel does the same in fp32 with scalars rounded to fp32 (u = 2^-24 each), one rounding per operation:
                     m'   fl(b1 m) then one fma:   bound_m = 2 u |b1 m| + u |(1 - b1) d| + u |m'| + 2^-149
                     v'   fl(d d), fl(b2 v), fma:   bound_v = 2 u b2 v + 2 u (1 - b2) d^2 + u v' + 2^-149
                     q    sqrt, division by bc2s, + eps:   rel_q = bound_v / (2 v') + 4 u     (v' = 0: q is eps rounded, u)
                     w'   bound_w = step (bound_m / q + |m' / q| (rel_q + 3 u)) + 2 u |w1| + u |w'| + 2^-149
                   m and v are also held to 2 ulp: for v (no cancellation) 2 ulp of v'; for m, whose two terms may cancel, 2 ulp of the
                   largest of |b1 m|, |(1 - b1) d| and |m'| -- with the default betas the roundings above sum to less than 1.7 ulp there.
  chain32          the fmaf chain both GEMMs are: acc = fl32(a_k b_k + acc) for k ascending from 0.f, evaluated in float64 per step
                   (the product of two fp32 values is exact in fp64; the sum is rounded once to fp64 and once to fp32, which is exact
                   whenever the partial sums are integers below 2^24 -- what the integer tests use it for).
"""
import math

import numpy as np

import _georef as G

LD = np.longdouble
EPS = 2.0 ** -52
U32 = 2.0 ** -24
TINY32 = 2.0 ** -149


# ------------------------------------------------------------------------------------------------ targets
def targets_smooth(labels, cen, tau, subtract_min=True):
    """labels (B,2), cen (C,2) fp64 [lng,lat] -> (y (B,C) longdouble, rel_y (B,C) float64)"""
    d, a = G.haversine_truth(np.asarray(labels, dtype=np.float64)[:, None, :], np.asarray(cen, dtype=np.float64)[None, :, :])
    u = G.U(a)
    j = np.argmin(d, axis=1)
    dmin = d[np.arange(d.shape[0]), j][:, None] if subtract_min else LD(0)
    umin = u[np.arange(d.shape[0]), j][:, None]
    t = (d - dmin) / LD(tau)
    y = np.exp(-t)
    rel = (16 * u + 16 * umin) / tau + (t.astype(np.float64) + 4) * EPS
    return y, rel


def targets_onehot(labels_clf, C, shift=0):
    lab = np.asarray(labels_clf, dtype=np.int64) + shift
    y = (np.arange(C)[None, :] == lab[:, None]).astype(LD)
    return y, np.zeros(y.shape)


def fsum_rows(x):
    return np.array([math.fsum(np.asarray(r, dtype=np.float64)) for r in x], dtype=np.float64)


# ------------------------------------------------------------------------------------------------ rows
def row_truth(logits, y, rel_y, grad_scale, use_S=True):
    """logits (B,C) fp32, y (B,C) longdouble, rel_y (B,C) -> dict of loss (B,), g (B,C), and their bounds, float64"""
    l32 = np.asarray(logits)
    assert l32.dtype == np.float32
    B, C = l32.shape
    l = l32.astype(LD)
    m = l.max(axis=1, keepdims=True)
    e = np.exp(l - m)
    S = fsum_rows(y).astype(LD)[:, None] if use_S else np.ones((B, 1), dtype=LD)
    Z = fsum_rows(e).astype(LD)[:, None]
    T = fsum_rows(y * l).astype(LD)[:, None]
    loss = (S * (m + np.log(Z)) - T)[:, 0]
    p = S * e / Z
    g = (p - y) * LD(grad_scale)
    n = math.ceil(C / 256) + 8
    rel_e = ((np.abs(l - m)).astype(np.float64) + 4) * EPS
    ry = rel_y.max(axis=1, keepdims=True)
    rel_S, rel_Z = ry + n * EPS, rel_e.max(axis=1, keepdims=True) + n * EPS
    err_T = fsum_rows(np.abs(y * l))[:, None] * (ry + (n + 1) * EPS)
    f = lambda v: np.asarray(v, dtype=np.float64)     # noqa: E731
    loss_bound = (np.abs(f(S * (m + np.log(Z)))) * (rel_S + 3 * EPS) + f(S) * (rel_Z + EPS) + err_T)[:, 0] + EPS * np.abs(f(loss))
    g_bound = abs(grad_scale) * (f(p) * (rel_S + rel_e + rel_Z + 3 * EPS) + f(y) * rel_y + EPS * np.abs(f(p - y))) + U32 * np.abs(f(g)) + TINY32
    return {"loss": f(loss), "loss_bound": loss_bound, "g": f(g), "g_bound": g_bound}


def loss_of(logits64, y, use_S=True):
    """the restated loss of float64 logits (for the finite difference): (B,) longdouble"""
    l = np.asarray(logits64, dtype=LD)
    m = l.max(axis=1, keepdims=True)
    S = y.sum(axis=1, keepdims=True) if use_S else LD(1)
    return (S * (m + np.log(np.exp(l - m).sum(axis=1, keepdims=True))) - (y * l).sum(axis=1, keepdims=True))[:, 0]


def grad_of(logits64, y, grad_scale=1.0, use_S=True):
    l = np.asarray(logits64, dtype=LD)
    m = l.max(axis=1, keepdims=True)
    e = np.exp(l - m)
    S = y.sum(axis=1, keepdims=True) if use_S else LD(1)
    return (S * e / e.sum(axis=1, keepdims=True) - y) * LD(grad_scale)


# ------------------------------------------------------------------------------------------------ the two products
def xbar_of(emb):
    """(B,P,1024) fp32 -> (B,1024) fp32: panels added in ascending order onto 0.f, then times 1.0f / P"""
    e = np.asarray(emb)
    assert e.dtype == np.float32 and e.ndim == 3
    acc = np.zeros((e.shape[0], e.shape[2]), dtype=np.float32)
    for p in range(e.shape[1]):
        acc = acc + e[:, p]
    return acc * (np.float32(1.0) / np.float32(e.shape[1]))


def chain32(A, Bm):
    """A (M,K), Bm (N,K) fp32 -> (M,N) fp32: acc = fl32(A[:,k] Bm[:,k] + acc), k ascending from 0.f"""
    A, Bm = np.asarray(A), np.asarray(Bm)
    assert A.dtype == np.float32 and Bm.dtype == np.float32
    acc = np.zeros((A.shape[0], Bm.shape[0]), dtype=np.float32)
    for k in range(A.shape[1]):
        acc = (A[:, k, None].astype(np.float64) * Bm[None, :, k].astype(np.float64) + acc.astype(np.float64)).astype(np.float32)
    return acc


def logits_of(xbar, W, bias):
    return chain32(xbar, W) + np.asarray(bias, dtype=np.float32)[None, :]


def grads_of(g, xbar):
    """dW (C,1024) = chain over b of g[b,c] xbar[b,j]; db (C,) = the fp32 sum of g[b,c], b ascending"""
    g, xbar = np.asarray(g), np.asarray(xbar)
    dW = chain32(np.ascontiguousarray(g.T), np.ascontiguousarray(xbar.T))
    db = np.zeros(g.shape[1], dtype=np.float32)
    for b in range(g.shape[0]):
        db = db + g[b]
    return dW, db


# ------------------------------------------------------------------------------------------------ AdamW
def adamw_truth(w, m, v, d, t, lr=2e-5, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.01, bias_correction_step=None, coupled=False):
    """float64 arrays in -> dict of the new w, m, v and the bounds of the fp32 kernel (see the module docstring)"""
    w, m, v, d = (np.asarray(x, dtype=np.float64) for x in (w, m, v, d))
    tb = t if bias_correction_step is None else bias_correction_step
    if coupled:
        d = d + wd * w
        w1 = w
    else:
        w1 = w * (1 - lr * wd)
    m2 = beta1 * m + (1 - beta1) * d
    v2 = beta2 * v + (1 - beta2) * d * d
    step = lr / (1 - beta1 ** tb) if tb > 0 else np.inf
    q = np.sqrt(v2) / math.sqrt(1 - beta2 ** tb) + eps if tb > 0 else np.full(v2.shape, np.nan)
    w2 = w1 - step * m2 / q
    bound_m = 2 * U32 * np.abs(beta1 * m) + U32 * np.abs((1 - beta1) * d) + U32 * np.abs(m2) + TINY32
    bound_v = 2 * U32 * beta2 * v + 2 * U32 * (1 - beta2) * d * d + U32 * v2 + TINY32
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_q = np.where(v2 > 0, bound_v / (2 * v2), 0.0) + 4 * U32
    bound_w = step * (bound_m / q + np.abs(m2 / q) * (rel_q + 3 * U32)) + 2 * U32 * np.abs(w1) + U32 * np.abs(w2) + TINY32
    return {"w": w2, "m": m2, "v": v2, "bound_w": bound_w, "bound_m": bound_m, "bound_v": bound_v,
            "m_scale": np.maximum(np.maximum(np.abs(beta1 * m), np.abs((1 - beta1) * d)), np.abs(m2))}


def ulp32(x):
    """the spacing of fp32 at |x| (float64 array), 2^-149 at the least"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.where(x > 0, x, 1.0)))
    return np.maximum(np.where(x > 0, 2.0 ** (np.maximum(e, -126.0) - 23), TINY32), TINY32)


# ------------------------------------------------------------------------------------------------ one whole step, for the planted mistakes
def step_truth(emb, W, bias, m_W, v_W, m_b, v_b, y, rel_y, t, mistake=None, **hyper):
    """A float64 step from fp32 emb (B,P,1024), W (C,1024), bias (C,) and float64 moments: panel mean and logits by the fp32 chains,
    row arithmetic and AdamW in float64.  `mistake` plants one of MISTAKES.  -> dict of loss (B,), g (B,C), dW, W, m_W, v_W, db, bias, m_b, v_b"""
    assert mistake is None or mistake in MISTAKES, mistake
    xbar = xbar_of(emb)
    logits = logits_of(xbar, W, bias)
    B, C = logits.shape
    r = row_truth(logits, y, rel_y, grad_scale=1.0 if mistake == "no_1_over_B" else 1.0 / B, use_S=mistake != "S_dropped")
    g = r["g"]
    if mistake == "g_transposed":                       # the (B,C) buffer read as (C,B)
        g = np.ascontiguousarray(g.reshape(C, B).T) if B != C else np.ascontiguousarray(g.T)
    dW = g.T @ xbar.astype(np.float64)
    db = g.sum(axis=0)
    kw = dict(hyper)
    if mistake == "betas_swapped":
        kw["beta1"], kw["beta2"] = hyper.get("beta2", 0.999), hyper.get("beta1", 0.9)
    bc = t - 1 if mistake == "bias_correction_t_minus_1" else None
    uw = adamw_truth(W, m_W, v_W, dW, t, bias_correction_step=bc, coupled=mistake == "coupled_decay", **kw)
    ub = adamw_truth(bias, m_b, v_b, db, t, bias_correction_step=bc, coupled=mistake == "coupled_decay", **kw)
    if mistake == "bias_not_updated":
        ub = dict(ub, w=np.asarray(bias, dtype=np.float64), m=np.asarray(m_b, dtype=np.float64), v=np.asarray(v_b, dtype=np.float64))
    return {"loss": r["loss"], "loss_bound": r["loss_bound"], "g": r["g"], "g_bound": r["g_bound"], "dW": dW, "db": db,
            "W": uw["w"], "m_W": uw["m"], "v_W": uw["v"], "W_bound": uw["bound_w"], "bias": ub["w"], "m_b": ub["m"], "v_b": ub["v"],
            "bias_bound": ub["bound_w"]}


MISTAKES = ("S_dropped", "no_rowmin", "no_1_over_B", "g_transposed", "bias_correction_t_minus_1", "coupled_decay", "betas_swapped",
            "bias_not_updated", "onehot_off_by_one", "neighbour_label")


def offenders(name, got, truth, bound, axes):
    """-> the elements of `got` outside `bound` of `truth`, worst first, as strings naming their index along `axes` (('row', 'cell'),
    ('cell', 'column'), ...).  NaN in `got` where the truth is finite is an offender."""
    got, truth, bound = (np.asarray(x, dtype=np.float64) for x in (got, truth, bound))
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.abs(got - truth) / bound
    ratio = np.where(np.isnan(got) != np.isnan(truth), np.inf, np.where(np.isnan(truth), 0.0, ratio))
    idx = np.argwhere(ratio > 1)
    order = np.argsort(-ratio[tuple(idx.T)], kind="stable") if len(idx) else []
    return [f"{name}[" + ", ".join(f"{a} {int(i)}" for a, i in zip(axes, idx[o])) + f"]: got {got[tuple(idx[o])]!r}, truth "
            f"{truth[tuple(idx[o])]!r}, {ratio[tuple(idx[o])]:.3g} x the bound" for o in order]
