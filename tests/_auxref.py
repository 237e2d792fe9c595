"""float64 restatement of pg_aux_heads_forward (csrc/aux_heads.hip) for the tests: the auxiliary heads' outputs, the two argmaxes in
torch's order, the tolerance of the two argmaxes over EVERY alternative class (the `_tol` of tests/test_gpu_certainty.py, i.e. the head
row of certainty.hip's table), and the rounding bound an fp32 evaluation of an output may differ from the exact value by.

    preds[b][a] = mean_p(emb[b]) . W[a] + bias[a]               rows of W: [regression | climate | month]
    cls[b]      = (argmax climate, argmax month), -1 where the classifier has no outputs
    tol[b]      = min over the alternatives c of both classifiers of (m - |e| g.beta) / (|e| |g| / 32),
                  m = preds[c0] - preds[c],  g = W[c0] - W[c];   +inf without alternatives, 0 where a margin is NaN
    code[b]     = 1 + c (climate class c sets tol), 101 + c (month class c), 0 (nothing does: tol = +inf)
"""
import numpy as np

DIM = 1024


def first_argmax(v) -> int:
    """torch.argmax's order: a NaN ranks above every number, ties go to the lowest index."""
    v = np.asarray(v, dtype=np.float64)
    nan = np.isnan(v)
    if nan.any():
        return int(np.nonzero(nan)[0][0])
    return int(np.argmax(v))                              # numpy: first occurrence of the maximum


def panel_mean(emb) -> np.ndarray:
    """(B, P, 1024) or (B, 1024) -> (B, 1024) float64"""
    emb = np.asarray(emb, dtype=np.float64)
    return emb.mean(axis=1) if emb.ndim == 3 else emb


def preds(emb, W, bias) -> np.ndarray:
    return panel_mean(emb) @ np.asarray(W, dtype=np.float64).T + np.asarray(bias, dtype=np.float64)[None, :]


def tol_of(m: float, g: np.ndarray, beta: np.ndarray, en: float) -> float:
    if np.isnan(m):
        return 0.0
    g2 = float(g @ g)
    if np.isnan(g2):
        return 0.0
    if g2 == 0:
        return np.inf
    t = (m - en * float(g @ beta)) / (en * np.sqrt(g2) / 32.0)
    return 0.0 if np.isnan(t) else t


def row(p, e, W, n_reg, n_climate, n_month, beta=None):
    """One row: p (A,) the outputs the decisions are taken on, e (1024,) the panel mean -> (cls (2,), tol, code)."""
    p = np.asarray(p, dtype=np.float64)
    W = np.asarray(W, dtype=np.float64)
    beta = np.zeros(DIM) if beta is None else np.asarray(beta, dtype=np.float64)
    en = float(np.linalg.norm(e))
    cls, best, code = [-1, -1], np.inf, 0
    for which, (off, n, base) in enumerate(((n_reg, n_climate, 1), (n_reg + n_climate, n_month, 101))):
        if n == 0:
            continue
        c0 = first_argmax(p[off:off + n])
        cls[which] = c0
        for c in range(n):
            if c == c0:
                continue
            t = tol_of(p[off + c0] - p[off + c], W[off + c0] - W[off + c], beta, en)
            if t < best:                                   # equal tolerances: the alternative visited first keeps it
                best, code = t, base + c
    return cls, best, code


def forward(emb, W, bias, n_reg, n_climate, n_month, beta=None, preds_from=None):
    """All rows.  `preds_from`: take the decisions on these outputs (e.g. the kernel's own fp32 ones) instead of the float64 ones.
    Returns dict(preds (B,A) f64, cls (B,2) i64, tol (B,) f64, code (B,) i64)."""
    P = preds(emb, W, bias)
    D = P if preds_from is None else np.asarray(preds_from, dtype=np.float64)
    E = panel_mean(emb)
    out = [row(D[b], E[b], W, n_reg, n_climate, n_month, beta) for b in range(P.shape[0])]
    return dict(preds=P, cls=np.array([o[0] for o in out], dtype=np.int64).reshape(-1, 2),
                tol=np.array([o[1] for o in out], dtype=np.float64), code=np.array([o[2] for o in out], dtype=np.int64))


def bound(emb, W, bias) -> np.ndarray:
    """(B, A) float64: how far an fp32 evaluation of preds[b][a] may be from the exact value, whatever its summation order --
    (1024 + P + 2) 2^-24 (|mean_p e| |W[a]| + |bias[a]|): K products, P panel adds, one scale, one bias add (textbook forward bound
    gamma_n |x|.|w| <= gamma_n |x|_2 |w|_2, unit roundoff 2^-24)."""
    emb = np.asarray(emb)
    P = emb.shape[1] if emb.ndim == 3 else 1
    en = np.linalg.norm(panel_mean(emb), axis=-1)
    wn = np.linalg.norm(np.asarray(W, dtype=np.float64), axis=-1)
    return (DIM + P + 2) * 2.0 ** -24 * (en[:, None] * wn[None, :] + np.abs(np.asarray(bias, dtype=np.float64))[None, :])
