"""Patch attribution restated in numpy float64 (what pg_token_attribution and SuperGuessr.attribute are tested against).

Definition (include/pigeon_hip.h, pg_token_attribution), for sample b, view p, token t, direction k:

    g[j]  = fp32( W[cells[b,k]][j] - W[against[b]][j] )      ONE fp32 rounding; W[cells[b,k]][j] itself where against[b] = -1 / None
    d     = sum_j h[b,p,t,j] * g[j]                           here: in float64 (the kernel: fp32, a fixed order)
    out   = d / (577 P)                                        here: in float64; the kernel: fp32( fp32(d) / fp32(577 P) ), one IEEE division

An index outside [0, C) (other than -1 in `against`) makes its column (cells) or its whole sample (against) NaN.

What is no token (`offset`), for the head  logit[c] = mean_p(e'_p) . W[c] + bias[c]  with  e_p = mean_t h[p,t,:]  and, on a de-biased
pass,  e'_p = e_p - |e_p|_2 beta:

    offset[b,k] = (bias[c] - bias[a]) - (1/P) sum_p |e_p|_2 (g . beta)          (the second term only with beta; bias[a] = 0 without a)

so that  out.sum over (p, t) + offset == logit[c] - logit[a]  exactly in real arithmetic (with g as rounded above).
"""
import numpy as np

TOKENS, HIDDEN = 577, 1024
U = 2.0 ** -24                                       # unit roundoff of fp32


def valid(cells, against, C):
    """(B,K) bool: the (b, k) columns whose indices the kernel accepts."""
    cells = np.asarray(cells, dtype=np.int64)
    B = cells.shape[0]
    a = np.full((B,), -1, dtype=np.int64) if against is None else np.asarray(against, dtype=np.int64)
    a_ok = (a == -1) | ((a >= 0) & (a < C))
    return ((cells >= 0) & (cells < C)) & a_ok[:, None]


def directions(W, cells, against=None):
    """(B,K,1024) fp32: g as the kernel forms it (one fp32 rounding); zeros where the column is not valid (see `valid`)."""
    W = np.asarray(W, dtype=np.float32)
    cells = np.asarray(cells, dtype=np.int64)
    C, B = W.shape[0], cells.shape[0]
    a = np.full((B,), -1, dtype=np.int64) if against is None else np.asarray(against, dtype=np.int64)
    ok = valid(cells, a, C)
    g = W[np.clip(cells, 0, C - 1)]                                           # (B,K,1024) fp32
    sub = np.where((a == -1)[:, None, None], np.float32(0), W[np.clip(a, 0, C - 1)][:, None, :])
    g = np.where((a == -1)[:, None, None], g, (g - sub).astype(np.float32))  # fp32 - fp32 in fp32: one rounding
    return np.where(ok[:, :, None], g, np.float32(0)).astype(np.float32)


def dots(hidden, W, cells, against=None, P=1, absolute=False):
    """(B,P,577,K) float64: d (absolute=False) or sum_j |h_j g_j| (absolute=True); NaN in columns that are not valid."""
    h = np.asarray(hidden, dtype=np.float32)
    n = h.shape[0]
    assert h.shape[1:] == (TOKENS, HIDDEN) and P >= 1 and n % P == 0
    B = n // P
    g = directions(W, cells, against).astype(np.float64)
    h = h.reshape(B, P * TOKENS, HIDDEN).astype(np.float64)
    if absolute:
        h, g = np.abs(h), np.abs(g)
    d = np.einsum("brj,bkj->brk", h, g).reshape(B, P, TOKENS, -1)
    ok = valid(cells, against, np.asarray(W).shape[0])
    return np.where(ok[:, None, None, :], d, np.nan)


def maps(hidden, W, cells, against=None, P=1):
    """(B,P,577,K) float64: the truth, d / (577 P)."""
    return dots(hidden, W, cells, against, P) / float(TOKENS * P)


def maps_exact_f32(hidden, W, cells, against=None, P=1):
    """(B,P,577,K) fp32 for inputs whose every partial sum is exact in fp32 (small integers): fp32(d) / fp32(577 P), one IEEE
    division -- what the kernel must return bit for bit, whatever its summation order."""
    d = dots(hidden, W, cells, against, P)
    assert np.nanmax(np.abs(d), initial=0.0) < 2 ** 24 and np.array_equal(np.nan_to_num(d), np.rint(np.nan_to_num(d)))
    return (d.astype(np.float32) / np.float32(TOKENS * P)).astype(np.float32)


def bound(hidden, W, cells, against=None, P=1):
    """(B,P,577,K) float64: the rounding bound of an fp32 dot product of 1024 terms in any order followed by one fp32 division:
    (1024 u sum_j |h_j g_j|) / (577 P) + u |truth|."""
    return HIDDEN * U * dots(hidden, W, cells, against, P, absolute=True) / float(TOKENS * P) + U * np.abs(maps(hidden, W, cells, against, P))


def embeddings(hidden):
    """(n,1024) float64: e = mean_t h[t,:]."""
    return np.asarray(hidden, dtype=np.float32).astype(np.float64).mean(axis=1)


def offset(W, bias, cells, against=None, norms=None, beta=None):
    """(B,K) float64: what is no token.  norms (B,P) = |e_p|_2 and beta (1024,) together, or neither."""
    W = np.asarray(W, dtype=np.float32)
    b = np.asarray(bias, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    C, B = W.shape[0], cells.shape[0]
    a = np.full((B,), -1, dtype=np.int64) if against is None else np.asarray(against, dtype=np.int64)
    off = b[np.clip(cells, 0, C - 1)] - np.where(a == -1, 0.0, b[np.clip(a, 0, C - 1)])[:, None]
    if beta is not None:
        gb = directions(W, cells, a).astype(np.float64) @ np.asarray(beta, dtype=np.float64)      # (B,K)
        off = off - np.asarray(norms, dtype=np.float64).mean(axis=1)[:, None] * gb
    return np.where(valid(cells, a, C), off, np.nan)


def logit_difference(hidden, W, bias, cells, against=None, P=1, beta=None):
    """(B,K) float64, computed the MODEL's way (token mean, de-bias, view mean, Linear with the fp32-rounded direction): what
    maps.sum((1,2)) + offset must reproduce."""
    e = embeddings(hidden)
    if beta is not None:
        e = e - np.linalg.norm(e, axis=1, keepdims=True) * np.asarray(beta, dtype=np.float64)[None, :]
    n = e.shape[0]
    q = e.reshape(n // P, P, HIDDEN).mean(axis=1)                                                  # (B,1024)
    g = directions(W, cells, against).astype(np.float64)
    b = np.asarray(bias, dtype=np.float64)
    C, cells = np.asarray(W).shape[0], np.asarray(cells, dtype=np.int64)
    a = np.full((cells.shape[0],), -1, dtype=np.int64) if against is None else np.asarray(against, dtype=np.int64)
    db = b[np.clip(cells, 0, C - 1)] - np.where(a == -1, 0.0, b[np.clip(a, 0, C - 1)])[:, None]
    return np.where(valid(cells, a, C), np.einsum("bj,bkj->bk", q, g) + db, np.nan)


# ---------------------------------------------------------------------------------------------- comparators
def compare_maps(got, want, tol=0.0):
    """Raise AssertionError naming the first (row, view, token, k) where `got` is not `want`: a different shape, a NaN on one side
    only, or |got - want| > tol (scalar or an array of want's shape; 0: equality)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.ndim != 4:
        raise AssertionError(f"maps: shape {got.shape}, expected (B,P,577,K) = {want.shape}")
    g, w = got.astype(np.float64), want.astype(np.float64)
    t = np.broadcast_to(np.asarray(tol, dtype=np.float64), w.shape)
    bad = (np.isnan(g) != np.isnan(w)) | (~np.isnan(w) & ~np.isnan(g) & ~(np.abs(g - w) <= t))
    if bad.any():
        b, p, tk, k = (int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"maps differ at row {b}, view {p}, token {tk}, k {k}: got {g[b, p, tk, k]!r}, expected "
                             f"{w[b, p, tk, k]!r} (tolerance {float(t[b, p, tk, k]):.3g}); {int(bad.sum())} of {bad.size} elements differ")


def compare_offset(got, want, tol=0.0):
    """The same for the (B,K) offsets (or logit differences): names (row, k)."""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape or got.ndim != 2:
        raise AssertionError(f"offset: shape {got.shape}, expected (B,K) = {want.shape}")
    g, w = got.astype(np.float64), want.astype(np.float64)
    t = np.broadcast_to(np.asarray(tol, dtype=np.float64), w.shape)
    bad = (np.isnan(g) != np.isnan(w)) | (~np.isnan(w) & ~np.isnan(g) & ~(np.abs(g - w) <= t))
    if bad.any():
        b, k = (int(i) for i in np.argwhere(bad)[0])
        raise AssertionError(f"offset differs at row {b}, k {k}: got {g[b, k]!r}, expected {w[b, k]!r} (tolerance {float(t[b, k]):.3g}); "
                             f"{int(bad.sum())} of {bad.size} elements differ")
