"""numpy restatement of the k-nearest-neighbour contract (include/pigeon_hip.h, csrc/knn.hip): the distance in float64 and as the
fp32 chain, the ordering rule, the 16-bit pass with its error bound and certificate, the comparators the GPU tests use, and the
banks they search.  No GPU, no torch."""
import numpy as np

D = 1024
KP = 128                                   # K': candidates the 16-bit pass keeps per query
U = 2.0 ** -24
GAMMA = 1030 * U                           # the exact stage's own relative error (1026 u, and the second order)


# ---------------------------------------------------------------------------------------------------------------------- the distance
def d2_f64(Q, X):
    """(B,N) float64: the true squared distances."""
    Q = np.asarray(Q, np.float64); X = np.asarray(X, np.float64)
    out = np.empty((Q.shape[0], X.shape[0]))
    for b in range(Q.shape[0]):
        t = Q[b][None, :] - X
        out[b] = np.einsum("nj,nj->n", t, t)
    return out


def d2_chain(Q, X):
    """(B,N) float32: the contract's chain, step by step -- t = fp32(q - x), acc = fp32(t * t + acc), j ascending.  t * t is exact
    in float64 (two 24-bit factors); the sum is rounded to float64 and then to fp32, which equals the fused fp32 result whenever
    the float64 sum is exact -- always when the partial sums are integers below 2^24, the case the exact tests use."""
    Q = np.asarray(Q, np.float32); X = np.asarray(X, np.float32)
    acc = np.zeros((Q.shape[0], X.shape[0]), np.float32)
    with np.errstate(all="ignore"):
        for j in range(Q.shape[1]):
            t = (Q[:, j][:, None] - X[:, j][None, :]).astype(np.float32).astype(np.float64)
            acc = (t * t + acc.astype(np.float64)).astype(np.float32)
    return acc


# ---------------------------------------------------------------------------------------------------------------------- the order
def order(d):
    """Row indices of one query's distances in the contract's order: ascending, ties to the lower row, NaN after +inf."""
    d = np.asarray(d)
    nan = np.isnan(d)
    return np.lexsort((np.arange(d.shape[0]), np.where(nan, 0, d), nan))


def topk(d, k, exclude=None):
    """d (B,N) -> idx (B,k) int64, d2 (B,k) of d's dtype: the contract's result for these distances; -1 / +inf past the end."""
    B, N = d.shape
    idx = np.full((B, k), -1, np.int64)
    out = np.full((B, k), np.inf, d.dtype)
    for b in range(B):
        o = order(d[b])
        if exclude is not None and 0 <= int(exclude[b]) < N:
            o = o[o != int(exclude[b])]
        o = o[:k]
        idx[b, :o.size] = o
        out[b, :o.size] = d[b, o]
    return idx, out


# ---------------------------------------------------------------------------------------------------------------------- the 16-bit pass
def half_norms(X):
    """hn = fp32(0.5 sum x^2), summed in float64."""
    X = np.asarray(X, np.float32).astype(np.float64)
    return (0.5 * np.einsum("nj,nj->n", X, X)).astype(np.float32)


def filter_keys(Q, X):
    """(B,N) float32: a(q,x) = fp32(hn[x] - S), S the fp32 rounding of the exact sum of the fp16 products -- the MFMA with an ideal
    accumulation.  The hardware's own order and rounding are inside eps()."""
    q16 = np.asarray(Q, np.float32).astype(np.float16).astype(np.float64)
    x16 = np.asarray(X, np.float32).astype(np.float16).astype(np.float64)
    S = (q16 @ x16.T).astype(np.float32)
    return (half_norms(X)[None, :] - S).astype(np.float32)


def filter_error(Q, X):
    """(B,N) float64: |a(q,x) - (0.5 d2_true - 0.5 |q|^2)|, what eps() must bound."""
    Q64 = np.asarray(Q, np.float32).astype(np.float64)
    want = 0.5 * d2_f64(Q, X) - 0.5 * np.einsum("bj,bj->b", Q64, Q64)[:, None]
    return np.abs(filter_keys(Q, X).astype(np.float64) - want)


def xmax_of(X):
    """The bank's largest row norm as the kernel takes it: from the largest fp32 half norm, 2^-22 high."""
    return float(np.sqrt(2.0 * float(half_norms(X).max()) * (1.0 + 4.0 * U)))


def eps(qnorm, xmax):
    """The bound on the 16-bit pass's error for a query of norm Q over a bank whose row norms are at most X (derivation: knn.hip):
         conversions    2^-10 Q X     both operands rounded to fp16, 2^-11 relative each, Cauchy-Schwarz
         subnormals     2^-20 (Q+X) + 2^-40   an fp16 subnormal is off by up to 2^-25 absolutely; |v|_1 <= 32 |v|_2
         accumulation   2^-13 Q X     1024 fp32 additions in an unknown order, at most 2 u each (truncation allowed)
         hn             2^-25 X^2     summed in fp64, rounded once
         subtraction    2^-24 (0.5 X^2 + Q X)
       times 1.01 for every second-order term."""
    Q, X = np.asarray(qnorm, np.float64) * (1.0 + 1e-12), float(xmax)
    return 1.01 * ((2.0 ** -10 + 2.0 ** -13 + U) * Q * X + U * X * X + 2.0 ** -20 * (Q + X) + 2.0 ** -40)


def candidates(Q, X):
    """The 16-bit pass restated: per query the KP rows of smallest (key, row) and the KP-th key (the cutoff)."""
    a = filter_keys(Q, X)
    cand, cutoff = [], []
    for b in range(a.shape[0]):
        o = order(a[b])[:KP]
        cand.append(o)
        cutoff.append(a[b, o[-1]])
    return cand, np.asarray(cutoff, np.float32)


def certify(Q, X, k, exclude=None, d2=None):
    """The whole fast path restated: (idx, d2, certified) of filter + rerank + certificate, d2 from d2_chain unless given."""
    Q = np.asarray(Q, np.float32); X = np.asarray(X, np.float32)
    B, N = Q.shape[0], X.shape[0]
    d2 = d2_chain(Q, X) if d2 is None else d2
    cand, cutoff = candidates(Q, X)
    idx = np.full((B, k), -1, np.int64)
    out = np.full((B, k), np.inf, np.float32)
    cert = np.zeros(B, bool)
    xm = xmax_of(X)
    for b in range(B):
        c = cand[b]
        if exclude is not None:
            c = c[c != int(exclude[b])]
        o = np.asarray(sorted(c.tolist(), key=lambda r: (np.isnan(d2[b, r]), 0 if np.isnan(d2[b, r]) else d2[b, r], r)), np.int64)[:k]
        idx[b, :o.size] = o
        out[b, :o.size] = d2[b, o]
        if N <= KP:
            cert[b] = True
            continue
        q64 = Q[b].astype(np.float64)
        qq = float(q64 @ q64)
        lb = 2.0 * (float(cutoff[b]) - float(eps(np.sqrt(qq), xm))) + qq * (1.0 - 1e-12)
        ok = np.all(np.abs(Q[b]) <= 65504) and lb > 0 and o.size == k and float(out[b, k - 1]) < lb * (1.0 - GAMMA)
        cert[b] = bool(ok)
    return idx, out, cert


# ---------------------------------------------------------------------------------------------------------------------- comparators
def compare_exact(idx, d2, ref_idx, ref_d2, what=""):
    """Every row and every distance equal, bit for bit (a NaN equals a NaN); the first difference is named."""
    idx, d2, ref_idx, ref_d2 = np.asarray(idx), np.asarray(d2), np.asarray(ref_idx), np.asarray(ref_d2)
    assert idx.shape == ref_idx.shape and d2.shape == ref_d2.shape, f"{what}: shapes {idx.shape} {d2.shape} against {ref_idx.shape} {ref_d2.shape}"
    bad_i = idx != ref_idx
    same_d = (d2 == ref_d2) | (np.isnan(d2) & np.isnan(ref_d2))
    bad = bad_i | ~same_d
    if bad.any():
        b, p = np.argwhere(bad)[0]
        raise AssertionError(f"{what}: query {b} position {p}: row {idx[b, p]} d2 {d2[b, p]!r}, expected row {ref_idx[b, p]} d2 {ref_d2[b, p]!r} "
                             f"({int(bad.sum())} of {bad.size} differ)")


def compare_truth(idx, d2, Q, X, k, exclude=None, d64=None):
    """The result against the float64 distances.  Every reported d2 within 1030 * 2^-24 * d of the float64 distance OF THE ROW
    REPORTED; the list ascending, equal values by row; no excluded, repeated or impossible row; at a position whose float64
    distance is further from both neighbours in the float64 order than the two bounds together, the row is the truth's; elsewhere
    the row's float64 distance lies within the two bounds of the truth's at that position (a row can only change places with one
    whose computed value can cross its own).  Returns the number of such ambiguous positions and the number of positions."""
    idx, d2 = np.asarray(idx), np.asarray(d2)
    d64 = d2_f64(Q, X) if d64 is None else d64
    B, N = d64.shape
    assert idx.shape == (B, k) and d2.shape == (B, k), f"shapes {idx.shape} {d2.shape}, expected {(B, k)}"
    ambiguous = total = 0
    for b in range(B):
        ex = -1 if exclude is None else int(exclude[b])
        t_rows = order(d64[b])
        if 0 <= ex < N:
            t_rows = t_rows[t_rows != ex]
        t_d = d64[b, t_rows]
        valid = min(k, t_rows.size)
        seen = set()
        for p in range(k):
            r, v = int(idx[b, p]), float(d2[b, p])
            where = f"query {b} position {p}"
            if p >= valid:
                assert r == -1 and v == np.inf, f"{where}: row {r} d2 {v} past the bank's end, expected -1 / inf"
                continue
            total += 1
            assert 0 <= r < N, f"{where}: row {r} is no row of the bank"
            assert r != ex, f"{where}: the excluded row {r} was returned"
            assert r not in seen, f"{where}: row {r} returned twice"
            seen.add(r)
            true = d64[b, r]
            assert abs(v - true) <= GAMMA * true, f"{where}: d2 {v!r} of row {r}, float64 {true!r}: off by {abs(v - true):.3e} > {GAMMA * true:.3e}"
            if p:
                pv, pr = float(d2[b, p - 1]), int(idx[b, p - 1])
                assert pv < v or (pv == v and pr < r), f"{where}: ({pv!r}, row {pr}) before ({v!r}, row {r}): not in order"
            lo = p == 0 or t_d[p] - t_d[p - 1] > GAMMA * (t_d[p] + t_d[p - 1])
            hi = p + 1 >= t_rows.size or t_d[p + 1] - t_d[p] > GAMMA * (t_d[p + 1] + t_d[p])
            if lo and hi:
                assert r == int(t_rows[p]), f"{where}: row {r} (float64 {true!r}), the truth is row {int(t_rows[p])} ({t_d[p]!r})"
            else:
                ambiguous += 1
                assert abs(true - t_d[p]) <= GAMMA * (true + t_d[p]), \
                    f"{where}: row {r} (float64 {true!r}) is outside the band of the truth's {t_d[p]!r} (row {int(t_rows[p])})"
    return ambiguous, total


# ---------------------------------------------------------------------------------------------------------------------- banks
def latent8(seed, N, B):
    """Embeddings on an 8-dimensional manifold around one base vector: X = fp32(base + 0.3 Z A^T), Q = fp32(base + 0.3 Zq A^T +
    0.02 G / 32)."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(D)
    base /= np.linalg.norm(base)                                                # a Gaussian direction of unit length
    A =rng.standard_normal((D, 8)) / 32
    Z = rng.standard_normal((N, 8))
    Zq = rng.standard_normal((B, 8))
    G = rng.standard_normal((B, D))
    X = (base + 0.3 * Z @ A.T).astype(np.float32)
    Q = (base + 0.3 * Zq @ A.T + 0.02 * G / 32).astype(np.float32)
    return X, Q


def clump(X, Q, seed=0):
    """300 near-copies X[7] (1 + 2^-13 g) inserted at row 2000 and queries 0..7 replaced by X[7] (1 + 2^-12 g): more rows within
    the 16-bit pass's rounding of each other than it keeps candidates."""
    rng = np.random.default_rng(1000 + seed)
    x7 = X[7].astype(np.float64)
    rows = (x7 * (1 + 2.0 ** -13 * rng.standard_normal((300, D)))).astype(np.float32)
    X2 = np.concatenate([X[:2000], rows, X[2000:]]).astype(np.float32)
    Q2 = Q.copy()
    Q2[:8] = (x7 * (1 + 2.0 ** -12 * rng.standard_normal((8, D)))).astype(np.float32)
    return np.ascontiguousarray(X2), np.ascontiguousarray(Q2)


def twins():
    """The rounding-twin bank: s = 1/32; the query and row 100 are A = fp32((1 + 2^-11) s) in every element -- every element an fp16
    tie, rounded to s, so the 16-bit pass loses 2^-10 |q||x|: the bound is attained.  The other 200 rows Y_i are fp16-exact: s
    everywhere but element i, s (1 - 2^-9 (1 + i // 8)).  A has d2 = 0 and is the true nearest; in fp16 every Y looks nearer."""
    s = 1.0 / 32
    A = np.full(D, np.float32((1 + 2.0 ** -11) * s), np.float32)
    Y = np.full((200, D), np.float32(s), np.float32)
    for i in range(200):
        Y[i, i] = np.float32(s * (1 - 2.0 ** -9 * (1 + i // 8)))
    X = np.concatenate([Y[:100], A[None, :], Y[100:]]).astype(np.float32)
    return np.ascontiguousarray(X), A[None, :].copy()


def integers(seed, N, B):
    """Integers in [-4, 4]: fp16-exact, every d2 an integer below 2^24, ties everywhere."""
    rng = np.random.default_rng(seed)
    return rng.integers(-4, 5, (N, D)).astype(np.float32), rng.integers(-4, 5, (B, D)).astype(np.float32)


def d2_int(Q, X):
    """(B,N) int64 exact squared distances of integer data."""
    Q = np.asarray(Q).astype(np.int64); X = np.asarray(X).astype(np.int64)
    return ((Q * Q).sum(1)[:, None] + (X * X).sum(1)[None, :] - 2 * Q @ X.T).astype(np.int64)
