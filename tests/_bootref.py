"""The numpy restatement of the bootstrap kernels (include/pigeon_hip.h, "Bootstrap intervals"; pigeon_amd/csrc/bootstrap.hip).

THE RESAMPLING CONTRACT.  Draws come from Philox4x32-10 with the multipliers 0xD2511F53 and 0xCD9E8D57 and the key increments
0x9E3779B9 and 0xBB67AE85.  The key is (seed & 0xffffffff, seed >> 32).  For draw j of replicate r the counter is
((j >> 1) & 0xffffffff, (j >> 1) >> 32, r, 0) and the output words are o0 .. o3; an even j uses u = o0 | o1 << 32, an odd j uses
u = o2 | o3 << 32.  The item index is idx(r, j) = floor(u * N / 2^64): the high 64 bits of the 128-bit product.
One replicate uses the same N indices for every column (the pairing), and replicate r depends on (seed, r, N, the column) only.

means:      out[r, m] = (sum_j x[m, idx(r, j)]) / N in the kernel's order: thread t of 256 adds j = t, t + 256, ... ascending from
            +0.0, the 64 lanes of a wave combine as v += v(lane xor o), o = 32 .. 1, the four waves as (w0 + w1) + (w2 + w3).
quantiles:  numpy.quantile(x[m, idx(r, :)], q, method='linear'), nothing else.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)
THREADS = 256


def philox(counter, key):
    """Philox4x32-10.  counter: four arrays (or ints) of 32-bit words, key: two 32-bit words -> four uint64 arrays of 32-bit words."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & MASK32 for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> S32) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> S32) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def words(seed, r, j):
    """o0 .. o3 of draw j (an array) of replicate r."""
    j = np.asarray(j, dtype=np.uint64)
    p = j >> np.uint64(1)
    return philox((p & MASK32, p >> S32, np.uint64(r), np.uint64(0)), (seed & 0xFFFFFFFF, seed >> 32))


def draws(seed, r, j):
    """u of draw j (an array) of replicate r: uint64."""
    j = np.asarray(j, dtype=np.uint64)
    o = words(seed, r, j)
    odd = (j & np.uint64(1)).astype(bool)
    return np.where(odd, o[2] | (o[3] << S32), o[0] | (o[1] << S32))


def mulhi64(u, n):
    """floor(u * n / 2^64) for a uint64 array u and an integer 0 <= n < 2^64, in 32-bit limbs."""
    u = np.asarray(u, dtype=np.uint64)
    n_lo, n_hi = np.uint64(int(n) & 0xFFFFFFFF), np.uint64(int(n) >> 32)
    u_lo, u_hi = u & MASK32, u >> S32
    with np.errstate(over="ignore"):
        k = (u_lo * n_lo) >> S32
        t = u_hi * n_lo + k
        w1, w2 = t & MASK32, t >> S32
        k = (u_lo * n_hi + w1) >> S32
        return u_hi * n_hi + w2 + k


def indices(N, seed, r, j0=0, count=None):
    """idx(r, j) for j = j0 .. j0 + count - 1 (count defaults to N - j0): int64."""
    count = int(N) - int(j0) if count is None else int(count)
    j = np.uint64(j0) + np.arange(count, dtype=np.uint64)
    return mulhi64(draws(seed, r, j), N).astype(np.int64)


def block_sum(v):
    """(..., 256) per-thread partial sums -> (...): the wave butterfly o = 32 .. 1, then (w0 + w1) + (w2 + w3)."""
    v = np.array(v, dtype=np.float64)
    lane = np.arange(THREADS)
    with np.errstate(invalid="ignore", over="ignore"):
        for o in (32, 16, 8, 4, 2, 1):
            v = v + v[..., lane ^ o]                   # within a wave: lane ^ o keeps the upper two bits
        return (v[..., 0] + v[..., 64]) + (v[..., 128] + v[..., 192])


def ordered_sum(g):
    """(..., N) values -> (...): thread t adds j = t, t + 256, ... ascending from +0.0, then block_sum.  A missing j is +0.0, which
    changes no partial sum (a partial sum is never -0.0: it starts at +0.0)."""
    g = np.asarray(g, dtype=np.float64)
    n = g.shape[-1]
    steps = -(-n // THREADS)
    pad = np.zeros(g.shape[:-1] + (steps * THREADS,), dtype=np.float64)
    pad[..., :n] = g
    pad = pad.reshape(g.shape[:-1] + (steps, THREADS))
    acc = np.zeros(g.shape[:-1] + (THREADS,), dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(steps):
            acc = acc + pad[..., s, :]
    return block_sum(acc)


def means(x, R, seed, replicates=None):
    """x (M, N) -> (R, M) float64 (or the rows `replicates` only)."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[1]
    rs = range(R) if replicates is None else replicates
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([ordered_sum(x[:, indices(N, seed, r)]) / np.float64(N) for r in rs])


def quantiles(x, R, seed, q, replicates=None):
    """x (M, N) -> (R, M, Q) float64: numpy.quantile of the gathered column, every value of every call.
    One thing numpy.quantile leaves open: -0.0 and +0.0 compare equal, its selection (numpy.partition) may leave either at a wanted
    position -- which one depends on the array's length and order, not on the data's meaning -- and _lerp's result can carry that
    sign.  The contract settles it: the order statistics are those of the stable sort, ties by item index.  So the value returned is
    _lerp of the gathered column in that order, and it is held to numpy.quantile here, on every call: equal as numbers everywhere,
    and equal bit for bit wherever the result is not a zero."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[1]
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    rs = range(R) if replicates is None else replicates
    order = np.argsort(x, axis=1, kind="stable")
    rule = [orders(N, v) for v in q]
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for r in rs:
            counts = np.bincount(indices(N, seed, r), minlength=N)
            rows = []
            for col, o in zip(x, order):
                g = np.repeat(col[o], counts[o])               # the resample, ascending, ties by item index
                mine = np.array([lerp(g[lo], g[hi], t) for lo, hi, t in rule])
                theirs = np.asarray(np.quantile(g, q, method="linear"), dtype=np.float64)
                same = (mine.view(np.uint64) == theirs.view(np.uint64)) | (np.isnan(mine) & np.isnan(theirs)) | ((mine == 0) & (theirs == 0))
                assert same.all(), f"replicate {r}: the restated rule gives {mine}, numpy.quantile {theirs}"
                rows.append(mine)
            out.append(np.stack(rows))
    return np.stack(out)


def rank_and_sorted(x):
    """x (M, N) -> rank (M, N) int32, sorted (M, N) float64: the stable ascending sort of every column, ties by item index."""
    x = np.asarray(x, dtype=np.float64)
    order = np.argsort(x, axis=1, kind="stable")
    rank = np.empty(x.shape, dtype=np.int32)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(x.shape[1], dtype=np.int32), x.shape), axis=1)
    return rank, np.take_along_axis(x, order, axis=1)


def orders(N, q):
    """(lo, hi, t) of numpy's linear quantile: h = q (N - 1), lo = floor(h), hi = min(lo + 1, N - 1), t = h - lo."""
    h = np.float64(q) * np.float64(N - 1)
    lo = int(np.floor(h))
    return lo, min(lo + 1, N - 1), float(h - np.floor(h))


def lerp(a, b, t):
    """numpy's _lerp for scalars."""
    a, b, t = np.float64(a), np.float64(b), np.float64(t)
    with np.errstate(invalid="ignore", over="ignore"):
        d = b - a
        return b - d * (np.float64(1) - t) if t >= 0.5 else a + d * t


def quantile_by_ranks(rank, sorted_cols, m, idx, q):
    """The contract's formula for one column and one resample: _lerp(sorted[rho_(lo)], sorted[rho_(hi)], t) of the drawn ranks' order
    statistics; NaN when a drawn rank is outside [0, N).  Returns (value, rho_(lo), rho_(hi))."""
    N = rank.shape[1]
    rho = np.sort(rank[m, idx].astype(np.int64))
    lo, hi, t = orders(N, q)
    if rho[0] < 0 or rho[-1] >= N:
        return np.float64(np.nan), int(rho[lo]), int(rho[hi])
    return lerp(sorted_cols[m, rho[lo]], sorted_cols[m, rho[hi]], t), int(rho[lo]), int(rho[hi])


# ------------------------------------------------------------------------------------------------------- holding an implementation
def check_index_stream(fn, N, seed, replicates, count, columns=1):
    """fn(seed, r, j (uint64 array), N, column) -> indices.  Raises AssertionError naming the first replicate and draw (and column)
    where it leaves the contract; every column must see the contract's one stream."""
    j = np.arange(count, dtype=np.uint64)
    for r in replicates:
        want = indices(N, seed, r, 0, count)
        for m in range(columns):
            got = np.asarray(fn(seed, r, j, N, m)).astype(np.int64)
            bad = np.nonzero(got != want)[0]
            if bad.size:
                d = int(bad[0])
                raise AssertionError(f"replicate {r}, draw {d}, column {m}: index {int(got[d])}, the contract gives {int(want[d])} "
                                     f"(N = {N}, seed = {seed})")


def check_quantile_rule(fn, x, seed, replicates, qs):
    """fn(resample sorted ascending (N,), q) -> value.  Raises AssertionError naming the replicate and the draw whose item is the
    order statistic numpy interpolates towards, for the first (replicate, q) where fn is not numpy.quantile bit for bit."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    for r in replicates:
        idx = indices(N, seed, r)
        col = x[idx]
        order = np.argsort(col, kind="stable")
        for q in qs:
            want = np.quantile(col, q, method="linear")
            got = np.float64(fn(col[order], q))
            if got.tobytes() != np.float64(want).tobytes():
                lo, hi, t = orders(N, q)
                raise AssertionError(f"replicate {r}, draw {int(order[hi])} (order statistic {hi} of {N}, q = {q}): {got!r}, "
                                     f"numpy.quantile gives {want!r}")
