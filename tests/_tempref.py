"""The temperature statistics (csrc/temper.hip, contract in include/pigeon_hip.h) restated in numpy longdouble, and the comparator the
GPU tests hold the kernel under.  numpy only: no torch device, no GPU.  tests/test_tempref_cpu.py pins the restatement against mpmath
and shows that the comparator rejects the mistakes it is for.

  truth(...)    per row and beta, in longdouble (64-bit significand; sums by numpy's pairwise np.sum, about log2(C) 2^-64 relative):
                m, the first argmax a, x_c = l_c - m, w_c = exp(beta x_c) (a -inf cell: w = 0 and x = 0 in the products),
                Z, A, Q, then nll = log Z - beta x_y, d1 = A / Z - x_y, d2 = max(0, Q / Z - (A / Z)^2), conf = 1 / Z; the state.
  bounds        derived from the operations the contract states, never from a kernel's output.  With eps = 2^-52, u = eps / 2:
                  x_c     one subtraction in fp64: relative u
                  w_c     the product beta x_c (relative u) on top of x_c's u puts 2 u |beta x_c| on the exponent; one exp (1 ulp,
                          as tests/_spreadref.py takes it):  relative e_w = eps + 2 u |beta x_c|
                  Z       sum_c w_c e_w + (C - 1) u Z: every term's own error, plus C - 1 additions of non-negative terms in any order
                  A       terms w_c x_c (non-positive): relative e_w + 2 u (x_c's rounding, the product):
                          sum_c |w_c x_c| (e_w + 2 u) + (C - 1) u |A|
                  Q       terms (w_c x_c) x_c (non-negative): relative e_w + 4 u (x_c twice, two products):
                          sum_c w_c x_c^2 (e_w + 4 u) + (C - 1) u Q
                  nll     err Z / Z + eps log Z (one log, 1 ulp) + 2 u |beta x_y| (x_y's rounding, the product)
                          + u (log Z + |beta x_y|) (the subtraction)
                  mean    A / Z: (err A + |mean| err Z) / Z + u |mean|
                  d1      err mean + u |x_y| + u (|mean| + |x_y|)
                  d2      q = Q / Z: err q = (err Q + q err Z) / Z + u q;  the square: 2 |mean| err mean + u mean^2;  the subtraction
                          cancels: its rounding is at most u (q + mean^2), and what it leaves carries BOTH operands' absolute errors:
                          err q + 2 |mean| err mean + u mean^2 + u (q + mean^2).  max(0, .) moves the value towards the truth (>= 0).
                  conf    err Z / Z^2 + u / Z
                Every bound is multiplied by 1.001 for the product terms left out (below 1e-25 relative), and carries 2^-58 of the
                value's magnitude for the longdouble truth's own error and 2^-800 for weights that underflow.
  totals        the sum over the valid rows: sum of the rows' bounds + (valid - 1) u sum |row value| (additions in any order).
                totals_in_order() adds given row values in the kernel's stated order, for the bit-for-bit check.
  NaN           an invalid row (state 2) has NaN row_stats and conf, and nothing else has.
"""
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "tests/_tempref.py needs an extended-precision long double"
EPS = 2.0 ** -52
U_ROUND = 2.0 ** -53
SECOND_ORDER = 1.001
TRUTH_REL = 2.0 ** -58
TINY = 2.0 ** -800
THREADS = 256
OUTPUTS = ("nll", "d1", "d2")


def states(logits, labels):
    """(N,) uint8 per the contract, and the first argmax (N,) (-1 where there is none)"""
    l = np.asarray(logits)
    assert l.dtype == np.float32 and l.ndim == 2
    N, C = l.shape
    y = np.asarray(labels, dtype=np.int64)
    st = np.full(N, 2, dtype=np.uint8)
    arg = np.full(N, -1, dtype=np.int64)
    for n in range(N):
        r = l[n]
        if not 0 <= y[n] < C or np.isnan(r).any() or (r == np.inf).any() or not (r > -np.inf).any() or r[y[n]] == -np.inf:
            continue
        arg[n] = int(np.argmax(r))                                   # numpy's argmax is the first maximum, as torch's
        st[n] = 1 if arg[n] == y[n] else 0
    return st, arg


def _row(r32, y, beta):
    """one valid row at one beta -> (values, bounds): dicts over nll, d1, d2, conf (floats)"""
    C = r32.shape[0]
    l = r32.astype(LD)
    m = l.max()
    masked = r32 == -np.inf
    x = np.where(masked, LD(0), l - m)
    b = LD(beta)
    t = b * x
    w = np.where(masked, LD(0), np.exp(t))
    Z, A, Q = w.sum(), (w * x).sum(), (w * x * x).sum()
    xy = x[y]
    mean, q = A / Z, Q / Z
    vals = {"nll": np.log(Z) - b * xy, "d1": mean - xy, "d2": max(LD(0), q - mean * mean), "conf": LD(1) / Z}
    # ---- bounds, in float64 arithmetic on the magnitudes
    wf, xf = w.astype(np.float64), np.abs(x.astype(np.float64))
    e_w = EPS + 2 * U_ROUND * np.abs(t.astype(np.float64))
    Zf, Af, Qf = float(Z), abs(float(A)), float(Q)
    errZ = math.fsum(wf * e_w) + (C - 1) * U_ROUND * Zf + C * TINY
    errA = math.fsum(wf * xf * (e_w + 2 * U_ROUND)) + (C - 1) * U_ROUND * Af + C * TINY
    errQ = math.fsum(wf * xf * xf * (e_w + 4 * U_ROUND)) + (C - 1) * U_ROUND * Qf + C * TINY
    logZ, bxy, axy = abs(math.log(Zf)), abs(float(b * xy)), abs(float(xy))
    am, qf = Af / Zf, Qf / Zf
    err_mean = (errA + am * errZ) / Zf + U_ROUND * am
    err_q = (errQ + qf * errZ) / Zf + U_ROUND * qf
    bounds = {
        "nll": errZ / Zf + EPS * logZ + 2 * U_ROUND * bxy + U_ROUND * (logZ + bxy) + TRUTH_REL * (logZ + bxy),
        "d1": err_mean + U_ROUND * axy + U_ROUND * (am + axy) + TRUTH_REL * (am + axy),
        "d2": err_q + 2 * am * err_mean + U_ROUND * am * am + U_ROUND * (qf + am * am) + TRUTH_REL * (qf + am * am),
        "conf": errZ / (Zf * Zf) + U_ROUND / Zf + TRUTH_REL / Zf,
    }
    return vals, {k: SECOND_ORDER * v + TINY for k, v in bounds.items()}


def truth(logits, labels, betas):
    """logits (N,C) fp32, labels (N,) int64, betas K floats -> dict: state (N,), argmax (N,), and (N,K) longdouble arrays nll, d1, d2,
    conf (NaN on invalid rows) with float64 bounds nll_bound, d1_bound, d2_bound, conf_bound."""
    l = np.asarray(logits)
    y = np.asarray(labels, dtype=np.int64)
    N, C = l.shape
    K = len(betas)
    st, arg = states(l, y)
    out = {"state": st, "argmax": arg, "betas": [float(b) for b in betas]}
    for k in OUTPUTS + ("conf",):
        out[k] = np.full((N, K), np.nan, dtype=LD)
        out[k + "_bound"] = np.full((N, K), np.nan)
    for n in range(N):
        if st[n] == 2:
            continue
        for k, beta in enumerate(out["betas"]):
            v, b = _row(l[n], int(y[n]), beta)
            for name in v:
                out[name][n, k], out[name + "_bound"][n, k] = v[name], b[name]
    return out


def compare(t, row_stats=None, conf=None, state=None):
    """t = truth(...); the kernel's outputs as arrays -> (errors, worst): messages that name row, beta index and output, and the
    worst |got - truth| / bound seen."""
    N, K = t["nll"].shape
    errors, worst = [], 0.0
    if state is not None:
        s = np.asarray(state).reshape(N)
        for n in range(N):
            if int(s[n]) != int(t["state"][n]):
                errors.append(f"row {n} state: got {int(s[n])}, the contract gives {int(t['state'][n])} (first argmax {int(t['argmax'][n])})")
    cols = []
    if row_stats is not None:
        rs = np.asarray(row_stats, dtype=np.float64).reshape(N, K, 3)
        cols += [(name, rs[:, :, j]) for j, name in enumerate(OUTPUTS)]
    if conf is not None:
        cols.append(("conf", np.asarray(conf, dtype=np.float64).reshape(N, K)))
    for name, got in cols:
        for n in range(N):
            for k in range(K):
                where = f"row {n} beta {k} ({t['betas'][k]!r}) {name}"
                v = got[n, k]
                if t["state"][n] == 2:
                    if not np.isnan(v):
                        errors.append(f"{where}: {v!r} where the contract gives NaN")
                    continue
                want, bound = t[name][n, k], t[name + "_bound"][n, k]
                r = float(abs(LD(v) - want) / LD(bound)) if np.isfinite(v) else np.inf
                worst = max(worst, r)
                if not r <= 1:
                    errors.append(f"{where}: got {v!r}, truth {float(want)!r}, |diff| / bound = {r:.3g}")
    return errors, worst


def totals_truth(t):
    """-> (totals (K,3) longdouble, bound (K,3) float64, counts (2,) int64) of the valid rows"""
    valid = t["state"] != 2
    K = t["nll"].shape[1]
    tot, bnd = np.zeros((K, 3), dtype=LD), np.zeros((K, 3))
    nv = int(valid.sum())
    for j, name in enumerate(OUTPUTS):
        for k in range(K):
            v = t[name][valid, k]
            tot[k, j] = v.sum() if nv else LD(0)
            mag = float(np.abs(v).sum()) if nv else 0.0
            bnd[k, j] = SECOND_ORDER * (float(t[name + "_bound"][valid, k].sum()) + max(nv - 1, 0) * U_ROUND * mag + TRUTH_REL * mag)
    return tot, bnd, np.array([nv, int((t["state"] == 1).sum())], dtype=np.int64)


def compare_totals(t, totals, counts):
    """-> (errors, worst): messages that name beta index and output"""
    tot, bnd, cnt = totals_truth(t)
    got = np.asarray(totals, dtype=np.float64).reshape(tot.shape)
    errors, worst = [], 0.0
    c = np.asarray(counts).reshape(2)
    for i, name in enumerate(("valid rows", "valid rows of state 1")):
        if int(c[i]) != int(cnt[i]):
            errors.append(f"counts[{i}] ({name}): got {int(c[i])}, the contract gives {int(cnt[i])}")
    for k in range(tot.shape[0]):
        for j, name in enumerate(OUTPUTS):
            v = got[k, j]
            if not np.isfinite(v):
                errors.append(f"totals beta {k} {name}: got {v!r}; an invalid row adds +0.0")
                continue
            if bnd[k, j] == 0.0:
                r = 0.0 if LD(v) == tot[k, j] else np.inf
            else:
                r = float(abs(LD(v) - tot[k, j]) / LD(bnd[k, j]))
            worst = max(worst, r)
            if not r <= 1:
                errors.append(f"totals beta {k} {name}: got {v!r}, truth {float(tot[k, j])!r}, |diff| / bound = {r:.3g}")
    return errors, worst


def _block_sum(v):
    """row_block.h's block_sum of 256 fp64 thread values"""
    v = np.asarray(v, dtype=np.float64).reshape(4, 64).copy()
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    return (v[0, 0] + v[1, 0]) + (v[2, 0] + v[3, 0])


def totals_in_order(row_stats, state):
    """the kernel's own sum over rows, in fp64: thread t adds rows t, t + 256, ... ascending (an invalid row as +0.0), then block_sum
    -> (K,3) float64"""
    rs = np.asarray(row_stats, dtype=np.float64)
    N, K, _ = rs.shape
    st = np.asarray(state).reshape(N)
    vals = np.where((st != 2)[:, None, None], rs, 0.0)
    out = np.zeros((K, 3))
    for k in range(K):
        for j in range(3):
            part = np.zeros(THREADS)
            for n0 in range(0, N, THREADS):
                chunk = vals[n0:n0 + THREADS, k, j]
                part[:chunk.shape[0]] = part[:chunk.shape[0]] + chunk
            out[k, j] = _block_sum(part)
    return out


# ------------------------------------------------------------------------------------------------ the reference's own minimiser
def total_d1(logits, labels, beta):
    """-> (sum over the valid rows of d1 at beta (longdouble), the sum of the rows' derived d1 bounds (float64))"""
    t = truth(logits, labels, [beta])
    valid = t["state"] != 2
    return t["d1"][valid, 0].sum(), float(t["d1_bound"][valid, 0].sum())


def _fast_d1(l64, y, beta):
    x = l64 - l64.max(axis=1, keepdims=True)
    w = np.exp(beta * x)
    return float(((w * x).sum(axis=1) / w.sum(axis=1) - x[np.arange(len(y)), y]).sum())


def bisect_beta(logits, labels, lo=1.0 / 64, hi=64.0, rel=2.0 ** -40):
    """plain bisection (in log beta) on the total first derivative over rows that are all valid and finite, in fp64 -> beta, or the
    end of [lo, hi] the derivative points at when it has one sign."""
    l64 = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    if _fast_d1(l64, y, lo) >= 0:
        return lo
    if _fast_d1(l64, y, hi) <= 0:
        return hi
    while hi / lo - 1 > rel:
        mid = math.sqrt(lo * hi)
        if _fast_d1(l64, y, mid) < 0:
            lo = mid
        else:
            hi = mid
    return math.sqrt(lo * hi)


def accepts(logits, labels, beta):
    """the acceptance rule of a fitted beta: the reference's total first derivative changes sign between beta (1 - 2^-39) and
    beta (1 + 2^-39), or its magnitude at beta is below the sum of the rows' derived first-derivative bounds."""
    d_lo, _ = total_d1(logits, labels, beta * (1 - 2.0 ** -39))
    d_hi, _ = total_d1(logits, labels, beta * (1 + 2.0 ** -39))
    if (d_lo <= 0 <= d_hi) or (d_hi <= 0 <= d_lo):
        return True
    d, bound = total_d1(logits, labels, beta)
    return bool(abs(d) <= bound)


# ------------------------------------------------------------------------------------------------ a plain fp64 implementation
MISTAKES = ("no_max_shift", "temperature_for_beta", "beta_missing_in_label_term", "last_maximum", "masked_weight_one",
            "no_squared_mean", "totals_include_invalid", "conf_of_label")


def plain(logits, labels, betas, mistake=None):
    """What a straightforward fp64 implementation computes -> dict(row_stats (N,K,3), conf (N,K), state (N,), totals (K,3), counts
    (2,)).  mistake=None passes compare() and compare_totals(); every name in MISTAKES plants the mistake the comparator is for."""
    assert mistake is None or mistake in MISTAKES
    l32 = np.asarray(logits)
    y = np.asarray(labels, dtype=np.int64)
    N, C = l32.shape
    K = len(betas)
    st, _ = states(l32, y)
    rs, cf = np.full((N, K, 3), np.nan), np.full((N, K), np.nan)
    for n in range(N):
        if st[n] == 2:
            continue
        l = l32[n].astype(np.float64)
        if mistake == "last_maximum":
            st[n] = 1 if C - 1 - int(np.argmax(l[::-1])) == y[n] else 0
        masked = l == -np.inf
        m = 0.0 if mistake == "no_max_shift" else l.max()
        x = np.where(masked, 0.0, l - m)
        for k, beta in enumerate(betas):
            b = 1.0 / beta if mistake == "temperature_for_beta" else float(beta)
            with np.errstate(over="ignore", invalid="ignore"):
                w = np.where(masked, 1.0 if mistake == "masked_weight_one" else 0.0, np.exp(b * x))
                Z, A, Q = w.sum(), (w * x).sum(), (w * x * x).sum()
                mean = A / Z
                rs[n, k, 0] = np.log(Z) - (1.0 if mistake == "beta_missing_in_label_term" else b) * x[y[n]]
                rs[n, k, 1] = mean - x[y[n]]
                rs[n, k, 2] = Q / Z if mistake == "no_squared_mean" else max(0.0, Q / Z - mean * mean)
                cf[n, k] = (w[y[n]] if mistake == "conf_of_label" else np.exp(b * (l.max() - m))) / Z
    valid = st != 2
    if mistake == "totals_include_invalid":
        totals = np.where(np.isnan(rs), 1.0, rs).sum(axis=0)
        counts = np.array([N, int((st == 1).sum())])
    else:
        totals = rs[valid].sum(axis=0) if valid.any() else np.zeros((K, 3))
        counts = np.array([int(valid.sum()), int((st == 1).sum())])
    return {"row_stats": rs, "conf": cf, "state": st, "totals": totals, "counts": counts}


# ------------------------------------------------------------------------------------------------ inputs
KINDS = ("gauss1", "gauss30", "tie", "constant", "neginf_cells", "underflow", "label_on_neginf", "label_negative", "label_2p40",
         "nan_cell", "posinf_cell", "gauss1")
INVALID_KINDS = ("label_on_neginf", "label_negative", "label_2p40", "nan_cell", "posinf_cell")


def make_rows(N, C, seed, kinds=KINDS):
    """N rows of C cells, row n of kind kinds[n % len(kinds)] (N < 3: Gaussian rows only) -> logits (N,C) fp32, labels (N,) int64,
    the kind of each row.  A kind that needs more cells than C has falls back to a Gaussian row."""
    rng = np.random.default_rng([511, seed, N, C])
    l = rng.standard_normal((N, C)).astype(np.float32)
    y = rng.integers(0, C, N).astype(np.int64)
    names = []
    for n in range(N):
        kind = kinds[n % len(kinds)] if N >= 3 else ("gauss1", "gauss30")[n % 2]
        if C < 3 and kind in ("tie", "neginf_cells", "underflow", "label_on_neginf"):
            kind = "gauss1"
        if kind == "gauss30":
            l[n] *= 30
        elif kind == "tie":                                          # the maximum three times; the label on the first or the last
            idx = np.sort(rng.choice(C, 3, replace=False))
            l[n, idx] = l[n].max() + 1
            y[n] = idx[0] if n % 2 == 0 else idx[2]
        elif kind == "constant":
            l[n] = np.float32(rng.standard_normal())
        elif kind == "neginf_cells":
            l[n, rng.random(C) < 0.3] = -np.inf
            l[n, 0] = 0.5
            y[n] = 0 if n % 2 else int(np.argmax(l[n] > -np.inf))
        elif kind == "underflow":                                    # every other weight underflows to 0 at every beta >= 1 / 64
            l[n] = l[n] * 10 - 1e6
            l[n, C // 2] = 3.0
            y[n] = C // 2 if n % 2 == 0 else 0
        elif kind == "label_on_neginf":
            l[n, y[n]] = -np.inf
        elif kind == "label_negative":
            y[n] = -1 - (n % 5)
        elif kind == "label_2p40":
            y[n] = 2 ** 40 + (n % 3)
        elif kind == "nan_cell":
            l[n, rng.integers(0, C)] = np.nan
        elif kind == "posinf_cell":
            l[n, rng.integers(0, C)] = np.inf
        names.append(kind)
    return l, y, names


def betas_of(K):
    """the first K of 16 betas: 1, 1/64 and 64 lead, and 1 (from K = 4) and 0.37 (from K = 12) come twice"""
    base = [1.0, 1.0 / 64, 64.0, 1.0, 0.37, 2.5, 7.0, 0.05, 1.3, 0.8, 20.0, 0.37, 3.3, 0.11, 45.0, 1.7]
    return base[:K]


def planted_labels(logits, beta0, seed):
    """labels sampled from softmax(beta0 * l), numpy default_rng(seed)"""
    l = np.asarray(logits, dtype=np.float64) * beta0
    p = np.exp(l - l.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    cdf = np.cumsum(p, axis=1)
    r = np.random.default_rng(seed).random(len(p))
    return np.minimum((cdf < r[:, None]).sum(axis=1), p.shape[1] - 1).astype(np.int64)


def stats_fn_np(logits, labels):
    """a numpy stats_fn for temperature.fit_beta: betas -> totals (K,3) in fp64"""
    l64 = np.asarray(logits, dtype=np.float64)
    y = np.asarray(labels, dtype=np.int64)
    x = l64 - l64.max(axis=1, keepdims=True)
    xy = x[np.arange(len(y)), y]

    def fn(betas):
        out = np.zeros((len(betas), 3))
        for k, b in enumerate(betas):
            w = np.exp(b * x)
            Z = w.sum(axis=1)
            mean = (w * x).sum(axis=1) / Z
            out[k] = [(np.log(Z) - b * xy).sum(), (mean - xy).sum(), np.maximum(0.0, (w * x * x).sum(axis=1) / Z - mean * mean).sum()]
        return out
    return fn


def ece_np(conf, correct, bins=15):
    """15 equal-width bins (j/15, (j+1)/15]: sum_j n_j / N |acc_j - conf_j|"""
    conf, correct = np.asarray(conf, dtype=np.float64), np.asarray(correct, dtype=np.float64)
    idx = np.clip(np.ceil(conf * bins).astype(np.int64) - 1, 0, bins - 1)
    e = 0.0
    for j in range(bins):
        sel = idx == j
        if sel.any():
            e += sel.sum() / len(conf) * abs(correct[sel].mean() - conf[sel].mean())
    return float(e)
