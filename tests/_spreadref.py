"""The guess spread (csrc/spread.hip, contract in include/pigeon_hip.h) restated in numpy, and the comparator the GPU tests hold the
kernel under.  numpy only: no torch device, no GPU.  tests/test_spreadref_cpu.py pins the restatement against mpmath and shows that
the comparator rejects the mistakes it is for.

  truth(...)    per (row, point): the weights w_c = exp(l_c - max l) in fp64 (one exp each), the distances d_c from
                _georef.haversine_truth (longdouble, rounded once to fp64), Z, sum w d and sum w s by math.fsum -- the exact sum of
                the fp64 terms, rounded once -- and, per quantile, the answer cell of  min { key_c : M(key_c) >= q Z }  found on the
                keys sorted by (key, index).  The running masses M are a longdouble cumulative sum (2^-64 per addition: 2e-15 Z at
                C = 40 000, three orders below the margin a tight quantile keeps); the total they are compared with is that
                sum's own last element, so q = 1 selects the last cell of positive weight exactly as the contract's
                "M(+inf) is the same sequence of additions as Z" does on the device.
  bounds        derived from the operations the contract states, never from a kernel's output.  With eps = 2^-52, u = eps / 2:
                  w_c     one subtraction in fp64 (relative u on x = l - max, so |x| u on the exponential) and one exp (1 ulp):
                          relative e_w = eps + |x| u
                  d_c     16 U(a_c) absolute: the per-element bound tests/_georef.py gives pg_haversine_matrix (plus u d_c: the
                          longdouble truth is rounded to fp64 once); written U_c below
                  Z       sum_c w_c e_w + C u Z: every term's own error, plus C fixed-order additions of non-negative terms
                  sum w d sum_c w_c (d_c (e_w + u) + 16 U_c) + C u sum: term errors (product: u), plus the additions
                  s_c     5000 exp(-d_c / 1492.7): the division puts t u on the exponent (t = d / 1492.7), the distance 16 U / 1492.7,
                          exp and the two multiplications eps + 2 u:  relative e_s = eps + 2 u + t u + 16 U_c / 1492.7
                  sum w s sum_c w_c s_c (e_w + e_s) + C u sum
                  N / Z   (err N + |N / Z| err Z) / Z + u |N / Z|, to first order; the product terms left out are below 1e-25
                          relative, covered by the factor 1.001 on the whole bound
                  radius  16 U(a_c) + eps key_c of the answer cell: its distance, and the one addition of the extent
  tight/loose   a quantile is TIGHT when |M - q Z| > 1e-12 Z at the answer and at its predecessor (the mass before the answer's key;
                for q == 1 the answer's own mass IS the total, so only the predecessor counts) and the answer's key is more than
                1e-6 km from both sorted neighbours.  A tight quantile must come out as the answer cell's key within the radius
                bound.  Any other quantile is LOOSE and may come out as the answer or either sorted neighbour.  compare() returns
                the loose count; the GPU tests assert it is at most 1 % of a case's quantiles, and the inputs they use show 0.
  NaN           where the contract gives NaN (a NaN or +inf logit, a non-finite point, a row of -inf only, a non-finite key) every
                output of that (row, point) must be NaN, and nowhere else.
"""
import math

import numpy as np

import _georef as G

LD = np.longdouble
EPS = 2.0 ** -52
U_ROUND = 2.0 ** -53
SCORE_MAX = 5000.0
DECAY_KM = 1492.7                                                   # pigeon_amd/config.py DECAY_CONSTANT
MASS_MARGIN = 1e-12
KEY_GAP_KM = 1e-6
LOOSE_CAP = 0.01
SECOND_ORDER = 1.001


def _as_points(points, B):
    p = np.asarray(points, dtype=np.float64)
    return p.reshape(B, -1, 2)


def truth(logits, centroids, points, quantiles, extent=None):
    """logits (B,C) fp32, centroids (C,2) fp64, points (B,2) or (B,G,2) fp64, extent (C,) fp64 or None -> a dict of (B,G[,nq]) arrays:
    expected_km, expected_score (fp64; NaN where the contract gives NaN), their bounds km_bound / score_bound, and per quantile
    cell (index of the answer cell), key, key_bound, tight (bool), lo_key / hi_key (the sorted neighbours' keys, NaN where there is
    none), mass_margin (min |M - q Z| / Z over the answer and its predecessor) and key_gap (km to the nearer neighbour)."""
    l32 = np.asarray(logits)
    assert l32.dtype == np.float32 and l32.ndim == 2
    B, C = l32.shape
    cen = np.asarray(centroids, dtype=np.float64)
    pts = _as_points(points, B)
    Gn = pts.shape[1]
    qs = [float(q) for q in quantiles]
    nq = len(qs)
    ext = np.zeros(C) if extent is None else np.asarray(extent, dtype=np.float64)
    out = {k: np.full((B, Gn), np.nan) for k in ("expected_km", "expected_score", "km_bound", "score_bound")}
    for k in ("key", "key_bound", "lo_key", "hi_key", "mass_margin", "key_gap"):
        out[k] = np.full((B, Gn, nq), np.nan)
    out["cell"] = np.full((B, Gn, nq), -1, dtype=np.int64)
    out["tight"] = np.zeros((B, Gn, nq), dtype=bool)
    for b in range(B):
        l = l32[b].astype(np.float64)
        if np.isnan(l).any() or (l == np.inf).any() or not (l > -np.inf).any():
            continue
        x = l - l.max()
        w = np.exp(x)
        e_w = EPS + np.abs(np.where(np.isfinite(x), x, 0.0)) * U_ROUND
        for g in range(Gn):
            p = pts[b, g]
            if not np.isfinite(p).all():
                continue
            with np.errstate(invalid="ignore"):
                d_ld, a = G.haversine_truth(p[None, :], cen)
            d = d_ld.astype(np.float64)
            key = d + ext
            if not (np.isfinite(key).all() and (key >= 0).all()):
                continue
            Ud = 16.0 * G.U(a) + U_ROUND * d                       # the kernel's bound, and the truth's one rounding to fp64
            Z = math.fsum(w)
            s = SCORE_MAX * np.exp(-d / DECAY_KM)
            Nd, Ns = math.fsum(w * d), math.fsum(w * s)
            errZ = math.fsum(w * e_w) + C * U_ROUND * Z
            errNd = math.fsum(w * (d * (e_w + U_ROUND) + Ud)) + C * U_ROUND * Nd
            e_s = EPS + 2 * U_ROUND + (d / DECAY_KM) * U_ROUND + Ud / DECAY_KM
            errNs = math.fsum(w * s * (e_w + e_s)) + C * U_ROUND * Ns
            out["expected_km"][b, g], out["expected_score"][b, g] = Nd / Z, Ns / Z
            out["km_bound"][b, g] = SECOND_ORDER * ((errNd + Nd / Z * errZ) / Z + U_ROUND * Nd / Z)
            out["score_bound"][b, g] = SECOND_ORDER * ((errNs + Ns / Z * errZ) / Z + U_ROUND * Ns / Z)
            order = np.lexsort((np.arange(C), key))
            ks, ws = key[order], w[order].astype(LD)
            cum = np.cumsum(ws)
            last = np.searchsorted(ks, ks, side="right") - 1        # the last index of every run of equal keys
            first = np.searchsorted(ks, ks, side="left")
            M = cum[last]                                           # M(key) includes every cell of the same key
            total = cum[-1]
            for j, q in enumerate(qs):
                target = LD(q) * total
                i = int(np.argmax(M >= target))                     # the first index that reaches it; index `total` always does
                i0, i1 = int(first[i]), int(last[i])
                before = cum[i0 - 1] if i0 > 0 else LD(0)
                margins = [abs(before - target)] + ([abs(M[i] - target)] if q != 1.0 else [])
                margin = float(min(margins) / total)
                lo = ks[i0 - 1] if i0 > 0 else np.nan
                hi = ks[i1 + 1] if i1 + 1 < C else np.nan
                gap = np.nanmin([ks[i] - lo, hi - ks[i], np.inf])
                cell = int(order[i0])
                out["cell"][b, g, j], out["key"][b, g, j] = cell, ks[i]
                out["key_bound"][b, g, j] = Ud[cell] + EPS * ks[i]
                out["lo_key"][b, g, j], out["hi_key"][b, g, j] = lo, hi
                out["mass_margin"][b, g, j], out["key_gap"][b, g, j] = margin, gap
                out["tight"][b, g, j] = margin > MASS_MARGIN and gap > KEY_GAP_KM
    out["quantiles"] = qs
    return out


def compare(t, expected_km, expected_score, radius_km):
    """t = truth(...); the three outputs as (B,G[,nq]) or, for G = 1, (B[,nq]) arrays -> (errors, loose, worst): a list of messages,
    each naming row, point and output (quantile), the number of loose quantiles, and the worst |got - truth| / bound seen on the
    expectations and the tight radii."""
    B, Gn, nq = t["key"].shape
    ek = np.asarray(expected_km, dtype=np.float64).reshape(B, Gn)
    es = np.asarray(expected_score, dtype=np.float64).reshape(B, Gn)
    rk = np.asarray(radius_km, dtype=np.float64).reshape(B, Gn, nq)
    errors, loose, worst = [], 0, 0.0
    for b in range(B):
        for g in range(Gn):
            where = f"row {b} point {g}"
            if np.isnan(t["expected_km"][b, g]):
                for name, v in (("expected_km", ek[b, g]), ("expected_score", es[b, g])):
                    if not np.isnan(v):
                        errors.append(f"{where} {name}: {v!r} where the contract gives NaN")
                for j in range(nq):
                    if not np.isnan(rk[b, g, j]):
                        errors.append(f"{where} quantile {j} (q = {t['quantiles'][j]}): {rk[b, g, j]!r} where the contract gives NaN")
                continue
            for name, v, want, bound in (("expected_km", ek[b, g], t["expected_km"][b, g], t["km_bound"][b, g]),
                                         ("expected_score", es[b, g], t["expected_score"][b, g], t["score_bound"][b, g])):
                r = abs(v - want) / bound if np.isfinite(v) else np.inf
                worst = max(worst, r)
                if not r <= 1:
                    errors.append(f"{where} {name}: got {v!r}, truth {want!r}, |diff| / bound = {r:.3g}")
            for j in range(nq):
                v, q = rk[b, g, j], t["quantiles"][j]
                r = abs(v - t["key"][b, g, j]) / t["key_bound"][b, g, j] if np.isfinite(v) else np.inf
                if t["tight"][b, g, j]:
                    worst = max(worst, r)
                    if not r <= 1:
                        errors.append(f"{where} quantile {j} (q = {q}): got {v!r}, the key of cell {t['cell'][b, g, j]} is "
                                      f"{t['key'][b, g, j]!r}, |diff| / bound = {r:.3g}")
                    continue
                loose += 1
                cands = [k for k in (t["lo_key"][b, g, j], t["key"][b, g, j], t["hi_key"][b, g, j]) if not np.isnan(k)]
                slack = t["key_bound"][b, g, j] + KEY_GAP_KM        # neighbours within the gap share the answer's bound
                if not (np.isfinite(v) and any(abs(v - k) <= slack for k in cands)):
                    errors.append(f"{where} quantile {j} (q = {q}, loose): got {v!r}, none of {cands}")
    return errors, loose, worst


def loose_allowed(t):
    """the cap of the issue: at most 1 % of a case's quantiles"""
    return int(LOOSE_CAP * t["tight"].size)


# ------------------------------------------------------------------------------------------------ a plain fp64 implementation
def haversine_np(p, cen, swap=False):
    """the textbook fp64 formula of the kernels (reference preprocessing/geo_utils.py), p (2,), cen (C,2) -> (C,) km"""
    p = p[::-1] if swap else p
    lng1, lat1 = np.deg2rad(p[0]), np.deg2rad(p[1])
    lng2, lat2 = np.deg2rad(cen[:, 0]), np.deg2rad(cen[:, 1])
    a = np.sin((lat1 - lat2) / 2) ** 2 + np.cos(lat1) * np.cos(lat2) * np.sin((lng1 - lng2) / 2) ** 2
    with np.errstate(invalid="ignore"):
        return 2 * 6378.137 * np.arcsin(np.sqrt(a))


MISTAKES = ("no_max_shift", "strict_greater", "unsorted_cumsum", "extent_left_out", "extent_in_expected", "lnglat_swapped",
            "neighbour_row_point", "z_over_topk", "rounded_score")


def plain(logits, centroids, points, quantiles, extent=None, mistake=None, topk=5):
    """What a straightforward fp64 implementation computes (np.sum, np.cumsum over the sorted keys) -> expected_km, expected_score
    (B,G), radius_km (B,G,nq).  mistake=None passes compare(); every name in MISTAKES plants the mistake the comparator is for."""
    assert mistake is None or mistake in MISTAKES
    l32 = np.asarray(logits)
    B, C = l32.shape
    cen = np.asarray(centroids, dtype=np.float64)
    pts = _as_points(points, B)
    Gn, nq = pts.shape[1], len(quantiles)
    ext = np.zeros(C) if extent is None else np.asarray(extent, dtype=np.float64)
    ek, es, rk = np.full((B, Gn), np.nan), np.full((B, Gn), np.nan), np.full((B, Gn, nq), np.nan)
    for b in range(B):
        l = l32[b].astype(np.float64)
        if np.isnan(l).any() or (l == np.inf).any() or not (l > -np.inf).any():
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            w = np.exp(l) if mistake == "no_max_shift" else np.exp(l - l.max())
        for g in range(Gn):
            p = pts[(b + 1) % B, g] if mistake == "neighbour_row_point" else pts[b, g]
            if not np.isfinite(p).all():
                continue
            d = haversine_np(p, cen, swap=mistake == "lnglat_swapped")
            key = d if mistake == "extent_left_out" else d + ext
            if not (np.isfinite(key).all() and (key >= 0).all()):
                continue
            Z = np.sort(w)[-topk:].sum() if mistake == "z_over_topk" else w.sum()
            s = SCORE_MAX * np.exp(-d / DECAY_KM)
            if mistake == "rounded_score":
                s = np.round(s)
            with np.errstate(invalid="ignore"):
                ek[b, g] = (w * (key if mistake == "extent_in_expected" else d)).sum() / Z
                es[b, g] = (w * s).sum() / Z
            order = np.arange(C) if mistake == "unsorted_cumsum" else np.lexsort((np.arange(C), key))
            ks = key[order]
            with np.errstate(invalid="ignore"):
                cum = np.cumsum(w[order])
            if mistake != "unsorted_cumsum":
                cum = cum[np.searchsorted(ks, ks, side="right") - 1]
            tot = cum[-1]
            for j, q in enumerate(quantiles):
                with np.errstate(invalid="ignore"):
                    ok = cum > q * tot if mistake == "strict_greater" else cum >= q * tot
                rk[b, g, j] = ks[int(np.argmax(ok))] if ok.any() else np.inf
    return ek, es, rk


# ------------------------------------------------------------------------------------------------ inputs
def centroids_of(C, seed):
    """C distinct cell centres over the globe, (C,2) fp64 [lng, lat]"""
    rng = np.random.default_rng([411, seed, C])
    return np.stack([rng.uniform(-180, 180, C), np.degrees(np.arcsin(rng.uniform(-1, 1, C)))], axis=1)


def gaussian_logits(B, C, seed, sigma=3.0):
    return (np.random.default_rng([412, seed, B, C]).standard_normal((B, C)) * sigma).astype(np.float32)


def points_of(B, Gn, seed):
    rng = np.random.default_rng([413, seed, B, Gn])
    return np.stack([rng.uniform(-180, 180, (B, Gn)), rng.uniform(-85, 85, (B, Gn))], axis=-1)


def extents_of(C, seed):
    """0 .. 400 km, a few exact zeros"""
    rng = np.random.default_rng([414, seed, C])
    e = rng.uniform(0, 400, C)
    e[rng.random(C) < 0.1] = 0.0
    return e


def uniform_quantile(C):
    """a q in (0.5, 0.9) for C cells of equal weight whose q C is no integer and stays 1/4 away from one"""
    for q in (0.5, 0.61, 0.7, 0.83, 0.9):
        if abs(q * C - round(q * C)) > 0.2:
            return q
    return (math.floor(0.6 * C) + 0.5) / C


# ------------------------------------------------------------------------------------------------ coverage metrics
def coverage_np(radius_km, true_km):
    """share of samples whose true distance is at most their radius; radius (N,), true_km (N,)"""
    r, t = np.asarray(radius_km, dtype=np.float64), np.asarray(true_km, dtype=np.float64)
    return float(np.mean(t <= r))
