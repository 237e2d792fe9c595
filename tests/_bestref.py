"""The guess by expected score (csrc/guess_best.hip, contract in include/pigeon_hip.h) restated in numpy, and the comparator the GPU
tests hold the kernel under.  numpy only: no torch device, no GPU.  tests/test_bestref_cpu.py pins the restatement against mpmath
and shows that the comparator rejects the mistakes it is for.

  truth(...)    E[b,j], the expectation of candidate j under row b's softmax, and its bound come from _spreadref.truth with the
                candidates broadcast as points (B, M, 2) and the one quantile 1.0: expected_score / score_bound for the objective
                'score', expected_km / km_bound for 'km'.  The table route -- pg_score_table, then the product of pg_guess_best --
                performs the operations that bound is derived from: the weights and Z are pg_guess_spread's, d is the same device
                function, every term is one product, every sum C fixed-order additions of terms of one sign, then one division.
                So `score_bound` and `km_bound` apply unchanged.  The one difference: the table holds 5000 * e and the term is
                w * (5000 * e), where pg_guess_spread forms (w * 5000) * e.  Either way it is two multiplications of one rounding
                each, and the bound's `eps + 2 u` term of e_s (exp, and the two multiplications) covers both orders.
                NaN where the contract gives NaN: a NaN or +inf logit, a row of -inf only, a non-finite candidate or centroid.
  best          per row the first index of the best true E (max for 'score', min for 'km') among the candidates that are no NaN,
                -1 where there is none, and the runner-up: the best E at any other index.
  tight/loose   a row is TIGHT when the gap between the best and the second-best true E exceeds four times the sum of their two
                bounds (a row with one candidate that is no NaN is tight).  A tight row's best_idx must be the true best.  A loose
                row may return the best or the runner-up.  compare() returns the loose count; the GPU tests assert it is at most
                1 % of a case's rows, and the inputs they use show 0.
  self-consistency, at zero tolerance: best_value is, bit for bit, expected[b, best_idx], and best_idx is the FIRST index of the best
                value of the returned `expected` row (NaN entries never win; -1 / NaN where the row has nothing else).
"""
import numpy as np

import _spreadref as S

LOOSE_CAP = 0.01
GAP_FACTOR = 4.0
OBJECTIVES = ("score", "km")


def _first_best(row, maximize):
    """the first index of the max (min) of `row` among its entries that are no NaN, -1 where there is none"""
    ok = ~np.isnan(row)
    if not ok.any():
        return -1
    v = np.where(ok, row, -np.inf if maximize else np.inf)
    return int(np.argmax(v) if maximize else np.argmin(v))


def spread_truth(logits, centroids, candidates):
    """_spreadref.truth with the candidates broadcast as every row's points: both objectives' E and bounds in one pass"""
    l32 = np.asarray(logits)
    cand = np.asarray(candidates, dtype=np.float64).reshape(-1, 2)
    return S.truth(l32, centroids, np.broadcast_to(cand[None], (l32.shape[0], cand.shape[0], 2)), (1.0,))


def truth(logits, centroids, candidates, objective="score", shared=None):
    """logits (B,C) fp32, centroids (C,2) fp64, candidates (M,2) fp64 -> dict: E, bound (B,M); best, second (B,) int64 (-1: none);
    gap (B,) = |E[best] - E[second]| (inf without a second); tight (B,) bool; maximize.  `shared`: spread_truth(...) of the same
    inputs, computed once for both objectives."""
    assert objective in OBJECTIVES
    t = spread_truth(logits, centroids, candidates) if shared is None else shared
    B = t["expected_km"].shape[0]
    maximize = objective == "score"
    E = t["expected_score" if maximize else "expected_km"]
    bound = t["score_bound" if maximize else "km_bound"]
    best = np.full(B, -1, dtype=np.int64)
    second = np.full(B, -1, dtype=np.int64)
    gap = np.full(B, np.inf)
    tight = np.ones(B, dtype=bool)
    for b in range(B):
        i = _first_best(E[b], maximize)
        best[b] = i
        if i < 0:
            continue
        rest = E[b].copy()
        rest[i] = np.nan
        k = _first_best(rest, maximize)
        second[b] = k
        if k >= 0:
            gap[b] = abs(E[b, i] - E[b, k])
            tight[b] = gap[b] > GAP_FACTOR * (bound[b, i] + bound[b, k])
    return dict(E=E, bound=bound, best=best, second=second, gap=gap, tight=tight, maximize=maximize)


def compare(t, best_idx, best_value, expected):
    """t = truth(...); best_idx (B,) integers, best_value (B,) and expected (B,M) fp64 -> (errors, loose, worst): a list of messages,
    each naming row and candidate, the number of loose rows, and the worst |got - truth| / bound seen on E."""
    E, bound, maximize = t["E"], t["bound"], t["maximize"]
    B, M = E.shape
    idx = np.asarray(best_idx).astype(np.int64).reshape(B)
    val = np.asarray(best_value, dtype=np.float64).reshape(B)
    exp = np.asarray(expected, dtype=np.float64).reshape(B, M)
    errors, loose, worst = [], 0, 0.0
    for b in range(B):
        for j in range(M):
            got, want = exp[b, j], E[b, j]
            if np.isnan(want):
                if not np.isnan(got):
                    errors.append(f"row {b} candidate {j} expected: {got!r} where the contract gives NaN")
                continue
            r = abs(got - want) / bound[b, j] if np.isfinite(got) else np.inf
            worst = max(worst, r)
            if not r <= 1:
                errors.append(f"row {b} candidate {j} expected: got {got!r}, truth {want!r}, |diff| / bound = {r:.3g}")
        own = _first_best(exp[b], maximize)
        if idx[b] != own:
            errors.append(f"row {b} candidate {int(idx[b])} best_idx: the first best of the returned expected row is candidate {own}")
        if idx[b] < -1 or idx[b] >= M:
            errors.append(f"row {b} candidate {int(idx[b])} best_idx: outside -1 .. {M - 1}")
            continue
        if idx[b] == -1:
            if not np.isnan(val[b]):
                errors.append(f"row {b} candidate -1 best_value: {val[b]!r} where nothing was chosen (NaN expected)")
        elif val[b].tobytes() != exp[b, idx[b]].tobytes():
            errors.append(f"row {b} candidate {int(idx[b])} best_value: {val[b]!r} is not expected[{b}, {int(idx[b])}] = {exp[b, idx[b]]!r}")
        if t["tight"][b]:
            if idx[b] != t["best"][b]:
                errors.append(f"row {b} candidate {int(idx[b])} best_idx: the true best is candidate {int(t['best'][b])} "
                              f"(gap {t['gap'][b]:.3g}, tight)")
        else:
            loose += 1
            if idx[b] not in (t["best"][b], t["second"][b]):
                errors.append(f"row {b} candidate {int(idx[b])} best_idx (loose): neither the true best {int(t['best'][b])} nor the "
                              f"runner-up {int(t['second'][b])}")
    return errors, loose, worst


def loose_allowed(t):
    """the cap of the issue: at most 1 % of a case's rows"""
    return int(LOOSE_CAP * t["tight"].size)


# ------------------------------------------------------------------------------------------------ a plain fp64 implementation
def table_np(candidates, centroids, kind="score"):
    """what pg_score_table computes, by the textbook fp64 formula: (M,C) km, or 5000 exp(-km / 1492.7)"""
    cand = np.asarray(candidates, dtype=np.float64).reshape(-1, 2)
    cen = np.asarray(centroids, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = np.stack([S.haversine_np(p, cen) for p in cand]) if len(cand) else np.zeros((0, len(cen)))
        return d if kind == "km" else S.SCORE_MAX * np.exp(-d / S.DECAY_KM)


MISTAKES = ("transposed_table", "unnormalised_weights", "last_on_tie", "dropped_k_step", "doubled_k_step", "neighbour_row",
            "candidate_shifted_by_a_tile", "min_for_max", "nan_candidate_wins", "poisoned_neighbour")


def plain(logits, table, maximize=True, mistake=None, tile=32, kc=32):
    """What a straightforward fp64 implementation of pg_guess_best computes from a table (M,C) -> best_idx (B,) int64, best_value (B,),
    expected (B,M).  mistake=None passes compare(); every name in MISTAKES plants the mistake the comparator is for (`tile`
    candidates per tile and `kc` cells per K step, as a tiled kernel would have them)."""
    assert mistake is None or mistake in MISTAKES
    l32 = np.asarray(logits)
    B, C = l32.shape
    tab = np.asarray(table, dtype=np.float64)
    if mistake == "transposed_table":
        tab = tab.T.copy()
    M = tab.shape[0]
    exp = np.full((B, M), np.nan)
    for b in range(B):
        src = (b + 1) % B if mistake == "neighbour_row" else b
        l = l32[src].astype(np.float64)
        if np.isnan(l).any() or (l == np.inf).any() or not (l > -np.inf).any():
            continue
        w = np.exp(l - l.max())
        Z = 1.0 if mistake == "unnormalised_weights" else w.sum()
        with np.errstate(invalid="ignore"):
            terms = tab * w[None, :]
            num = terms.sum(axis=1)
            if mistake == "dropped_k_step":
                num = num - terms[:, kc:2 * kc].sum(axis=1)
            if mistake == "doubled_k_step":
                num = num + terms[:, kc:2 * kc].sum(axis=1)
            exp[b] = num / Z
    if mistake == "candidate_shifted_by_a_tile":
        exp = np.roll(exp, -tile, axis=1)
    if mistake == "poisoned_neighbour":
        bad = np.isnan(exp).all(axis=1)
        exp[np.roll(bad, 1) & ~bad] = np.nan
    idx = np.full(B, -1, dtype=np.int64)
    val = np.full(B, np.nan)
    for b in range(B):
        i = _first_best(exp[b], maximize != (mistake == "min_for_max"))
        if i >= 0 and mistake == "last_on_tie":
            i = int(np.flatnonzero(exp[b] == exp[b, i])[-1])
        if mistake == "nan_candidate_wins" and np.isnan(exp[b]).any() and not np.isnan(exp[b]).all():
            i = int(np.flatnonzero(np.isnan(exp[b]))[0])
        idx[b] = i
        if i >= 0:
            val[b] = exp[b, i]
    return idx, val, exp


# ------------------------------------------------------------------------------------------------ inputs
def candidates_of(M, seed, centroids=None):
    """M candidate points over the globe, (M,2) fp64 [lng, lat].  From M = 8 on the first ones are the edge cases: both poles, two
    points on the antimeridian and, with `centroids`, a point equal to a cell centre."""
    rng = np.random.default_rng([421, seed, M])
    cand = np.stack([rng.uniform(-180, 180, M), np.degrees(np.arcsin(rng.uniform(-1, 1, M)))], axis=1)
    if M >= 8:
        cand[0], cand[1], cand[2], cand[3] = (0.0, 90.0), (37.5, -90.0), (180.0, 12.25), (-180.0, -47.0)
        if centroids is not None:
            cand[4] = np.asarray(centroids, dtype=np.float64)[len(centroids) // 2]
    return cand
