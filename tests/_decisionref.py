"""High-precision statements of the kernels that turn an embedding into the discrete outputs (csrc/head.hip, csrc/refine.hip,
csrc/certainty.hip) and the inputs at which they go wrong.  numpy only: no torch device, no GPU.  tests/test_decisionref_cpu.py pins
every function here (the recorded reference outputs, the oracle, fp32 emulations of the kernels' summation orders) and shows that
the comparisons reject the mistakes they are for; tests/test_gpu_decision.py holds the kernels to them.

u = 2^-24 is the unit roundoff of fp32.  The bounds are derived, not measured:

  head_logits_truth   t = (1/P sum_p emb_p) . W[c] + bias[c] in fp64 and the magnitude sum S = sum_k (1/P sum_p |emb_p,k|) |W[c,k]| +
                      |bias[c]|.  The kernel adds P panels (P roundings), multiplies by the rounded 1/P (2), runs a 1024-long fmaf
                      chain (1024) and adds the bias (1 on the sum, which is u |t|): (1024 + P + 2) u S + u |t|.
  softmax_truth       fp64 probabilities of the fp32 logits.  (|l - max| + ceil(C/256) + 16) u p + 2^-126: the rounding of l - max
                      carried through exp; ceil(C/256) + 8 additions of positive terms in the kernel's order (a thread's strided
                      chain, six butterfly steps, two adds across the waves); a 4-ulp expf, the division and the rounding of the
                      stored value take the rest; the absolute term is the subnormal range, flushed or not.
  topk_expected       the order (logit desc, index asc).  Softmax is monotone, so this is the order of the probabilities except where
                      two different logits round to the same probability.  One such class is certain: cells whose fp64 probability
                      is below 2^-151 are exactly 0 in fp32 (-inf cells among them) and rank among themselves by index alone.
  distances_truth     the fp64 L2 distance from the fp32 panel mean (q_mean32: bit-reproducible).  16 u d: 2 u on every squared
                      difference, 16 + 6 on the lane chain and the butterfly, halved by the square root, plus its own rounding.
  candidate_record    the 4-float and 12-float records of refine_candidates_kernel.  Tie rules, stated once: the nearest prototype
                      is the lowest bank row, the farthest member the lowest position of the member list, the runner-up the next in
                      that same order.
  select              refine_select_kernel: exp(s / T), the sequential sum, p * (ex / sum), the first-maximum argmax in which NaN is
                      the maximum, and the haversine veto (_georef.haversine_mixed_truth).

Keyword switches turn on one deliberate mistake each (in the manner of tests/_opticsref.py); the CPU tests check that every one is
caught on the family built for it."""
from types import SimpleNamespace

import numpy as np

import _georef

U32 = 2.0 ** -24
TINY = 2.0 ** -126
ZERO_BELOW = 2.0 ** -151                                            # an fp64 probability below this is exactly 0 in fp32
DIM = 1024
SENTINEL = -7.25                                                    # what the GPU tests fill their guard elements with
GUARD = 64
F32 = np.float32


def rng_of(*key):
    return np.random.default_rng([2026, *key])


# ================================================================================================================ head: logits
def q_mean32(q):
    """(..., P, 1024) fp32 -> (..., 1024) fp32: the panel mean in the kernels' order ((e0 + e1) + e2 ...) * fl(1 / P)"""
    q = np.asarray(q)
    assert q.dtype == F32
    acc = q[..., 0, :].copy()
    for p in range(1, q.shape[-2]):
        acc = acc + q[..., p, :]
    return acc * (F32(1) / F32(q.shape[-2])) if q.shape[-2] > 1 else acc


def head_logits_truth(emb, W, bias, drop_last_k_tile=False, first_panel_only=False):
    """emb (B,P,1024), W (C,1024), bias (C,) fp32 -> (t, S) fp64 (B,C)"""
    e, W64, b64 = np.asarray(emb, dtype=np.float64), np.asarray(W, dtype=np.float64), np.asarray(bias, dtype=np.float64)
    if first_panel_only:
        e = e[:, :1]
    K = DIM - 32 if drop_last_k_tile else DIM
    t = e.mean(axis=1)[:, :K] @ W64[:, :K].T + b64
    S = np.abs(e).mean(axis=1)[:, :K] @ np.abs(W64[:, :K]).T + np.abs(b64)
    return t, S


def logits_bound(t, S, P):
    return (DIM + P + 2) * U32 * S + U32 * np.abs(t)


def logits_emulated(emb, W, bias):
    """head_logits_kernel in numpy fp32: panels added from a zero accumulator, * fl(1/P), the fmaf chain over k = 0 .. 1023 (the
    product is exact in fp64, the sum rounds once to fp64 and once to fp32: an fmaf up to rare double roundings), + bias"""
    emb = np.asarray(emb)
    assert emb.dtype == F32
    a = np.zeros((emb.shape[0], DIM), dtype=F32)
    for p in range(emb.shape[1]):
        a = a + emb[:, p]
    a = (a * (F32(1) / F32(emb.shape[1]))).astype(np.float64)
    W64 = np.asarray(W, dtype=np.float64)
    acc = np.zeros((emb.shape[0], W64.shape[0]), dtype=F32)
    for k in range(DIM):
        acc = (a[:, k:k + 1] * W64[None, :, k] + acc).astype(F32)
    return acc + np.asarray(bias, dtype=F32)[None]


def gaussian_logits_case(rng, B, C, P):
    """embeddings and weights of mixed sign and size: (emb (B,P,1024), W (C,1024), bias (C,)) fp32"""
    emb = (rng.standard_normal((B, P, DIM)) * 0.7 + 0.1).astype(F32)
    W = (rng.uniform(-1, 1, (C, DIM)) / 4).astype(F32)
    return emb, W, rng.uniform(-1, 1, C).astype(F32)


def integer_logits_case(rng, B, C, P):
    """Panel sums that are multiples of P, small integer weights and biases: every partial sum is an integer below 2^24 and
    x * fl(1/P) is exact, so the fp64 truth rounded to fp32 is what the kernel must write, bit for bit."""
    mean = rng.integers(-6, 7, (B, DIM))
    parts = rng.integers(-5, 6, (B, P, DIM))
    parts[:, P - 1] = 0
    parts[:, P - 1] = P * mean - parts.sum(axis=1)
    W = rng.integers(-7, 8, (C, DIM))
    bias = rng.integers(-50, 51, C)
    assert np.abs(parts).max() < 2 ** 10 and (np.abs(mean) @ np.abs(W).T).max() + 50 < 2 ** 24
    return parts.astype(F32), W.astype(F32), bias.astype(F32)


# ---- controlled logits: emb[b,0,b] = 1 and zero elsewhere, so logits[b,c] = W[c,b] + bias[c] exactly
LOGIT_FAMILIES = ("gauss", "wide", "levels", "equal", "ties")
TIE_FAMILIES = ("levels", "equal", "ties")                          # zero top-k exceptions are allowed on these


def logit_rows(tag, C, rng):
    """one row (C,) fp32 of family `tag`"""
    if tag == "gauss":
        return rng.normal(0, 3, C).astype(F32)
    if tag == "wide":
        # -|N(0, 60)| with one 0: most of the probability mass is one cell and the far cells underflow.  No cell is left in the
        # band whose fp32 probability is subnormal (flushed or not): those are moved down to where the probability is exactly 0.
        l = (-np.abs(rng.normal(0, 60, C))).astype(F32)
        l[rng.integers(0, C)] = 0
        p = softmax_truth(l)
        l[(p >= 2.0 ** -152) & (p <= 2.0 ** -124)] -= F32(40)
        p = softmax_truth(l)
        assert not ((p >= ZERO_BELOW) & (p <= 2.0 ** -125)).any()
        return l
    if tag == "levels":
        return rng.choice(np.array([-3.0, -1.5, 0.0, 1.5, 3.0], dtype=F32), C)
    if tag == "equal":
        return np.full(C, F32(rng.normal(0, 3)), dtype=F32)
    if tag == "ties":
        # groups of equal values above everything else, at c, c + 1, c + 64 and c + 256: the next lane, another wave of the same
        # pass, the same thread's next visit.  The cells below them are distinct multiples of 2^-10 in a random order, spread over
        # at most +-19: l - max is exact and no two of them round to the same probability, so the whole order is decided.
        step = 2.0 ** -10 * 2 ** int(np.log2(max(1, 16384 // C)))
        l = ((rng.permutation(C) - C // 2) * step).astype(F32)
        assert np.abs(l).max() < 20 and len(np.unique(l)) == C
        for g, c in enumerate(rng.permutation(max(C - 256, 1))[:12]):
            for o in (0, 1, 64, 256):
                if c + o < C:
                    l[c + o] = F32(40 - g)
        return l
    raise KeyError(tag)


def controlled_case(C, rng, mask=None):
    """-> (L (5,C) fp32: one row per LOGIT_FAMILIES, bias (C,) fp32).  mask: None, "neginf" (bias = -inf on a third of the cells),
    "posinf" (+inf on one cell: every probability of every row is NaN) or "nan" (a NaN cell: the same)."""
    L = np.stack([logit_rows(t, C, rng) for t in LOGIT_FAMILIES])
    bias = np.zeros(C, dtype=F32)
    if mask == "neginf":
        bias[rng.random(C) < 1 / 3] = -np.inf
        if np.isinf(bias).all():
            bias[rng.integers(0, C)] = 0
    elif mask in ("posinf", "nan"):
        bias[rng.integers(0, C)] = np.inf if mask == "posinf" else np.nan
    return L, bias


# ================================================================================================================ softmax, top-k
def all_nan_row(l32):
    """the kernel's probabilities of this row are all NaN: a NaN or a +inf logit (inf - inf), or nothing but -inf (0 / 0)"""
    l = np.asarray(l32)
    return bool(np.isnan(l).any() or (l == np.inf).any() or (l == -np.inf).all())


def softmax_truth(l32):
    """(C,) fp32 logits without NaN / +inf -> fp64 probabilities"""
    l = np.asarray(l32)
    assert l.dtype == F32
    l = l.astype(np.float64)
    e = np.exp(l - l.max())
    return e / e.sum()


def softmax_bound(l32, p):
    l = np.asarray(l32, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        rel = np.where(p > 0, np.abs(l - l.max()), 0.0)
    return (rel + -(-l.shape[-1] // 256) + 16) * U32 * p + TINY


def wave_sum32(v):
    """common.h wave_sum over the last axis (64 lanes): six butterfly steps; every lane ends with the same bits"""
    v = np.asarray(v, dtype=F32)
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., lanes ^ o]
    return v[..., 0]


def softmax_emulated(l32):
    """head_row_kernel's probabilities in numpy fp32, in its order: thread tid adds cells tid, tid + 256, ..., the wave butterfly,
    (w0 + w1) + (w2 + w3), then the division"""
    l = np.asarray(l32)
    assert l.dtype == F32
    C = l.shape[0]
    fin = l[~np.isnan(l)]
    mx = F32(max(fin.max(), -np.finfo(F32).max)) if fin.size else -np.finfo(F32).max
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp((l - mx).astype(F32)).astype(F32)
        pad = np.zeros(-(-C // 256) * 256, dtype=F32)
        pad[:C] = e
        acc = np.zeros(256, dtype=F32)
        for visit in pad.reshape(-1, 256):
            acc = acc + visit                                       # a padded 0 adds nothing: the bits are the unpadded chain's
        w = wave_sum32(acc.reshape(4, 64))
        sm = (w[0] + w[1]) + (w[2] + w[3])
        return (e / sm).astype(F32)


def _rank(values, k, ties_highest=False, no_retire=False):
    """k indices by (value desc, index asc), a NaN above every number"""
    v = np.asarray(values, dtype=np.float64)
    idx = np.arange(v.shape[0])
    key = np.where(np.isnan(v), np.inf, v)
    order = np.lexsort((-idx if ties_highest else idx, -key))
    return np.repeat(order[:1], k) if no_retire else order[:k]


def effective_logits(l32):
    """fp64 logits with the cells whose probability is exactly 0 in fp32 set to -inf (one tie class)"""
    l = np.asarray(l32).astype(np.float64)
    return np.where(softmax_truth(np.asarray(l32)) < ZERO_BELOW, -np.inf, l)


def topk_expected(l32, k, ties_highest=False, no_retire=False):
    if all_nan_row(l32):
        return np.arange(k)
    return _rank(effective_logits(l32), k, ties_highest, no_retire)


def topk_emulated(p32, k):
    """the selection rounds of head_row_kernel on fp32 probabilities"""
    return _rank(p32, k)


def topk_slack(l32):
    """8 u (1 + |l - max|) per cell; 0 for the cells whose probability is exactly 0 (they tie with each other only)"""
    eff = effective_logits(l32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(eff), 8 * U32 * (1 + np.abs(eff - eff.max())), 0.0)


def topk_check(l32, k, got_val, got_idx, got_argmax, got_llh, centroids):
    """-> the positions at which the kernel's list differs from topk_expected, every one of them an allowed exception; raises
    AssertionError on anything else (see the module docstring of tests/test_gpu_decision.py for the rules)"""
    l32, got_val, got_idx = np.asarray(l32), np.asarray(got_val), np.asarray(got_idx)
    C = l32.shape[0]
    want = topk_expected(l32, k)
    if all_nan_row(l32):
        assert np.isnan(got_val).all(), "an all-NaN row lists a number"
        assert np.array_equal(got_idx, want) and got_argmax == 0, "an all-NaN row lists 0 .. k-1"
        assert np.array_equal(np.asarray(got_llh), np.asarray(centroids)[0]), "centroid of an all-NaN row"
        return []
    assert not np.isnan(got_val).any(), "NaN among the listed probabilities"
    assert (got_val[:-1] >= got_val[1:]).all(), "listed values ascend somewhere"
    assert ((got_idx >= 0) & (got_idx < C)).all() and len(set(got_idx.tolist())) == k, "indices repeat or leave the range"
    assert got_argmax == got_idx[0], "argmax is not the head of the list"
    assert np.array_equal(np.asarray(got_llh), np.asarray(centroids)[got_idx[0]]), "pred_llh is not the centroid row, bit for bit"
    eff, slack = effective_logits(l32), topk_slack(l32)
    diff = np.flatnonzero(got_idx != want)
    for r in diff:
        a, e = got_idx[r], want[r]
        close = (eff[a] == eff[e]) or abs(eff[a] - eff[e]) <= max(slack[a], slack[e])
        assert close, f"position {r}: cell {a} (logit {l32[a]!r}) listed where cell {e} (logit {l32[e]!r}) belongs"
    rest = np.ones(C, dtype=bool)
    rest[got_idx] = False
    if rest.any():
        c, last = np.flatnonzero(rest)[np.argmax(eff[rest])], got_idx[-1]
        assert eff[c] == eff[last] or eff[c] <= eff[last] + max(slack[c], slack[last]), \
            f"cell {c} (logit {l32[c]!r}) is not listed, cell {last} (logit {l32[last]!r}) is"
    return diff.tolist()


# ================================================================================================================ refiner: records
def distances_truth(rows, qbar32):
    """rows (n,1024) fp32, qbar32 (1024,) fp32 -> fp64 (n,)"""
    rows, qbar32 = np.asarray(rows), np.asarray(qbar32)
    assert rows.dtype == F32 and qbar32.dtype == F32
    return np.sqrt(((rows.astype(np.float64) - qbar32.astype(np.float64)) ** 2).sum(axis=-1))


def distances_emulated(rows, qbar32):
    """row_sqdist + sqrtf in numpy fp32: lane l owns columns i * 256 + l * 4 + e (i, e = 0 .. 3) as one fmaf chain, then the butterfly"""
    d = (np.asarray(rows, dtype=F32) - np.asarray(qbar32, dtype=F32)).reshape(-1, 4, 64, 4).astype(np.float64)
    s = np.zeros((d.shape[0], 64), dtype=F32)
    for i in range(4):
        for e in range(4):
            s = (d[:, i, :, e] * d[:, i, :, e] + s).astype(F32)
    return np.sqrt(wave_sum32(s)).astype(F32)


def record_ints(rec12):
    """(..., 12) fp32 -> (..., 5) int32: pid1, pid2, t1, t2, count"""
    return np.ascontiguousarray(np.asarray(rec12, dtype=F32)[..., [5, 6, 9, 10, 11]]).view(np.int32)


def _top2(d, ids, farthest=False, ties_highest=False):
    """(best, runner-up) of `ids` by (d asc | desc, id asc); -1 where there is none"""
    if len(ids) == 0:
        return -1, -1
    key = -np.asarray(d, dtype=np.float64) if farthest else np.asarray(d, dtype=np.float64)
    order = np.lexsort((-np.asarray(ids) if ties_highest else np.asarray(ids), key))
    return int(order[0]), (int(order[1]) if len(ids) > 1 else -1)


def _empty12():
    rec = np.array([-100000.0, 0, 0, 0, np.inf, 0, 0, -1, -1, 0, 0, 0], dtype=F32)
    rec.view(np.int32)[[5, 6, 9, 10, 11]] = [-1, -1, -1, -1, 0]      # the int32 fields are written as bits, never as float values
    return rec


def candidate_record(bank, qbar32, cell, ties_highest=False, runner_up_own_wave=False, swap_near_far=False, drop_tail=False):
    """-> (rec4, rec12, truth) fp32 records of one (query, candidate); truth = dict of the fp64 distances behind the fields
    (d1, d2, far1, far2, and all prototype / member distances).  The distance fields are the fp64 distances rounded to fp32."""
    s, e = int(bank.cell_off[cell]), int(bank.cell_off[cell + 1])
    ids = np.arange(s, e)
    if drop_tail:                                                   # every wave loses the row its paired loop leaves over
        ids = np.array([r for r in ids if not (((e - s) - (r - s) % 4 + 3) // 4 % 2 == 1 and r + 4 >= e)], dtype=np.int64)
    if len(ids) == 0:
        return _empty12()[:4].copy(), _empty12(), dict(empty=True)
    d = distances_truth(bank.proto_emb[ids], qbar32)
    a, b = _top2(d, ids, farthest=swap_near_far, ties_highest=ties_highest)
    if runner_up_own_wave and b >= 0:
        same = np.flatnonzero(((ids - ids[a]) % 4 == 0) & (ids != ids[a]))
        b = int(same[_top2(d[same], ids[same], farthest=swap_near_far, ties_highest=ties_highest)[0]]) if len(same) else -1
    pid, cnt = int(ids[a]), int(bank.proto_count[ids[a]])
    rec = _empty12()
    ri = rec.view(np.int32)
    rec[0] = -d[a]
    rec[4], ri[5], ri[6] = (d[b] if b >= 0 else np.inf), pid, (int(ids[b]) if b >= 0 else -1)
    truth = dict(empty=False, proto_d=d, proto_ids=ids, d1=d[a], d2=d[b] if b >= 0 else np.inf)
    if cnt == 1:
        rec[1:3], rec[3], ri[11] = bank.proto_lnglat[pid], e - s, 1
        return rec[:4].copy(), rec, truth
    ms, me = int(bank.member_off[pid]), int(bank.member_off[pid + 1])
    pos = np.arange(ms, me)
    md = distances_truth(bank.train_emb[bank.member_idx[ms:me]], qbar32)
    fa, fb = _top2(md, pos, farthest=not swap_near_far, ties_highest=ties_highest)
    if runner_up_own_wave and fb >= 0:
        same = np.flatnonzero(((pos - pos[fa]) % 4 == 0) & (pos != pos[fa]))
        fb = int(same[_top2(md[same], pos[same], farthest=not swap_near_far, ties_highest=ties_highest)[0]]) if len(same) else -1
    t1 = int(bank.member_idx[pos[fa]])
    rec[1:3], rec[3] = bank.train_lnglat[t1], (e - s) + (me - ms)
    rec[7], rec[8] = md[fa], (md[fb] if fb >= 0 else -1)
    ri[9], ri[10], ri[11] = t1, (int(bank.member_idx[pos[fb]]) if fb >= 0 else -1), cnt
    truth.update(member_d=md, member_rows=bank.member_idx[ms:me], far1=md[fa], far2=md[fb] if fb >= 0 else -1.0)
    return rec[:4].copy(), rec, truth


# ================================================================================================================ refiner: selection
UNDERFLOW_BAND = (-104.0, -87.0)                                    # exp of an argument in here is subnormal in fp32: no family has one


def _argmax_torch(v):
    """first maximum; a NaN is the maximum (the first NaN wins)"""
    v = np.asarray(v)
    nan = np.flatnonzero(np.isnan(v))
    return int(nan[0]) if len(nan) else int(np.argmax(v))


def select(scores, cand_prob, T, init_llh, points, max_km):
    """scores (topk,) fp32, cand_prob (topk,) fp32 or None, init_llh (2,) fp64, points (topk,2) fp32 -> dict(refined, choice, gap,
    veto_km, clear).  gap: the relative distance of the best from the second product in fp64 with exp(x) = 0 for x < -104 (0: the
    two are equal, or every product is 0 / NaN -- the first wins either way; inf: one candidate).  clear: no exponent lies in
    UNDERFLOW_BAND, so fp32's exp is 0 exactly where the fp64 one was taken as 0."""
    s = np.asarray(scores, dtype=F32)
    n = s.shape[0]
    cp = np.asarray(cand_prob, dtype=F32) if cand_prob is not None else np.array([1.0] + [0.0] * (n - 1), dtype=F32)
    x = s / F32(T)
    with np.errstate(under="ignore", invalid="ignore", divide="ignore"):
        ex = np.where(x < -104, F32(0), np.exp(x)).astype(F32)
        sm = F32(0)
        for v in ex:
            sm = F32(sm + v)
        fin = cp * (ex / sm)
    refined = _argmax_torch(fin)
    x64 = s.astype(np.float64) / float(F32(T))
    prod = cp.astype(np.float64) * np.where(x64 < -104, 0.0, np.exp(x64))
    top = np.sort(prod)[::-1]
    gap = np.inf if n == 1 else (0.0 if not top[0] > 0 else float((top[0] - top[1]) / top[0]))
    km, _ = _georef.haversine_mixed_truth(np.asarray(points, dtype=F32)[refined], np.asarray(init_llh, dtype=np.float64))
    km = float(km)
    choice = _argmax_torch(cp) if km > max_km else refined
    clear = not ((x64 >= UNDERFLOW_BAND[0]) & (x64 <= UNDERFLOW_BAND[1])).any()
    return dict(refined=refined, choice=choice, gap=gap, veto_km=km, clear=clear)


# ================================================================================================================ banks
def _assemble(rng, q, cells):
    """cells: a list of cells, each a list of prototypes (distance m, member distances or None).  Every row is q plus its distance
    on one coordinate (random coordinate and sign), so its L2 distance from q is exactly |m|."""
    protos = [p for c in cells for p in c]
    n_p = len(protos)
    cell_off = np.concatenate([[0], np.cumsum([len(c) for c in cells])]).astype(np.int64)
    count = np.array([1 if m is None else len(m) for _, m in protos], dtype=np.int32)
    member_off = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    n_t = int(member_off[-1])

    def rows(dist):
        out = np.broadcast_to(q, (len(dist), DIM)).copy()
        col = (rng.integers(0, DIM) + 37 * np.arange(len(dist))) % DIM   # neighbours never share a coordinate: no two equal rows in a cell
        out[np.arange(len(dist)), col] += (np.asarray(dist) * rng.choice([-1, 1], len(dist))).astype(F32)
        return out
    member_d = np.concatenate([[d] if m is None else np.asarray(m) for d, m in protos]).astype(np.int64)
    member_idx = rng.permutation(n_t).astype(np.int64)              # list position and training row disagree
    train_emb = np.empty((n_t, DIM), dtype=F32)
    train_emb[member_idx] = rows(member_d)

    def lnglat(n):
        return np.stack([rng.uniform(-180, 180, n), rng.uniform(-80, 80, n)], axis=1).astype(F32)
    return SimpleNamespace(proto_emb=rows([d for d, _ in protos]), cell_off=cell_off, proto_lnglat=lnglat(n_p), proto_count=count,
                           member_off=member_off, member_idx=member_idx, train_emb=train_emb, train_lnglat=lnglat(n_t))


PROTO_SMALL = tuple(range(1, 18))
PROTO_LARGE = (31, 32, 33, 63, 64, 65, 255, 256, 257)
MEMBER_SIZES = (2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 33)


def integer_bank(rng):
    """-> (bank, q (1024,) fp32 integer-valued, kinds: one tag per cell):
    prototype cells of every size 1 .. 17 with the nearest row at every position; the sizes around the wave and unroll strides with
    the nearest at the first and the last positions; every ordered (nearest, runner-up) pair and every tied pair for n <= 12; member
    clusters with the farthest member at every position and every tied pair; singleton clusters and empty cells in between."""
    q = rng.integers(-8, 9, DIM).astype(F32)
    cells, kinds = [], []

    def proto_cell(n, first, second, tied, kind):
        base = int(rng.integers(2, 7))
        d = base + 2 + rng.integers(0, 20, n)
        d[first] = base
        if second is not None:
            d[second] = base if tied else base + 1
        cells.append([(int(x), None) for x in d]); kinds.append(kind)
    for n in PROTO_SMALL:
        for i in range(n):
            proto_cell(n, i, None if n == 1 else int((i + 1 + rng.integers(0, n - 1)) % n), False, "nearest_small")
    for n in PROTO_LARGE:
        for i in sorted({0, 3, 4, 7, 8} | set(range(n - 9, n))):
            proto_cell(n, i, int((i + 1 + rng.integers(0, n - 1)) % n), False, "nearest_large")
    for n in range(2, 13):
        for i in range(n):
            for j in range(n):
                if i != j:
                    proto_cell(n, i, j, False, "ordered_pair")
                if i < j:
                    proto_cell(n, i, j, True, "tied_protos")

    def member_cell(size, first, second, tied, kind):
        m = rng.integers(1, 16, size)
        m[first] = 30
        m[second] = 30 if tied else 20
        cluster = (int(rng.integers(2, 7)), [int(x) for x in m])
        single = (cluster[0] + 1 + int(rng.integers(0, 5)), None)   # a singleton cluster farther away, before or after
        cells.append([[cluster], [cluster, single], [single, cluster]][len(cells) % 3]); kinds.append(kind)
    for size in MEMBER_SIZES:
        for i in range(size):
            member_cell(size, i, int((i + 1 + rng.integers(0, size - 1)) % size), False, "farthest")
        for i in range(size):
            for j in range(i + 1, size):
                member_cell(size, i, j, True, "tied_members")
    order = rng.permutation(len(cells))
    mixed, tags = [], []
    for n, c in enumerate(order):
        if n % 9 == 4:
            mixed.append([]); tags.append("empty")
        mixed.append(cells[c]); tags.append(kinds[c])
    return _assemble(rng, q, mixed), q, tags


def integer_panels(qbar, P, rng, B=1):
    """(B,P,1024) fp32 integer panels whose mean is qbar exactly, partial sums included"""
    d = rng.integers(-4, 5, (B, P, DIM))
    d[:, P - 1] = 0
    d[:, P - 1] = -d.sum(axis=1)
    return (qbar[None, None, :] + d).astype(F32)


def gaussian_bank(rng, cells=36):
    """cells of 0 .. 20 Gaussian prototypes, half of them clusters of 2 .. 6 members around the prototype"""
    n_per = rng.integers(1, 21, cells)
    n_per[rng.random(cells) < 0.1] = 0
    cell_off = np.concatenate([[0], np.cumsum(n_per)]).astype(np.int64)
    n_p = int(cell_off[-1])
    count = np.where(rng.random(n_p) < 0.5, rng.integers(2, 7, n_p), 1).astype(np.int32)
    member_off = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    n_t = int(member_off[-1])
    member_idx = rng.permutation(n_t).astype(np.int64)
    proto = rng.standard_normal((n_p, DIM)).astype(F32)
    train = np.empty((n_t, DIM), dtype=F32)
    train[member_idx] = np.repeat(proto, count, axis=0) + F32(0.3) * rng.standard_normal((n_t, DIM)).astype(F32)

    def lnglat(n):
        return np.stack([rng.uniform(-180, 180, n), rng.uniform(-80, 80, n)], axis=1).astype(F32)
    return SimpleNamespace(proto_emb=proto, cell_off=cell_off, proto_lnglat=lnglat(n_p), proto_count=count, member_off=member_off,
                           member_idx=member_idx, train_emb=train, train_lnglat=lnglat(n_t))


def queries_near(bank, cells, radius, P, rng):
    """one query per cell in `cells` (non-empty), about `radius` away from one of its prototypes: (len(cells), P, 1024) fp32"""
    out = np.empty((len(cells), P, DIM), dtype=F32)
    for n, c in enumerate(cells):
        row = bank.proto_emb[rng.integers(bank.cell_off[c], bank.cell_off[c + 1])]
        g = rng.standard_normal(DIM)
        centre = row + radius * g / np.linalg.norm(g)
        out[n] = (centre[None] + 0.1 * radius / 32 * rng.standard_normal((P, DIM))).astype(F32)
    return out


def selection_case(records, n_cells, B, topk, k, rng, T, max_km, probs="given", repeat=False, only=None):
    """Candidate lists over the cells of a bank whose records (cell -> rec4) are known, redrawn until the promise of `select` holds:
    gap 0 or >= 1e-3, veto distance at least 1 km from max_km, no exponent in the subnormal band.  probs: "given" (descending, as a
    head lists them), "none", "zeros".  repeat: the first cell of a list appears twice in it.  only: draw from these cells alone.
    -> dict(cand (B,k) i64, prob (B,k) f32 or None, init (B,2) f64, expect: list of select() results)"""
    pool = np.arange(n_cells) if only is None else np.asarray(only)
    cand, prob, init, expect = np.empty((B, k), np.int64), np.zeros((B, k), F32), np.empty((B, 2)), []
    for b in range(B):
        for attempt in range(200):
            c = rng.choice(pool, k, replace=len(pool) < k)
            p = np.sort(rng.uniform(0.001, 1, k))[::-1] / k if probs == "given" else np.zeros(k)
            if repeat and topk > 1:
                c[topk - 1] = c[0]
                if b % 2 == 0:
                    p[topk - 1] = p[0]                              # the same record twice: gap 0 where it is the best, the first wins
            p = p.astype(F32)
            ll = np.array([rng.uniform(-180, 180), rng.uniform(-80, 80)])
            rec = np.stack([records[int(x)] for x in c[:topk]])
            r = select(rec[:, 0], None if probs == "none" else p[:topk], T, ll, rec[:, 1:3], max_km)
            if r["clear"] and (r["gap"] == 0 or r["gap"] >= 1e-3) and abs(r["veto_km"] - max_km) >= 1:
                break
        else:
            raise AssertionError("no candidate list with the promised gaps in 200 draws")
        cand[b], prob[b], init[b] = c, p, ll
        expect.append(r)
    return dict(cand=cand, prob=None if probs == "none" else prob, init=init, expect=expect)


# ================================================================================================================ certainty
def _tol(m, g, beta, en):
    g2 = float(g @ g)
    if not np.isfinite(m) and m > 0:
        return np.inf
    if g2 == 0:
        return np.inf
    return (m - en * float(g @ beta)) / (en * np.sqrt(g2) / 32.0)


def _head_tol_restated(logits, e, W, idx, beta, wmax, wbmax):
    C = W.shape[0]
    en = np.linalg.norm(e)
    c0 = idx[0]
    best, code = np.inf, 0
    for j in range(1, len(idx)):
        t = _tol(logits[c0] - logits[idx[j]], W[c0] - W[idx[j]], beta, en)
        if t < best:
            best, code = t, j
    if len(idx) < C:
        gmax = np.linalg.norm(W[c0]) + wmax
        t = (logits[c0] - logits[idx[-1]] - en * (float(W[c0] @ beta) + wbmax)) / (en * gmax / 32.0)
        if t < best:
            best, code = t, -1
    return best, code


def _refine_tol_restated(rec, ints, L, cand, topk, n_eval, C, W, bankp, bankt, e, beta, wmax, wbmax, T, r, ch, fin_r, cell_off=None,
                         member_off=None, member_idx=None):
    en = np.linalg.norm(e)
    S = L + rec[:, 0] / T
    if ints[r, 0] < 0 and all(ints[j, 0] < 0 for j in range(topk)):
        return np.inf, 0                                         # a set of empty cells: nothing can change
    if not (fin_r >= 1e-30) or ints[r, 0] < 0:
        return 0.0, -9                                           # underflow, or an empty cell winning a set that is not all empty

    def pair_s(a, j):
        pa, pj = ints[a, 0], ints[j, 0]
        da, dj = -rec[a, 0], -rec[j, 0]
        ia = (1.0 / T) / da if (pa >= 0 and da > 0) else 0.0
        ij = (1.0 / T) / dj if (pj >= 0 and dj > 0) else 0.0
        g = W[cand[a]] - W[cand[j]] + (ia * bankp[pa] if pa >= 0 else 0) - (ij * bankp[pj] if pj >= 0 else 0) + (ij - ia) * e
        return _tol(S[a] - S[j], g, beta, en)
    best, code = np.inf, 0
    for j in range(topk):
        if j == r:
            continue
        t = pair_s(r, j)
        if t < best:
            best, code = t, 1000 + j
    for j in range(topk, n_eval):
        t_in = _tol(L[topk - 1] - L[j], W[cand[topk - 1]] - W[cand[j]], beta, en)
        t = t_in if r == topk - 1 else max(t_in, pair_s(r, j))
        if t < best:
            best, code = t, 2000 + j
    if n_eval > topk and n_eval < C:
        gmax = np.linalg.norm(W[cand[topk - 1]]) + wmax
        t = (L[topk - 1] - L[n_eval - 1] - en * (float(W[cand[topk - 1]] @ beta) + wbmax)) / (en * gmax / 32.0)
        if t < best:
            best, code = t, 2999
    for which, x in enumerate((r, ch)):
        if which == 1 and ch == r:
            break
        p1, t1 = ints[x, 0], ints[x, 2]
        if p1 >= 0:                                              # nearest prototype against EVERY other prototype of the cell
            lo, hi = cell_off[cand[x]], cell_off[cand[x] + 1]
            w = e - bankp[p1]
            dw = np.linalg.norm(w)
            for j in range(lo, hi):
                if j == p1:
                    continue
                l = e - bankp[j]
                dl = np.linalg.norm(l)
                t = _tol(dl - dw, l / dl - w / dw, beta, en)
                if t < best:
                    best, code = t, 3000 + which
        if t1 >= 0 and p1 >= 0:                                  # farthest member against every other member of the cluster
            w = e - bankt[t1]
            dw = np.linalg.norm(w)
            for jj in range(member_off[p1], member_off[p1 + 1]):
                j = member_idx[jj]
                if j == t1:
                    continue
                l = e - bankt[j]
                dl = np.linalg.norm(l)
                t = _tol(dw - dl, w / dw - l / dl, beta, en)
                if t < best:
                    best, code = t, 4000 + which
    return best, code
