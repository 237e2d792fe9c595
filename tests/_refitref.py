"""A numpy restatement of the refiner's selection (refine_select_kernel, csrc/refine.hip) at every point of a grid, on plain arrays of
records -- no bank: what pg_refine_sweep (csrc/refine_sweep.hip, contract: include/pigeon_hip.h) must write.

fp32 where the kernel is fp32: ex_j = exp(score_j / T), the sequential sum over j < topk, fin_j = cp_j * (ex_j / sum) without a max
shift; torch.argmax's order (first maximum, the first NaN wins); the veto distance by oracle.pigeon_oracle.haversine with the initial
point in float64 and the refined point in float32; the veto fires on `>`; the fallback is argmax(cp) over j < topk.

`select_grid` also says per (g, row) whether the decision is TIGHT: the two largest fin within 2^-20 relative (a device expf one ulp
off may pick the other), a sum in the subnormal range, or the veto distance within 1e-9 relative of max_km (a device sin one ulp off
may flip it).  Everything else is unambiguous and is compared at zero tolerance.

`mistake=` plants one deliberate error; tests/test_refitref_cpu.py shows that each is caught at a named (row, g).
"""
import numpy as np
import torch

from oracle.pigeon_oracle import haversine

MISTAKES = ("sum_all", "max_shift", "veto_ge", "fallback_zero", "renorm", "swap_tr", "veto_bit_lost")
F32 = np.float32


def grid_index(nT, nR, iK, iT, iR):
    return (iK * nT + iT) * nR + iR


def argmax_torch(v):
    """(B,t) -> (B,) first maximum per row; a NaN is the maximum and the first NaN wins"""
    B, t = v.shape
    bi = np.zeros(B, dtype=np.int64)
    bv = v[:, 0].copy()
    for j in range(1, t):
        x = v[:, j]
        take = ~np.isnan(bv) & (np.isnan(x) | (x > bv))
        bv = np.where(take, x, bv)
        bi = np.where(take, j, bi)
    return bi


def veto_distances(init, lnglat):
    """init (B,2) float64, lnglat (B,n,2) float32 -> (B,n) float64 km, with torch's promotion (the reference's call)"""
    B, n, _ = lnglat.shape
    x = torch.from_numpy(np.repeat(np.asarray(init, dtype=np.float64), n, axis=0))
    y = torch.from_numpy(np.ascontiguousarray(lnglat, dtype=np.float32).reshape(B * n, 2))
    return haversine(x, y).numpy().reshape(B, n)


def records(scratch):
    """scratch (B,n,SC) float32 records -> (score (B,n), lnglat (B,n,2))"""
    scratch = np.asarray(scratch, dtype=np.float32)
    return scratch[:, :, 0], scratch[:, :, 1:3]


def select_grid(score, lnglat, cand_prob, init, topks, temps, max_kms, mistake=None):
    """score (B,n) f32, lnglat (B,n,2) f32, cand_prob (B,>=n) f32 or None, init (B,2) f64; topks / temps / max_kms sequences.
    Returns (choice (G,B) uint8: candidate in bits 0-5, bit 7 = vetoed; tight (G,B) bool; dist (B,n) float64)."""
    assert mistake is None or mistake in MISTAKES
    score = np.asarray(score, dtype=F32)
    B, n = score.shape
    if cand_prob is None:
        cp_all = np.zeros((B, n), dtype=F32)
        cp_all[:, 0] = 1
    else:
        cp_all = np.asarray(cand_prob, dtype=F32)[:, :n]
    dist = veto_distances(init, lnglat)
    nK, nT, nR = len(topks), len(temps), len(max_kms)
    choice = np.zeros((nK * nT * nR, B), dtype=np.uint8)
    tight = np.zeros((nK * nT * nR, B), dtype=bool)
    rows = np.arange(B)
    with np.errstate(all="ignore"):
        for iT, T in enumerate(temps):
            z = (score / F32(T)).astype(F32)
            for iK, topk in enumerate(topks):
                zt = z[:, :topk]
                if mistake == "max_shift":
                    zt = (zt - zt.max(axis=1, keepdims=True)).astype(F32)
                ex = np.exp(zt).astype(F32)
                ex_sum = np.exp(z).astype(F32) if mistake == "sum_all" else ex
                s = np.zeros(B, dtype=F32)
                for j in range(ex_sum.shape[1]):                     # torch.sum of <= 64 elements: sequential
                    s = (s + ex_sum[:, j]).astype(F32)
                cp = cp_all[:, :topk]
                if mistake == "renorm":
                    cs = np.zeros(B, dtype=F32)
                    for j in range(topk):
                        cs = (cs + cp[:, j]).astype(F32)
                    cp = (cp / cs[:, None]).astype(F32)
                fin = (cp * (ex / s[:, None]).astype(F32)).astype(F32)
                refined = argmax_torch(fin)
                fallback = np.zeros(B, dtype=np.int64) if mistake == "fallback_zero" else argmax_torch(cp_all[:, :topk])
                # tight: the runner-up of fin within 2^-20 relative of the winner, or a subnormal sum
                # (a rival whose score and probability are the winner's own bits has the winner's product on any device: not tight)
                top = fin[rows, refined].astype(np.float64)[:, None]
                within = np.isfinite(top) & np.isfinite(fin) & (np.abs(top - fin) <= 2.0 ** -20 * np.abs(top))
                other = (zt != zt[rows, refined][:, None]) | (cp != cp[rows, refined][:, None])
                close = (within & other).any(axis=1)
                close |= (s > 0) & (s < F32(2.0 ** -120))
                d = dist[rows, refined]
                for iR, max_km in enumerate(max_kms):
                    veto = (d >= max_km) if mistake == "veto_ge" else (d > max_km)
                    g = grid_index(nR, nT, iK, iR, iT) if mistake == "swap_tr" else grid_index(nT, nR, iK, iT, iR)
                    bit = 0 if mistake == "veto_bit_lost" else 0x80
                    choice[g] = np.where(veto, fallback | bit, refined).astype(np.uint8)
                    near = np.isfinite(d) & np.isfinite(max_km) & (np.abs(d - max_km) <= 1e-9 * abs(max_km))
                    tight[g] = close | near
    return choice, tight, dist


GAUSSIAN_GRID = (list(range(1, 13)), [0.05, 0.6, 1.6, 20.0], [0.0, 500.0, 2500.0, float("inf")])


def gaussian_batch(seed=11, B=300, n=12):
    """The seeded batch of the Gaussian-score GPU test: records (B,n,4) f32 with scores -|N(30, 3)|, points around the initial
    prediction (a few degrees off, so the thresholds of GAUSSIAN_GRID cut through them), softmax-like candidate probabilities in
    descending order, initial predictions (B,2) f64."""
    rng = np.random.default_rng(seed)
    scratch = np.zeros((B, n, 4), dtype=np.float32)
    scratch[:, :, 0] = -np.abs(rng.normal(30.0, 3.0, (B, n))).astype(np.float32)
    init = np.stack([rng.uniform(-170, 170, B), rng.uniform(-70, 70, B)], axis=1)
    scratch[:, :, 1] = (init[:, None, 0] + rng.normal(0, 8.0, (B, n))).astype(np.float32)
    scratch[:, :, 2] = np.clip(init[:, None, 1] + rng.normal(0, 8.0, (B, n)), -89, 89).astype(np.float32)
    p = np.sort(rng.dirichlet(np.full(n, 0.7), B), axis=1)[:, ::-1]
    return scratch, np.ascontiguousarray(p, dtype=np.float32), init


def first_difference(a, b):
    """(row, g) of the first element at which two (G,B) choice arrays differ, or None"""
    where = np.argwhere(np.asarray(a) != np.asarray(b))
    if where.size == 0:
        return None
    g, row = where[0]
    return int(row), int(g)


def totals(choice, values, n_eval):
    """choice (G,B) uint8, values (B,n_eval,V) float64 -> (G,V+2) float64 by a host gather and numpy's sum: the columns, the rows whose
    choice is not candidate 0, the vetoed rows.  A byte whose index is >= n_eval gives its grid point NaN."""
    choice = np.asarray(choice)
    G, B = choice.shape
    V = values.shape[2]
    out = np.empty((G, V + 2), dtype=np.float64)
    rows = np.arange(B)
    for g in range(G):
        idx = (choice[g] & 63).astype(np.int64)
        if (idx >= n_eval).any():
            out[g] = np.nan
            continue
        out[g, :V] = values[rows, idx].sum(axis=0)
        out[g, V] = (idx != 0).sum()
        out[g, V + 1] = ((choice[g] & 0x80) != 0).sum()
    return out
