"""tests/_bankref.py pinned on the CPU (no GPU, no torch device): with sigma = 0 it is tests/_decisionref.py's restatement; each of
six planted mistakes changes tol or code on the case built for it; and a Monte Carlo over bank perturbations drawn under the error
model agrees with it -- rows it calls certain at kappa = 6 never change an output in 200 draws, and among the rows that the sigma = 0
rule calls certain at the exact tier's floor (5e-6) but the bank rule does not, some do change."""
from types import SimpleNamespace

import numpy as np
import pytest

import _bankref as br
from _decisionref import DIM, F32, _refine_tol_restated, gaussian_bank, rng_of

EPS_B, KAPPA, EPS_EXACT = 3e-4, 6.0, 5e-6


def _unit(rng):
    g = rng.standard_normal(DIM)
    return g / np.linalg.norm(g)


def _copy(bank):
    return SimpleNamespace(**{k: np.array(v) for k, v in vars(bank).items()})


def _dist(rows, e):
    return np.linalg.norm(rows.astype(np.float64) - e, axis=1)


def _query_near(bank, cell, radius, rng, scale=1.0, clustered=None):
    """(1,1024) fp32 at `radius` from one prototype of `cell` (scaled by `scale` first): the nearest by a wide margin"""
    lo, hi = int(bank.cell_off[cell]), int(bank.cell_off[cell + 1])
    rows = [p for p in range(lo, hi) if clustered is None or (bank.proto_count[p] > 1) == clustered]
    p = rows[int(rng.integers(0, len(rows)))]
    return (scale * bank.proto_emb[p].astype(np.float64) + radius * _unit(rng)).astype(F32)[None], p


def plant_proto(bank, e, cell, near, gap, rng):
    """another prototype of `cell` moved to distance d(near) + gap from e"""
    lo, hi = int(bank.cell_off[cell]), int(bank.cell_off[cell + 1])
    other = next(p for p in range(lo, hi) if p != near)
    d1 = _dist(bank.proto_emb[near:near + 1], e)[0]
    bank.proto_emb[other] = (e + (d1 + gap) * _unit(rng)).astype(F32)


def plant_member(bank, e, proto, gap, rng):
    """a member of `proto`'s cluster moved to gap inside the farthest one's distance"""
    mem = bank.member_idx[int(bank.member_off[proto]):int(bank.member_off[proto + 1])]
    d = _dist(bank.train_emb[mem], e)
    far = int(np.argmax(d))
    other = mem[(far + 1) % len(mem)]
    bank.train_emb[other] = (e + (d[far] - gap) * _unit(rng)).astype(F32)


def _cells(bank, min_protos=2, clustered=False):
    n = np.diff(bank.cell_off)
    out = []
    for c in np.flatnonzero(n >= min_protos):
        cnt = bank.proto_count[int(bank.cell_off[c]):int(bank.cell_off[c + 1])]
        if not clustered or (cnt > 1).any():
            out.append(int(c))
    return out


def _probs(k, rng, lead=0.5):
    p = np.sort(rng.uniform(0.01, 0.1, k))[::-1]
    p[0] = lead
    return p.astype(F32)


class Case:
    """rows of one bank: `rows` (from br.make_row), and everything `decisions` needs"""

    def __init__(self, bank, queries, cands, probs, topk, n_eval, T, seed, with_beta):
        rng = rng_of(77, seed)
        self.bank, self.topk, self.n_eval, self.T = bank, topk, n_eval, T
        self.C = bank.cell_off.shape[0] - 1
        self.W = (rng.standard_normal((self.C, DIM)) * 0.3).astype(F32).astype(np.float64)
        self.beta = (3e-4 * rng.standard_normal(DIM) / 32).astype(F32).astype(np.float64) if with_beta else np.zeros(DIM)
        self.wmax = float(np.linalg.norm(self.W, axis=1).max())
        self.wbmax = float(np.abs(self.W @ self.beta).max())
        self.rows = [br.make_row(bank, q, c, p, topk, n_eval, T) for q, c, p in zip(queries, cands, probs)]

    def args(self, i):
        return br.row_args(self.rows[i], self.topk, self.n_eval, self.C, self.W, self.bank, self.beta, self.wmax, self.wbmax, self.T)

    def tol(self, i, sigma, mistake=None):
        pos, kw = self.args(i)
        return br.refine_tol_bank(*pos, sigma=sigma, mistake=mistake, **kw)

    def plain(self, i):
        pos, kw = self.args(i)
        return _refine_tol_restated(*pos, **kw)


def general_case(seed, topk, n_eval, k, T, with_beta, B=6):
    rng = rng_of(11, seed)
    bank = gaussian_bank(rng, cells=24)
    C = bank.cell_off.shape[0] - 1
    qs, cs, ps = [], [], []
    for _ in range(B):
        cand = rng.permutation(C)[:k]
        full = [c for c in cand[:topk] if bank.cell_off[c + 1] > bank.cell_off[c]]
        q = _query_near(bank, full[0], 20.0, rng)[0] if full else rng.standard_normal((1, DIM)).astype(F32)
        qs.append(np.repeat(q, 2, axis=0) + (0.01 * rng.standard_normal((2, DIM))).astype(F32))       # two panels
        cs.append(cand)
        ps.append(np.sort(rng.uniform(0.01, 0.3, k))[::-1].astype(F32))
    return Case(bank, qs, cs, ps, topk, n_eval, T, seed, with_beta)


def planted_case(name):
    """the case named for a mistake: one row whose tightest decision is the one the mistake touches -> (case, sigma)"""
    rng = rng_of(23, br.MISTAKES.index(name))
    bank = _copy(gaussian_bank(rng, cells=16))
    T, sigma = 1.6, KAPPA * EPS_B
    if name in ("no_inv_t", "boundary_term"):
        # two candidates near one prototype each, at distances that differ by 6e-3 T; equal probabilities inside the set
        a, b, c = _cells(bank)[:3]
        q, pa = _query_near(bank, a, 12.0, rng)
        e = q[0].astype(np.float64)
        lo = int(bank.cell_off[b])
        if name == "no_inv_t":
            bank.proto_emb[lo] = (e + (12.0 + 6e-3 * T) * _unit(rng)).astype(F32)
            return Case(bank, [q], [np.array([a, b])], [np.array([0.3, 0.3], F32)], 2, 2, T, 1, False), sigma
        # the set boundary is the tightest: the last member of the set wins (so getting in is all an outsider needs) and the
        # candidate just outside has almost its probability; the last evaluated one has next to none (code 2999 stays loose)
        d = _cells(bank)[3]
        return Case(bank, [q], [np.array([b, a, c, d])], [np.array([0.4, 0.2, 0.2 * (1 - 1e-3), 1e-6], F32)], 2, 4, T, 2, False), sigma
    if name in ("winner_only", "query_norm"):
        a, b = _cells(bank)[:2]
        q, p = _query_near(bank, a, 12.0, rng, scale=3.0 if name == "query_norm" else 1.0)
        plant_proto(bank, q[0].astype(np.float64), a, p, 6e-3 if name == "winner_only" else 2e-2, rng)
        return Case(bank, [q], [np.array([a, b])], [_probs(2, rng)], 2, 2, T, 3, False), sigma
    if name == "drop_farthest":
        a, b = _cells(bank, clustered=True)[:2]
        q, p = _query_near(bank, a, 12.0, rng, clustered=True)
        plant_member(bank, q[0].astype(np.float64), p, 6e-3, rng)
        return Case(bank, [q], [np.array([a, b])], [_probs(2, rng)], 2, 2, T, 4, False), sigma
    if name == "empty_norm":
        # a one-prototype cell without a cluster against an empty cell: the only decision is the score pair, margin 100000 / T
        bank = SimpleNamespace(proto_emb=rng.standard_normal((1, DIM)).astype(F32), cell_off=np.array([0, 1, 1], np.int64),
                               proto_lnglat=np.zeros((1, 2), F32), proto_count=np.ones(1, np.int32), member_off=np.array([0, 1], np.int64),
                               member_idx=np.zeros(1, np.int64), train_emb=rng.standard_normal((1, DIM)).astype(F32),
                               train_lnglat=np.zeros((1, 2), F32))
        q = (bank.proto_emb[0].astype(np.float64) + 12.0 * _unit(rng)).astype(F32)[None]
        return Case(bank, [q], [np.array([0, 1])], [np.array([0.5, 0.4], F32)], 2, 2, T, 5, False), 3e4
    raise KeyError(name)


GENERAL = [(1, 1, 1, 1.6, False), (2, 4, 6, 0.6, True), (5, 9, 12, 1.6, True), (3, 3, 3, 1.0, False)]


@pytest.fixture(scope="module")
def planted():
    return {m: planted_case(m) for m in br.MISTAKES}


@pytest.fixture(scope="module")
def monte_carlo_case():
    """8 queries on a 12-cell Gaussian bank, every one nearest to one prototype by a wide margin, with a second prototype planted
    gap behind it (even rows) or a second member planted gap inside the farthest one (odd rows).  The bank's noise moves such a
    margin by about eps_b * 32 * sqrt(2) / 32 = 4.2e-4 (rows of norm 32): gaps below 6 x that are not certain under the bank rule,
    all of them are under the sigma = 0 rule, whose floor is about 6 * 5e-6 * |g| = 4e-5."""
    rng = rng_of(31)
    bank = _copy(gaussian_bank(rng, cells=12))
    gaps = (1e-4, 1e-4, 3e-4, 3e-4, 8e-4, 8e-4, 2e-2, 2e-2)
    near, clus = _cells(bank), _cells(bank, clustered=True)
    C = bank.cell_off.shape[0] - 1
    qs, cs, ps = [], [], []
    for i, gap in enumerate(gaps):
        a = (clus if i % 2 else near)[i // 2]
        q, p = _query_near(bank, a, 10.0, rng, clustered=True if i % 2 else None)
        e = q[0].astype(np.float64)
        if i % 2:
            plant_member(bank, e, p, gap, rng)
        else:
            plant_proto(bank, e, a, p, gap, rng)
        others = [c for c in rng.permutation(C) if c != a][:3]
        qs.append(q); cs.append(np.array([a] + others)); ps.append(_probs(4, rng))
    return Case(bank, qs, cs, ps, 2, 4, 1.6, 9, False)


def test_sigma_zero_is_the_plain_restatement(planted, monte_carlo_case):
    cases = [general_case(n, *g) for n, g in enumerate(GENERAL)] + [c for c, _ in planted.values()] + [monte_carlo_case]
    codes = set()
    for case in cases:
        for i in range(len(case.rows)):
            t, c, _ = case.tol(i, 0.0)
            want_t, want_c = case.plain(i)
            assert t == want_t and c == want_c, (i, t, want_t, c, want_c)
            codes.add(c // 1000)
    assert {1, 2, 3, 4} <= codes


def test_a_bank_error_only_lowers_tolerances():
    case = general_case(1, *GENERAL[1])
    for i in range(len(case.rows)):
        ts = [case.tol(i, s)[0] for s in (0.0, 1e-4, 1e-3, 1e-2, 1.0)]
        assert all(a >= b for a, b in zip(ts[:-1], ts[1:])), ts


@pytest.mark.parametrize("mistake", br.MISTAKES)
def test_planted_mistake_is_caught(planted, mistake):
    case, sigma = planted[mistake]
    t, c, _ = case.tol(0, sigma)
    bt, bc, _ = case.tol(0, sigma, mistake=mistake)
    want = dict(no_inv_t=1001, winner_only=3000, boundary_term=2002, query_norm=3000, drop_farthest=4000, empty_norm=1001)[mistake]
    assert c == want, (c, t)                                         # the case is about the decision it was built for
    assert (bt, bc) != (t, c) and (bc != c or abs(bt - t) > 1e-2 * max(abs(t), abs(bt))), (t, c, bt, bc)
    assert case.tol(0, 0.0, mistake=mistake)[:2] == case.tol(0, 0.0)[:2]     # no mistake shows without a bank error


def test_monte_carlo_agrees_with_the_certain_rows(monte_carlo_case):
    case = monte_carlo_case
    bank, T, topk = case.bank, case.T, case.topk
    thr = KAPPA * EPS_EXACT
    n = len(case.rows)
    certain = [case.tol(i, KAPPA * EPS_B)[0] > thr for i in range(n)]
    certain0 = [case.tol(i, 0.0)[0] > thr for i in range(n)]
    assert all(certain0), certain0                                    # every planted gap is far above the query-only floor
    assert sum(certain) >= 2 and sum(not c for c in certain) >= 4, certain
    bp, bt = bank.proto_emb.astype(np.float64), bank.train_emb.astype(np.float64)
    base = [br.refine64(bp, bt, bank, r["e"], r["cand"], r["L"], topk, T) for r in case.rows]
    for r, b in zip(case.rows, base):
        assert b[0] == r["r"] and b[1] == r["ints"][r["r"], 0] and b[2] == r["ints"][r["r"], 2]    # refine64 is the records' refinement
    rng = rng_of(41)
    changed = np.zeros(n, dtype=int)
    for _ in range(200):
        pp, pt = br.perturb(bp, EPS_B, rng), br.perturb(bt, EPS_B, rng)
        for i, r in enumerate(case.rows):
            changed[i] += br.refine64(pp, pt, bank, r["e"], r["cand"], r["L"], topk, T) != base[i]
    print("changed", changed.tolist(), "certain", certain)
    assert all(changed[i] == 0 for i in range(n) if certain[i]), (changed, certain)
    assert any(changed[i] > 0 for i in range(n) if certain0[i] and not certain[i]), (changed, certain)
