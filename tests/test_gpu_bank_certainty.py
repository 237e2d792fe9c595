"""pg_refine_certainty_bank (csrc/certainty.hip): the refiner's certainty for a bank whose rows carry an error, against the float64
statement tests/_bankref.py, and the layers above it -- hip_ops.refine_certainty(bank_sigma=), HostBank.embedding_rel_tol,
ProtoRefiner(bank_rel_tol=), the deferred engine, `run.py embed --exact` with its sidecar and `run.py evaluate --bank-rel-tol`
(run with -m gpu on an MI355X).

Shapes: B = 1 and 8, P = 1 and 4, cells of 1, 2 and 17 prototypes, an empty cell winning and losing, clusters of 1, 2 and 6 members,
(topk, n_eval, k) in {(1, 1, 1), (2, 4, 6), (5, 9, 12)}, with and without a systematic part beta.

Comparison with the restatement: |got - want| <= 5e-3 |want| + 1e-5, the tolerance tests/test_gpu_certainty.py::
test_refine_certainty_vs_restatement uses for the same quantity; codes are compared where the restated tolerance of the deciding
decision and the smallest one of another code differ by more than that."""
import ctypes
import json
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _bankref as br
from _decisionref import DIM, F32, rng_of

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1, 1), (2, 4, 6), (5, 9, 12)]
CELL_SIZES = (1, 2, 17, 0, 3, 5, 1, 2, 0, 4, 6, 2, 3, 1)          # cells 3 and 8 are empty
EMPTY = (3, 8)
T, MAX_KM = 1.6, 1e9


def close(got, want):
    return (np.isinf(want) and np.isinf(got) and got > 0) or abs(got - want) <= 5e-3 * abs(want) + 1e-5


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops
    _lib.require_gpu()
    return dict(lib=_lib, ops=hip_ops, L=_lib.load())


def small_bank(rng):
    """Gaussian prototypes in cells of CELL_SIZES; cluster sizes cycle 1, 2, 6 (members = prototype + 0.3 N(0, 1))"""
    cell_off = np.concatenate([[0], np.cumsum(CELL_SIZES)]).astype(np.int64)
    n_p = int(cell_off[-1])
    count = np.array([(1, 2, 6)[i % 3] for i in range(n_p)], dtype=np.int32)
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


@pytest.fixture(scope="module")
def world(env):
    """The bank, 8 queries of 4 panels and, per shape, the candidate lists: row 0 near the 17-prototype cell, 1 near the
    one-prototype cell, 2 near the two-prototype cell, 3 with an empty cell inside the set (it loses), 4 with a set of empty cells
    only (nothing can change: code 0), 5 with an empty cell first and no probability on the others (it wins: code -9), 6 and 7 drawn."""
    rng = rng_of(501)
    bank = small_bank(rng)
    C = len(CELL_SIZES)
    full = [c for c in range(C) if c not in EMPTY]
    near = [2, 0, 1, 4, 5, 9, 10, 12]
    q = np.empty((8, 4, DIM), dtype=F32)
    for b, c in enumerate(near):
        row = bank.proto_emb[int(bank.cell_off[c]) + (b % CELL_SIZES[c])]
        q[b] = row[None] + 0.5 * rng.standard_normal((4, DIM)).astype(F32)
    lists = {}
    for topk, n_eval, k in SHAPES:
        cand = np.empty((8, k), dtype=np.int64)
        prob = np.empty((8, k), dtype=F32)
        for b in range(8):
            rest = [c for c in rng.permutation(full) if c != near[b]]
            cand[b] = ([near[b]] + rest)[:k]
            p = np.sort(rng.uniform(0.02, 0.3, k))[::-1]
            prob[b] = p / (1.3 * p.sum())
        if topk > 1:
            cand[3, 1] = EMPTY[0]
        cand[4, :topk] = [EMPTY[i % 2] for i in range(topk)]
        cand[5, 0] = EMPTY[1]
        prob[5, 1:] = 0.0
        lists[(topk, n_eval, k)] = (cand, prob)
    Wt = (rng.standard_normal((C, DIM)) * 0.02).astype(F32)             # (small: the set boundary must not decide every row)
    beta = (3e-4 * rng.standard_normal(DIM) / 32).astype(F32)
    return dict(bank=bank, db=env["ops"].DeviceBank(bank, device=DEV), q=q, lists=lists, W=Wt, beta=beta, C=C)


def run_kernels(env, world, shape, P, B, with_beta, sigmas, bank=None, db=None, q=None, cand=None, prob=None, temperature=T):
    """refine_forward_ex once, then refine_certainty per sigma -> (context for the restatement, {sigma: (tol, code) numpy})"""
    ops = env["ops"]
    topk, n_eval, k = shape
    bank, db = (world["bank"], world["db"]) if bank is None else (bank, db)
    if q is None:
        q = world["q"][:B, :P]
        cand, prob = (a[:B] for a in world["lists"][shape])
    W, C = world["W"], world["C"]
    beta = world["beta"] if with_beta else None
    Wd = torch.from_numpy(W).to(DEV)
    wst = torch.tensor([float(np.linalg.norm(W, axis=1).max()), float(np.abs(W @ beta).max()) if with_beta else 0.0], dtype=torch.float32)
    qd, cd, pd_ = torch.from_numpy(np.ascontiguousarray(q)).to(DEV), torch.from_numpy(cand).to(DEV), torch.from_numpy(prob).to(DEV)
    init = torch.zeros((q.shape[0], 2), dtype=torch.float64, device=DEV)
    _, _, ch, refined, sc = ops.refine_forward_ex(db, qd, init, cd, pd_, topk, n_eval, temperature, MAX_KM)
    out = {}
    for s in sigmas:
        tol, code = ops.refine_certainty(db, qd, cd, pd_, topk, sc, Wd, None if beta is None else torch.from_numpy(beta).to(DEV),
                                         wst.to(DEV), temperature, refined, ch, bank_sigma=s)
        out[s] = (tol.cpu().numpy(), code.cpu().numpy())
    ctx = dict(bank=bank, q=q, cand=cand, prob=prob, sc=sc.cpu(), refined=refined.cpu().numpy(), ch=ch.cpu().numpy(), shape=shape,
               W=W.astype(np.float64), beta=(beta.astype(np.float64) if with_beta else np.zeros(DIM)), wst=wst.double().numpy(), C=C,
               T=temperature, raw=(db, qd, cd, pd_, sc, Wd, wst.to(DEV), refined, ch))
    return ctx, out


def restated(ctx, b, sigma):
    """_bankref.refine_tol_bank of row b on the records the kernel left (as tests/test_gpu_certainty.py feeds its restatement)"""
    topk, n_eval, k = ctx["shape"]
    bank, sc, Tq = ctx["bank"], ctx["sc"], ctx["T"]
    ints = sc[b][:, [5, 6, 9, 10]].contiguous().view(torch.int32).numpy()
    rec = sc[b].double().numpy()
    qm = torch.from_numpy(np.ascontiguousarray(ctx["q"][b])).mean(dim=0).double().numpy()
    prob = ctx["prob"][b]
    with np.errstate(divide="ignore", under="ignore", invalid="ignore"):
        L = np.log(prob[:n_eval]).astype(np.float64)
        r, c = int(ctx["refined"][b]), int(ctx["ch"][b])
        ex = np.exp((sc[b, :topk, 0] / Tq).float().numpy()).astype(np.float32)
        fin_r = float(prob[r]) * float(ex[r] / ex.sum(dtype=np.float32))
        return br.refine_tol_bank(rec, ints, L, ctx["cand"][b], topk, n_eval, ctx["C"], ctx["W"], bank.proto_emb.astype(np.float64),
                                  bank.train_emb.astype(np.float64), qm, ctx["beta"], float(ctx["wst"][0]), float(ctx["wst"][1]), Tq, r, c,
                                  fin_r, cell_off=bank.cell_off, member_off=bank.member_off, member_idx=bank.member_idx, sigma=sigma)


# ------------------------------------------------------------------------------------------------ 1. sigma = 0 is the old entry point
@pytest.mark.parametrize("shape", SHAPES)
def test_sigma_zero_equals_refine_certainty(env, world, shape):
    """pg_refine_certainty_bank(bank_sigma = 0) against pg_refine_certainty: torch.equal on tol and code, every shape"""
    L, lib, ops = env["L"], env["lib"], env["ops"]
    topk, n_eval, k = shape
    seen = set()
    for P in (1, 4):
        for B in (1, 8):
            for with_beta in (False, True):
                ctx, out = run_kernels(env, world, shape, P, B, with_beta, (0.0,))
                db, qd, cd, pd_, sc, Wd, wst, refined, ch = ctx["raw"]
                beta = torch.from_numpy(world["beta"]).to(DEV) if with_beta else None
                tol = torch.full((B,), -7.0, dtype=torch.float32, device=DEV)
                code = torch.full((B,), -77, dtype=torch.int32, device=DEV)
                lib.check(L.pg_refine_certainty_bank(ctypes.byref(db.struct), ops._p(qd), B, P, ops._p(cd), ops._p(pd_), k, topk, n_eval,
                                                     ops._p(sc), ops._p(Wd), Wd.shape[0], ops._p(beta), ops._p(wst), T, ops._p(refined),
                                                     ops._p(ch), ops._p(tol), ops._p(code), 0.0, ops._stream()), "pg_refine_certainty_bank")
                old_t, old_c = out[0.0]
                assert torch.equal(tol.cpu(), torch.from_numpy(old_t)) and torch.equal(code.cpu(), torch.from_numpy(old_c)), (P, B, with_beta)
                seen |= set((old_c // 1000).tolist()) | set(old_c[old_c <= 0].tolist())
    if topk > 1:
        assert {1, 3, 4} & seen and 0 in seen and -9 in seen, seen      # pairs / picks decide rows; the all-empty set; the empty winner


# ------------------------------------------------------------------------------------------------ 2. against the restatement
# Bk far below every margin of this bank, of the size of its tightest ones (the member near-ties), of the size of the prototype and
# score margins (the member decisions are then 0), above all of them
SIGMAS = (1e-5, 3e-3, 4.0, 400.0)


@pytest.mark.parametrize("with_beta", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_against_restatement_three_regimes(env, world, shape, with_beta):
    regimes = {s: set() for s in SIGMAS}
    for P in (1, 4):
        ctx, out = run_kernels(env, world, shape, P, 8, with_beta, (0.0,) + SIGMAS)
        for b in range(8):
            t0 = restated(ctx, b, 0.0)[0]
            for s in SIGMAS:
                want, wcode, rival = restated(ctx, b, s)
                got, gcode = float(out[s][0][b]), int(out[s][1][b])
                print(f"shape {shape} P {P} row {b} sigma {s:g}: tol {got!r} restated {want!r} code {gcode} / {wcode} (sigma 0: {t0!r})")
                assert close(got, want), (P, b, s, got, want, gcode, wcode)
                if not close(rival, want) and not close(want, rival):
                    assert gcode == wcode, (P, b, s, gcode, wcode, got, want, rival)
                if np.isfinite(t0) and t0 > 0:
                    regimes[s].add("same" if want >= 0.999 * t0 else ("zero" if want == 0 else "less"))
    if shape[0] > 1:                                                # (topk = 1 = n_eval: no decision at all)
        assert regimes[SIGMAS[0]] == {"same"}, regimes
        assert "less" in regimes[SIGMAS[1]], regimes
        assert "zero" in regimes[SIGMAS[3]], regimes


# ------------------------------------------------------------------------------------------------ 3. the sharp threshold
def _axis_row(q, col, dist):
    row = q.copy()
    row[col] += dist
    return row


def _threshold_case(kind, rng):
    """Integer rows: every distance is exact in fp32.  -> (bank, cand, prob, topk, T, margin m, bsum, |g|, code)"""
    q = rng.integers(-8, 9, DIM).astype(F32)
    ll = np.zeros((4, 2), F32)
    if kind == "proto":                                             # one cell, two single-member prototypes at 3 and 5
        rows = np.stack([_axis_row(q, 10, 3.0), _axis_row(q, 500, -5.0)])
        bank = SimpleNamespace(proto_emb=rows, cell_off=np.array([0, 2], np.int64), proto_lnglat=ll[:2], proto_count=np.ones(2, np.int32),
                               member_off=np.array([0, 1, 2], np.int64), member_idx=np.array([0, 1], np.int64), train_emb=rows.copy(),
                               train_lnglat=ll[:2])
        return q, bank, np.array([[0]]), np.array([[1.0]], F32), 1, 1.6, 2.0, float((rows.astype(np.float64) ** 2).sum()), np.sqrt(2.0), 3000
    if kind == "member":                                            # one prototype at 3 whose two members sit at 7 and 4
        proto = _axis_row(q, 10, 3.0)[None]
        train = np.stack([_axis_row(q, 77, 7.0), _axis_row(q, 900, -4.0)])
        bank = SimpleNamespace(proto_emb=proto, cell_off=np.array([0, 1], np.int64), proto_lnglat=ll[:1], proto_count=np.array([2], np.int32),
                               member_off=np.array([0, 2], np.int64), member_idx=np.array([1, 0], np.int64), train_emb=train, train_lnglat=ll[:2])
        return q, bank, np.array([[0]]), np.array([[1.0]], F32), 1, 1.6, 3.0, float((train.astype(np.float64) ** 2).sum()), np.sqrt(2.0), 4000
    # two cells of one single-member prototype at 3 and 5, equal probabilities (log 1 = 0: the scores are -3 / T and -5 / T), T = 2
    rows = np.stack([_axis_row(q, 10, 3.0), _axis_row(q, 500, -5.0)])
    bank = SimpleNamespace(proto_emb=rows, cell_off=np.array([0, 1, 2], np.int64), proto_lnglat=ll[:2], proto_count=np.ones(2, np.int32),
                           member_off=np.array([0, 1, 2], np.int64), member_idx=np.array([0, 1], np.int64), train_emb=rows.copy(),
                           train_lnglat=ll[:2])
    return q, bank, np.array([[0, 1]]), np.array([[1.0, 1.0]], F32), 2, 2.0, 1.0, float((rows.astype(np.float64) ** 2).sum()) / 4.0, np.sqrt(2.0) / 2.0, 1001


@pytest.mark.parametrize("kind", ["proto", "member", "score"])
def test_sharp_threshold_on_integer_rows(env, world, kind):
    """One decision, exact distances: just below sigma* = 32 m / sqrt(bsum) the tolerance is the formula's, just above it is 0 with
    the decision's code.  `score`: m = (5 - 3) / T and bsum = (|p1|^2 + |p2|^2) / T^2 -- without the 1 / T the threshold would sit at
    sigma* / T and the value below sigma* would be 0."""
    q, bank, cand, prob, topk, Tq, m, bsum, gnorm, code = _threshold_case(kind, rng_of(77))
    db = env["ops"].DeviceBank(bank, device=DEV)
    star = 32.0 * m / np.sqrt(bsum)
    below, above = float(F32(star * (1 - 1e-3))), float(F32(star * (1 + 1e-3)))
    w = dict(world, W=np.zeros((len(bank.cell_off) - 1, DIM), F32), C=len(bank.cell_off) - 1)     # equal head rows: the scores move through the distances only
    ctx, out = run_kernels(env, w, (topk, topk, topk), 1, 1, False, (0.0, below, above, star / Tq * 1.01), bank=bank, db=db, q=q[None, None],
                           cand=cand.astype(np.int64), prob=prob, temperature=Tq)
    en = float(np.linalg.norm(q.astype(np.float64)))
    A = en * gnorm / 32.0
    bk = below * np.sqrt(bsum) / 32.0
    want = np.sqrt((m - bk) * (m + bk)) / A
    t0, c0 = out[0.0]
    assert close(float(t0[0]), m / A) and int(c0[0]) == code, (t0, c0, m / A)
    tb, cb = out[below]
    print(f"{kind}: sigma* {star!r}; below: tol {float(tb[0])!r} formula {want!r}; above: {out[above]}")
    assert np.isfinite(tb[0]) and tb[0] > 0 and close(float(tb[0]), want) and int(cb[0]) == code, (tb, cb, want)
    ta, ca = out[above]
    assert float(ta[0]) == 0.0 and int(ca[0]) == code, (ta, ca)
    tm, _ = out[star / Tq * 1.01]                                    # (T != 1: where a weight of 1 instead of 1 / T would already give 0)
    assert tm[0] > 0
    assert restated(ctx, 0, below)[1] == code and close(float(tb[0]), restated(ctx, 0, below)[0])


# ------------------------------------------------------------------------------------------------ 4. monotone in sigma
@pytest.mark.parametrize("shape", SHAPES + [(1, 3, 4)])
def test_tolerance_never_grows_with_sigma(env, world, shape):
    """(1, 3, 4): a set of one candidate with candidates beyond it -- row 1 sits in a cell of one single-member prototype, so its only
    decisions are set-boundary ones, which no bank error moves"""
    if shape not in world["lists"]:
        cand, prob = world["lists"][(2, 4, 6)]
        world["lists"][shape] = (np.ascontiguousarray(cand[:, :4]), np.ascontiguousarray(prob[:, :4]))
    sig = (0.0, 1e-3, 0.1, 4.0, 400.0)
    for with_beta in (False, True):
        ctx, out = run_kernels(env, world, shape, 4, 8, with_beta, sig)
        tols = np.stack([out[s][0] for s in sig])
        codes = np.stack([out[s][1] for s in sig])
        assert (tols[:-1] >= tols[1:]).all(), tols
        t0, c0 = out[0.0]
        if shape == (1, 3, 4):
            assert c0[1] >= 2000 and np.isfinite(t0[1]), (c0, t0)
        boundary_only = np.array([all(c in (0, 2999) or 2000 <= c < 2999 for _, c in _decision_list(ctx, b)) and ctx["refined"][b] == shape[0] - 1
                                  for b in range(8)])
        assert (tols[:, boundary_only] == tols[0, boundary_only]).all() and (codes[:, boundary_only] == codes[0, boundary_only]).all()
        assert (tols[:, c0 == 0] == tols[0, c0 == 0]).all()
        moved = (tols[-1] < tols[0])
        assert moved.any() or shape == (1, 1, 1)


def _decision_list(ctx, b):
    topk, n_eval, k = ctx["shape"]
    bank, sc = ctx["bank"], ctx["sc"]
    ints = sc[b][:, [5, 6, 9, 10]].contiguous().view(torch.int32).numpy()
    prob = ctx["prob"][b]
    with np.errstate(divide="ignore", under="ignore", invalid="ignore"):
        L = np.log(prob[:n_eval]).astype(np.float64)
        r, c = int(ctx["refined"][b]), int(ctx["ch"][b])
        ex = np.exp((sc[b, :topk, 0] / ctx["T"]).float().numpy()).astype(np.float32)
        fin_r = float(prob[r]) * float(ex[r] / ex.sum(dtype=np.float32))
        qm = torch.from_numpy(np.ascontiguousarray(ctx["q"][b])).mean(dim=0).double().numpy()
        return br.decisions(sc[b].double().numpy(), ints, L, ctx["cand"][b], topk, n_eval, ctx["C"], ctx["W"], bank.proto_emb.astype(np.float64),
                            bank.train_emb.astype(np.float64), qm, ctx["beta"], float(ctx["wst"][0]), float(ctx["wst"][1]), ctx["T"], r, c, fin_r,
                            bank.cell_off, bank.member_off, bank.member_idx, 0.0)


# ------------------------------------------------------------------------------------------------ 5. refusals, the host fields
def test_refusals_and_the_bank_field(env, world, tmp_path):
    from pigeon_amd.evaluate import _resolve_bank_rel_tol
    from pigeon_amd.proto_refiner import HostBank, ProtoRefiner
    L, lib, ops = env["L"], env["lib"], env["ops"]
    ctx, _ = run_kernels(env, world, (2, 4, 6), 4, 8, False, (0.0,))
    db, qd, cd, pd_, sc, Wd, wst, refined, ch = ctx["raw"]
    for bad in (-1.0, float("nan"), -1e-30):
        with pytest.raises(lib.PigeonHipError, match="bank_sigma"):
            ops.refine_certainty(db, qd, cd, pd_, 2, sc, Wd, None, wst, T, refined, ch, bank_sigma=bad)
        tol = torch.zeros((8,), dtype=torch.float32, device=DEV)
        code = torch.zeros((8,), dtype=torch.int32, device=DEV)
        rc = L.pg_refine_certainty_bank(ctypes.byref(db.struct), ops._p(qd), 8, 4, ops._p(cd), ops._p(pd_), 6, 2, 4, ops._p(sc), ops._p(Wd),
                                        Wd.shape[0], None, ops._p(wst), T, ops._p(refined), ops._p(ch), ops._p(tol), ops._p(code), bad,
                                        ops._stream())
        assert rc == -1 and b"bank_sigma" in L.pg_last_error()       # PG_EINVAL, by name
    bank = world["bank"]
    for bad in (-1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="bank_rel_tol"):
            ProtoRefiner(topk=2, bank=bank, device=DEV, bank_rel_tol=bad)
    fields = {f: getattr(bank, f) for f in HostBank.FIELDS}
    assert ProtoRefiner(topk=2, bank=bank, device=DEV).bank_rel_tol == 0.0
    hb = HostBank(embedding_rel_tol=2.5e-4, **fields)
    assert ProtoRefiner(topk=2, bank=hb, device=DEV).bank_rel_tol == 2.5e-4                 # the bank's own declaration
    assert ProtoRefiner(topk=2, bank=hb, device=DEV, bank_rel_tol=0.0).bank_rel_tol == 0.0  # an explicit number wins
    assert ProtoRefiner(topk=2, bank=hb, device=DEV, bank_rel_tol=1e-3).bank_rel_tol == 1e-3
    new, old = os.path.join(str(tmp_path), "new.npz"), os.path.join(str(tmp_path), "old.npz")
    hb.save(new)
    back = HostBank.load(new)
    assert back.embedding_rel_tol == 2.5e-4 and all(np.array_equal(getattr(back, f), fields[f]) for f in HostBank.FIELDS)
    np.savez(old, **fields)                                          # a file from before the field
    assert HostBank.load(old).embedding_rel_tol is None
    HostBank(**fields).save(new)
    assert HostBank.load(new).embedding_rel_tol is None and "embedding_rel_tol" not in np.load(new).files
    with pytest.raises(ValueError):
        HostBank(embedding_rel_tol=-1e-4, **fields)
    with pytest.raises(ValueError, match="kappa"):                  # a bank error without the z-score it is scaled by
        r = ProtoRefiner(topk=2, bank=hb, device=DEV)
        r.forward_certain(qd, torch.zeros((8, 2), device=DEV), cd, pd_, Wd, wst)
    assert _resolve_bank_rel_tol(None, None) is None and _resolve_bank_rel_tol("3e-4", None) == 3e-4 and _resolve_bank_rel_tol(1e-3, None) == 1e-3


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_end_to_end_small_tower(env, tmp_path):
    """A 2-layer tower and a 36-cell bank through certain_forward and evaluate_model.  Two rows get a second prototype planted half
    of the bank's threshold behind the nearest one: certain with an exact bank (after the exact tier), not certain at 3e-4."""
    from pigeon_amd import synthetic as syn
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    from pigeon_amd.evaluate import certain_forward, evaluate_model
    from pigeon_amd.proto_refiner import ProtoRefiner
    from pigeon_amd.super_guessr import SuperGuessr
    C, N, TOL = 36, 6, 3e-4
    gp = os.path.join(str(tmp_path), "g.csv")
    syn.write_geocell_csv(gp, syn.make_geocells(C, seed=0))
    vit = HipCLIPVisionModel(syn.make_vit_weights(seed=11, layers=2, affine_jitter=True), layers=2).to(DEV)
    W, b = syn.make_head_weights(C, seed=1)
    px = syn.make_pixels(4 * N, seed=3, panorama=True).to(DEV)
    model = SuperGuessr(vit, panorama=True, freeze_base=True, num_candidates=5, geocell_path=gp, exact_top1=True, margin_autocalibrate=False)
    with torch.no_grad():
        model.cell_layer.weight.copy_(W * 64); model.cell_layer.bias.copy_(b)
    model = model.to(DEV).eval()
    kappa = model.certainty.kappa
    exact = vit._encoder(torch.device(DEV)).forward_precise(px.reshape(-1, 3, 336, 336)).reshape(N, 4, 1024).mean(dim=1).double().cpu().numpy()
    hb = syn.make_bank(C, 9, seed=5, empty_frac=0.0, max_members=6, center=exact.mean(axis=0).astype(F32), radius=float(np.linalg.norm(exact.std(axis=0))))
    hb.proto_emb = hb.proto_emb.copy()
    probe = ProtoRefiner(topk=5, max_refinement=1e9, temperature=1.6, bank=hb, device=DEV).eval()
    _, info = certain_forward(model, probe, pixel_values=px)
    rng, planted, cells = rng_of(61), [], set()
    for i in np.flatnonzero(info["certain"].cpu().numpy()):          # rows that are certain before anything is planted
        c = int(info["refined_geocell"][i])
        if c in cells or len(planted) == 2:
            continue
        lo, hi = int(hb.cell_off[c]), int(hb.cell_off[c + 1])
        d = np.linalg.norm(hb.proto_emb[lo:hi].astype(np.float64) - exact[i], axis=1)
        p1 = lo + int(np.argmin(d))
        other = next(p for p in range(lo, hi) if p != p1)
        g = rng.standard_normal(DIM)
        bk = kappa * TOL * np.sqrt(2.0) * np.linalg.norm(hb.proto_emb[p1].astype(np.float64)) / 32.0
        hb.proto_emb[other] = (exact[i] + (d.min() + 0.5 * bk) * g / np.linalg.norm(g)).astype(F32)
        planted.append(int(i)); cells.add(c)
    assert len(planted) == 2, info["certain"]
    r0 = ProtoRefiner(topk=5, max_refinement=1e9, temperature=1.6, bank=hb, device=DEV).eval()
    rb = ProtoRefiner(topk=5, max_refinement=1e9, temperature=1.6, bank=hb, device=DEV, bank_rel_tol=TOL).eval()
    assert r0.bank_rel_tol == 0.0 and rb.bank_rel_tol == TOL
    thr_x = model.certainty.threshold(True)

    def compare(c0, cb, same, cause, rtol, rcode):
        """c0 / cb: certain with the exact bank / at TOL; same(mask): outputs equal on the masked rows"""
        assert not (cb & ~c0).any()                                  # a subset
        same(c0 & cb)
        differ = np.flatnonzero(c0 & ~cb)
        assert set(planted) <= set(differ.tolist()), (planted, differ)
        # what keeps them uncertain is a decision of the refiner; `cause` (why a row left the FAST pass) names it too unless the head
        # had already sent the row to the exact tier (cause 1 comes first, include/pigeon_hip.h)
        assert (rtol[differ] <= thr_x).all() and ((rcode[differ] >= 1000) | (rcode[differ] == -9)).all(), (rtol, rcode)
        assert ((cause[differ] >= 1000) | (cause[differ] == -9) | (cause[differ] == 1)).all(), cause
        assert (rtol[planted] == 0).all() and (rcode[planted] // 1000 == 3).all()
        return differ

    out0, i0 = certain_forward(model, r0, pixel_values=px)
    outb, ib = certain_forward(model, rb, pixel_values=px)
    c0, cb = i0["certain"].cpu().numpy(), ib["certain"].cpu().numpy()
    print(f"certain at 0: {c0.tolist()}; at {TOL:g}: {cb.tolist()}; causes {ib['cause'].tolist()}; refine tol {ib['refine_tol'].tolist()} "
          f"(at 0: {i0['refine_tol'].tolist()}); reencoded {ib['reencoded'].tolist()}")

    def same_forward(mask):
        both = torch.from_numpy(mask).to(DEV)
        for k in ("refined_LLH", "refined_geocell"):
            assert torch.equal(i0[k][both], ib[k][both])
        assert torch.equal(out0.preds_geocell[both], outb.preds_geocell[both])
    differ = compare(c0, cb, same_forward, ib["cause"].cpu().numpy(), ib["refine_tol"].cpu().numpy(), ib["refine_code"].cpu().numpy())
    assert set(differ.tolist()) <= set(ib["reencoded"].tolist())     # re-encoded once, and still uncertain
    assert model.engine(rb).check_nothing_dropped() == 0

    class Panoramas(torch.utils.data.Dataset):
        def __len__(self):
            return N

        def __getitem__(self, i):
            return {"pixel_values": px[i].cpu(), "labels": torch.zeros(2, dtype=torch.float64), "labels_clf": torch.tensor(0)}
    res0 = evaluate_model(model, Panoramas(), None, None, r0, batch_size=4)
    resb = evaluate_model(model, Panoramas(), None, None, rb, batch_size=4)       # (raises if the queue dropped a row)
    g0, gb = res0["geocell_certain"], resb["geocell_certain"]
    print(f"evaluate_model: certain at 0 {g0.tolist()}, at {TOL:g} {gb.tolist()}, exact passes {[f['slots_run'] for f in resb['exact_passes']]}")
    assert not (gb & ~g0).any() and set(planted) <= set(np.flatnonzero(g0 & ~gb).tolist())
    assert resb["uncertain_after_exact"] == int((~gb).sum()) >= len(planted) and res0["uncertain_after_exact"] == int((~g0).sum())
    assert sum(f["slots_run"] for f in resb["exact_passes"]) >= int((g0 & ~gb).sum())
    assert np.array_equal(res0["preds"][g0 & gb], resb["preds"][g0 & gb]) and np.array_equal(res0["preds_geocells"][g0 & gb], resb["preds_geocells"][g0 & gb])


# ------------------------------------------------------------------------------------------------ 7. run.py
def _main(monkeypatch, args):
    import importlib
    monkeypatch.setattr(sys, "argv", ["run.py"] + args)
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import run as run_py
    importlib.reload(run_py)
    return run_py.main()


def test_run_py_embed_exact_and_the_sidecar(env, monkeypatch, tmp_path):
    from pigeon_amd.certainty import CalibrationError, Certainty
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    monkeypatch.delenv("PIGEON_PIXEL_BYTES", raising=False)
    dirs = {flag: os.path.join(str(tmp_path), "emb_" + (flag.strip("-") or "fast")) for flag in ("--exact", "")}
    for flag, d in dirs.items():
        _main(monkeypatch, ["embed", "random", "--synthetic", "8", "--layers", "2", "--yfcc", "--out-dir", d] + ([flag] if flag else []))
    meta = {flag: json.load(open(os.path.join(d, "embedding_meta.json"))) for flag, d in dirs.items()}
    rows = np.load(os.path.join(dirs["--exact"], "train.npy")).reshape(-1, 1024)
    px = torch.stack([torch.randn((3, 336, 336), generator=torch.Generator().manual_seed(1234 + i)) for i in range(8)])
    vit = HipCLIPVisionModel(seed=0, layers=2).to(DEV)
    want = vit.embed_precise(px.to(DEV))
    assert np.load(os.path.join(dirs["--exact"], "train_indices.npy")).reshape(-1).tolist() == list(range(8))
    assert torch.equal(torch.from_numpy(rows), want.cpu())          # bit for bit
    ex, fa = meta["--exact"], meta[""]
    assert ex["encoder"] == "exact" and ex["embedding_rel_tol"] == Certainty().rel_tol_exact and ex["debias"] is False
    assert fa["encoder"] == "fast" and fa["embedding_rel_tol"] > ex["embedding_rel_tol"] and fa["embedding_rel_tol"] <= 1e-3
    for m in (ex, fa):
        assert m["fingerprint"] == vit.fingerprint() and m["mma_dtype"] in ("f16", "bf16") and isinstance(m["debias"], bool)
    assert not np.array_equal(np.load(os.path.join(dirs[""], "train.npy")).reshape(-1, 1024), rows)
    # a sidecar written with other weights (the 2-layer tower's, handed to a 3-layer one) ends `evaluate` with both fingerprints named
    side = os.path.join(dirs["--exact"], "embedding_meta.json")
    with pytest.raises(CalibrationError) as why:
        _main(monkeypatch, ["evaluate", "none", "--synthetic", "4", "--layers", "3", "--geocells", "300", "--bank-rel-tol", side])
    assert ex["fingerprint"] in str(why.value) and "this encoder" in str(why.value)
