"""The decision tier (run with -m gpu on an MI355X): every element the kernels that turn an embedding into the discrete outputs write
-- pg_head_forward, pg_head_margin, pg_refine_forward, pg_refine_forward_ex, pg_head_certainty, pg_refine_certainty -- against the
statements of tests/_decisionref.py, at the shapes where the kernels' loops change form (the 64 x 64 logit tiles, the 256-wide row
passes, C = 38400 / 38401 where the probabilities move from LDS to device scratch, the 4-wave / 2-row walk over a cell's prototypes,
the 64-lane selection blocks) and on the input families where a selection goes wrong: exact ties, underflow, masked cells, NaN.
tests/test_decisionref_cpu.py pins those statements and shows that each comparison rejects the mistakes it is for.

The kernels are called through the C ABI with every output placed in front of sentinel elements, which must stay untouched; no input
may change.  No input is outside a kernel's contract.

Top-k rule (topk_check): the kernel's list is compared with the order (logit desc, index asc).  A differing position is allowed only
where the two logits differ by at most 8 u (1 + |l - max|) and the reported values are equal or correctly ordered; the tie families
allow none, the others fewer than 1 % of the listed positions.  Independently: values descend, indices are distinct and in range,
argmax is the head of the list, pred_llh is the centroid row bit for bit, and no unlisted cell beats the last listed one by more
than the same slack."""
import ctypes
import time

import numpy as np
import pytest
import torch

import _decisionref as D

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32 = np.float32
T0 = time.time()
SENT_I = -77


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops
    _lib.require_gpu()
    return dict(lib=_lib, ops=hip_ops, L=_lib.load())


def guarded(n, dtype=torch.float32):
    return torch.full((n + D.GUARD,), D.SENTINEL if dtype.is_floating_point else SENT_I, dtype=dtype, device=DEV)


def take(buf, n, what):
    """the n output elements of a guarded buffer (numpy); the sentinels behind them untouched"""
    torch.cuda.synchronize()
    assert bool((buf[n:] == (D.SENTINEL if buf.dtype.is_floating_point else SENT_I)).all()), f"{what}: wrote past its output"
    return buf[:n].cpu().numpy()


def dev(a):
    return a if torch.is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.int32)


def unchanged(pairs, what):
    for t, keep in pairs:
        assert torch.equal(t.view(torch.int32), keep.view(torch.int32)), f"{what}: an input changed"


def show(capsys, text):
    with capsys.disabled():
        print("\n" + text)


# ================================================================================================================ raw calls
def raw_head(env, emb, W, bias, cent, k):
    """emb (B,P,1024), W (C,1024), bias (C,) fp32, cent (C,2) fp64 (numpy or device tensors) -> dict of numpy outputs"""
    ops = env["ops"]
    ins = [dev(emb), dev(W), dev(bias), dev(cent)]
    keep = [t.clone() for t in ins]
    B, P, C = ins[0].shape[0], ins[0].shape[1], ins[1].shape[0]
    lg, tv, ti, am, llh = guarded(B * C), guarded(B * k), guarded(B * k, torch.int64), guarded(B, torch.int64), guarded(2 * B, torch.float64)
    env["lib"].check(env["L"].pg_head_forward(ops._p(ins[0]), B, P, ops._p(ins[1]), ops._p(ins[2]), ops._p(ins[3]), C, k, ops._p(lg),
                                              ops._p(tv), ops._p(ti), ops._p(am), ops._p(llh), ops._stream()), "pg_head_forward")
    what = f"head_forward B={B} C={C} k={k}"
    out = dict(logits=take(lg, B * C, what).reshape(B, C), val=take(tv, B * k, what).reshape(B, k), idx=take(ti, B * k, what).reshape(B, k),
               argmax=take(am, B, what), llh=take(llh, 2 * B, what).reshape(B, 2), logits_dev=lg[:B * C].view(B, C))
    unchanged(zip(ins, keep), what)
    return out


def raw_refine(env, db, q, init, cand, prob, topk, n_eval, T, max_km, ext=True):
    """-> dict(scratch (B,n,SC), llh (B,2), cell, choice, refined) numpy + the device scratch / refined / choice for the certainty call"""
    ops = env["ops"]
    ins = [dev(q), dev(init), dev(cand)] + ([dev(prob)] if prob is not None else [])
    keep = [t.clone() for t in ins]
    B, P, k = ins[0].shape[0], ins[0].shape[1], ins[2].shape[1]
    n, SC = (n_eval, 12) if ext else (topk, 4)
    sc, llh, cell, ch, rf = guarded(B * n * SC), guarded(2 * B), guarded(B, torch.int64), guarded(B, torch.int32), guarded(B, torch.int32)
    pp = ops._p(ins[3]) if prob is not None else ops._p(None)
    if ext:
        rc = env["L"].pg_refine_forward_ex(ctypes.byref(db.struct), ops._p(ins[0]), B, P, ops._p(ins[1]), ops._p(ins[2]), pp, k, topk, n_eval,
                                           float(T), float(max_km), ops._p(sc), ops._p(llh), ops._p(cell), ops._p(ch), ops._p(rf), ops._stream())
    else:
        rc = env["L"].pg_refine_forward(ctypes.byref(db.struct), ops._p(ins[0]), B, P, ops._p(ins[1]), ops._p(ins[2]), pp, k, topk,
                                        float(T), float(max_km), ops._p(sc), ops._p(llh), ops._p(cell), ops._p(ch), ops._stream())
    what = f"refine_forward{'_ex' if ext else ''} B={B} topk={topk} n_eval={n_eval} k={k}"
    env["lib"].check(rc, what)
    out = dict(scratch=take(sc, B * n * SC, what).reshape(B, n, SC), llh=take(llh, 2 * B, what).reshape(B, 2), cell=take(cell, B, what),
               choice=take(ch, B, what), refined=take(rf, B if ext else 0, what), scratch_dev=sc[:B * n * SC].view(B, n, SC),
               refined_dev=rf[:B], choice_dev=ch[:B], q_dev=ins[0], cand_dev=ins[2], prob_dev=ins[3] if prob is not None else None)
    if not ext:
        assert bool((rf == SENT_I).all())
    unchanged(zip(ins, keep), what)
    return out


# ================================================================================================================ logits
LOGIT_B = (1, 63, 64, 65, 130)
LOGIT_C = (1, 63, 64, 65, 129, 1031)


@pytest.mark.parametrize("P", [1, 2, 3, 4, 5])
def test_logits_per_element(env, P, capsys):
    """pg_head_forward's logits, B in 1, 63 .. 65, 130 x C in 1, 63 .. 65, 129, 1031: the Gaussian family within (1024 + P + 2) u S + u |t|
    of the fp64 truth at every element, the integer family equal to it bit for bit; row 64 of B = 65 has the bits of the same row run
    alone."""
    worst, found = 0.0, []
    for bi, B in enumerate(LOGIT_B):
        for ci, C in enumerate(LOGIT_C):
            cent = D.rng_of(20).uniform(-90, 90, (C, 2))
            emb, W, bias = D.gaussian_logits_case(D.rng_of(21, P, bi, ci), B, C, P)
            got = raw_head(env, emb, W, bias, cent, 1)["logits"]
            t, S = D.head_logits_truth(emb, W, bias)
            r = np.abs(got - t) / D.logits_bound(t, S, P)
            worst = max(worst, float(r.max()))
            if not r.max() <= 1:
                i, j = np.unravel_index(int(np.nanargmax(r)), r.shape)
                found.append(f"gauss B={B} C={C} P={P} element ({i},{j}): {r.max():.3g} of the bound")
            if B == 65:
                alone = raw_head(env, emb[64:], W, bias, cent, 1)["logits"]
                if not np.array_equal(bits(alone[0]), bits(got[64])):
                    found.append(f"gauss B=65 C={C} P={P}: row 64 differs from the same row run alone")
            emb, W, bias = D.integer_logits_case(D.rng_of(22, P, bi, ci), B, C, P)
            got = raw_head(env, emb, W, bias, cent, 1)["logits"]
            want = D.head_logits_truth(emb, W, bias)[0].astype(F32)
            if not np.array_equal(bits(got), bits(want)):
                i, j = np.argwhere(got != want)[0]
                found.append(f"integer B={B} C={C} P={P}: {int((got != want).sum())} elements differ, the first ({i},{j}) {got[i, j]!r} for {want[i, j]!r}")
    show(capsys, f"pg_head_forward logits P={P}: Gaussian family worst {worst:.3g} of the bound; integer family bit-equal: {not found}")
    assert not found, "\n".join(found)


# ================================================================================================================ softmax, top-k
SOFTMAX_C = (1, 2, 255, 256, 257, 1031, 38400, 38401)


@pytest.mark.parametrize("C", SOFTMAX_C)
def test_softmax_topk_controlled(env, C, capsys):
    """Controlled logits (emb[b,0,b] = 1: logits[b,c] = W[c,b] + bias[c], decided to the bit) of every family, unmasked with a NaN row,
    with bias = -inf on a third of the cells, with one +inf cell and with one NaN cell (all probabilities NaN: list 0 .. k-1);
    k = 1, min(C, 50) and, for C <= 1031, C.  Listed probabilities within the softmax bound; lists through topk_check."""
    fams = D.LOGIT_FAMILIES
    nb = len(fams) + 1
    cent = D.rng_of(30).uniform(-90, 90, (C, 2))
    cent_d = dev(cent)
    W = torch.zeros((C, 1024), dtype=torch.float32, device=DEV)
    worst, exc, listed, found = dict.fromkeys(fams, 0.0), dict.fromkeys(fams, 0), dict.fromkeys(fams, 0), []
    for mi, mask in enumerate((None, "neginf", "posinf", "nan")):
        L, bias = D.controlled_case(C, D.rng_of(31, SOFTMAX_C.index(C), mi), mask)
        emb = np.zeros((nb, 1, 1024), dtype=F32)
        emb[np.arange(nb), 0, np.arange(nb)] = 1
        rows = [(t, L[i] + bias) for i, t in enumerate(fams)]
        W[:, :nb] = 0
        W[:, :len(fams)] = dev(np.ascontiguousarray(L.T))
        if mask is None:
            emb[nb - 1, 0, nb - 1] = np.nan                          # a NaN row: W[:, nb - 1] is 0, NaN * 0 = NaN in every cell
            rows.append(("nanrow", np.full(C, np.nan, dtype=F32)))
        for k in sorted({1, min(C, 50)} | ({C} if C <= 1031 else set())):
            o = raw_head(env, emb, W, bias, cent_d, k)
            for b, (tag, l32) in enumerate(rows):
                if not np.array_equal(o["logits"][b], l32, equal_nan=True):
                    found.append(f"C={C} mask={mask} {tag}: the logits are not W[c,b] + bias[c]")
                    continue
                try:
                    e = D.topk_check(l32, k, o["val"][b], o["idx"][b], int(o["argmax"][b]), o["llh"][b], cent)
                except AssertionError as err:
                    found.append(f"C={C} mask={mask} k={k} {tag}: {err}")
                    continue
                if tag == "nanrow" or D.all_nan_row(l32):
                    continue
                exc[tag] += len(e); listed[tag] += k
                p = D.softmax_truth(l32)
                idx = o["idx"][b]
                r = np.abs(o["val"][b] - p[idx]) / D.softmax_bound(l32, p)[idx]
                worst[tag] = max(worst[tag], float(r.max()))
                if not r.max() <= 1:
                    found.append(f"C={C} mask={mask} k={k} {tag}: probability of cell {idx[int(np.argmax(r))]} at {r.max():.3g} of the bound")
    show(capsys, f"head_row_kernel C={C}, worst of the softmax bound per family: " + ", ".join(f"{t} {v:.3g}" for t, v in worst.items())
         + "; top-k exceptions: " + ", ".join(f"{t} {exc[t]}/{listed[t]}" for t in fams))
    assert not found, "\n".join(found[:20])
    for t in fams:
        assert exc[t] == 0 if t in D.TIE_FAMILIES else exc[t] < 0.01 * listed[t], (t, exc[t], listed[t])


@pytest.mark.parametrize("C", [1, 2, 257, 1031])
def test_head_margin(env, C, capsys):
    """pg_head_margin on logits of every family: margin = l[top1] - l[top2] bit for bit with (value desc, index asc) for both; with
    ties the margin is exactly 0 and top2 the next tied index; C = 1: +inf and top2 = top1."""
    ops, rng = env["ops"], D.rng_of(40, C)
    L = np.stack([D.logit_rows(t, C, rng) for t in D.LOGIT_FAMILIES])
    B, P = L.shape[0], 2
    ins = [dev(L), dev(rng.standard_normal((B, P, 1024)).astype(F32)), dev(rng.standard_normal((C, 1024)).astype(F32))]
    keep = [t.clone() for t in ins]
    mg, sn, t2 = guarded(B), guarded(B), guarded(B, torch.int64)
    env["lib"].check(env["L"].pg_head_margin(ops._p(ins[0]), B, C, ops._p(ins[1]), P, ops._p(ins[2]), ops._p(mg), ops._p(sn), ops._p(t2),
                                             ops._stream()), "pg_head_margin")
    mg, sn, t2 = take(mg, B, "head_margin"), take(sn, B, "head_margin"), take(t2, B, "head_margin")
    unchanged(zip(ins, keep), "head_margin")
    zero = 0
    for b, tag in enumerate(D.LOGIT_FAMILIES):
        if C == 1:
            assert np.isposinf(mg[b]) and t2[b] == 0 and sn[b] == 0, tag
            continue
        a, c = D._rank(L[b], 2)
        assert t2[b] == c and np.array_equal(bits(mg[b]), bits(L[b, a] - L[b, c])), (tag, mg[b], t2[b], a, c)
        if L[b, c] == L[b, a]:
            assert mg[b] == 0 and c > a, tag
            zero += 1
        assert tag not in ("equal", "ties") or L[b, c] == L[b, a]
    assert zero >= (2 if C > 1 else 0)


# ================================================================================================================ candidate records
@pytest.fixture(scope="module")
def ibank(env):
    bank, q, tags = D.integer_bank(D.rng_of(3))
    recs = [D.candidate_record(bank, q, c) for c in range(len(tags))]
    return dict(bank=bank, q=q, tags=np.array(tags), rec12=np.stack([r[1] for r in recs]), rec4={c: r[0] for c, r in enumerate(recs)},
                db=env["ops"].DeviceBank(bank, device=DEV))


@pytest.mark.parametrize("P", [1, 3, 4])
def test_candidate_records_integer_bank(env, ibank, P, capsys):
    """every cell of the integer bank, 64 to a query (topk = n_eval = k = 64): every field of every 12-float record equal to
    candidate_record bit for bit, and the 4-float record of the plain call equal to its first four fields"""
    n = len(ibank["tags"])
    Bq = -(-n // 64)
    cand = (np.arange(Bq * 64) % n).reshape(Bq, 64).astype(np.int64)
    q = D.integer_panels(ibank["q"], P, D.rng_of(50, P), B=Bq)
    assert np.array_equal(D.q_mean32(q), np.repeat(ibank["q"][None], Bq, axis=0))
    init = np.zeros((Bq, 2))
    ex = raw_refine(env, ibank["db"], q, init, cand, None, 64, 64, 1.6, 1e9)
    pl = raw_refine(env, ibank["db"], q, init, cand, None, 64, 64, 1.6, 1e9, ext=False)
    want = ibank["rec12"][cand]
    bad = np.argwhere((bits(ex["scratch"]) != bits(want)).any(axis=2))
    found = [f"cell {cand[b, j]} ({ibank['tags'][cand[b, j]]}, {int(np.diff(ibank['bank'].cell_off)[cand[b, j]])} prototypes): got {ex['scratch'][b, j].tolist()} "
             f"ints {D.record_ints(ex['scratch'][b, j]).tolist()}, want {want[b, j].tolist()} ints {D.record_ints(want[b, j]).tolist()}" for b, j in bad[:8]]
    kinds = {t: int((ibank["tags"][cand[bad[:, 0], bad[:, 1]]] == t).sum()) for t in set(ibank["tags"])} if len(bad) else {}
    show(capsys, f"integer bank P={P}: {n} cells, {len(bad)} records differ {kinds}")
    assert not found, "\n".join(found)
    assert np.array_equal(bits(pl["scratch"]), bits(ex["scratch"][:, :, :4])), "the 4-float record differs from the extended one"
    assert np.array_equal(pl["llh"], ex["llh"]) and np.array_equal(pl["cell"], ex["cell"]) and np.array_equal(pl["choice"], ex["choice"])


def test_candidate_records_gaussian_bank(env, capsys):
    """queries at 1e-3, 0.1, 1 and 10 from a prototype, P = 1 .. 4: the score, the runner-up distance and both member distances within
    16 u d of the fp64 distance (from the fp32 mean) of the row the kernel names; that row is the truth's, except where two truth
    distances lie within 32 u d of each other (counted, at most 1 % of the records)"""
    rng = D.rng_of(60)
    bank = D.gaussian_bank(rng)
    db = env["ops"].DeviceBank(bank, device=DEV)
    C = len(bank.cell_off) - 1
    full = np.flatnonzero(np.diff(bank.cell_off) > 0)
    worst, found, exceptions, records = {}, [], 0, 0
    for radius in (1e-3, 0.1, 1.0, 10.0):
        for P in (1, 2, 3, 4):
            q = D.queries_near(bank, rng.permutation(full)[:8], radius, P, rng)
            cand = np.stack([rng.permutation(C) for _ in range(len(q))]).astype(np.int64)
            got = raw_refine(env, db, q, np.zeros((len(q), 2)), cand, None, C, C, 1.6, 1e9)["scratch"]
            qm = D.q_mean32(q)
            for b in range(len(q)):
                for j in range(C):
                    rec, ints = got[b, j], D.record_ints(got[b, j])
                    _, want, tr = D.candidate_record(bank, qm[b], int(cand[b, j]))
                    records += 1
                    if tr["empty"]:
                        if not np.array_equal(bits(rec), bits(want)):
                            found.append(f"empty cell {cand[b, j]}: {rec.tolist()}")
                        continue
                    wi = D.record_ints(want)
                    checks = [(-rec[0], ints[0], wi[0], tr["proto_ids"], tr["proto_d"]), (rec[4], ints[1], wi[1], tr["proto_ids"], tr["proto_d"])]
                    if ints[0] == wi[0] and wi[4] > 1:
                        checks += [(rec[7], ints[2], wi[2], tr["member_rows"], tr["member_d"]), (rec[8], ints[3], wi[3], tr["member_rows"], tr["member_d"])]
                    for fi, (dist, row, want_row, ids, dd) in enumerate(checks):
                        if want_row < 0:
                            if row != -1:
                                found.append(f"r={radius} P={P} cell {cand[b, j]} field {fi}: row {row} where there is none")
                            continue
                        at = np.flatnonzero(ids == row)
                        if len(at) == 0:
                            found.append(f"r={radius} P={P} cell {cand[b, j]} field {fi}: row {row} is not of this cell / cluster")
                            continue
                        d_row, d_want = dd[at[0]], dd[np.flatnonzero(ids == want_row)[0]]
                        ratio = abs(float(dist) - d_row) / (D.U32 * d_row)
                        worst[radius] = max(worst.get(radius, 0.0), ratio)
                        if not ratio <= 16:
                            found.append(f"r={radius} P={P} cell {cand[b, j]} field {fi}: distance {dist!r} at {ratio:.3g} u d of {d_row!r}")
                        if row != want_row:
                            exceptions += 1
                            if abs(d_row - d_want) > 32 * D.U32 * d_want:
                                found.append(f"r={radius} P={P} cell {cand[b, j]} field {fi}: row {row} (d {d_row!r}) for row {want_row} (d {d_want!r})")
                    if ints[0] == wi[0]:
                        same = np.array_equal(bits(rec[[1, 2, 3]]), bits(want[[1, 2, 3]])) if ints[2] == wi[2] else rec[3] == want[3]
                        if not (same and ints[4] == wi[4]):
                            found.append(f"r={radius} P={P} cell {cand[b, j]}: point / rows / count {rec.tolist()} for {want.tolist()}")
    show(capsys, "refine_candidates_kernel, Gaussian bank, worst |d32 - d| / (u d) per radius: " + ", ".join(f"{r:g}: {v:.3g}" for r, v in worst.items())
         + f"; {exceptions} near-tie exceptions in {records} records")
    assert not found, "\n".join(found[:20])
    assert exceptions <= 0.01 * records


# ================================================================================================================ selection
SELECT_SHAPES = [(1, 1), (5, 8), (64, 64), (5, 100)]
SELECT_VARIANTS = [("given", 1.6, 5000.0, {}), ("none", 1.6, 5000.0, dict(probs="none")), ("zeros", 1.6, 5000.0, dict(probs="zeros")),
                   ("repeat", 1.6, 5000.0, dict(repeat=True)), ("empties", 1.6, 5000.0, dict(only="empties")), ("all_underflow", 0.01, 5000.0, {}),
                   ("some_underflow", 0.025, 5000.0, {}), ("all_vetoed", 1.6, 1.0, {}), ("none_vetoed", 1.6, 1e5, {})]


@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_selection(env, ibank, B, capsys):
    """refine_select_kernel behind pg_refine_forward_ex and pg_refine_forward, one query per lane in 64-lane blocks: B = 1, 64, 65, 130;
    (topk, k) = (1,1), (5,8), (64,64), (5,100); P = 1, 3, 4 in turn; probabilities given, None and zeros; the same cell twice in a list;
    sets of only empty cells; T = 0.01 (every exponential 0, the product NaN, the first candidate wins) and T = 0.025 (only distance 2
    survives); max_km = 1, 5000 and 1e5.  Every family keeps the promise of _decisionref.select (gap 0 or >= 1e-3, veto distance
    >= 1 km from max_km), so out_llh, out_cell, out_choice and out_refined are equal to it without exception."""
    n = len(ibank["tags"])
    empties = np.flatnonzero(ibank["tags"] == "empty")
    found, seen = [], dict(vetoed=0, kept=0, zero_gap=0, later=0)
    for si, (topk, k) in enumerate(SELECT_SHAPES):
        for vi, (name, T, max_km, kw) in enumerate(SELECT_VARIANTS):
            P = (1, 3, 4)[(si + vi) % 3]
            kw = dict(kw, only=empties) if kw.get("only") == "empties" else kw
            case = D.selection_case(ibank["rec4"], n, B, topk, k, D.rng_of(70, B, si, vi), T, max_km, **kw)
            q = D.integer_panels(ibank["q"], P, D.rng_of(71, B, si, vi), B=B)
            n_eval = min(k, topk + 3)
            ex = raw_refine(env, ibank["db"], q, case["init"], case["cand"], case["prob"], topk, n_eval, T, max_km)
            pl = raw_refine(env, ibank["db"], q, case["init"], case["cand"], case["prob"], topk, topk, T, max_km, ext=False)
            want_ch = np.array([r["choice"] for r in case["expect"]])
            want_rf = np.array([r["refined"] for r in case["expect"]])
            want_cell = case["cand"][np.arange(B), want_ch]
            want_llh = np.stack([ibank["rec4"][int(c)][1:3] for c in want_cell])
            for o, which in ((ex, "ex"), (pl, "plain")):
                ok = (np.array_equal(o["choice"], want_ch) and np.array_equal(o["cell"], want_cell) and np.array_equal(bits(o["llh"]), bits(want_llh))
                      and (which == "plain" or np.array_equal(o["refined"], want_rf)))
                if not ok:
                    b = int(np.flatnonzero((o["choice"] != want_ch) | (o["cell"] != want_cell) | (bits(o["llh"]) != bits(want_llh)).any(axis=1)
                                           | ((o["refined"] != want_rf) if which == "ex" else False))[0])
                    found.append(f"{which} {name} topk={topk} k={k} P={P}: query {b} choice {o['choice'][b]} cell {o['cell'][b]} llh {o['llh'][b].tolist()}"
                                 f" for {case['expect'][b]} cell {want_cell[b]} llh {want_llh[b].tolist()}")
            for r in case["expect"]:
                seen["vetoed" if r["veto_km"] > max_km else "kept"] += 1
                seen["zero_gap"] += r["gap"] == 0
                seen["later"] += r["refined"] > 0
    show(capsys, f"selection B={B}: {len(SELECT_SHAPES) * len(SELECT_VARIANTS)} calls x 2 entry points, {seen}")
    assert not found, "\n".join(found[:20])
    assert min(seen.values()) > 0


# ================================================================================================================ certainty at its limits
def raw_head_certainty(env, o, emb, W, kx, wst):
    ops = env["ops"]
    B, C = o["logits"].shape
    ins = [o["logits_dev"].contiguous(), dev(emb), dev(W), dev(o["idx"]), dev(wst)]
    keep = [t.clone() for t in ins]
    tol, code, mg, sn = guarded(B), guarded(B, torch.int32), guarded(B), guarded(B)
    env["lib"].check(env["L"].pg_head_certainty(ops._p(ins[0]), B, C, ops._p(ins[1]), ins[1].shape[1], ops._p(ins[2]), ops._p(ins[3]), kx, ops._p(None),
                                                ops._p(ins[4]), ops._p(tol), ops._p(code), ops._p(mg), ops._p(sn), ops._stream()), "pg_head_certainty")
    out = take(tol, B, "head_certainty"), take(code, B, "head_certainty"), take(mg, B, "head_certainty"), take(sn, B, "head_certainty")
    unchanged(zip(ins, keep), "head_certainty")
    return out


@pytest.mark.parametrize("P", [1, 3])
def test_head_certainty_limits(env, P):
    """pg_head_certainty against the moved restatement (2e-3 relative, as tests/test_gpu_certainty.py) with kx = 1, 2 and C, at C = 2 and
    C = 300; two cells with identical weight rows and different biases: +inf; an exact tie for the top-1: 0."""
    for C in (2, 300):
        rng = D.rng_of(80, P, C)
        emb, W, bias = D.gaussian_logits_case(rng, 9, C, P)
        W = W * 4
        cent = rng.uniform(-90, 90, (C, 2))
        wst = np.array([np.linalg.norm(W, axis=1).max(), 0.0], dtype=F32)
        pe = emb.astype(np.float64).mean(axis=1)
        for kx in sorted({1, 2, C}):
            o = raw_head(env, emb, W, bias, cent, kx)
            tol, code, _, _ = raw_head_certainty(env, o, emb, W, kx, wst)
            for i in range(emb.shape[0]):
                t, c = D._head_tol_restated(o["logits"][i].astype(np.float64), pe[i], W.astype(np.float64), o["idx"][i], np.zeros(1024), float(wst[0]), 0.0)
                assert abs(float(tol[i]) - t) <= 2e-3 * abs(t) + 1e-6, (C, kx, i, float(tol[i]), t)
                assert int(code[i]) == c, (C, kx, i, int(code[i]), c)
    # identical weight rows, different biases: no embedding error can move the margin
    rng = D.rng_of(81, P)
    emb, W, bias = D.gaussian_logits_case(rng, 5, 2, P)
    W[1] = W[0]
    bias[:] = (0.25, -0.5)
    cent = rng.uniform(-90, 90, (2, 2))
    wst = np.array([np.linalg.norm(W, axis=1).max(), 0.0], dtype=F32)
    o = raw_head(env, emb, W, bias, cent, 2)
    tol, code, mg, _ = raw_head_certainty(env, o, emb, W, 2, wst)
    assert np.isposinf(tol).all() and (code == 0).all() and (o["idx"][:, 0] == 0).all() and (mg > 0).all()
    # an exact tie for the top-1 (controlled logits: emb[b,p,b] = 1 in every panel): tolerance 0, set by the tied candidate
    C, nb = 300, 6
    Wt = (rng.uniform(-1, 1, (C, 1024)) / 4).astype(F32)
    emb = np.zeros((nb, P, 1024), dtype=F32)
    emb[np.arange(nb), :, np.arange(nb)] = 1
    for b in range(nb):
        Wt[[3 + b, 70 + 2 * b], b] = 5.0                             # two cells at logit 5 in row b, everything else below 0.25
    cent = rng.uniform(-90, 90, (C, 2))
    wst = np.array([np.linalg.norm(Wt, axis=1).max(), 0.0], dtype=F32)
    for kx in (2, 9, C):
        o = raw_head(env, emb, Wt, np.zeros(C, dtype=F32), cent, kx)
        assert np.array_equal(o["idx"][:, :2], np.stack([3 + np.arange(nb), 70 + 2 * np.arange(nb)], axis=1))
        tol, code, mg, _ = raw_head_certainty(env, o, emb, Wt, kx, wst)
        assert (tol == 0).all() and (code == 1).all() and (mg == 0).all(), (kx, tol, code)


def _restated_refine(bank, q, cand, prob, topk, n_eval, T, C, W, wst, o):
    sc = o["scratch"]
    ints = D.record_ints(sc)[..., :4]
    rec, qm = sc.astype(np.float64), D.q_mean32(q).astype(np.float64)
    bp, bt, Wd = bank.proto_emb.astype(np.float64), bank.train_emb.astype(np.float64), W.astype(np.float64)
    out = []
    for b in range(q.shape[0]):
        L = np.log(prob[b, :n_eval]).astype(np.float64)
        r, c = int(o["refined"][b]), int(o["choice"][b])
        ex = np.exp((sc[b, :topk, 0] / F32(T)).astype(F32)).astype(F32)
        fin_r = float(prob[b, r]) * float(ex[r] / ex.sum(dtype=F32))
        out.append(D._refine_tol_restated(rec[b], ints[b], L, cand[b], topk, n_eval, C, Wd, bp, bt, qm[b], np.zeros(1024), float(wst[0]), 0.0, T, r, c,
                                          fin_r, cell_off=bank.cell_off, member_off=bank.member_off, member_idx=bank.member_idx))
    return out


def raw_refine_certainty(env, db, o, k, topk, n_eval, W, wst, T):
    ops = env["ops"]
    B, P = o["q_dev"].shape[0], o["q_dev"].shape[1]
    ins = [o["q_dev"], o["cand_dev"], o["prob_dev"], o["scratch_dev"].contiguous(), dev(W), dev(wst), o["refined_dev"].contiguous(), o["choice_dev"].contiguous()]
    assert o["prob_dev"] is not None
    keep = [t.clone() for t in ins]
    tol, code = guarded(B), guarded(B, torch.int32)
    env["lib"].check(env["L"].pg_refine_certainty(ctypes.byref(db.struct), ops._p(ins[0]), B, P, ops._p(ins[1]), ops._p(ins[2]), k, topk, n_eval,
                                                  ops._p(ins[3]), ops._p(ins[4]), ins[4].shape[0], ops._p(None), ops._p(ins[5]), float(T), ops._p(ins[6]),
                                                  ops._p(ins[7]), ops._p(tol), ops._p(code), ops._stream()), "pg_refine_certainty")
    out = take(tol, B, "refine_certainty"), take(code, B, "refine_certainty")
    unchanged(zip(ins, keep), "refine_certainty")
    return out


@pytest.mark.parametrize("P", [1, 3])
def test_refine_certainty_limits(env, ibank, P, capsys):
    """pg_refine_certainty against the moved restatement (5e-3 relative, as tests/test_gpu_certainty.py) at its limits topk = 64,
    n_eval = k = 96 and at topk = n_eval = k = 1; on the integer bank a pair of tied prototypes gives tolerance 0 with code 3000, a
    pair of tied members tolerance 0 with code 4000."""
    from pigeon_amd import synthetic
    hb = synthetic.make_bank(130, 9, seed=5, empty_frac=0.1, max_members=6)
    db = env["ops"].DeviceBank(hb, device=DEV)
    C, B = 130, 10
    codes = set()
    for topk, n_eval, k in ((64, 96, 96), (1, 1, 1)):
        rng = D.rng_of(90, P, topk)
        cand = np.stack([rng.permutation(C)[:k] for _ in range(B)]).astype(np.int64)
        sizes = np.diff(hb.cell_off)
        if topk == 1:
            cand[:, 0] = rng.permutation(np.flatnonzero(sizes > 0))[:B]
        near = np.array([c[np.flatnonzero(sizes[c] > 0)[0]] for c in cand])     # every query sits near its first non-empty candidate
        q = D.queries_near(hb, near, 10.0, P, rng)
        logit = np.sort(rng.normal(0, 1.2, (B, k)), axis=1)[:, ::-1]
        prob = np.exp(logit - 6.0)
        prob = (prob / (prob.sum(1, keepdims=True) * 1.3)).astype(F32)
        init = np.stack([rng.uniform(-180, 180, B), rng.uniform(-80, 80, B)], axis=1)
        W = (rng.standard_normal((C, 1024)) * 0.3).astype(F32)
        wst = np.array([np.linalg.norm(W, axis=1).max(), 0.0], dtype=F32)
        T = 1.6
        o = raw_refine(env, db, q, init, cand, prob, topk, n_eval, T, 1000.0)
        tol, code = raw_refine_certainty(env, db, o, k, topk, n_eval, W, wst, T)
        for b, (t, cd) in enumerate(_restated_refine(hb, q, cand, prob, topk, n_eval, T, C, W, wst, o)):
            got = float(tol[b])
            assert (np.isinf(t) and np.isinf(got)) or abs(got - t) <= 5e-3 * abs(t) + 1e-5, (topk, b, got, t, int(code[b]), cd)
            if np.isfinite(t) and abs(t) > 1e-3:
                assert int(code[b]) == cd, (topk, b, int(code[b]), cd, got, t)
            codes.add(cd // 1000)
    show(capsys, f"refine certainty limits P={P}: decision classes setting the tolerance {sorted(codes)}")
    # the integer bank's exact ties
    tags, n = ibank["tags"], len(ibank["tags"])
    W = (D.rng_of(91).standard_normal((n, 1024)) * 0.3).astype(F32)
    wst = np.array([np.linalg.norm(W, axis=1).max(), 0.0], dtype=F32)
    for kind, want in (("tied_protos", 3000), ("tied_members", 4000)):
        cells = np.flatnonzero(tags == kind)
        q = D.integer_panels(ibank["q"], P, D.rng_of(92, P), B=len(cells))
        prob = np.ones((len(cells), 1), dtype=F32)
        o = raw_refine(env, ibank["db"], q, np.zeros((len(cells), 2)), cells[:, None].astype(np.int64), prob, 1, 1, 1.6, 1e9)
        tol, code = raw_refine_certainty(env, ibank["db"], o, 1, 1, 1, W, wst, 1.6)
        assert (tol == 0).all() and (code == want).all(), (kind, tol[tol != 0][:5], code[code != want][:5])


def test_wall_time_of_this_file(capsys):
    show(capsys, f"tests/test_gpu_decision.py: {time.time() - T0:.0f} s since import")
