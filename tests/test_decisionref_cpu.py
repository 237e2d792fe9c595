"""tests/_decisionref.py pinned, without a GPU: the restatements against the recorded outputs of the reference (tests/golden/head.npz,
refine.npz) and against the oracle, fp32 numpy emulations of the kernels' summation orders against every derived bound on every
input family -- and every comparison the GPU tier (tests/test_gpu_decision.py) makes shown to reject the mistake it is there for."""
import os

import numpy as np
import pytest
import torch

import _decisionref as D
from oracle import pigeon_oracle as orc
from pigeon_amd import synthetic

F32 = np.float32


def show(capsys, text):
    with capsys.disabled():
        print("\n" + text)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.int32)


@pytest.fixture(scope="module")
def ibank():
    bank, q, tags = D.integer_bank(D.rng_of(3))
    recs = [D.candidate_record(bank, q, c) for c in range(len(tags))]
    return dict(bank=bank, q=q, tags=np.array(tags), recs=recs)


# ================================================================================================================ the reference's outputs
def test_head_truth_reproduces_the_reference(golden_dir, capsys):
    """head.npz from the real reference: the fp64 logits are within the derived bound of its logits_first8, topk_expected of them is
    its top-50 bit for bit, and its top-50 probabilities are within the softmax bound plus the logit bound carried through exp
    (a logit error d moves a probability by at most 2 d p)."""
    g = np.load(os.path.join(golden_dir, "head.npz"))
    C, seed, B, eseed, k = [int(x) for x in g["meta"]]
    W, b = synthetic.make_head_weights(C, seed=seed)
    emb = (torch.randn((B, 4, 1024), generator=torch.Generator().manual_seed(eseed)) * 0.7 + 0.1).numpy()
    t, S = D.head_logits_truth(emb, W.numpy(), b.numpy())
    bound = D.logits_bound(t, S, 4)
    r8 = np.abs(g["logits_first8"] - t[:, :8]) / bound[:, :8]
    worst_p = 0.0
    for i in range(B):
        l32 = t[i].astype(F32)
        assert np.array_equal(D.topk_expected(l32, k), g["topk_indices"][i]), i
        p = D.softmax_truth(l32)
        pb = D.softmax_bound(l32, p) + 2 * (bound[i].max() + D.U32 * np.abs(t[i]).max()) * p
        idx = g["topk_indices"][i]
        worst_p = max(worst_p, float((np.abs(g["topk_values"][i] - p[idx]) / pb[idx]).max()))
        assert g["preds_geocell"][i] == idx[0]
    show(capsys, f"reference head: logits_first8 at {r8.max():.3g} of the bound, top-50 probabilities at {worst_p:.3g}")
    assert r8.max() <= 1 and worst_p <= 1


@pytest.mark.parametrize("tag", ["default", "evaluate", "tight", "noprobs3d", "vetoedge"])
def test_record_and_select_reproduce_the_reference(golden_dir, tag):
    g = np.load(os.path.join(golden_dir, "refine.npz"))
    C, ppc, bseed = [int(x) for x in g["meta"]]
    bank = synthetic.make_bank(C, ppc, seed=bseed, empty_frac=0.05)
    emb, init, prob = g["embedding"][:, None, :], g["initial_preds"], g["candidate_probs"]
    topk, T, mr = g[f"{tag}_params"] if f"{tag}_params" in g.files else (5, 1.6, 1000.0)
    if tag == "noprobs3d":
        emb, prob = emb + np.array([0.1, -0.1, 0.2, -0.2], dtype=F32)[None, :, None], None
    if tag == "vetoedge":
        init = g["vetoedge_init"]
    topk = int(topk)
    qm = D.q_mean32(emb)
    for i in range(emb.shape[0]):
        cells = g["candidate_cells"][i, :topk]
        rec = np.stack([D.candidate_record(bank, qm[i], int(c))[0] for c in cells])
        r = D.select(rec[:, 0], None if prob is None else prob[i, :topk], float(T), init[i], rec[:, 1:3], float(mr))
        assert cells[r["choice"]] == g[f"{tag}_cell"][i], (tag, i)
        assert np.array_equal(rec[r["choice"], 1:3], g[f"{tag}_LLH"][i]), (tag, i)


def test_record_and_select_match_the_oracle_on_the_integer_bank(ibank):
    """every cell of the integer bank, 64 to a query, through oracle.pigeon_oracle.proto_refiner_forward: the same point and cell;
    then a cell at a time (topk = 1), which pins every record's point to the oracle's pick, ties included"""
    bank, q, recs = ibank["bank"], ibank["q"], ibank["recs"]
    n = len(recs)
    cells = np.arange(n)
    _, llh, cell = orc.proto_refiner_forward(bank, torch.from_numpy(np.repeat(q[None], n, axis=0)), torch.zeros((n, 2), dtype=torch.float64),
                                             torch.from_numpy(cells[:, None]), None, 1, 1.6, 1e9)
    want = np.stack([r[0][1:3] for r in recs])
    assert np.array_equal(cell.numpy(), cells) and np.array_equal(llh.numpy(), want)
    rng = D.rng_of(4)
    rec4 = {c: recs[c][0] for c in range(n)}
    case = D.selection_case(rec4, n, 24, 64, 64, rng, 1.6, 5000.0)
    _, llh, cell = orc.proto_refiner_forward(bank, torch.from_numpy(np.repeat(q[None], 24, axis=0)), torch.from_numpy(case["init"]),
                                             torch.from_numpy(case["cand"]), torch.from_numpy(case["prob"]), 64, 1.6, 5000.0)
    for b, r in enumerate(case["expect"]):
        c = int(case["cand"][b, r["choice"]])
        assert int(cell[b]) == c and np.array_equal(llh[b].numpy(), rec4[c][1:3]), b


# ================================================================================================================ certainty restatements
def _certainty_inputs():
    rng = D.rng_of(5)
    bank = D.gaussian_bank(rng, cells=14)
    C, topk, n_eval, T = 14, 3, 5, 1.6
    full = np.flatnonzero(np.diff(bank.cell_off) > 0)
    cand = rng.permutation(full)[:n_eval]
    e = D.q_mean32(D.queries_near(bank, cand[:1], 1.0, 2, rng))[0]
    rec = np.stack([D.candidate_record(bank, e, int(c))[1] for c in cand])
    ints = D.record_ints(rec)[:, :4]
    W = rng.standard_normal((C, 1024)) * 0.3
    beta = rng.standard_normal(1024) * 1e-5
    L = np.log(np.sort(rng.uniform(0.01, 0.2, n_eval))[::-1])
    return dict(bank=bank, cand=cand, e=e.astype(np.float64), rec=rec.astype(np.float64), ints=ints, W=W, beta=beta, L=L, C=C, topk=topk,
                n_eval=n_eval, T=T, logits=rng.normal(0, 2, C), idx=rng.permutation(C)[:6])


PINNED_HEAD = (0.01555844583110118, 1)
PINNED_REFINE = (0.046212789414238474, 2999)


def certainty_values(head_tol, refine_tol):
    x = _certainty_inputs()
    idx = x["idx"][np.argsort(-x["logits"][x["idx"]])]
    h = head_tol(x["logits"], x["e"], x["W"], idx, x["beta"], 9.0, 0.01)
    bank = x["bank"]
    r = refine_tol(x["rec"], x["ints"], x["L"], x["cand"], x["topk"], x["n_eval"], x["C"], x["W"], bank.proto_emb.astype(np.float64),
                   bank.train_emb.astype(np.float64), x["e"], x["beta"], 9.0, 0.01, x["T"], 0, 0, 0.5, cell_off=bank.cell_off,
                   member_off=bank.member_off, member_idx=bank.member_idx)
    return h, r


def test_certainty_restatements_unchanged_by_the_move():
    """_tol, _head_tol_restated and _refine_tol_restated moved here from tests/test_gpu_certainty.py: on a fixed seed they give the
    values they gave there (recorded before the move), and tolerance +inf for a zero gradient, 0 for a zero margin"""
    h, r = certainty_values(D._head_tol_restated, D._refine_tol_restated)
    assert h[1] == PINNED_HEAD[1] and h[0] == pytest.approx(PINNED_HEAD[0], rel=1e-11)
    assert r[1] == PINNED_REFINE[1] and r[0] == pytest.approx(PINNED_REFINE[0], rel=1e-11)
    g = np.ones(1024)
    assert D._tol(1.0, np.zeros(1024), g, 2.0) == np.inf and D._tol(0.0, g, np.zeros(1024), 2.0) == 0.0
    assert D._tol(np.inf, g, g, 2.0) == np.inf
    import test_gpu_certainty as old
    assert old._tol is D._tol and old._head_tol_restated is D._head_tol_restated and old._refine_tol_restated is D._refine_tol_restated


# ================================================================================================================ emulations inside the bounds
def test_integer_families_are_exact():
    """x * fl(1/P) is exact for the panel sums of the integer families, so the emulated kernel gives the truth's bits"""
    for P in (1, 2, 3, 4, 5):
        m = np.arange(-5000, 5001)
        assert np.array_equal((m * P).astype(F32) * (F32(1) / F32(P)), m.astype(F32)), P
        emb, W, bias = D.integer_logits_case(D.rng_of(6, P), 5, 9, P)
        t, _ = D.head_logits_truth(emb, W, bias)
        assert np.array_equal(t, np.rint(t)) and np.array_equal(D.logits_emulated(emb, W, bias), t.astype(F32)), P
        q = D.rng_of(7, P).integers(-8, 9, 1024).astype(F32)
        assert np.array_equal(D.q_mean32(D.integer_panels(q, P, D.rng_of(8, P), B=3)), np.repeat(q[None], 3, axis=0)), P


def test_logits_emulation_inside_the_bound(capsys):
    worst = 0.0
    for P in (1, 2, 3, 4, 5):
        emb, W, bias = D.gaussian_logits_case(D.rng_of(9, P), 7, 33, P)
        t, S = D.head_logits_truth(emb, W, bias)
        worst = max(worst, float((np.abs(D.logits_emulated(emb, W, bias) - t) / D.logits_bound(t, S, P)).max()))
    show(capsys, f"emulated head logits: worst {worst:.3g} of the bound")
    assert worst <= 1


SOFTMAX_C = (1, 2, 255, 256, 257, 1031, 38400, 38401)


def test_softmax_and_topk_emulation(capsys):
    """the fp32 emulation of head_row_kernel on every family, masked and unmasked, C = 1 .. 38401: probabilities inside the bound, zero
    top-k exceptions on the tie families, below 1 % of the listed positions on the others; all-NaN rows list 0 .. k-1"""
    worst, exc, listed = dict.fromkeys(D.LOGIT_FAMILIES, 0.0), dict.fromkeys(D.LOGIT_FAMILIES, 0), dict.fromkeys(D.LOGIT_FAMILIES, 0)
    cen = D.rng_of(10).uniform(-90, 90, (38401, 2))
    for ci, C in enumerate(SOFTMAX_C):
        for mi, mask in enumerate((None, "neginf", "posinf", "nan")):
            L, bias = D.controlled_case(C, D.rng_of(11, ci, mi), mask)
            for tag, row in zip(D.LOGIT_FAMILIES, L):
                l32 = row + bias
                p32 = D.softmax_emulated(l32)
                for k in sorted({1, min(C, 50)} | ({C} if C <= 1031 else set())):
                    idx = D.topk_emulated(p32, k)
                    e = D.topk_check(l32, k, p32[idx], idx, idx[0], cen[idx[0]], cen)
                    exc[tag] += len(e); listed[tag] += k
                if mask in ("posinf", "nan"):
                    assert np.isnan(p32).all() and D.all_nan_row(l32)
                    continue
                p = D.softmax_truth(l32)
                worst[tag] = max(worst[tag], float((np.abs(p32 - p) / D.softmax_bound(l32, p)).max()))
    show(capsys, "emulated softmax, worst of the bound per family: " + ", ".join(f"{t} {v:.3g}" for t, v in worst.items())
         + "; top-k exceptions: " + ", ".join(f"{t} {exc[t]} of {listed[t]}" for t in D.LOGIT_FAMILIES))
    assert max(worst.values()) <= 1
    for t in D.LOGIT_FAMILIES:
        assert exc[t] == 0 if t in D.TIE_FAMILIES else exc[t] < 0.01 * listed[t], t
    nan_row = np.full(300, np.nan, dtype=F32)
    assert np.array_equal(D.topk_emulated(D.softmax_emulated(nan_row), 7), np.arange(7)) and np.array_equal(D.topk_expected(nan_row, 7), np.arange(7))
    assert D.all_nan_row(np.full(5, -np.inf, dtype=F32)) and np.isnan(D.softmax_emulated(np.full(5, -np.inf, dtype=F32))).all()


def test_distance_emulation_inside_the_bound(capsys):
    """queries at 1e-3, 0.1, 1 and 10 from a prototype, P = 1 .. 4: the fp32 emulation of the lane chain and the butterfly against the
    fp64 distance from the fp32 mean, on every prototype and training row of the Gaussian bank"""
    rng = D.rng_of(12)
    bank = D.gaussian_bank(rng)
    full = np.flatnonzero(np.diff(bank.cell_off) > 0)
    worst = {}
    for radius in (1e-3, 0.1, 1.0, 10.0):
        for P in (1, 2, 3, 4):
            qm = D.q_mean32(D.queries_near(bank, full[:6], radius, P, rng))
            for q in qm:
                for rows in (bank.proto_emb, bank.train_emb):
                    d = D.distances_truth(rows, q)
                    worst[radius] = max(worst.get(radius, 0.0), float((np.abs(D.distances_emulated(rows, q) - d) / (D.U32 * d)).max()))
    show(capsys, "emulated distances, worst |d32 - d| / (u d) per radius: " + ", ".join(f"{r:g}: {v:.3g}" for r, v in worst.items()))
    assert max(worst.values()) <= 16
    bank, q = D.integer_bank(D.rng_of(3))[:2]
    assert np.array_equal(D.distances_emulated(bank.proto_emb[:500], q), D.distances_truth(bank.proto_emb[:500], q).astype(F32))


# ================================================================================================================ the families' promises
def test_integer_bank_is_what_it_says(ibank):
    bank, q, tags, recs = ibank["bank"], ibank["q"], ibank["tags"], ibank["recs"]
    sizes = np.diff(bank.cell_off)
    for n in D.PROTO_SMALL:                                         # the nearest row at every position of every size
        sel = np.flatnonzero((tags == "nearest_small") & (sizes == n))
        assert sorted(int(D.record_ints(recs[c][1])[0] - bank.cell_off[c]) for c in sel) == list(range(n)), n
    for n in D.PROTO_LARGE:
        sel = np.flatnonzero((tags == "nearest_large") & (sizes == n))
        assert sorted(int(D.record_ints(recs[c][1])[0] - bank.cell_off[c]) for c in sel) == sorted({0, 3, 4, 7, 8} | set(range(n - 9, n)))
    pairs = {(int(sizes[c]),) + tuple(int(x - bank.cell_off[c]) for x in D.record_ints(recs[c][1])[:2])
             for c in np.flatnonzero(tags == "ordered_pair")}
    assert pairs == {(n, i, j) for n in range(2, 13) for i in range(n) for j in range(n) if i != j}
    tied = np.flatnonzero(tags == "tied_protos")
    assert all(recs[c][1][4] == -recs[c][1][0] and D.record_ints(recs[c][1])[0] < D.record_ints(recs[c][1])[1] for c in tied)
    assert len(tied) == sum(n * (n - 1) // 2 for n in range(2, 13))
    for kind, eq in (("farthest", False), ("tied_members", True)):
        sel = np.flatnonzero(tags == kind)
        assert len(sel) == sum(s if kind == "farthest" else s * (s - 1) // 2 for s in D.MEMBER_SIZES)
        for c in sel:
            r = recs[c][1]
            p1, _, t1, t2, cnt = D.record_ints(r)
            assert cnt in D.MEMBER_SIZES and (r[7] == r[8]) == eq and r[7] == 30 and t1 != t2
            pos = bank.member_idx[bank.member_off[p1]:bank.member_off[p1 + 1]].tolist()
            assert pos.index(t1) < pos.index(t2) if eq else True
    assert (bank.member_idx != np.arange(len(bank.member_idx))).mean() > 0.99
    for c in np.flatnonzero(tags == "empty"):
        assert np.array_equal(bits(recs[c][1]), bits(D._empty12()))
    d = D.distances_truth(bank.proto_emb, q)
    assert np.array_equal(d, np.rint(d)) and d.min() >= 2            # exact integers; -d / 0.01 is far below the underflow band


SELECT_SETTINGS = [(1.6, 5000.0), (1.6, 1.0), (1.6, 1e5), (0.01, 5000.0), (0.025, 5000.0)]


def test_selection_families_keep_their_promise(ibank, capsys):
    """gap exactly 0 or >= 1e-3, veto distance >= 1 km from max_km, no exponent in the subnormal band -- and with that the fp32
    restatement picks what the fp64 products pick.  T = 0.01: every exponential is 0 and candidate 0 wins; T = 0.025: only the
    cells at distance 2 keep a non-zero exponential."""
    rec4 = {c: r[0] for c, r in enumerate(ibank["recs"])}
    n = len(rec4)
    empties = np.flatnonzero(ibank["tags"] == "empty")
    seen = dict(zero_gap=0, vetoed=0, kept=0, refined_not_first=0)
    for si, (T, max_km) in enumerate(SELECT_SETTINGS):
        for vi, kw in enumerate((dict(), dict(probs="none"), dict(probs="zeros"), dict(repeat=True), dict(only=empties))):
            case = D.selection_case(rec4, n, 12, 5, 8, D.rng_of(13, si, vi), T, max_km, **kw)
            for b, r in enumerate(case["expect"]):
                assert r["clear"] and (r["gap"] == 0 or r["gap"] >= 1e-3) and abs(r["veto_km"] - max_km) >= 1
                rec = np.stack([rec4[int(c)] for c in case["cand"][b, :5]])
                x = rec[:, 0].astype(np.float64) / float(F32(T))
                cp = case["prob"][b, :5].astype(np.float64) if case["prob"] is not None else np.array([1.0, 0, 0, 0, 0])
                prod = cp * np.where(x < -104, 0.0, np.exp(x))
                if prod.max() > 0:
                    assert prod[r["refined"]] == prod.max() and r["refined"] == int(np.argmax(prod))
                else:
                    assert r["refined"] == 0
                if T == 0.01 or "only" in kw or kw.get("probs") == "zeros":
                    assert r["refined"] == 0
                seen["zero_gap"] += r["gap"] == 0
                seen["vetoed" if r["veto_km"] > max_km else "kept"] += 1
                seen["refined_not_first"] += r["refined"] != 0
    show(capsys, f"selection families: {seen}")
    assert min(seen.values()) > 0


# ================================================================================================================ the mistakes are caught
def test_every_mistake_switch_is_caught(ibank):
    bank, q, tags, recs = ibank["bank"], ibank["q"], ibank["tags"], ibank["recs"]

    def differing(kinds, **switch):
        sel = np.flatnonzero(np.isin(tags, kinds))
        return sum(not np.array_equal(bits(D.candidate_record(bank, q, int(c), **switch)[1]), bits(recs[c][1])) for c in sel), len(sel)
    n, of = differing(["tied_protos"], ties_highest=True)
    assert n == of                                                  # every tied pair of prototypes swaps nearest and runner-up
    n, of = differing(["tied_members"], ties_highest=True)
    assert n == of
    n, of = differing(["ordered_pair"], runner_up_own_wave=True)    # caught wherever the two are not 4 rows apart
    assert n == sum(1 for c in np.flatnonzero(tags == "ordered_pair") if np.diff(D.record_ints(recs[c][1])[:2])[0] % 4 != 0) > 0.6 * of
    n, of = differing(["farthest"], runner_up_own_wave=True)
    assert n > 0.5 * of
    n, of = differing(["nearest_small", "nearest_large", "farthest"], swap_near_far=True)
    assert n >= of - 1                                              # all but the one-prototype cell
    n, of = differing(["nearest_small"], drop_tail=True)
    sizes = np.diff(bank.cell_off)
    lost = sum(1 for c in np.flatnonzero(tags == "nearest_small")
               if (lambda i, m: ((m - i % 4 + 3) // 4) % 2 == 1 and i + 4 >= m)(int(D.record_ints(recs[c][1])[0] - bank.cell_off[c]), int(sizes[c])))
    assert n >= lost >= 30                                          # the cells whose nearest (or runner-up) row is a wave's left-over row
    # head: the last K tile, the panels p >= 1
    for P in (2, 3, 5):
        emb, W, bias = D.integer_logits_case(D.rng_of(14, P), 3, 5, P)
        t, _ = D.head_logits_truth(emb, W, bias)
        got = D.logits_emulated(emb, W, bias)
        assert np.array_equal(got, t.astype(F32))
        assert not np.array_equal(got, D.head_logits_truth(emb, W, bias, drop_last_k_tile=True)[0].astype(F32))
        assert not np.array_equal(got, D.head_logits_truth(emb, W, bias, first_panel_only=True)[0].astype(F32))
        emb, W, bias = D.gaussian_logits_case(D.rng_of(15, P), 3, 5, P)
        t, S = D.head_logits_truth(emb, W, bias)
        for kw in (dict(drop_last_k_tile=True), dict(first_panel_only=True)):
            assert (np.abs(D.head_logits_truth(emb, W, bias, **kw)[0] - t) > D.logits_bound(t, S, P)).mean() > 0.9
    # top-k: ties to the highest index, a selected cell not retired
    cen = D.rng_of(16).uniform(-90, 90, (1031, 2))
    for tag in D.LOGIT_FAMILIES:
        l32 = D.logit_rows(tag, 1031, D.rng_of(17))
        p32 = D.softmax_emulated(l32)
        for kw in (dict(ties_highest=True), dict(no_retire=True)):
            idx = D.topk_expected(l32, 50, **kw)
            if np.array_equal(idx, D.topk_expected(l32, 50)):
                assert tag not in D.TIE_FAMILIES and "ties_highest" in kw
                continue
            try:
                e = D.topk_check(l32, 50, p32[idx], idx, idx[0], cen[idx[0]], cen)
            except AssertionError:
                continue
            assert tag in D.TIE_FAMILIES and len(e) > 0, (tag, kw)  # a wrong tie order passes as "exceptions": these families allow none
