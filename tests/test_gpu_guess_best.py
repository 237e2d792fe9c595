"""pg_score_table and pg_guess_best on the GPU (run with -m gpu on an MI355X), through the C ABI.

Where the inputs are exact nothing is approximate: logits of 0 / -inf make every weight 1 or 0 and Z a small integer, an integer table
keeps every partial sum below 2^53, so `expected` is one known value per element and must equal numpy's integer arithmetic at zero
tolerance -- a dropped K step, a tile at the wrong rows, a row past B or a candidate past M show up as a location.  The edge shapes
come from pg_guess_best_plan, not from constants copied out of the kernel.  Gaussian logits are held under tests/_bestref.py: the numpy
restatement with derived bounds and the tight / loose rule (at most 1 % loose rows, asserted; the inputs show 0).  Every output sits
between guard regions that must keep their pattern, and no input may change."""
import numpy as np
import pytest
import torch

import _bestref as R
import _georef as G
import _spreadref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
IDX_SENTINEL = -77
C_LIST = (1, 2, 3, 63, 64, 65, 257, 2076, 9601)
M_LIST = (1, 2, 63, 64, 65, 257, 2077)
GAUSS_SHAPES = ((17, 257, 257), (5, 65, 2076), (3, 2076, 65))        # B * M * C <= 2e6: the longdouble restatement runs on these
FORM1_M = 64 * 256                                                   # with one row tile: 256 candidate tiles of 64


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops
    _lib.require_gpu()
    return dict(lib=_lib, ops=hip_ops, L=_lib.load(), plan=hip_ops.guess_best_plan(3, 65, 65))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(n, dtype=torch.float64, sentinel=G.SENTINEL):
    buf = torch.full((n + 2 * G.GUARD,), sentinel, dtype=dtype, device=DEV)
    return buf, buf[G.GUARD:G.GUARD + n]


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def run(env, logits, table, maximize=True, want_expected=True):
    """logits numpy / device (B,C) fp32, table numpy / device (M,C) fp64 -> (best_idx (B,) int32, best_value (B,), expected (B,M) or
    None) device tensors, through the C ABI; guards and inputs checked"""
    ops = env["ops"]
    lg = logits if torch.is_tensor(logits) else dev(logits)
    tb = table if torch.is_tensor(table) else dev(table)
    B, Cn = lg.shape
    M = tb.shape[0]
    assert tb.shape == (M, Cn) and lg.dtype == torch.float32 and tb.dtype == torch.float64
    keep = [lg.clone(), tb.clone()]
    bi, bv = guarded(B, torch.int32, IDX_SENTINEL), guarded(B)
    be = guarded(B * M) if want_expected else None
    env["lib"].check(env["L"].pg_guess_best(ops._p(lg), B, Cn, ops._p(tb), M, 1 if maximize else 0, ops._p(bi[1]), ops._p(bv[1]),
                                            ops._p(be[1] if want_expected else None), ops._stream()), "pg_guess_best")
    torch.cuda.synchronize()
    for pair, name, sentinel in ((bi, "best_idx", IDX_SENTINEL), (bv, "best_value", G.SENTINEL), (be, "expected", G.SENTINEL)):
        if pair is None:
            continue
        buf, view = pair
        n = view.numel()
        assert bool((buf[:G.GUARD] == sentinel).all()) and bool((buf[G.GUARD + n:] == sentinel).all()), f"{name}: wrote outside its output"
    for t, k in zip((lg, tb), keep):
        assert torch.equal(t.view(torch.uint8), k.view(torch.uint8)), "an input changed"
    return bi[1].clone(), bv[1].clone(), be[1].clone().reshape(B, M) if want_expected else None


def table_of(env, cand, cen, kind):
    return env["ops"].score_table(dev(cand), dev(cen), kind=kind)


def first_best(exp, maximize):
    """numpy (B,M) -> the first index of the best entry that is no NaN, -1 where there is none"""
    return np.array([R._first_best(row, maximize) for row in exp], dtype=np.int64)


# ================================================================================================================ exact inputs
def exact_case(env, B, Cn, M, maximize, seed=0):
    rng = np.random.default_rng([91, B, Cn, M, seed])
    live = rng.random((B, Cn)) < 0.6
    live[np.arange(B), rng.integers(0, Cn, B)] = True                # every row has a cell
    logits = np.where(live, 0.0, -np.inf).astype(np.float32)
    table = rng.integers(-1000, 1001, (M, Cn)).astype(np.int64)
    num = live.astype(np.int64) @ table.T                            # (B,M), exact
    want = num.astype(np.float64) / live.sum(axis=1, keepdims=True).astype(np.float64)       # one correctly rounded division
    idx, val, exp = run(env, logits, table.astype(np.float64), maximize)
    got = exp.cpu().numpy()
    wrong = np.argwhere(got != want)
    assert wrong.size == 0, (f"(B, C, M) = {(B, Cn, M)}: {len(wrong)} elements differ, the first at row {wrong[0][0]} candidate "
                             f"{wrong[0][1]}: got {got[tuple(wrong[0])]!r}, want {want[tuple(wrong[0])]!r}")
    want_idx = first_best(want, maximize)
    got_idx = idx.cpu().numpy().astype(np.int64)
    assert (got_idx == want_idx).all(), f"(B, C, M) = {(B, Cn, M)}: best_idx differs first at row {np.argwhere(got_idx != want_idx)[0][0]}"
    assert (val.cpu().numpy() == want[np.arange(B), want_idx]).all(), f"(B, C, M) = {(B, Cn, M)}: best_value"


def edges(n):
    return (n - 1, n, n + 1, 2 * n - 1, 2 * n, 2 * n + 1)


def test_exact_inputs_cells(env):
    kc = env["plan"]["cells_per_step"]
    for i, Cn in enumerate(sorted(set(C_LIST + edges(kc)))):
        exact_case(env, 3, Cn, 65, maximize=i % 2 == 0)


def test_exact_inputs_candidates(env):
    ct = env["plan"]["candidates_per_tile"]
    for i, M in enumerate(sorted(set(M_LIST + edges(ct)))):
        exact_case(env, 17, 65, M, maximize=i % 2 == 1)


def test_exact_inputs_rows(env):
    rt, kc, ct = (env["plan"][k] for k in ("rows_per_tile", "cells_per_step", "candidates_per_tile"))
    for i, B in enumerate(sorted(set((1, 3, 17) + edges(rt)))):
        exact_case(env, B, kc + 1, ct + 1, maximize=i % 2 == 0)
    exact_case(env, 2 * rt + 1, 2 * kc + 1, 2 * ct + 1, True)


def test_exact_inputs_large_tile_form(env):
    """the shapes at which the plan switches to its larger tiles, with that form's own edges"""
    plan = env["ops"].guess_best_plan(65, 5, FORM1_M // 2 + 1)
    assert plan["form"] == 1 and plan["form"] != env["plan"]["form"]
    rt, ct = plan["rows_per_tile"], plan["candidates_per_tile"]
    for B in (rt + 1, 2 * rt - 1):
        M = ct * (-(-256 // -(-B // rt)) - 1) + 1                    # the fewest candidates that still give 256 workgroups, one in the last tile
        assert env["ops"].guess_best_plan(B, 37, M)["form"] == 1 and env["ops"].guess_best_plan(B, 37, M - 1)["form"] == 0
        exact_case(env, B, 37, M, True)
        exact_case(env, B, 37, M - 1, False)                         # the same shape, one candidate fewer: the small form's last case


def test_one_hot_rows_return_the_table_column(env):
    """one finite logit per row: weight 1, Z = 1, every other term 0 * finite -- E[b,j] is table[j,c] itself"""
    B, Cn, M = 17, 257, 65
    cen = S.centroids_of(Cn, 3)
    cand = R.candidates_of(M, 3, cen)
    rng = np.random.default_rng(17)
    cells = rng.integers(0, Cn, B)
    logits = np.full((B, Cn), -np.inf, dtype=np.float32)
    logits[np.arange(B), cells] = rng.normal(0, 5, B).astype(np.float32)
    for kind in R.OBJECTIVES:
        tab = table_of(env, cand, cen, kind)
        idx, val, exp = run(env, logits, tab, maximize=kind == "score")
        want = tab[:, dev(cells)].t().contiguous()
        assert bits_equal(exp, want), f"{kind}: not the table's column of the row's cell"
        assert (idx.cpu().numpy() == first_best(want.cpu().numpy(), kind == "score")).all()


def test_exact_ties_return_the_first(env):
    ct = env["plan"]["candidates_per_tile"]
    B, Cn, M = 5, 65, 4 * ct + 3
    logits = S.gaussian_logits(B, Cn, 8)
    rng = np.random.default_rng(8)
    for j, j2 in ((3, 9), (5, 5 + 2 * ct), (ct - 1, ct), (0, M - 1)):
        for maximize in (True, False):
            table = rng.uniform(100, 200, (M, Cn))
            table[j] = 900.0 + rng.uniform(0, 1, Cn) if maximize else rng.uniform(0, 1, Cn)
            table[j2] = table[j]
            idx, val, exp = run(env, logits, table, maximize)
            assert bits_equal(exp[:, j], exp[:, j2]), "duplicated candidates differ"
            assert (idx.cpu().numpy() == j).all(), f"candidates {j} and {j2} tie: got {idx.cpu().numpy()}"
            assert bits_equal(val, exp[:, j])
    big = torch.rand((FORM1_M, 5), dtype=torch.float64, device=DEV)  # the large-tile form, the twins 200 tiles apart
    big[70] = 2.0
    big[70 + 200 * 64] = 2.0
    assert env["ops"].guess_best_plan(B, 5, FORM1_M)["form"] == 1
    idx, val, _ = run(env, S.gaussian_logits(B, 5, 9), big, True, want_expected=False)
    assert (idx.cpu().numpy() == 70).all() and (np.abs(val.cpu().numpy() - 2.0) <= 16 * G.EPS).all()         # (sum w 2) / Z: five roundings


# ================================================================================================================ gaussian logits
@pytest.fixture(scope="module")
def gauss():
    """per shape: the inputs and the restatement, computed once and left unchanged"""
    out = {}
    for i, (B, Cn, M) in enumerate(GAUSS_SHAPES):
        logits, cen = S.gaussian_logits(B, Cn, i, (1.0, 3.0, 6.0)[i]), S.centroids_of(Cn, i)
        cand = R.candidates_of(M, i, cen)                            # both poles, the antimeridian, a centroid itself
        out[(B, Cn, M)] = dict(logits=logits, cen=cen, cand=cand, shared=R.spread_truth(logits, cen, cand))
    return out


@pytest.mark.parametrize("shape", GAUSS_SHAPES)
def test_gaussian_logits_under_the_comparator(env, gauss, capsys, shape):
    g = gauss[shape]
    for objective in R.OBJECTIVES:
        t = R.truth(g["logits"], g["cen"], g["cand"], objective, shared=g["shared"])
        tab = table_of(env, g["cand"], g["cen"], objective)
        idx, val, exp = run(env, g["logits"], tab, maximize=objective == "score")
        errors, loose, worst = R.compare(t, idx.cpu().numpy(), val.cpu().numpy(), exp.cpu().numpy())
        with capsys.disabled():
            print(f"\nguess_best {shape} {objective}: worst |got - truth| / bound {worst:.3g}, {loose} loose of {len(t['tight'])} rows, "
                  f"smallest top-2 gap {t['gap'].min():.3g}")
        assert not errors, errors[:5]
        assert loose <= R.loose_allowed(t), f"{loose} loose rows of {len(t['tight'])}"
        _, val2, none = run(env, g["logits"], tab, maximize=objective == "score", want_expected=False)
        assert none is None and bits_equal(val, val2), "the answer depends on whether `expected` is asked for"


@pytest.mark.parametrize("shape", GAUSS_SHAPES[1:])
def test_against_guess_spread(env, gauss, shape):
    """the same expectation by the other kernel: pg_guess_spread asked about every candidate, within the sum of both bounds"""
    g = gauss[shape]
    B, Cn, M = shape
    pts = np.ascontiguousarray(np.broadcast_to(g["cand"][None], (B, M, 2)))
    ek, es, _ = env["ops"].guess_spread(dev(g["logits"]), dev(g["cen"]), dev(pts), (1.0,))
    for objective, other in (("score", es), ("km", ek)):
        _, _, exp = run(env, g["logits"], table_of(env, g["cand"], g["cen"], objective), maximize=objective == "score")
        bound = g["shared"]["score_bound" if objective == "score" else "km_bound"]
        diff = (exp - other).abs().cpu().numpy()
        assert (diff <= 2 * bound).all(), f"{objective}: {np.argwhere(~(diff <= 2 * bound))[:3]}"


def test_km_table_is_the_haversine_matrix(env):
    cen = S.centroids_of(2076, 2)
    cand = R.candidates_of(257, 2, cen)
    tab = table_of(env, cand, cen, "km")
    assert torch.equal(tab, env["ops"].haversine_matrix(dev(cand), dev(cen)))
    score = table_of(env, cand, cen, "score")
    assert torch.equal(score, 5000.0 * torch.exp(-tab / 1492.7)) or float((score - 5000.0 * torch.exp(-tab / 1492.7)).abs().max()) <= 5000 * 4 * G.EPS
    assert float(tab[4, 2076 // 2]) <= 1e-9 and float(score[4, 2076 // 2]) >= 5000.0 - 1e-8       # the candidate ON a centroid


# ================================================================================================================ the same bits
def test_same_bits_alone_in_a_batch_and_at_any_position(env):
    B, Cn, M = 17, 257, 65
    logits = dev(S.gaussian_logits(B, Cn, 12, 4.0))
    table = torch.rand((257, Cn), dtype=torch.float64, device=DEV) * 5000
    idx, val, exp = run(env, logits, table[:M].contiguous())
    for b in range(B):
        i1, v1, e1 = run(env, logits[b:b + 1].contiguous(), table[:M].contiguous())
        assert bits_equal(e1[0], exp[b]) and bits_equal(v1, val[b:b + 1]) and int(i1[0]) == int(idx[b]), f"row {b} alone differs"
    rolled = torch.roll(logits, 5, dims=0).contiguous()
    assert bits_equal(run(env, rolled, table[:M].contiguous())[2], torch.roll(exp, 5, dims=0)), "a row's bits depend on its position"
    wide = run(env, logits, table)[2]
    assert bits_equal(wide[:, :M], exp), "M = 65 against the first 65 of M = 257"
    back = run(env, logits, torch.flip(table, dims=(0,)).contiguous())[2]
    assert bits_equal(torch.flip(back, dims=(1,)), wide), "a candidate's bits depend on its position"


def test_same_bits_across_the_tile_size_switch(env):
    B, Cn = 17, 65
    ops = env["ops"]
    small = FORM1_M - ops.guess_best_plan(B, Cn, FORM1_M)["candidates_per_tile"]         # one candidate tile fewer: the other form
    assert ops.guess_best_plan(B, Cn, FORM1_M)["form"] == 1 and ops.guess_best_plan(B, Cn, small)["form"] == 0
    logits = dev(S.gaussian_logits(B, Cn, 13, 4.0))
    table = torch.rand((FORM1_M, Cn), dtype=torch.float64, device=DEV) * 5000
    i1, v1, e1 = run(env, logits, table)
    i0, v0, e0 = run(env, logits, table[:small].contiguous())
    assert bits_equal(e1[:, :small], e0), "the two tile sizes give different bits"
    want = first_best(e1.cpu().numpy(), True)
    assert (i1.cpu().numpy() == want).all() and bits_equal(v1, e1[torch.arange(B, device=DEV), dev(want)])
    assert (i0.cpu().numpy() == first_best(e0.cpu().numpy(), True)).all()


# ================================================================================================================ non-finite input
def test_non_finite_input_stays_in_its_row_and_column(env):
    B, Cn, M = 7, 65, 70
    cen = S.centroids_of(Cn, 5)
    cand = R.candidates_of(M, 5, cen)
    clean = S.gaussian_logits(B, Cn, 5)
    clean[6, 10:] = -np.inf                                          # masked cells: weight 0, an ordinary row
    for objective in R.OBJECTIVES:
        mx = objective == "score"
        ref = run(env, clean, table_of(env, cand, cen, objective), mx)
        logits = clean.copy()
        logits[1, 40] = np.nan
        logits[2, 0] = np.inf
        logits[3, :] = -np.inf
        bad_cand = cand.copy()
        bad_cand[33] = (np.nan, 10.0)
        bad_cand[66] = (20.0, np.inf)
        tab = table_of(env, bad_cand, cen, objective)
        assert bool(torch.isnan(tab[[33, 66]]).all()) and not bool(torch.isnan(tab[[32, 34, 65, 67]]).any())
        idx, val, exp = run(env, logits, tab, mx)
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        assert (idx[1:4] == -1).all() and np.isnan(val[1:4]).all() and bool(torch.isnan(exp[1:4]).all())
        good_rows, good_cols = [0, 4, 5, 6], [j for j in range(M) if j not in (33, 66)]
        assert bool(torch.isnan(exp[:, [33, 66]]).all()), "a NaN candidate has an expectation"
        assert bits_equal(exp[good_rows][:, good_cols], ref[2][good_rows][:, good_cols]), "a neighbour of a non-finite row or candidate changed"
        want = first_best(exp.cpu().numpy(), mx)
        assert (idx == want).all() and not np.isin(idx, (33, 66)).any()
        assert (val[good_rows] == exp.cpu().numpy()[good_rows, want[good_rows]]).all()
        every = run(env, clean, torch.full((M, Cn), float("nan"), dtype=torch.float64, device=DEV), mx)
        assert (every[0].cpu().numpy() == -1).all() and bool(torch.isnan(every[1]).all())       # every E is NaN: -1 / NaN


def test_front_end(env):
    ops = env["ops"]
    logits = dev(S.gaussian_logits(5, 65, 1))
    table = torch.rand((70, 65), dtype=torch.float64, device=DEV)
    i0, v0, e0 = run(env, logits, table)
    idx, val, exp = ops.guess_best(logits, table, return_expected=True)
    assert idx.dtype == torch.int64 and torch.equal(idx, i0.to(torch.int64)) and bits_equal(val, v0) and bits_equal(exp, e0)
    low = ops.guess_best(logits, table, maximize=False)
    assert len(low) == 2 and torch.equal(low[0], torch.from_numpy(first_best(e0.cpu().numpy(), False)).to(DEV))
    none = ops.guess_best(logits, table[:0].contiguous(), return_expected=True)
    assert (none[0] == -1).all() and bool(torch.isnan(none[1]).all()) and none[2].shape == (5, 0)
    empty = ops.guess_best(logits[:0].contiguous(), table)
    assert empty[0].shape == (0,) and empty[1].shape == (0,)
    assert ops.score_table(dev(np.zeros((0, 2))), dev(S.centroids_of(4, 0))).shape == (0, 4)
    for bad, word in (((logits.double(), table), "dtype"), ((logits, table.float()), "dtype"), ((logits, table[:, :64].contiguous()), "table"),
                      ((logits.t(), table), "contiguous"), ((logits.cpu(), table), "device tensor")):
        with pytest.raises(env["lib"].PigeonHipError, match=word):
            ops.guess_best(*bad)
    with pytest.raises(env["lib"].PigeonHipError, match="candidates"):
        ops.score_table(table, dev(S.centroids_of(4, 0)))
