"""pg_guess_spread on the GPU (run with -m gpu on an MI355X), through the C ABI, against tests/_spreadref.py: the numpy restatement of
the contract with derived bounds, and the tight / loose rule for the quantiles (at most 1 % loose, asserted; the inputs show 0).

Where the weights are exact (logits of 0 and -inf only) nothing is approximate: a radius must be pg_haversine_matrix's float64 value
for the answer cell plus the extent, one fp64 addition, bit for bit -- the test that fails if spread.hip and geo_proto.hip stop sharing
csrc/haversine.h.  Every output sits between guard regions that must keep their pattern, and no input may change."""
import math

import numpy as np
import pytest
import torch

import _georef as G
import _spreadref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
SMALL_C = (1, 2, 63, 64, 65, 257, 2076)
WORST = {"ratio": 0.0}


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops
    _lib.require_gpu()
    plan = hip_ops.guess_spread_plan(1)
    return dict(lib=_lib, ops=hip_ops, L=_lib.load(), top=plan["lds_cells"])


def all_c(env):
    return SMALL_C + (env["top"], env["top"] + 1)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(n):
    buf = torch.full((n + 2 * G.GUARD,), G.SENTINEL, dtype=torch.float64, device=DEV)
    return buf, buf[G.GUARD:G.GUARD + n]


def run(env, logits, cen, pts, qs, ext=None):
    """numpy in -> (expected_km (B,G), expected_score (B,G), radius_km (B,G,nq)) device tensors, through the C ABI; guards checked"""
    import ctypes as C
    ops = env["ops"]
    B, Cn = logits.shape
    pts = np.asarray(pts, dtype=np.float64).reshape(B, -1, 2)
    Gn, nq = pts.shape[1], len(qs)
    ins = [dev(logits), dev(cen), dev(pts)] + ([dev(ext)] if ext is not None else [])
    keep = [t.clone() for t in ins]
    bufs = [guarded(B * Gn), guarded(B * Gn), guarded(B * Gn * nq)]
    q = (C.c_double * nq)(*[float(v) for v in qs])
    env["lib"].check(env["L"].pg_guess_spread(ops._p(ins[0]), B, Cn, ops._p(ins[1]), ops._p(ins[3] if ext is not None else None),
                                              ops._p(ins[2]), Gn, q, nq, ops._p(bufs[0][1]), ops._p(bufs[1][1]), ops._p(bufs[2][1]),
                                              ops._stream()), "pg_guess_spread")
    torch.cuda.synchronize()
    for (buf, view), name in zip(bufs, ("expected_km", "expected_score", "radius_km")):
        n = view.numel()
        assert bool((buf[:G.GUARD] == G.SENTINEL).all()) and bool((buf[G.GUARD + n:] == G.SENTINEL).all()), f"{name}: wrote outside its output"
    for t, k in zip(ins, keep):
        assert torch.equal(t.view(torch.uint8), k.view(torch.uint8)), "an input changed"
    return bufs[0][1].clone().reshape(B, Gn), bufs[1][1].clone().reshape(B, Gn), bufs[2][1].clone().reshape(B, Gn, nq)


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def held(env, capsys, logits, cen, pts, qs, ext=None, what=""):
    got = run(env, logits, cen, pts, qs, ext)
    t = S.truth(logits, cen, pts, qs, ext)
    errors, loose, worst = S.compare(t, *(g.cpu().numpy() for g in got))
    WORST["ratio"] = max(WORST["ratio"], worst)
    with capsys.disabled():
        print(f"\nguess_spread {what}: worst |got - truth| / bound {worst:.3g}, {loose} loose of {t['tight'].size} quantiles "
              f"(worst so far {WORST['ratio']:.3g})")
    assert not errors, errors[:5]
    assert loose <= S.loose_allowed(t), f"{loose} loose quantiles of {t['tight'].size}"
    return got, t


# ================================================================================================================ exact weights
def test_exact_weights_radius_is_the_matrix_element(env):
    """logits of 0 / -inf: weights 1 / 0, every mass an exact integer.  radius == pg_haversine_matrix(point, answer cell) + extent"""
    for Cn in all_c(env):
        rng = np.random.default_rng([77, Cn])
        B, Gn = 3, 2
        live = max(1, (2 * Cn) // 3)
        logits = np.full((B, Cn), -np.inf, dtype=np.float32)
        for b in range(B):
            logits[b, rng.permutation(Cn)[:live]] = 0.0
        cen, pts, ext = S.centroids_of(Cn, 1), S.points_of(B, Gn, Cn), S.extents_of(Cn, 2)
        q = S.uniform_quantile(live)
        rank = math.ceil(q * live) - 1                               # the answer among the live cells' sorted keys
        d = env["ops"].haversine_matrix(dev(pts.reshape(-1, 2)), dev(cen)).reshape(B, Gn, Cn)
        for extent in (None, ext):
            key = d if extent is None else d + dev(extent)           # one fp64 addition
            _, _, rk = run(env, logits, cen, pts, (q, 1.0), extent)
            masked = torch.where(dev(logits)[:, None, :] == 0, key, torch.full_like(key, float("inf")))
            want = torch.sort(masked, dim=-1).values
            assert bits_equal(rk[..., 0], want[..., rank]), f"C = {Cn}, q = {q}: not the matrix element of the answer cell"
            assert bits_equal(rk[..., 1], want[..., live - 1]), f"C = {Cn}, q = 1: not the farthest live cell's"


def test_lds_and_scratch_forms_give_the_same_bits(env, capsys):
    """the largest LDS-form C against one cell more, that cell masked: its thread adds one +0.0, every other addition is the same"""
    top = env["top"]
    assert env["ops"].guess_spread_plan(top)["form"] == 0 and env["ops"].guess_spread_plan(top + 1)["form"] == 1
    B, Gn, qs = 3, 2, (0.5, 0.9, 1.0)
    logits = S.gaussian_logits(B, top + 1, 4)
    logits[:, top] = -np.inf
    cen, pts, ext = S.centroids_of(top + 1, 4), S.points_of(B, Gn, 4), S.extents_of(top + 1, 4)
    big, _ = held(env, capsys, logits, cen, pts, qs, ext, f"C = {top + 1} (scratch)")
    small, _ = held(env, capsys, np.ascontiguousarray(logits[:, :top]), cen[:top], pts, qs, ext[:top], f"C = {top} (LDS)")
    for a, b, name in zip(big, small, ("expected_km", "expected_score", "radius_km")):
        assert bits_equal(a, b), f"{name}: the LDS form and the scratch form differ"


# ================================================================================================================ the comparator
@pytest.mark.parametrize("B,Gn,nq", [(1, 1, 1), (3, 2, 2), (17, 1, 4)])
def test_gaussian_logits_under_the_comparator(env, capsys, B, Gn, nq):
    qs = (0.5, 0.9, 1.0, 0.25)[:nq]
    for Cn in all_c(env):
        for extent in ((None, S.extents_of(Cn, 3)) if Cn in (65, 2076, env["top"] + 1) else (None,)):
            held(env, capsys, S.gaussian_logits(B, Cn, 0), S.centroids_of(Cn, 0), S.points_of(B, Gn, 0), qs, extent,
                 f"C = {Cn}, B = {B}, G = {Gn}, nq = {nq}" + (", extents" if extent is not None else ""))


def test_antimeridian_poles_and_a_centroid(env, capsys):
    Cn = 257
    cen = S.centroids_of(Cn, 6)
    cen[0], cen[1], cen[2], cen[3] = (180.0, 10.0), (-180.0, -20.0), (33.0, 90.0), (-70.0, -90.0)
    pts = np.array([[[180.0, 10.5], [-179.99999, 10.0]], [[-180.0, -20.0], [179.9999999, 0.0]], [[12.0, 90.0], [-140.0, -90.0]],
                    [cen[40], cen[2]]])
    logits = S.gaussian_logits(4, Cn, 6)
    logits[3, 40] = 30.0                                             # a confident head asked about its own centroid
    (ek, es, rk), t = held(env, capsys, logits, cen, pts, (0.5, 0.9), None, "antimeridian, poles, on a centroid")
    assert t["cell"][3, 0, 0] == 40 and float(rk[3, 0, 0]) < 1e-9   # radius 0, to the distance kernel's rounding


# ================================================================================================================ stated properties
def test_one_dominant_cell(env):
    for Cn in (65, 2076, env["top"] + 1):
        logits = np.full((2, Cn), -100.0, dtype=np.float32)
        logits[0, 7], logits[1, Cn - 1] = 0.0, 0.0
        cen, pts = S.centroids_of(Cn, 8), S.points_of(2, 2, 8)
        d = env["ops"].haversine_matrix(dev(pts.reshape(-1, 2)), dev(cen)).reshape(2, 2, Cn)
        ek, es, rk = run(env, logits, cen, pts, (0.01, 0.5, 0.999, 1.0))
        for b, cell in ((0, 7), (1, Cn - 1)):
            want = d[b, :, cell]
            assert bits_equal(rk[b], want[:, None].expand(2, 4).contiguous()), f"C = {Cn}: a radius is not the dominant cell's key"
            assert bool(((ek[b] - want).abs() <= 4 * G.EPS * want).all()), f"C = {Cn}: expected_km is not the dominant cell's distance"


def test_integer_logits_shifted_by_a_constant_give_the_same_bits(env):
    for Cn in (64, 2076):
        rng = np.random.default_rng([9, Cn])
        logits = rng.integers(-8, 9, (3, Cn)).astype(np.float32)
        cen, pts, ext = S.centroids_of(Cn, 9), S.points_of(3, 2, 9), S.extents_of(Cn, 9)
        a = run(env, logits, cen, pts, (0.5, 0.9), ext)
        b = run(env, logits + np.float32(37), cen, pts, (0.5, 0.9), ext)
        c = run(env, logits - np.float32(1000), cen, pts, (0.5, 0.9), ext)
        assert all(bits_equal(x, y) and bits_equal(x, z) for x, y, z in zip(a, b, c))


def test_a_row_is_the_same_bits_alone_at_every_position_and_as_either_point(env):
    qs = (0.5, 0.9, 1.0)
    for Cn in (65, 2076, env["top"] + 1):                            # odd C: the row's alignment changes with its position
        cen, ext = S.centroids_of(Cn, 10), S.extents_of(Cn, 10)
        row, other = S.gaussian_logits(1, Cn, 10), S.gaussian_logits(17, Cn, 11)
        p, po = S.points_of(1, 1, 10), S.points_of(17, 2, 11)
        alone = run(env, row, cen, p, qs, ext)
        same = run(env, np.repeat(row, 17, axis=0), cen, np.repeat(p, 17, axis=0), qs, ext)       # every position at once
        for a, s in zip(alone, same):
            assert bits_equal(s, a.expand_as(s).contiguous()), f"C = {Cn}: a position of B = 17 differs from the row alone"
        for pos in (0, 8, 16):                                       # among other rows, as the first and as the second point
            logits = other.copy(); logits[pos] = row[0]
            for g in (0, 1):
                pts = po.copy(); pts[pos, g] = p[0, 0]
                got = run(env, logits, cen, pts, qs, ext)
                for a, s in zip(alone, got):
                    assert bits_equal(s[pos, g], a[0, 0]), f"C = {Cn}: position {pos}, point {g} differs from the row alone"


def test_non_finite_input_stays_in_its_row_and_point(env, capsys):
    Cn, qs = 257, (0.5, 1.0)
    cen, ext = S.centroids_of(Cn, 12), S.extents_of(Cn, 12)
    logits, pts = S.gaussian_logits(6, Cn, 12), S.points_of(6, 2, 12)
    clean = run(env, logits, cen, pts, qs, ext)
    logits[1, 200] = np.nan
    logits[2, 0] = np.inf
    logits[3, :] = -np.inf
    logits[4, 5:50] = -np.inf                                        # masked cells: an ordinary row
    pts[5, 1, 0] = np.nan
    pts[0, 0, 1] = np.inf
    (ek, es, rk), t = held(env, capsys, logits, cen, pts, qs, ext, "NaN rows between intact neighbours")
    nan = torch.isnan(ek).cpu().numpy()
    assert nan.tolist() == [[True, False], [True, True], [True, True], [True, True], [False, False], [False, True]]
    assert bool(torch.isnan(rk[torch.isnan(ek)]).all()) and bool(torch.isnan(es[torch.isnan(ek)]).all())
    for a, c in zip((ek, es, rk), clean):                            # the intact (row, point)s: the bits of the clean batch
        assert bits_equal(a[0, 1], c[0, 1]) and bits_equal(a[5, 0], c[5, 0])
    # centroids and extents reach every row
    for bad_cen, bad_ext in ((np.nan, None), (None, np.inf), (None, np.nan), (None, -1e9)):
        c2, e2 = cen.copy(), ext.copy()
        if bad_cen is not None:
            c2[Cn - 1, 1] = bad_cen
        if bad_ext is not None:
            e2[3] = bad_ext
        got = run(env, S.gaussian_logits(2, Cn, 12), c2, S.points_of(2, 1, 12), qs, e2)
        assert all(bool(torch.isnan(g).all()) for g in got)


def test_front_end_shapes_and_names(env):
    ops, lib = env["ops"], env["lib"]
    Cn = 65
    logits, cen, pts = dev(S.gaussian_logits(3, Cn, 1)), dev(S.centroids_of(Cn, 1)), dev(S.points_of(3, 2, 1))
    ek, es, rk = ops.guess_spread(logits, cen, pts, (0.5, 0.9))
    assert ek.shape == (3, 2) and es.shape == (3, 2) and rk.shape == (3, 2, 2)
    ek1, es1, rk1 = ops.guess_spread(logits, cen, pts[:, 0].contiguous(), (0.5, 0.9))
    assert ek1.shape == (3,) and rk1.shape == (3, 2) and bits_equal(ek1, ek[:, 0]) and bits_equal(rk1, rk[:, 0])
    raw = run(env, logits.cpu().numpy(), cen.cpu().numpy(), pts.cpu().numpy(), (0.5, 0.9))
    assert bits_equal(ek, raw[0]) and bits_equal(es, raw[1]) and bits_equal(rk, raw[2])
    empty = ops.guess_spread(logits[:0], cen, pts[:0], (0.5,))
    assert empty[0].shape == (0, 2) and empty[2].shape == (0, 2, 1)
    for bad, word in ((dict(logits=logits.double()), "dtype"), (dict(cen=cen[:-1]), "centroids"), (dict(pts=pts[:2]), "points"),
                      (dict(pts=pts.float()), "dtype"), (dict(ext=torch.zeros(Cn - 1, dtype=torch.float64, device=DEV)), "extent_km"),
                      (dict(cen=cen.cpu()), "device"), (dict(logits=logits.t().contiguous().t()), "contiguous"),
                      (dict(qs=()), "quantiles"), (dict(qs=(0.1,) * 5), "quantiles"), (dict(qs=(0.0,)), "quantiles[0]")):
        kw = dict(logits=logits, cen=cen, pts=pts, ext=None, qs=(0.5,))
        kw.update(bad)
        with pytest.raises(lib.PigeonHipError, match=word.replace("[", r"\[").replace("]", r"\]")):
            ops.guess_spread(kw["logits"], kw["cen"], kw["pts"], kw["qs"], extent_km=kw["ext"])
