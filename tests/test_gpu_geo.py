"""The geo tier (run with -m gpu on an MI355X): every element pg_haversine_matrix, pg_haversine_pairs, pg_smooth_labels and
pg_proto_build write, against the high-precision statements of tests/_georef.py -- longdouble truths with a derived per-element
bound (16 U for the distances), torch's CPU reduction bit for bit for the means -- at the shapes around the 256-wide blocks and on the
input families where a distance kernel goes wrong: identical and near points, the antimeridian, the poles, antipodes.
tests/test_georef_cpu.py pins those statements and shows that each comparison rejects the mistakes it is for.

The kernels are called through the C ABI with every output placed in front of sentinel elements, which must stay untouched; no input
may change.  No input is outside a kernel's contract."""
import time

import numpy as np
import pytest
import torch

import _georef as G

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32_CODE, BF16_CODE, F64_CODE = 0, 1, 3
MATRIX_SHAPES = [(1, 1), (3, 255), (2, 256), (5, 257), (70, 1000)]
PAIR_COUNTS = [1, 255, 256, 257, 5000]


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops, geo_utils
    _lib.require_gpu()
    assert (_lib.PG_DTYPE_F32, _lib.PG_DTYPE_BF16, _lib.PG_DTYPE_F64) == (F32_CODE, BF16_CODE, F64_CODE)
    return dict(lib=_lib, ops=hip_ops, L=_lib.load(), geo=geo_utils)


def guarded(n, dtype=torch.float64):
    return torch.full((n + G.GUARD,), G.SENTINEL, dtype=dtype, device=DEV)


def take(buf, n, what):
    """the n output elements of a guarded buffer (numpy); the sentinels behind them untouched"""
    torch.cuda.synchronize()
    assert bool((buf[n:] == G.SENTINEL).all()), f"{what}: wrote past its output"
    return buf[:n].cpu().numpy()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def raw_matrix(env, x, y):
    """x (N,2) fp32/fp64, y (M,2) fp64 numpy -> (N,M) fp64 numpy through pg_haversine_matrix"""
    ops, N, M = env["ops"], x.shape[0], y.shape[0]
    dx, dy, out = dev(x), dev(y), guarded(N * M)
    env["lib"].check(env["L"].pg_haversine_matrix(ops._p(dx), F64_CODE if x.dtype == np.float64 else F32_CODE, ops._p(dy), N, M,
                                                  ops._p(out), ops._stream()), "pg_haversine_matrix")
    got = take(out, N * M, f"haversine_matrix {N} x {M}").reshape(N, M)
    assert np.array_equal(dx.cpu().numpy(), x) and np.array_equal(dy.cpu().numpy(), y), "an input changed"
    return got


def raw_pairs(env, x, y):
    """x (N,2) fp64, y (N,2) fp32/fp64 numpy -> (N,) fp64 numpy through pg_haversine_pairs"""
    ops, N = env["ops"], x.shape[0]
    dx, dy, out = dev(x), dev(y), guarded(N)
    env["lib"].check(env["L"].pg_haversine_pairs(ops._p(dx), ops._p(dy), F64_CODE if y.dtype == np.float64 else F32_CODE, N,
                                                 ops._p(out), ops._stream()), "pg_haversine_pairs")
    got = take(out, N, f"haversine_pairs {N}")
    assert np.array_equal(dx.cpu().numpy(), x) and np.array_equal(dy.cpu().numpy(), y), "an input changed"
    return got


def report(capsys, title, worst):
    with capsys.disabled():
        print(f"\n{title}: " + ", ".join(f"{t} {v:.3g}" for t, v in worst.items()))


def rng_of(*key):
    return np.random.default_rng([2026, *key])


# ================================================================================================================ haversine, fp64
def test_matrix_f64(env, capsys):
    """pg_haversine_matrix, fp64 x: shapes (1,1), (3,255), (2,256), (5,257), (70,1000), each filled from every family in turn (column j
    is a partner of row j % N, so the family reaches the first and the last column).  Every element within 16 U of the longdouble
    truth, none NaN; the worst ratio per family printed.  geo_utils.haversine_matrix, given y as the strided (2,M) view SuperGuessr
    passes, returns the same bits."""
    worst, cross, found = dict.fromkeys(G.TAGS, 0.0), 0.0, []
    for si, (N, M) in enumerate(MATRIX_SHAPES):
        for ti, tag in enumerate(G.TAGS):
            x, y, fam = G.matrix_case(tag, N, M, rng_of(1, si, ti))
            got = raw_matrix(env, x, y)
            assert not np.isnan(got).any(), (tag, N, M)
            r = G.ratio(got, *G.haversine_truth(x[:, None, :], y[None, :, :]))
            worst[tag] = max(worst[tag], float(r[fam].max()))
            cross = max(cross, float(r[~fam].max())) if N > 1 else cross
            if r.max() > 16:
                i, j = np.unravel_index(int(r.argmax()), r.shape)
                found.append(f"{tag} ({N},{M}) element ({i},{j}): {r.max():.3g} U")
            y_view = dev(y).t()                                      # (2,M) with strides (1,2)
            assert M == 1 or not y_view.is_contiguous()
            via = env["geo"].haversine_matrix(dev(x), y_view)
            torch.cuda.synchronize()
            assert np.array_equal(via.cpu().numpy(), got), f"geo_utils.haversine_matrix differs from the raw call: {tag} ({N},{M})"
    report(capsys, f"pg_haversine_matrix fp64, worst |got - truth| / U per family (unrelated pairs {cross:.3g})", worst)
    assert not found, "\n".join(found)


def test_pairs_f64(env, capsys):
    """pg_haversine_pairs, fp64 y: N = 1, 255, 256, 257, 5000 of every family; within 16 U, none NaN."""
    worst, found = dict.fromkeys(G.TAGS, 0.0), []
    for ni, N in enumerate(PAIR_COUNTS):
        for ti, tag in enumerate(G.TAGS):
            rng = rng_of(2, ni, ti)
            x = G.anchors(tag, N, rng)
            y = G.partners(tag, x, rng)
            got = raw_pairs(env, x, y)
            assert not np.isnan(got).any(), (tag, N)
            r = G.ratio(got, *G.haversine_truth(x, y))
            worst[tag] = max(worst[tag], float(r.max()))
            if r.max() > 16:
                found.append(f"{tag} N = {N} element {int(r.argmax())}: {r.max():.3g} U")
    report(capsys, "pg_haversine_pairs fp64, worst |got - truth| / U per family", worst)
    assert not found, "\n".join(found)


def test_matrix_f64_self_distance_and_symmetry(env, capsys):
    """Stated properties of pg_haversine_matrix on a point set against itself (256 points: both ends of 8 pairs of every family).  The
    kernel's fused longitude difference leaves the rounding error of lng * pi/180 behind, so d(x, x) is about 1e-13 km, not 0, and
    D[i,j] and D[j,i] differ in the last bits (pg_haversine_blocks is built around both).  Bounded: d(x, x) <= 16 U, |D - D^T| <= 32 U."""
    x, y, _ = G.family_pairs(77, 8)
    pts = np.concatenate([x, y])
    D = raw_matrix(env, pts, pts)
    _, a = G.haversine_truth(pts[:, None, :], pts[None, :, :])
    u = G.U(a)
    diag, asym = np.diagonal(D), np.abs(D - D.T)
    with capsys.disabled():
        print(f"\npg_haversine_matrix on {len(pts)} points against themselves: largest d(x, x) {diag.max():.3g} km ({(diag / np.diagonal(u)).max():.3g} U), "
              f"{int((diag != 0).sum())} of {len(pts)} non-zero; largest |D[i,j] - D[j,i]| {asym.max():.3g} km ({(asym / u).max():.3g} U), "
              f"{int((asym != 0).sum() // 2)} asymmetric pairs")
    assert (diag >= 0).all() and (diag <= 16 * np.diagonal(u)).all()
    assert (asym <= 32 * u).all()


# ================================================================================================================ haversine, fp32 arms
def test_matrix_f32x(env, capsys):
    """haversine_matrix_kernel<float>: the fp32 point is x.  Against haversine_mixed_truth (fp32 deg2rad, correctly rounded fp32 cos of
    the latitude, the rest exact): within 16 U where the truth's a < 1 - 4 eps, NaN where a > 1 + 4 eps, either in between -- and that
    band holds at most 2 % of all elements."""
    worst, found, band, total, nans = dict.fromkeys(G.TAGS, 0.0), [], 0, 0, 0
    for si, (N, M) in enumerate(MATRIX_SHAPES):
        for ti, tag in enumerate(G.TAGS):
            x, y, fam = G.matrix_case(tag, N, M, rng_of(3, si, ti))
            x32 = x.astype(np.float32)
            got = raw_matrix(env, x32, y)
            bad, either, r = G.mixed_verdict(got, *G.haversine_mixed_truth(x32[:, None, :], y[None, :, :]))
            band, total, nans = band + int(either.sum()), total + got.size, nans + int(np.isnan(got).sum())
            worst[tag] = max(worst[tag], float(r[fam].max()))
            if bad.any():
                i, j = np.argwhere(bad)[0]
                found.append(f"{tag} ({N},{M}): {int(bad.sum())} elements, the first ({i},{j}) = {got[i, j]!r}, {r[i, j]:.3g} U")
    report(capsys, f"pg_haversine_matrix fp32 x, worst ratio per family ({nans} NaN, {band} of {total} elements = {band / total:.3%} in the either band)", worst)
    assert not found, "\n".join(found)
    assert band <= 0.02 * total


def test_pairs_f32y(env, capsys):
    """haversine_pairs_kernel<float>: the fp32 point is y.  The same three-way comparison."""
    worst, found, band, total, nans = dict.fromkeys(G.TAGS, 0.0), [], 0, 0, 0
    for ni, N in enumerate(PAIR_COUNTS):
        for ti, tag in enumerate(G.TAGS):
            rng = rng_of(4, ni, ti)
            x = G.anchors(tag, N, rng)
            y32 = G.partners(tag, x, rng).astype(np.float32)
            got = raw_pairs(env, x, y32)
            bad, either, r = G.mixed_verdict(got, *G.haversine_mixed_truth(y32, x))
            band, total, nans = band + int(either.sum()), total + got.size, nans + int(np.isnan(got).sum())
            worst[tag] = max(worst[tag], float(r.max()))
            if bad.any():
                i = int(np.flatnonzero(bad)[0])
                found.append(f"{tag} N = {N}: {int(bad.sum())} elements, the first {i} = {got[i]!r}, {r[i]:.3g} U")
    report(capsys, f"pg_haversine_pairs fp32 y, worst ratio per family ({nans} NaN, {band} of {total} elements = {band / total:.3%} in the either band)", worst)
    assert not found, "\n".join(found)
    assert nans > 0, "next to antipodes the contract's a exceeds 1"
    assert band <= 0.02 * total


# ================================================================================================================ refusals
def test_refusals_by_name(env):
    ops, L, Err = env["ops"], env["L"], env["lib"].PigeonHipError
    x = torch.zeros((65536, 2), dtype=torch.float64, device=DEV)
    y = torch.zeros((4, 2), dtype=torch.float64, device=DEV)
    out = guarded(65536 * 4)
    st = ops._stream()
    assert L.pg_haversine_matrix(ops._p(x), F64_CODE, ops._p(y), 65536, 4, ops._p(out), st) != 0
    assert b"at most 65535 rows" in L.pg_last_error()
    for code in (BF16_CODE, 2, 7, -1):
        assert L.pg_haversine_matrix(ops._p(x), code, ops._p(y), 4, 4, ops._p(out), st) != 0
        assert b"x dtype must be PG_DTYPE_F32 or PG_DTYPE_F64" in L.pg_last_error()
        assert L.pg_haversine_pairs(ops._p(y), ops._p(y), code, 4, ops._p(out), st) != 0
        assert b"y dtype must be PG_DTYPE_F32 or PG_DTYPE_F64" in L.pg_last_error()
    take(out, 65536 * 4, "a refused call")
    assert bool((out == G.SENTINEL).all()), "a refused call wrote"
    with pytest.raises(Err, match="at most 65535 rows"):
        ops.haversine_matrix(x, y)
    geo, host = env["geo"], torch.zeros((4, 2), dtype=torch.float64)
    with pytest.raises(Err, match="no CPU fallback"):
        geo.haversine_matrix(host, host.t())
    with pytest.raises(Err, match="no CPU fallback"):
        geo.haversine(host, host)
    with pytest.raises(Err, match="no CPU fallback"):
        geo.smooth_labels(host)
    with pytest.raises(Err, match="float64 expected"):
        geo.haversine_matrix(y, y.float().t())
    with pytest.raises(Err, match=r"y_rows must have shape \(\*,2\)"):
        ops.haversine_matrix(y, torch.zeros((4, 3), dtype=torch.float64, device=DEV))
    with pytest.raises(Err, match=r"x must have shape \(\*,2\)"):
        ops.haversine_matrix(torch.zeros((4, 3), dtype=torch.float64, device=DEV), y)
    with pytest.raises(Err, match="x must be fp32 or fp64"):
        ops.haversine_matrix(y.half(), y)
    with pytest.raises(Err, match="haversine_pairs: x"):
        ops.haversine_pairs(y, torch.zeros((5, 2), dtype=torch.float64, device=DEV))
    with pytest.raises(Err, match=r"\(N,M\) float64 distances expected"):
        geo.smooth_labels(torch.zeros(4, dtype=torch.float64, device=DEV))
    with pytest.raises(Err, match="expected dtype"):
        ops.smooth_labels(torch.zeros((2, 2), dtype=torch.float32, device=DEV), 65.0)


# ================================================================================================================ smooth labels
SMOOTH_M = [1, 63, 64, 65, 255, 256, 257, 1000]


def raw_smooth(env, d, c):
    ops, (N, M) = env["ops"], d.shape
    dd, out = dev(d), guarded(N * M)
    env["lib"].check(env["L"].pg_smooth_labels(ops._p(dd), N, M, float(c), ops._p(out), ops._stream()), "pg_smooth_labels")
    got = take(out, N * M, f"smooth_labels {N} x {M}").reshape(N, M)
    assert np.array_equal(dd.cpu().numpy(), d, equal_nan=True), "the input changed"
    return got


@pytest.mark.parametrize("c", [65.0, 1.0])
def test_smooth_labels(env, c, capsys):
    """Rows of real distances (0 .. 20 037 km) of length 1, 63 .. 65, 255 .. 257 and 1000, 1 and 70 of them, the row minimum in column 0,
    in the last column and in a column >= 256: within (4 + t) eps truth + 4 2^-1074 of the longdouble truth.  Constant 65 is the
    product's; with constant 1 most of a row underflows: entries with t > 745.2 must be exactly 0."""
    worst, found, zeros = 0.0, [], 0
    for mi, M in enumerate(SMOOTH_M):
        for N in (1, 70):
            for col in sorted({0, M - 1, min(M - 1, 300)}):
                d = G.smooth_inputs(rng_of(5, mi, N, col), N, M, col)
                assert (d.argmin(axis=1) == col).all()
                got = raw_smooth(env, d, c)
                r = G.smooth_ratio(got, d, c)
                worst = max(worst, float(r.max()))
                if r.max() > 1:
                    i, j = np.unravel_index(int(r.argmax()), r.shape)
                    found.append(f"({N},{M}) minimum in column {col}, element ({i},{j}): {r.max():.3g} of the bound")
                _, t = G.smooth_truth(d, c)
                assert (got[t > 745.2] == 0).all(), (N, M, col)
                assert (got[np.arange(N), col] == 1).all()
                zeros += int((t > 745.2).sum())
    with capsys.disabled():
        print(f"\npg_smooth_labels constant {c:g}: worst {worst:.3g} of the bound; {zeros} entries past t = 745.2")
    assert not found, "\n".join(found)
    assert zeros > 0 if c == 1.0 else zeros == 0


def test_smooth_labels_special_rows(env):
    """A NaN at column 0, at the last column or past column 256 zeroes its whole row; an all-+inf row and a row holding -inf are all 0:
    equal to the oracle's torch statement.  A +inf entry is 0 in place -- the zeros are the oracle's -- and leaves the rest of its row
    alone: the finite entries are within the smooth bound of their own truth, as are the ordinary rows next to the special ones (two
    exp implementations differ in the last bit, so those entries are not compared for equality)."""
    from oracle import geo_oracle
    for M in SMOOTH_M:
        named = G.special_rows(M)
        ordinary = G.smooth_inputs(rng_of(6, M), 3, M, M // 2)
        d = np.concatenate([ordinary[:1], np.stack([r for _, r in named]), ordinary[1:]])
        got = raw_smooth(env, d, 65.0)
        want = geo_oracle.smooth_labels(torch.from_numpy(d), 65.0).numpy()
        for k, (name, _) in enumerate(named, start=1):
            if name == "posinf" and M > 1:
                col = M // 2
                assert got[k, col] == 0 and np.array_equal(got[k] == 0, want[k] == 0), f"M = {M}: row {name}"
                rest = np.delete(np.arange(M), col)
                assert (got[k, rest] > 0).all() and got[k, 0] == 1
                assert G.smooth_ratio(got[k:k + 1, rest], d[k:k + 1, rest], 65.0).max() <= 1, f"M = {M}: row {name}, the finite entries"
            else:
                assert (want[k] == 0).all() and np.array_equal(got[k], want[k]), f"M = {M}: row {name}"
        keep = [0, len(d) - 2, len(d) - 1]
        assert G.smooth_ratio(got[keep], d[keep], 65.0).max() <= 1, f"M = {M}: an ordinary row next to the special ones"


# ================================================================================================================ prototype means
COUNTS = [0, 1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, 4095, 4096, 4097]


def raw_proto(env, bank, off, idx):
    """bank (Ntr,1024) or (Ntr,4,1024) fp32, CSR member lists -> (P,1024) fp32 through pg_proto_build"""
    ops, P = env["ops"], len(off) - 1
    panels = 1 if bank.ndim == 2 else bank.shape[1]
    db, doff, didx, out = dev(bank), dev(off), dev(idx), guarded(P * 1024, torch.float32)
    env["lib"].check(env["L"].pg_proto_build(ops._p(db), panels, bank.shape[0], ops._p(doff), ops._p(didx), P, ops._p(out),
                                             ops._stream()), "pg_proto_build")
    got = take(out, P * 1024, f"proto_build {P} prototypes").reshape(P, 1024)
    assert np.array_equal(db.cpu().numpy(), bank) and np.array_equal(didx.cpu().numpy(), idx) and np.array_equal(doff.cpu().numpy(), off)
    return got


@pytest.mark.parametrize("panels", [1, 4])
def test_proto_means(env, panels):
    """Member counts around every chunk boundary of torch's cascade sum up to its third level (16 rows, 256, 4096), 0 .. 4097 members
    in one call, member lists with repeats, a bank of randn * 10^U(-3,3) so that the order of the additions shows in the bits: equal
    to torch's mean(dim=1).mean(dim=0) on the CPU and to its restatement _georef.cascade_mean.  No members: zeros."""
    rng = rng_of(7, panels)
    bank = G.wide_rows(rng, (300, 1024) if panels == 1 else (300, 4, 1024))
    counts = [COUNTS[i] for i in rng.permutation(len(COUNTS))]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    idx = rng.integers(0, 300, int(off[-1])).astype(np.int64)
    got = raw_proto(env, bank, off, idx)
    t = torch.from_numpy(bank)
    flat = bank if panels == 1 else G.panel_mean(bank)
    for p, n in enumerate(counts):
        ix = idx[off[p]:off[p + 1]]
        assert np.array_equal(got[p], G.cascade_mean(flat, ix)), f"{n} members: differs from cascade_mean"
        if n == 0:
            assert (got[p] == 0).all()
            continue
        rows = t[torch.from_numpy(ix)]
        want = (rows.mean(dim=1) if panels == 4 else rows).mean(dim=0).numpy()
        assert np.array_equal(got[p], want), f"{n} members: differs from torch"
        if n >= 32:
            assert not np.array_equal(got[p], G.ordered_mean(flat, ix)), f"{n} members: the inputs do not tell the orders apart"


def test_proto_mean_524289_members(env, capsys):
    """One prototype of 524 289 members gathered from a 500-row bank: above 524 288 torch's chunk grows from 16 to 32 rows
    (level_power 5).  One block reads all of them; the wall time is printed.  Compared on a 64-column slice (the CPU statements give
    the same bits on a slice as on the full width, tests/test_georef_cpu.py)."""
    n = 524289
    assert G.ceil_log2(n) // 4 == 5 and G.ceil_log2(n - 1) // 4 == 4
    rng = rng_of(8)
    bank = G.wide_rows(rng, (500, 1024))
    idx = rng.integers(0, 500, n).astype(np.int64)
    off = np.array([0, n], dtype=np.int64)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    got = raw_proto(env, bank, off, idx)
    wall = time.perf_counter() - t0
    with capsys.disabled():
        print(f"\npg_proto_build, one prototype of {n} members: {wall:.3f} s wall (upload, kernel, download)")
    cols = slice(192, 256)
    narrow = np.ascontiguousarray(bank[:, cols])
    want = torch.from_numpy(narrow)[torch.from_numpy(idx)].mean(dim=0).numpy()
    assert np.array_equal(got[0, cols], want), "differs from torch"
    assert np.array_equal(got[0, cols], G.cascade_mean(narrow, idx)), "differs from cascade_mean"
    assert not np.array_equal(got[0, cols], G.ordered_mean(narrow, idx))
