"""tests/_georef.py pinned, without a GPU: the longdouble truths against mpmath at 50 digits, the oracle's fp64 functions and the
recorded reference outputs against the truths, cascade_mean against torch's own reduction bit for bit -- and every comparison the GPU
tier (tests/test_gpu_geo.py) makes shown to reject the mistakes it is there for, on numpy stand-ins of the kernels."""
import os

import numpy as np
import pytest
import torch

import _georef as G
from oracle import geo_oracle

LD = np.longdouble
PER_TAG = 60


@pytest.fixture(scope="module")
def pairs():
    x, y, tags = G.family_pairs(2026, PER_TAG)
    return dict(x=x, y=y, tags=tags, truth=G.haversine_truth(x, y), mixed_x=G.haversine_mixed_truth(x.astype(np.float32), y),
                mixed_y=G.haversine_mixed_truth(y.astype(np.float32), x))


def per_family(tags, r):
    return {t: float(np.max(r[tags == t])) for t in G.TAGS}


def show(capsys, title, worst):
    with capsys.disabled():
        print(f"\n{title}: " + ", ".join(f"{t} {v:.3g}" for t, v in worst.items()))


# ================================================================================================================ the truths
def _mpf(mp, v):
    hi = float(v)
    return mp.mpf(hi) + mp.mpf(float(LD(v) - LD(hi)))


def test_truths_agree_with_mpmath(pairs, capsys):
    """Both truths against the textbook formula evaluated by mpmath at 50 digits (an independent form: asin(sqrt a) with the product of
    cosines): below 0.01 U on every family, `a` to 1e-17, NaN exactly where mpmath's a exceeds 1."""
    mp = pytest.importorskip("mpmath")
    with mp.workdps(50):
        k = mp.mpf(G.PI180_DIGITS)
        R2 = 2 * mp.mpf("6378.137")
        x, y, tags = pairs["x"], pairs["y"], pairs["tags"]
        assert abs(_mpf(mp, G.PI180) - k) < mp.mpf(2) ** -68 and abs(k - mp.pi / 180) < mp.mpf(10) ** -49

        def dist(plng, plat, cosp, qlng, qlat, sphere=False):
            a = mp.sin((plat - qlat) / 2) ** 2 + cosp * mp.cos(qlat) * mp.sin((plng - qlng) / 2) ** 2
            if sphere:                                               # on the sphere a <= 1; 50 digits leave 1e-50 at exact antipodes
                assert a < 1 + mp.mpf(10) ** -45
                a = min(a, mp.mpf(1))
            return (R2 * mp.asin(mp.sqrt(a)) if a <= 1 else None), a

        r64, r32 = np.zeros(len(x)), np.zeros(len(x))
        d, a = pairs["truth"]
        dm, am = pairs["mixed_x"]
        p32 = x.astype(np.float32) * G.DEG2RAD_F32
        nans = 0
        for i in range(len(x)):
            xl, xp, yl, yp = (mp.mpf(float(v)) * k for v in (x[i, 0], x[i, 1], y[i, 0], y[i, 1]))
            want, wa = dist(xl, xp, mp.cos(xp), yl, yp, sphere=True)
            assert abs(_mpf(mp, a[i]) - wa) < 1e-17
            r64[i] = float(abs(_mpf(mp, d[i]) - want) / mp.mpf(float(G.U(float(wa)))))
            pl, pp = mp.mpf(float(p32[i, 0])), mp.mpf(float(p32[i, 1]))
            want, wa = dist(pl, pp, mp.mpf(float(np.float32(float(mp.cos(pp))))), yl, yp)
            assert abs(_mpf(mp, am[i]) - wa) < 1e-17
            if want is None:
                nans += 1
                assert np.isnan(dm[i]), (tags[i], i)
            elif wa < 1 - 4 * G.EPS:
                r32[i] = float(abs(_mpf(mp, dm[i]) - want) / mp.mpf(float(G.U(float(wa)))))
    show(capsys, "longdouble truth vs mpmath, fp64 [U]", per_family(tags, r64))
    show(capsys, f"longdouble truth vs mpmath, mixed ({nans} NaN) [U]", per_family(tags, r32))
    assert r64.max() < 0.01 and r32.max() < 0.01
    assert nans > 0, "the mixed contract's a exceeds 1 next to antipodes"


def test_families(pairs):
    x, y, tags = pairs["x"], pairs["y"], pairs["tags"]
    assert x.dtype == y.dtype == np.float64 and x.shape == y.shape == (len(G.TAGS) * PER_TAG, 2)
    assert (np.abs(x[:, 1]) <= 90).all() and (np.abs(x[:, 0]) <= 180).all()
    f = lambda t: (x[tags == t], y[tags == t])
    a, b = f("identical"); assert np.array_equal(a, b)
    a, b = f("antimeridian"); assert (a[:, 0] > 179.99).all() and (b[:, 0] < -179.99).all() and (a[:, 0] < 180).all()
    a, b = f("antimeridian_180"); assert (a[:, 0] == 180).all() and (b[:, 0] == -180).all() and np.array_equal(a[:, 1], b[:, 1])
    a, b = f("poles"); assert (np.abs(a[:, 1]) == 90).all() and (np.abs(b[::4, 1]) == 90).all() and (b[8::16, 1] == -a[8::16, 1]).all()
    a, b = f("origin"); assert (a == 0).all() and (b[0] == 0).all()
    a, b = f("antipode"); assert (np.abs(a[:, 0] - b[:, 0]) == 180).all() and np.array_equal(a[:, 1], -b[:, 1])
    d, _ = pairs["truth"]
    assert (d[tags == "identical"] == 0).all() and (d[tags == "antimeridian_180"] < 1e-15).all()
    assert np.allclose(d[tags == "antipode"].astype(np.float64), np.pi * G.R_KM, rtol=1e-15)
    x2, y2, fam = G.matrix_case("near_1e-07", 5, 257, np.random.default_rng(0))
    assert fam[0, 0] and fam[256 % 5, 256] and fam.sum() == 257 and np.abs(x2[np.arange(257) % 5] - y2).max() < 1e-5


# ================================================================================================================ the references
def test_oracle_and_golden_within_bound(pairs, golden_dir, capsys):
    """oracle/geo_oracle.py's three fp64 functions on every family, and the reference's own recorded outputs (tests/golden/geo.npz):
    within 16 U of the truth.  What the plain fp64 formula reaches is printed (about 3 U)."""
    x, y, tags = pairs["x"], pairs["y"], pairs["tags"]
    d, a = pairs["truth"]
    tx, ty = torch.from_numpy(x), torch.from_numpy(y)
    for name, got in (("haversine_np", geo_oracle.haversine_np(x, y)), ("haversine", geo_oracle.haversine(tx, ty).numpy())):
        assert got.dtype == np.float64
        r = G.ratio(got, d, a)
        show(capsys, f"oracle {name} vs truth [U]", per_family(tags, r))
        assert r.max() <= 16
    worst = {}
    for t in G.TAGS:
        xm, ym, _ = G.matrix_case(t, 5, 257, np.random.default_rng(7))
        got = geo_oracle.haversine_matrix(torch.from_numpy(xm), torch.from_numpy(ym).t()).numpy()
        worst[t] = float(G.ratio(got, *G.haversine_truth(xm[:, None, :], ym[None, :, :])).max())
    show(capsys, "oracle haversine_matrix vs truth [U]", worst)
    assert max(worst.values()) <= 16
    g = np.load(os.path.join(golden_dir, "geo.npz"))
    gx, gy = g["x"], g["y"]
    rm = G.ratio(g["matrix_f64"], *G.haversine_truth(gx[:, None, :], gy[None, :, :]))
    rp = G.ratio(g["pairs_f64y"], *G.haversine_truth(gx, gy[:len(gx)]))
    with capsys.disabled():
        print(f"\nrecorded reference outputs vs truth [U]: matrix {rm.max():.3g}, pairs {rp.max():.3g}")
    assert rm.max() <= 16 and rp.max() <= 16


def test_oracle_smooth_labels_within_bound(golden_dir, capsys):
    rng = np.random.default_rng(5)
    worst = 0.0
    for c in (65.0, 1.0):
        for M, col in ((1, 0), (65, 64), (1000, 300)):
            d = G.smooth_inputs(rng, 7, M, col)
            got = geo_oracle.smooth_labels(torch.from_numpy(d), c).numpy()
            worst = max(worst, float(G.smooth_ratio(got, d, c).max()))
            if c == 1.0:
                _, t = G.smooth_truth(d, c)
                assert (got[t > 745.2] == 0).all()
    g = np.load(os.path.join(golden_dir, "geo.npz"))
    finite = np.isfinite(g["smooth_in"]).all(axis=1)
    worst = max(worst, float(G.smooth_ratio(g["smooth_out"][finite], g["smooth_in"][finite], float(g["smooth_constant"])).max()))
    with capsys.disabled():
        print(f"\noracle smooth_labels vs truth: {worst:.3g} of the bound")
    assert finite.any() and worst <= 1


@pytest.mark.parametrize("n", [15, 16, 17, 255, 256, 257, 4095, 4096, 4097, 65537])
def test_cascade_mean_is_torch_mean(n):
    rows = G.wide_rows(np.random.default_rng(n), (n, 1024))
    want = torch.from_numpy(rows).mean(dim=0).numpy()
    assert np.array_equal(G.cascade_mean(rows), want)
    assert np.array_equal(G.cascade_mean(np.ascontiguousarray(rows[:, 64:128])), want[64:128]), "a 64-column slice: the same bits"
    assert np.array_equal(torch.from_numpy(np.ascontiguousarray(rows[:, 64:128])).mean(dim=0).numpy(), want[64:128])


@pytest.mark.parametrize("n", [524288, 524289, 1048577])
def test_cascade_mean_is_torch_mean_gathered(n):
    """level_power 4 at 524 288 members, 5 above: gathers from a 500-row bank"""
    rng = np.random.default_rng(n)
    bank = G.wide_rows(rng, (500, 1024))
    idx = rng.integers(0, 500, n)
    assert G.ceil_log2(n) // 4 == (4 if n == 524288 else 5)
    want = torch.from_numpy(bank)[torch.from_numpy(idx)].mean(dim=0).numpy()
    assert np.array_equal(G.cascade_mean(bank, idx), want)
    narrow = np.ascontiguousarray(bank[:, :64])
    assert np.array_equal(G.cascade_mean(narrow, idx), want[:64])
    assert np.array_equal(torch.from_numpy(narrow)[torch.from_numpy(idx)].mean(dim=0).numpy(), want[:64])


def test_panel_mean_is_torch_mean():
    b = G.wide_rows(np.random.default_rng(4), (300, 4, 1024))
    assert np.array_equal(G.panel_mean(b), torch.from_numpy(b).mean(dim=1).numpy())


def test_cascade_mean_small_counts():
    rows = G.wide_rows(np.random.default_rng(3), (40, 1024))
    assert np.array_equal(G.cascade_mean(rows[:0]), np.zeros(1024, np.float32))
    for n in (1, 2, 3, 31, 32, 33):
        assert np.array_equal(G.cascade_mean(rows, np.arange(n)[::-1]), torch.from_numpy(rows[:n][::-1].copy()).mean(dim=0).numpy()), n


# ================================================================================================================ planted mistakes
def standin_f64(x, y, mutant=None):
    """the fp64 arms as numpy would compute them (x - y for the matrix kernel; the pairs kernel's y - x has the same squares)"""
    if mutant == "swapped":
        x, y = x[..., ::-1], y[..., ::-1]
    xr, yr = np.deg2rad(x), np.deg2rad(y)
    p = np.cos(xr[..., 1]) ** 2 if mutant == "cos_squared" else np.cos(xr[..., 1]) * np.cos(yr[..., 1])
    a = np.sin((xr[..., 1] - yr[..., 1]) / 2) ** 2 + p * np.sin((xr[..., 0] - yr[..., 0]) / 2) ** 2
    with np.errstate(invalid="ignore"):
        return ((6371000.0 if mutant == "R6371" else 6378137.0) * (2 * np.arcsin(np.sqrt(a)))) / 1000


def standin_mixed(p32, q, mutant=None):
    """the fp32 arms in plain float64 after the fp32 steps"""
    assert p32.dtype == np.float32 and q.dtype == np.float64
    pr = p32.astype(np.float64) * float(G.PI180) if mutant == "deg2rad64" else (p32 * G.DEG2RAD_F32).astype(np.float64)
    cosp = np.cos(pr[..., 1]) if mutant == "cos64" else np.cos(pr[..., 1]).astype(np.float32).astype(np.float64)
    qr = q * float(G.PI180)
    a = np.sin((pr[..., 1] - qr[..., 1]) / 2) ** 2 + cosp * np.cos(qr[..., 1]) * np.sin((pr[..., 0] - qr[..., 0]) / 2) ** 2
    with np.errstate(invalid="ignore"):
        return (6378137.0 * (2 * np.arcsin(np.sqrt(a)))) / 1000


def test_fp64_comparison_rejects_mistakes(pairs, capsys):
    x, y, tags = pairs["x"], pairs["y"], pairs["tags"]
    d, a = pairs["truth"]
    r = G.ratio(standin_f64(x, y), d, a)
    show(capsys, "numpy fp64 stand-in vs truth [U]", per_family(tags, r))
    assert r.max() <= 16, "the plain fp64 formula is the same algorithm: the same bound"
    for mutant in ("swapped", "R6371", "cos_squared"):
        bad = G.ratio(standin_f64(x, y, mutant), d, a) > 16
        assert bad.any(), mutant
        with capsys.disabled():
            print(f"  {mutant}: rejected on {sorted(set(map(str, tags[bad])))}")


def test_mixed_comparison_rejects_mistakes(pairs, capsys):
    x, y, tags = pairs["x"], pairs["y"], pairs["tags"]
    for which, p32, q in (("mixed_x", x.astype(np.float32), y), ("mixed_y", y.astype(np.float32), x)):
        d, a = pairs[which]
        bad, either, r = G.mixed_verdict(standin_mixed(p32, q), d, a)
        show(capsys, f"float64 stand-in of the mixed contract ({which}; {int(np.isnan(d).sum())} NaN in the truth, "
                     f"{int(either.sum())} in the either band) [U]", per_family(tags, r))
        assert not bad.any() and r.max() <= 16
        assert either.mean() <= 0.02
        assert np.isnan(d).sum() > 0
        for mutant in ("deg2rad64", "cos64"):
            bad, _, _ = G.mixed_verdict(standin_mixed(p32, q, mutant), d, a)
            assert bad.any(), mutant
            with capsys.disabled():
                print(f"  {mutant}: rejected on {sorted(set(map(str, tags[bad])))}")
        # a kernel that never returns NaN (a clamped to 1) is rejected too
        clamped = np.where(np.isnan(d), np.pi * G.R_KM, d.astype(np.float64))
        assert G.mixed_verdict(clamped, d, a)[0].any()


def standin_smooth(d, c, mutant=None):
    with np.errstate(invalid="ignore", over="ignore"):
        m = np.nanmin(d, axis=1, keepdims=True) if mutant == "nan_not_propagated" else d.min(axis=1, keepdims=True)
        v = np.exp(-(d - (0.0 if mutant == "no_shift" else m)) / c)
    if mutant == "inf_left":                                       # the minimum over the finite entries only, and no inf -> 0
        with np.errstate(invalid="ignore", over="ignore"):
            v = np.exp(-(d - np.where(np.isfinite(d), d, np.inf).min(axis=1, keepdims=True)) / c)
        return np.where(np.isnan(v), 0.0, v)
    return np.nan_to_num(v, nan=0.0, posinf=0.0, neginf=0.0)


def test_smooth_comparison_rejects_mistakes():
    rng = np.random.default_rng(11)
    d = G.smooth_inputs(rng, 7, 300, 299)
    assert G.smooth_ratio(standin_smooth(d, 65.0), d, 65.0).max() <= 1
    assert G.smooth_ratio(standin_smooth(d, 65.0, "no_shift"), d, 65.0).max() > 1
    sp = np.stack([r for _, r in G.special_rows(300)])
    want = geo_oracle.smooth_labels(torch.from_numpy(sp), 65.0).numpy()
    assert np.array_equal(standin_smooth(sp, 65.0), want)
    names = [n for n, _ in G.special_rows(300)]
    for n in ("nan_first", "nan_last", "nan_far", "neginf", "all_posinf"):
        assert (want[names.index(n)] == 0).all(), n
    row = want[names.index("posinf")]
    assert row[150] == 0 and (np.delete(row, 150) > 0).all() and row[0] == 1
    assert not np.array_equal(standin_smooth(sp, 65.0, "nan_not_propagated"), want)
    assert not np.array_equal(standin_smooth(sp, 65.0, "inf_left"), want)


@pytest.mark.parametrize("n", [32, 257, 4096])
def test_ordered_mean_is_not_torch_mean(n):
    rows = G.wide_rows(np.random.default_rng(n), (n, 1024))
    want = torch.from_numpy(rows).mean(dim=0).numpy()
    assert not np.array_equal(G.ordered_mean(rows), want)
    assert np.allclose(G.ordered_mean(rows), want, rtol=1e-3, atol=1e-2 * np.abs(rows).max())
