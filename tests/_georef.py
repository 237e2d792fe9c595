"""High-precision statements of the geo kernels (csrc/geo_proto.hip) and the inputs at which they go wrong.  numpy only: no torch
device, no GPU.  tests/test_georef_cpu.py pins every function here (mpmath at 50 digits, torch's own reductions) and shows that the
comparisons reject the mistakes they are for; tests/test_gpu_geo.py holds the kernels to them.

Truths are computed in np.longdouble (64-bit significand, 2^-64 per operation) with the 50-digit pi/180 the kernels carry.

  haversine_truth        the distance of two fp64 points on the sphere of R = 6378.137 km.  Written in the form whose two terms are
                         both non-negative,  a = sin^2(dlat/2) cos^2(dlng/2) + cos^2(mlat) sin^2(dlng/2),  1 - a = cos^2(dlat/2)
                         cos^2(dlng/2) + sin^2(mlat) sin^2(dlng/2)  (mlat the mean latitude; cos p1 cos p2 = cos^2(dlat/2) - sin^2(mlat)),
                         d = 2 R atan2(sqrt a, sqrt(1 - a)): exact antipodes keep their full relative accuracy, where the textbook
                         asin(sqrt a) loses half the digits.  The differences are taken in degrees (exact for nearby points).
  haversine_mixed_truth  the contract of the two fp32 template arms: the fp32 point is multiplied by float32(pi/180) IN fp32, the
                         cosine of its latitude is the correctly rounded fp32 value, everything after that is exact.  This is not a
                         distance on a sphere any more: next to antipodes its `a` really exceeds 1 and the answer is NaN.
  U(a)                   the unit of the bound: 6378.137 eps / sqrt(max(1 - a, eps)), eps = 2^-52.  The two angle differences carry at
                         most pi eps of absolute error each, which moves a by at most 2 sqrt(a) pi eps; dd/da = R / sqrt(a (1 - a)), so
                         the distance moves by 2 pi R eps / sqrt(1 - a) = 6.3 U; the remaining operations add a few eps d.  The tests
                         allow 16 U.  numpy's own fp64 formula reaches 3 to 4.5 U (printed by test_georef_cpu.py).
  smooth_truth           exp(-(d - rowmin d) / c).  Bound (4 + t) eps truth + 4 2^-1074 with t = (d - rowmin) / c: the subtraction and
                         the division put t eps on the exponent, exp adds an ulp; the absolute term holds the subnormal range.
  cascade_mean           ATen's cascade_sum order (SumKernel.cpp multi_row_sum) restated: what torch.mean(dim=0) computes on the CPU for
                         a (n, W) fp32 block, bit for bit.  ordered_mean is the plain left-to-right sum, the negative control.
"""
from fractions import Fraction

import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
R_KM = 6378.137
R_LD = LD(6378137) / LD(1000)                                       # 6378.137 is no double
PI180_DIGITS = "0.017453292519943295769236907684886127134428718885417"
_PI180_HI = float(Fraction(PI180_DIGITS))                           # the double the kernels multiply by
PI180 = LD(_PI180_HI) + LD(float(Fraction(PI180_DIGITS) - Fraction(_PI180_HI)))     # two doubles: no string parsing in longdouble
DEG2RAD_F32 = np.float32(_PI180_HI)                                 # (float)DEG2RAD_D: the double constant rounded to fp32
MIN_SUBNORMAL = 2.0 ** -1074
SENTINEL = -7.25                                                    # what the GPU tests fill their guard elements with
GUARD = 64

assert np.finfo(LD).nmant >= 63, "np.longdouble must be wider than float64 for these truths"


def _ld(v):
    v = np.asarray(v)
    assert v.dtype == np.float64, v.dtype
    return v.astype(LD)


# ------------------------------------------------------------------------------------------------ haversine
def haversine_truth(x_deg, y_deg):
    """x, y (..., 2) fp64 [lng, lat] degrees, broadcast against each other -> (d_km, a), both longdouble"""
    x, y = _ld(x_deg), _ld(y_deg)
    dlng = x[..., 0] - y[..., 0]
    dlng = dlng - 360 * np.rint(dlng / 360)                         # exact in degrees; sin^2 and cos^2 of the half are unchanged
    hl = dlng * PI180 / 2
    hp = (x[..., 1] - y[..., 1]) * PI180 / 2
    hm = (x[..., 1] + y[..., 1]) * PI180 / 2
    sl, cl = np.sin(hl) ** 2, np.cos(hl) ** 2
    a = np.sin(hp) ** 2 * cl + np.cos(hm) ** 2 * sl
    b = np.cos(hp) ** 2 * cl + np.sin(hm) ** 2 * sl
    return 2 * R_LD * np.arctan2(np.sqrt(a), np.sqrt(b)), a


def haversine_mixed_truth(p32_deg, q64_deg):
    """p (..., 2) fp32, q (..., 2) fp64 -> (d_km, a) longdouble; d is NaN where a > 1"""
    p = np.asarray(p32_deg)
    assert p.dtype == np.float32, p.dtype
    pr = p * DEG2RAD_F32                                            # the fp32 multiply
    assert pr.dtype == np.float32
    plng, plat = pr[..., 0].astype(LD), pr[..., 1].astype(LD)
    cosp = np.cos(plat).astype(np.float32).astype(LD)              # correctly rounded fp32 cos
    q = _ld(q64_deg) * PI180
    s1, s0 = np.sin((plat - q[..., 1]) / 2), np.sin((plng - q[..., 0]) / 2)
    a = s1 * s1 + cosp * np.cos(q[..., 1]) * (s0 * s0)
    with np.errstate(invalid="ignore"):
        d = 2 * R_LD * np.arcsin(np.sqrt(a))
    return d, a


def U(a):
    """the unit of the haversine bound, fp64 km"""
    one_minus = np.maximum(1 - np.asarray(a, dtype=LD), LD(EPS))
    return (LD(R_KM) * LD(EPS) / np.sqrt(one_minus)).astype(np.float64)


def ratio(got, truth, a):
    """|got - truth| / U(a), fp64; inf where got is not finite"""
    with np.errstate(invalid="ignore"):
        r = (np.abs(np.asarray(got, dtype=np.float64).astype(LD) - truth) / U(a).astype(LD)).astype(np.float64)
    return np.where(np.isfinite(got), r, np.inf)


def mixed_verdict(got, truth, a):
    """The fp32 arms: -> (bad, either, ratio).  Where a < 1 - 4 eps the element must be within 16 U of the truth; where a > 1 + 4 eps
    it must be NaN; in between either a NaN or a value within 16 U is accepted (`either` marks that band)."""
    got = np.asarray(got, dtype=np.float64)
    a = np.asarray(a, dtype=LD)
    below, above = a < 1 - 4 * LD(EPS), a > 1 + 4 * LD(EPS)
    either = ~below & ~above
    with np.errstate(invalid="ignore"):
        r = ratio(got, truth, np.minimum(a, 1))
    within = r <= 16
    bad = (below & ~within) | (above & ~np.isnan(got)) | (either & ~(within | np.isnan(got)))
    return bad, either, np.where(below, r, 0.0)


# ---- input families
NEAR = (1e-12, 1e-9, 1e-7, 1e-5, 1e-3, 1e-1)
NEAR_ANTI = (1e-9, 1e-6, 1e-3)
TAGS = ("identical",) + tuple(f"near_{s:g}" for s in NEAR) + ("global", "antimeridian", "antimeridian_180", "poles", "origin",
                                                               "antipode") + tuple(f"nearanti_{s:g}" for s in NEAR_ANTI)


def anchors(tag, n, rng):
    """n first points (n, 2) fp64 of family `tag`"""
    lng, lat = rng.uniform(-179, 179, n), rng.uniform(-89, 89, n)
    if tag == "global":
        lng, lat = rng.uniform(-180, 180, n), rng.uniform(-90, 90, n)
    elif tag == "antimeridian":
        lng = 180 - 10.0 ** rng.uniform(-10, -3, n)                 # 179.9999...
    elif tag == "antimeridian_180":
        lng = np.full(n, 180.0)
    elif tag == "poles":
        lat = np.where(rng.integers(0, 2, n) == 1, 90.0, -90.0)
    elif tag == "origin":
        lng, lat = np.zeros(n), np.zeros(n)
    elif tag == "antipode" or tag.startswith("nearanti_"):
        lng = np.rint(lng * 2.0 ** 20) / 2.0 ** 20                  # lng -+ 180 is exact
    return np.stack([lng, lat], axis=1)


def partners(tag, x, rng):
    """the second point of every pair, (n, 2) fp64"""
    n = x.shape[0]
    glob = np.stack([rng.uniform(-180, 180, n), rng.uniform(-90, 90, n)], axis=1)
    anti = np.stack([np.where(x[:, 0] > 0, x[:, 0] - 180, x[:, 0] + 180), -x[:, 1]], axis=1)
    if tag == "identical":
        return x.copy()
    if tag.startswith("near_"):
        return x + rng.normal(0, float(tag[5:]), (n, 2))
    if tag == "global":
        return glob
    if tag == "antimeridian":
        return np.stack([-180 + 10.0 ** rng.uniform(-10, -3, n), x[:, 1] + rng.normal(0, 1e-4, n)], axis=1)
    if tag == "antimeridian_180":
        return np.stack([np.full(n, -180.0), x[:, 1]], axis=1)
    if tag == "poles":                                              # a pole again (the same or the other one, any longitude), or anywhere
        i = np.arange(n)                                            # every 16th pair is the two opposite poles
        pole = np.stack([glob[:, 0], np.where(i % 16 == 8, -x[:, 1], x[:, 1])], axis=1)
        return np.where((i % 4 == 0)[:, None], pole, glob)
    if tag == "origin":                                             # (0, 0) itself, then near and far points in turn
        near = rng.normal(0, 1, (n, 2)) * 10.0 ** rng.uniform(-12, 0, (n, 1))
        y = np.where((np.arange(n) % 2 == 1)[:, None], near, glob)
        y[::7] = 0.0
        return y
    if tag == "antipode":
        return anti
    if tag.startswith("nearanti_"):
        return anti + rng.normal(0, float(tag[9:]), (n, 2))
    raise KeyError(tag)


def family_pairs(seed, per_tag):
    """-> x (n, 2), y (n, 2) fp64 and the family tag of every pair, `per_tag` pairs of every family in TAGS"""
    rng = np.random.default_rng(seed)
    xs, ys, tags = [], [], []
    for tag in TAGS:
        x = anchors(tag, per_tag, rng)
        xs.append(x); ys.append(partners(tag, x, rng)); tags += [tag] * per_tag
    return np.concatenate(xs), np.concatenate(ys), np.array(tags)


def matrix_case(tag, N, M, rng):
    """-> x (N, 2), y (M, 2), family (N, M) bool.  Column j is a partner of row j % N in family `tag`: element (j % N, j) belongs to the
    family -- the first and the last column included -- and the other elements of the column are unrelated pairs."""
    x = anchors(tag, N, rng)
    rows = np.arange(M) % N
    y = partners(tag, x[rows], rng)
    fam = np.zeros((N, M), dtype=bool)
    fam[rows, np.arange(M)] = True
    return x, y, fam


# ------------------------------------------------------------------------------------------------ smooth labels
def smooth_truth(d, c):
    """d (N, M) finite fp64, c > 0 -> (exp(-(d - rowmin) / c), t = (d - rowmin) / c), longdouble"""
    d = _ld(d)
    assert np.isfinite(d).all()
    t = (d - d.min(axis=-1, keepdims=True)) / LD(c)
    return np.exp(-t), t


def smooth_inputs(rng, N, M, min_col):
    """rows of real distances, 0 .. 20 037 km, the row minimum in column min_col"""
    d = rng.uniform(0, np.pi * R_KM, (N, M))
    d[:, min_col % M] = d.min(axis=1) * rng.uniform(0, 1, N)
    return d


def special_rows(M):
    """[(name, row)]: a NaN at column 0 / the last column / a column >= 256 (where the row has one), a +inf entry, a -inf entry, and an
    all-+inf row"""
    base = np.linspace(10.0, 5000.0, M)
    out = []
    for name, col, v in (("nan_first", 0, np.nan), ("nan_last", M - 1, np.nan), ("nan_far", min(M - 1, 300), np.nan),
                         ("posinf", M // 2, np.inf), ("neginf", M // 3, -np.inf)):
        r = base.copy(); r[col] = v
        out.append((name, r))
    out.append(("all_posinf", np.full(M, np.inf)))
    return out


def smooth_bound(truth, t):
    return ((4 + t) * LD(EPS) * truth + 4 * LD(MIN_SUBNORMAL)).astype(LD)


def smooth_ratio(got, d, c):
    """|got - truth| / bound per element (fp64) of finite rows"""
    truth, t = smooth_truth(d, c)
    return (np.abs(np.asarray(got, dtype=np.float64).astype(LD) - truth) / smooth_bound(truth, t)).astype(np.float64)


# ------------------------------------------------------------------------------------------------ prototype means
def wide_rows(rng, shape):
    """randn * 10^U(-3, 3) per row, fp32: the order of the additions shows in the bits"""
    return (rng.standard_normal(shape) * 10.0 ** rng.uniform(-3, 3, shape[:-1] + (1,))).astype(np.float32)


def panel_mean(bank4):
    """torch's mean(dim=1) of a (n, 4, W) fp32 bank: four rows are fewer than a chunk, so left to right, then / 4"""
    b = np.asarray(bank4)
    assert b.dtype == np.float32 and b.ndim == 3 and b.shape[1] == 4
    return (((b[:, 0] + b[:, 1]) + b[:, 2]) + b[:, 3]) / np.float32(4)


def _seqsum(blk):
    """(g, k, W) fp32 -> (g, W): the k items of every group added left to right into a zero accumulator"""
    acc = np.zeros((blk.shape[0], blk.shape[2]), dtype=np.float32)
    for j in range(blk.shape[1]):
        acc = acc + blk[:, j]
    return acc


def _level(items, step):
    """items (k, W) reach an accumulator in order, and the accumulator is flushed after every `step` of them
    -> (the k // step flushed values, what is left in the accumulator at the end)"""
    full = items.shape[0] // step
    flushed = _seqsum(items[:full * step].reshape(full, step, items.shape[1]))
    return flushed, _seqsum(items[None, full * step:])[0]


def ceil_log2(n):
    """ATen utils::CeilLog2: 1 for n <= 2"""
    return 1 if n <= 2 else int(n - 1).bit_length()


def cascade_mean(rows, idx=None):
    """torch.mean(rows[idx], dim=0) of (n, W) fp32 rows on the CPU, bit for bit (idx=None: all rows in order; n = 0 gives zeros, the
    kernel's convention, where torch gives NaN).  ATen adds the rows in chunks of 2^level_power, level_power = max(4, CeilLog2(n) // 4),
    into a level-0 accumulator that starts from zero for every chunk; a finished chunk goes to level 1, every 2^level_power chunks
    level 1 goes to level 2, likewise level 2 to level 3; the tail rows stay in level 0; the sum is ((l0 + l1) + l2) + l3."""
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.ndim == 2
    idx = np.arange(rows.shape[0]) if idx is None else np.asarray(idx)
    n, W = len(idx), rows.shape[1]
    if n == 0:
        return np.zeros(W, dtype=np.float32)
    step = 1 << max(4, ceil_log2(n) // 4)
    chunks = n // step
    sums = np.empty((chunks, W), dtype=np.float32)
    slab = 512                                                      # chunks gathered at a time
    for s in range(0, chunks, slab):
        e = min(chunks, s + slab)
        sums[s:e] = _seqsum(rows[idx[s * step:e * step]].reshape(e - s, step, W))
    l0 = _seqsum(rows[idx[chunks * step:]][None])[0]
    to2, l1 = _level(sums, step)
    to3, l2 = _level(to2, step)
    l3 = _seqsum(to3[None])[0]
    return (((l0 + l1) + l2) + l3) / np.float32(n)


def ordered_mean(rows, idx=None):
    rows = np.asarray(rows)
    assert rows.dtype == np.float32 and rows.ndim == 2
    idx = np.arange(rows.shape[0]) if idx is None else np.asarray(idx)
    if len(idx) == 0:
        return np.zeros(rows.shape[1], dtype=np.float32)
    return _seqsum(rows[idx][None])[0] / np.float32(len(idx))
