"""The bootstrap kernels against tests/_bootref.py (run with -m gpu on an MI355X): the index stream with `==`, the resampled means bit
for bit in the restated order, the resampled quantiles bit for bit against numpy.quantile of the gathered column, and the pairing and
independence properties of the contract.  A NaN compares equal to a NaN; every other value by its bits."""
import math

import numpy as np
import pytest
import torch

import _bootref as B

pytestmark = pytest.mark.gpu

DEV = "cuda"
SEEDS = (5, (0xfeedface << 32) | 0x1234567)
QS = (0, 0.025, 1 / 3, 0.5, 0.975, 1)
R_FULL = 65


@pytest.fixture(scope="module")
def ops():
    from pigeon_amd import _lib, hip_ops
    _lib.require_gpu()
    return hip_ops


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def first_difference(a, b):
    a, b = np.asarray(a), np.asarray(b)
    bad = np.argwhere(~((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))
    return None if not len(bad) else (tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])], len(bad))


# --------------------------------------------------------------------------------------------------------------------- indices
@pytest.mark.parametrize("N", [1, 2, 3, 255, 256, 257, 2 ** 31 - 1])
def test_indices(ops, N):
    for seed in SEEDS:
        for r in (0, 1, R_FULL - 1):
            for j0 in (0, 7, 2 ** 33 - 151):                         # even, odd, and 300 draws that cross j = 2^33
                got = ops.bootstrap_indices(N, seed, r, j0, 300, DEV).cpu().numpy()
                want = B.indices(N, seed, r, j0, 300)
                assert got.dtype == np.int64 and np.array_equal(got, want), (N, seed, r, j0, np.nonzero(got != want)[0][:4])
    assert ops.bootstrap_indices(N, 1, 0, 0, 0, DEV).shape == (0,)


def test_indices_are_the_stream_the_checker_accepts(ops):
    def fn(seed, r, j, N, m):
        return ops.bootstrap_indices(N, seed, r, int(j[0]), len(j), DEV).cpu().numpy()
    B.check_index_stream(fn, 1000, SEEDS[1], (0, 1, 64), 513, columns=2)


# ----------------------------------------------------------------------------------------------------------------------- means
def mean_columns(N, M, seed):
    rng = np.random.default_rng(seed)
    ints = rng.integers(-1000, 1000, (M, N)).astype(np.float64)
    gauss = rng.standard_normal((M, N)) * 10.0 ** rng.integers(-3, 4, (M, 1))
    return ints, gauss


@pytest.mark.parametrize("N", [1, 2, 255, 256, 257, 1000])
def test_means(ops, N):
    cols = ops.bootstrap_plan(N, 1, 1)["columns_per_workgroup"]
    M = cols + 1
    seed = SEEDS[N % 2]
    ints, gauss = mean_columns(N, M, N)
    idx = [B.indices(N, seed, r) for r in range(R_FULL)]
    for name, x in (("integers", ints), ("gaussian", gauss)):
        want = B.means(x, R_FULL, seed)
        dx = torch.from_numpy(x).to(DEV)
        for R in (1, 3, R_FULL):
            for m in (1, 2, M):
                got = ops.bootstrap_means(dx[:m].contiguous(), R, seed).cpu().numpy()
                assert got.shape == (R, m)
                assert same_bits(got, want[:R, :m]), (name, N, R, m, first_difference(got, want[:R, :m]))
        full = ops.bootstrap_means(dx, R_FULL, seed).cpu().numpy()
        for r in range(R_FULL):
            for m in range(M):
                g = x[m, idx[r]]
                if name == "integers":
                    assert full[r, m] == float(int(g.sum())) / N              # sums of integers below 2^53 are exact in any order
                else:
                    assert abs(full[r, m] - math.fsum(g) / N) <= N * 2.0 ** -53 * float(np.abs(g).sum()) / N, (N, r, m)


def test_means_nan_and_inf_reach_only_the_replicates_that_drew_them(ops):
    N, seed = 1000, SEEDS[0]
    x = np.random.default_rng(8).standard_normal((3, N))
    x[0, 17] = np.nan
    x[1, 400] = np.inf
    x[1, 401] = -np.inf
    got = ops.bootstrap_means(torch.from_numpy(x).to(DEV), R_FULL, seed).cpu().numpy()
    assert same_bits(got, B.means(x, R_FULL, seed)), first_difference(got, B.means(x, R_FULL, seed))
    idx = np.stack([B.indices(N, seed, r) for r in range(R_FULL)])
    drew_nan = (idx == 17).any(axis=1)
    drew_pos, drew_neg = (idx == 400).any(axis=1), (idx == 401).any(axis=1)
    assert 0 < drew_nan.sum() < R_FULL and 0 < (drew_pos & ~drew_neg).sum() and 0 < (drew_pos & drew_neg).sum() and 0 < (~drew_pos & ~drew_neg).sum()
    assert np.array_equal(np.isnan(got[:, 0]), drew_nan)
    assert np.array_equal(np.isnan(got[:, 1]), drew_pos & drew_neg)
    assert np.array_equal(got[:, 1] == np.inf, drew_pos & ~drew_neg) and np.array_equal(got[:, 1] == -np.inf, drew_neg & ~drew_pos)
    assert np.isfinite(got[:, 2]).all()


# ------------------------------------------------------------------------------------------------------------------- quantiles
def quantile_columns(N, seed):
    """constant, two-valued, all-distinct, signed zeros and subnormals, and a Gaussian rounded into ties: one more than a workgroup takes."""
    rng = np.random.default_rng(seed)
    special = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310, -1e-310, 2.2250738585072014e-308])
    return np.stack([np.full(N, 3.25), np.where(rng.random(N) < 0.4, -1.5, 7.0), rng.permutation(N) * 0.37 - 11.0,
                     special[rng.integers(0, len(special), N)], np.round(rng.standard_normal(N), 1)])


def quantile_case(ops, which):
    bins = ops.bootstrap_plan(1, 1, 1)["bins"]
    N = {"1": 1, "2": 2, "3": 3, "bins-1": bins - 1, "bins": bins, "bins+1": bins + 1, "3bins+7": 3 * bins + 7}[which]
    return N, bins, (R_FULL if N <= 3 else 12)


@pytest.mark.parametrize("which", ["1", "2", "3", "bins-1", "bins", "bins+1", "3bins+7"])
def test_quantiles(ops, which):
    N, bins, R = quantile_case(ops, which)
    seed = SEEDS[len(which) % 2]
    x = quantile_columns(N, N)
    assert x.shape[0] == ops.bootstrap_plan(N, R, 1, len(QS))["columns_per_workgroup"] + 1
    plan = ops.bootstrap_plan(N, R, x.shape[0], len(QS))
    if N > bins:
        assert plan["shift"] > 0 and N % (1 << plan["shift"]) != 0 and plan["passes"] == 2
    else:
        assert plan["shift"] == 0 and plan["passes"] == 1
    rank, srt = B.rank_and_sorted(x)
    want = B.quantiles(x, R, seed, QS)
    got = ops.bootstrap_quantiles(torch.from_numpy(rank).to(DEV), torch.from_numpy(srt).to(DEV), R, QS, seed).cpu().numpy()
    assert got.shape == (R, x.shape[0], len(QS))
    assert same_bits(got, want), (N, first_difference(got, want))
    if N > bins:
        # neither path of the fine pass is vacuous: the two order statistics of one quantile in one coarse bin, and in two
        same = different = 0
        for r in range(R):
            idx = B.indices(N, seed, r)
            for q in QS:
                _, lo, hi = B.quantile_by_ranks(rank, srt, 2, idx, q)
                same += (lo >> plan["shift"]) == (hi >> plan["shift"]) and lo != hi
                different += (lo >> plan["shift"]) != (hi >> plan["shift"])
        assert same > 0 and different > 0, (same, different)


def test_quantiles_when_the_wanted_orders_need_several_fine_passes(ops):
    N, R, seed = 2 ** 20 + 1, 2, SEEDS[1]
    plan = ops.bootstrap_plan(N, R, 2, len(QS))
    assert plan["shift"] == 9 and plan["passes"] == 3, plan          # 8 wanted orders a fine pass, 12 wanted
    rng = np.random.default_rng(6)
    x = np.stack([rng.standard_normal(N), np.round(rng.standard_normal(N), 2)])
    rank, srt = B.rank_and_sorted(x)
    got = ops.bootstrap_quantiles(torch.from_numpy(rank).to(DEV), torch.from_numpy(srt).to(DEV), R, QS, seed).cpu().numpy()
    want = B.quantiles(x, R, seed, QS)
    assert same_bits(got, want), first_difference(got, want)


def test_an_out_of_range_rank_gives_nan_between_intact_guards(ops):
    bins = ops.bootstrap_plan(1, 1, 1)["bins"]
    for N in (300, bins + 1):
        R, seed = 24, SEEDS[0]
        x = quantile_columns(N, 77)[[2, 4, 1]]
        rank, srt = B.rank_and_sorted(x)
        want = B.quantiles(x, R, seed, QS)
        bad = rank.copy()
        bad[1, 5], bad[1, 9], bad[2, 11] = N, -1, 2 ** 31 - 1
        idx = np.stack([B.indices(N, seed, r) for r in range(R)])
        drew = np.stack([np.zeros(R, bool), ((idx == 5) | (idx == 9)).any(axis=1), (idx == 11).any(axis=1)], axis=1)
        assert 0 < drew[:, 1].sum() < R and 0 < drew[:, 2].sum() < R
        guard = torch.full((R + 2, 3, len(QS)), -777.0, dtype=torch.float64, device=DEV)
        got = ops.bootstrap_quantiles(torch.from_numpy(bad).to(DEV), torch.from_numpy(srt).to(DEV), R, QS, seed, out=guard[1:R + 1])
        assert got.data_ptr() == guard[1].data_ptr()
        host = guard.cpu().numpy()
        assert (host[0] == -777.0).all() and (host[R + 1] == -777.0).all()
        assert np.array_equal(np.isnan(host[1:R + 1]), np.broadcast_to(drew[:, :, None], want.shape))
        assert same_bits(np.where(drew[:, :, None], np.nan, host[1:R + 1]), np.where(drew[:, :, None], np.nan, want))


# ------------------------------------------------------------------------------------------------- pairing and independence
def test_paired_differences_are_exact(ops):
    from pigeon_amd import bootstrap as boot
    bins = ops.bootstrap_plan(1, 1, 1)["bins"]
    for N in (257, bins + 1):
        # the resamples are the same, so the sums differ by exactly N; a mean x and the mean x + 1 are rounded on one grid, and their
        # difference is exactly 1, while both lie in one binade: values in [300, 500) keep every mean and mean + 1 inside [256, 512)
        a = np.random.default_rng(N).integers(300, 499, N).astype(np.float64)
        reps = boot.replicates({"a": a, "b": a + 1}, {"mean": ("mean_diff", "b", "a"), "median": ("median_diff", "b", "a")}, R=R_FULL, seed=3)
        assert (reps["mean"] == 1.0).all() and (reps["median"] == 1.0).all()
        assert reps["mean"].shape == (R_FULL,)


def test_a_column_alone_equals_itself_among_others_and_a_replicate_does_not_depend_on_R(ops):
    bins = ops.bootstrap_plan(1, 1, 1)["bins"]
    N, seed = bins + 1, SEEDS[1]
    x = np.concatenate([quantile_columns(N, 1), quantile_columns(N, 2)])[:9]       # three workgroups of columns
    rank, srt = B.rank_and_sorted(x)
    drank, dsrt, dx = torch.from_numpy(rank).to(DEV), torch.from_numpy(srt).to(DEV), torch.from_numpy(x).to(DEV)
    full_q = ops.bootstrap_quantiles(drank, dsrt, R_FULL, QS, seed).cpu().numpy()
    full_m = ops.bootstrap_means(dx, R_FULL, seed).cpu().numpy()
    for m in (0, 4, 6, 8):                                            # first, last of a group, inside one, the lone last
        alone_q = ops.bootstrap_quantiles(drank[m:m + 1].contiguous(), dsrt[m:m + 1].contiguous(), R_FULL, QS, seed).cpu().numpy()
        assert same_bits(alone_q[:, 0], full_q[:, m]), m
        one_q = ops.bootstrap_quantiles(drank[m:m + 1].contiguous(), dsrt[m:m + 1].contiguous(), R_FULL, QS[3:4], seed).cpu().numpy()
        assert same_bits(one_q[:, 0, 0], full_q[:, m, 3]), "a quantile does not depend on the others in the call"
        assert same_bits(ops.bootstrap_means(dx[m:m + 1].contiguous(), R_FULL, seed).cpu().numpy()[:, 0], full_m[:, m]), m
    for r in (0, 1, 40):
        assert same_bits(ops.bootstrap_quantiles(drank, dsrt, r + 1, QS, seed).cpu().numpy()[r], full_q[r]), r
        assert same_bits(ops.bootstrap_means(dx, r + 1, seed).cpu().numpy()[r], full_m[r]), r
    assert not same_bits(ops.bootstrap_means(dx, 2, seed + 1).cpu().numpy(), full_m[:2])


def test_many_replicates_walk_the_grid(ops):
    """More (replicate, column group) pairs than workgroups: the stride loop, checked on the replicates at both ends and the seam."""
    N, M, seed = 3, 2, SEEDS[0]
    R = (1 << 20) + 5
    assert ops.bootstrap_plan(N, R, M)["workgroups"] == 1 << 20
    x = np.array([[1.0, 2.0, 4.0], [-1.0, 0.5, 8.0]])
    rank, srt = B.rank_and_sorted(x)
    gm = ops.bootstrap_means(torch.from_numpy(x).to(DEV), R, seed).cpu().numpy()
    gq = ops.bootstrap_quantiles(torch.from_numpy(rank).to(DEV), torch.from_numpy(srt).to(DEV), R, (0.5,), seed).cpu().numpy()
    pick = [0, 1, (1 << 20) - 1, 1 << 20, R - 1]
    assert same_bits(gm[pick], B.means(x, R, seed, replicates=pick))
    assert same_bits(gq[pick], B.quantiles(x, R, seed, (0.5,), replicates=pick))


def test_bootstrap_summary_equals_the_restatement(ops):
    from pigeon_amd import bootstrap as boot
    rng = np.random.default_rng(12)
    N, R, seed = 777, 200, 42
    km, km_best = rng.gamma(2.0, 300.0, N), rng.gamma(2.0, 280.0, N)
    cols = {"km": km, "km_best": km_best, "hit": (km < 400).astype(np.float64), "flat": np.full(N, 2.5)}
    stats = {"Mean": ("mean", "km"), "Median": ("median", "km"), "Hit": ("mean", "hit"), "q90": ("quantile", "km_best", 0.9),
             "dmean": ("mean_diff", "km_best", "km"), "dmedian": ("median_diff", "km_best", "km"), "flat": ("median", "flat"), "flatmean": ("mean", "flat")}
    table = boot.bootstrap(cols, stats, R=R, seed=seed, level=0.9)
    x = np.stack([km, km_best, cols["hit"], cols["flat"]])
    m, q = B.means(x, R, seed), B.quantiles(x, R, seed, (0.5, 0.9))
    reps = {"Mean": m[:, 0], "Median": q[:, 0, 0], "Hit": m[:, 2], "q90": q[:, 1, 1], "dmean": m[:, 1] - m[:, 0], "dmedian": q[:, 1, 0] - q[:, 0, 0],
            "flat": q[:, 3, 0], "flatmean": m[:, 3]}
    for key, v in reps.items():
        row = table[key]
        lo, hi = np.quantile(v, [(1.0 - 0.9) / 2.0, (1.0 + 0.9) / 2.0])
        assert (row["lo"], row["hi"], row["se"]) == (float(lo), float(hi), float(np.std(v, ddof=1)) if np.ptp(v) else 0.0), key
        assert row["lo"] <= row["hi"]
    assert table["Mean"]["estimate"] == float(np.mean(km)) and table["Median"]["estimate"] == float(np.median(km))
    assert table["dmedian"]["estimate"] == float(np.median(km_best)) - float(np.median(km))
    assert table["dmean"]["share_le_zero"] == float(np.mean(reps["dmean"] <= 0)) and "share_le_zero" not in table["Mean"]
    assert (table["flat"]["lo"], table["flat"]["hi"], table["flat"]["se"]) == (2.5, 2.5, 0.0), "a constant column's interval collapses"
    assert (table["flatmean"]["lo"], table["flatmean"]["hi"]) == (2.5, 2.5)
    assert table["Mean"]["lo"] < table["Mean"]["estimate"] < table["Mean"]["hi"]
