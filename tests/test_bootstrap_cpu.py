"""The bootstrap's host side with the library loaded and no GPU: pg_bootstrap_plan's fields and monotonicity, every refusal by name
(each is returned before any HIP call, so none needs a device), `bootstrap()`'s argument checks and `metric_columns` on a hand-made
results tuple."""
import ctypes as C

import numpy as np
import pytest

from pigeon_amd import bootstrap as boot
from pigeon_amd import evaluate as ev

PG_EINVAL = -1
ONE = C.c_void_p(1 << 20)                             # a non-null pointer that is never followed: every call below is refused first
NULL = C.c_void_p(0)


def plan(lib, N, R=1, M=1, Q=1):
    o = (C.c_int32 * 8)()
    assert lib.pg_bootstrap_plan(N, R, M, Q, o) == 0, lib.pg_last_error()
    return dict(zip(("bins", "shift", "passes", "cols", "threads", "lds", "max_n", "grid"), o))


def test_plan_fields(hip_lib):
    p = plan(hip_lib, 1)
    assert p["threads"] == 256 and p["cols"] >= 1 and p["bins"] >= 256 and p["bins"] & (p["bins"] - 1) == 0
    assert p["max_n"] >= 2 ** 24
    assert p["lds"] == p["cols"] * p["bins"] * 4 <= 160 * 1024
    assert (p["shift"], p["passes"], p["grid"]) == (0, 1, 1)
    bins = p["bins"]
    assert plan(hip_lib, bins)["shift"] == 0 and plan(hip_lib, bins)["passes"] == 1
    q = plan(hip_lib, bins + 1)
    assert q["shift"] == 1 and q["passes"] == 2, "one rank past the coarse bins: bins of two ranks and a fine pass"
    for N in (2, 3, bins - 1, bins + 1, 3 * bins + 7, 10 ** 5, p["max_n"]):
        s = plan(hip_lib, N)["shift"]
        assert ((N - 1) >> s) < bins and (s == 0 or ((N - 1) >> (s - 1)) >= bins), N
    big = plan(hip_lib, p["max_n"], Q=16)
    assert big["shift"] == 12 and big["passes"] == 1 + 32, "2^shift fine counters a wanted order: one order a pass at the largest N"
    assert plan(hip_lib, 10 ** 5, Q=16)["passes"] == 2
    assert plan(hip_lib, 1000, R=7, M=p["cols"])["grid"] == 7 and plan(hip_lib, 1000, R=7, M=p["cols"] + 1)["grid"] == 14
    assert plan(hip_lib, 1000, R=2 ** 32, M=100)["grid"] == 2 ** 20


def test_plan_is_monotone(hip_lib):
    last = None
    for N in (1, 2, 255, 4095, 4096, 4097, 8192, 8193, 10 ** 5, 10 ** 6, 2 ** 24):
        p = plan(hip_lib, N, R=3, M=5, Q=3)
        if last is not None:
            assert p["shift"] >= last["shift"] and p["passes"] >= last["passes"]
            assert all(p[k] == last[k] for k in ("bins", "cols", "threads", "lds", "max_n", "grid"))
        last = p
    grids = [plan(hip_lib, 100, R=R, M=M)["grid"] for R in (1, 2, 50) for M in (1, 4, 5, 9)]
    assert grids == sorted(grids) or all(plan(hip_lib, 100, R=R, M=5)["grid"] <= plan(hip_lib, 100, R=R + 1, M=5)["grid"] for R in (1, 9))
    passes = [plan(hip_lib, 2 ** 20, Q=Q)["passes"] for Q in range(1, 17)]
    assert passes == sorted(passes)


def refused(lib, rc, *names):
    assert rc == PG_EINVAL
    msg = lib.pg_last_error().decode()
    assert all(n in msg for n in names), msg
    return msg


def test_every_refusal_names_its_argument(hip_lib):
    lib = hip_lib
    o = (C.c_int32 * 8)()
    max_n = plan(lib, 1)["max_n"]
    q = (C.c_double * 2)(0.5, 0.25)
    for who, call in (("bootstrap_plan", lambda N, R, M, Q: lib.pg_bootstrap_plan(N, R, M, Q, o)),
                      ("bootstrap_means", lambda N, R, M, Q: lib.pg_bootstrap_means(ONE, M, N, R, 0, ONE, NULL)),
                      ("bootstrap_quantiles", lambda N, R, M, Q: lib.pg_bootstrap_quantiles(ONE, ONE, M, N, R, 0, q, Q, ONE, NULL))):
        refused(lib, call(0, 1, 1, 1), who, "N")
        refused(lib, call(-5, 1, 1, 1), who, "N")
        refused(lib, call(max_n + 1, 1, 1, 1), who, "N", str(max_n + 1))
        refused(lib, call(10, 0, 1, 1), who, "R")
        refused(lib, call(10, -1, 1, 1), who, "R")
        refused(lib, call(10, 2 ** 32 + 1, 1, 1), who, "R")
        refused(lib, call(10, 1, 0, 1), who, "M")
        if who != "bootstrap_means":
            refused(lib, call(10, 1, 1, 0), who, "Q")
            refused(lib, call(10, 1, 1, 17), who, "Q")
    refused(lib, lib.pg_bootstrap_plan(10, 1, 1, 1, None), "bootstrap_plan", "out")
    refused(lib, lib.pg_bootstrap_means(NULL, 1, 10, 1, 0, ONE, NULL), "bootstrap_means", "null", "x")
    refused(lib, lib.pg_bootstrap_means(ONE, 1, 10, 1, 0, NULL, NULL), "bootstrap_means", "null", "out")
    refused(lib, lib.pg_bootstrap_quantiles(NULL, ONE, 1, 10, 1, 0, q, 2, ONE, NULL), "bootstrap_quantiles", "null", "rank")
    refused(lib, lib.pg_bootstrap_quantiles(ONE, NULL, 1, 10, 1, 0, q, 2, ONE, NULL), "bootstrap_quantiles", "null", "sorted")
    refused(lib, lib.pg_bootstrap_quantiles(ONE, ONE, 1, 10, 1, 0, None, 2, ONE, NULL), "bootstrap_quantiles", "null", "q")
    refused(lib, lib.pg_bootstrap_quantiles(ONE, ONE, 1, 10, 1, 0, q, 2, NULL, NULL), "bootstrap_quantiles", "null", "out")
    for bad in (-0.01, 1.0000001, float("nan"), float("inf"), float("-inf")):
        qq = (C.c_double * 2)(0.5, bad)
        refused(lib, lib.pg_bootstrap_quantiles(ONE, ONE, 1, 10, 1, 0, qq, 2, ONE, NULL), "bootstrap_quantiles", "q[1]")
    refused(lib, lib.pg_bootstrap_indices(0, 0, 0, 0, 4, ONE, NULL), "bootstrap_indices", "N")
    refused(lib, lib.pg_bootstrap_indices(10, 0, -1, 0, 4, ONE, NULL), "bootstrap_indices", "r")
    refused(lib, lib.pg_bootstrap_indices(10, 0, 2 ** 32, 0, 4, ONE, NULL), "bootstrap_indices", "r")
    refused(lib, lib.pg_bootstrap_indices(10, 0, 0, -1, 4, ONE, NULL), "bootstrap_indices", "j0")
    refused(lib, lib.pg_bootstrap_indices(10, 0, 0, 0, -4, ONE, NULL), "bootstrap_indices", "count")
    refused(lib, lib.pg_bootstrap_indices(10, 0, 0, 2 ** 63 - 2, 4, ONE, NULL), "bootstrap_indices", "count")
    refused(lib, lib.pg_bootstrap_indices(10, 0, 0, 0, 4, NULL, NULL), "bootstrap_indices", "null", "out")


def test_bootstrap_argument_checks(hip_lib):
    km = np.arange(10.0)
    cols = {"km": km, "other": km + 1}
    ok = {"m": ("mean", "km")}
    for columns, stats, kw, match in (
            ({}, ok, {}, "non-empty"),
            ([1, 2], ok, {}, "mapping"),
            ({"km": km.reshape(2, 5)}, ok, {}, "'km' must be one-dimensional"),
            ({"km": km, "short": km[:3]}, ok, {}, "one length"),
            ({"km": np.array(["a", "b"])}, ok, {}, "'km' is not numeric"),
            ({"km": km[:0]}, ok, {}, "0 items"),
            (cols, {}, {}, "no statistic"),
            (cols, {"m": ("mode", "km")}, {}, "unknown kind 'mode'"),
            (cols, {"m": ("mean", "kmm")}, {}, "'kmm'"),
            (cols, {"m": ("mean", "km", "other")}, {}, "takes 1 arguments"),
            (cols, {"m": ("mean_diff", "km")}, {}, "takes 2 arguments"),
            (cols, {"m": ("quantile", "km")}, {}, "takes 2 arguments"),
            (cols, {"m": ("quantile", "km", 1.5)}, {}, "not in \\[0, 1\\]"),
            (cols, {"m": ("quantile", "km", float("nan"))}, {}, "not in \\[0, 1\\]"),
            (cols, {f"q{i}": ("quantile", "km", i / 20) for i in range(17)}, {}, "17 distinct quantiles"),
            (cols, ok, {"R": 0}, "R must be a positive integer"),
            (cols, ok, {"R": 2.5}, "R must be a positive integer"),
            (cols, ok, {"seed": -1}, "seed"),
            (cols, ok, {"seed": 2 ** 64}, "seed"),
            (cols, ok, {"level": 1.0}, "level"),
            (cols, ok, {"level": 0}, "level"),
            ({"km": km, "holey": np.where(km == 3, np.nan, km)}, {"m": ("median", "holey")}, {}, "'holey' holds a NaN"),
            ({"km": km, "holey": np.where(km == 3, np.nan, km)}, {"m": ("median_diff", "km", "holey")}, {}, "'holey' holds a NaN"),
    ):
        with pytest.raises(ValueError, match=match):
            boot.bootstrap(columns, stats, **kw)
    # a NaN is a value like any other to a mean: accepted by the checks (the call then needs a GPU, which is not asked for here)
    cols2, stats2, N = boot._normalise({"holey": np.where(km == 3, np.nan, km)}, [("mean", "holey")], 5, 0, 0.9)
    assert N == 10 and list(stats2.values()) == [("mean", "holey")]
    with pytest.raises(SystemExit):
        boot.main(["--columns", "nowhere.npz"])


def hand_made(n=23, seed=0):
    rng = np.random.default_rng(seed)
    labels = np.stack([rng.uniform(-180, 180, n), rng.uniform(-80, 80, n)], axis=1)
    preds = (labels + rng.standard_normal((n, 2)) * np.where(np.arange(n)[:, None] % 3 == 0, 0.01, 8.0)).astype(np.float32)
    cell_labels = rng.integers(0, 9, n)
    top5 = np.stack([rng.permutation(9)[:5] for _ in range(n)])
    cell_preds = np.where(np.arange(n) % 2 == 0, cell_labels, top5[:, 0])
    preds_mt, labels_mt = rng.standard_normal((n, 6)), rng.standard_normal((n, 6))
    preds_climate, labels_climate = rng.standard_normal((n, 28)), np.eye(28)[rng.integers(0, 28, n)]
    preds_month, labels_month = rng.standard_normal((n, 12)), rng.integers(0, 12, n)
    return (preds, cell_preds, preds_mt, preds_climate, preds_month, top5, labels, cell_labels, labels_mt, labels_climate, labels_month)


class Scaler:
    def inverse_transform(self, v):
        return np.asarray(v) * 0.5 + 0.25


@pytest.mark.parametrize("multi_task", [False, True])
def test_metric_columns_reproduce_every_metric_exactly(multi_task):
    res = hand_made()
    if not multi_task:
        res = res[:2] + (None, None, None) + res[5:8] + (None, None, None)
    want = ev.compute_geoguessr_metrics(res, scaler=Scaler())
    cols, stats = boot.metric_columns(res, scaler=Scaler())
    assert set(want) == set(stats), set(want) ^ set(stats)
    assert len(want) == (23 if multi_task else 15)
    for key, value in want.items():
        kind, name = stats[key]
        got = np.mean(cols[name]) if kind == "mean" else np.median(cols[name])
        assert kind in ("mean", "median") and got == value, (key, got, value)
        assert boot._estimate(cols, stats[key]) == float(value)
    assert len({len(c) for c in cols.values()}) == 1


def test_metric_columns_of_the_other_guesses():
    res = hand_made(seed=4)
    n = len(res[0])
    rng = np.random.default_rng(9)
    best = (np.asarray(res[6]) + rng.standard_normal((n, 2))).astype(np.float64)
    taken = rng.integers(0, 2, n).astype(bool)
    nn = (np.asarray(res[6])[:, None, :] + rng.standard_normal((n, 3, 2)) * 5).astype(np.float32)
    from pigeon_amd.geo_utils import haversine_np
    want = dict(ev.best_guess_metrics(best, haversine_np, res[6], taken), **ev.neighbour_metrics(nn, haversine_np, res[6], res[0]))
    cols, stats = boot.metric_columns(res[:2] + (None, None, None) + res[5:8] + (None, None, None), best_LLH=best, best_taken=taken, nn_lnglat=nn)
    for key, value in want.items():
        kind, name = stats[key]
        assert (np.mean(cols[name]) if kind == "mean" else np.median(cols[name])) == value, key
    diffs = {k: s for k, s in stats.items() if " - " in k}
    assert diffs == {"Mean_km_error_best - Mean_km_error": ("mean_diff", "km_best", "km"),
                     "Median_km_error_best - Median_km_error": ("median_diff", "km_best", "km"),
                     "Geoguessr_score_best - Geoguessr_score": ("mean_diff", "score_best", "score"),
                     "Mean_km_error_nn - Mean_km_error": ("mean_diff", "km_nn", "km"),
                     "Median_km_error_nn - Median_km_error": ("median_diff", "km_nn", "km"),
                     "Geoguessr_score_nn - Geoguessr_score": ("mean_diff", "score_nn", "score")}
    boot._normalise(cols, stats, 10, 0, 0.95)


def test_country_hits_is_what_country_accuracy_averages(monkeypatch):
    from pigeon_amd import regions
    hits = np.array([True, False, True, True])
    monkeypatch.setattr(regions, "find_regions", lambda bank, pts: (np.arange(len(pts)), {}))
    monkeypatch.setattr(regions, "contains", lambda bank, pts, which: hits)
    got = regions.country_hits(np.zeros((4, 2)), np.zeros((4, 2)), None)
    assert got.dtype.kind == "i" and got.tolist() == [1, 0, 1, 1]
    assert regions.country_accuracy(np.zeros((4, 2)), np.zeros((4, 2)), None) == 0.75


def test_summarise_on_known_replicates():
    cols = {"a": np.array([1.0, 2.0, 6.0]), "b": np.array([0.0, 2.0, 1.0])}
    stats = {"m": ("mean", "a"), "d": ("median_diff", "a", "b")}
    reps = {"m": np.arange(101.0), "d": np.linspace(-1, 1, 101)}
    t = boot.summarise(cols, stats, reps, 0.5)
    assert t["m"] == dict(estimate=3.0, se=float(np.std(np.arange(101.0), ddof=1)), lo=25.0, hi=75.0)
    assert t["d"]["estimate"] == 1.0 and t["d"]["share_le_zero"] == 51 / 101 and "share_le_zero" not in t["m"]
    text = boot.report(t, 0.5)
    assert "m: 3 [25, 75]" in text and "paired differences" in text and text.index("paired") < text.index("d: 1 [")
    flat = boot.summarise({"a": np.full(5, 0.1)}, {"m": ("mean", "a")}, {"m": np.full(37, 10032.564784442313)}, 0.95)["m"]
    assert (flat["lo"], flat["hi"], flat["se"]) == (10032.564784442313, 10032.564784442313, 0.0), "equal replicates have no spread"
    assert boot.summarise({"a": np.full(5, 0.1)}, {"m": ("mean", "a")}, {"m": np.array([2.0])}, 0.95)["m"]["se"] == 0.0
