"""The guess spread without a GPU: tests/_spreadref.py is pinned against mpmath, its comparator is shown to reject the mistakes it is
for, the coverage metrics are checked on planted arrays, and everything pg_guess_spread decides before its first HIP call -- every
PG_EINVAL refusal, the no-op cases, pg_guess_spread_plan -- is called through the library.  Serving keys with stub models, as
tests/test_serve_cpu.py does."""
import base64
import ctypes as C
import io
import re
from collections import namedtuple

import numpy as np
import pytest
import torch

import _georef as G
import _spreadref as S

QS = (0.5, 0.9, 1.0)
GRID_C = (2, 3, 63, 64, 65, 257, 2076)


# ================================================================================================================ the restatement
def _mp_case(logits, cen, pt, ext, qs):
    """one row, one point in mpmath at 50 digits -> expected_km, expected_score, [(answer cell, key)] per quantile"""
    import mpmath as mp
    mp.mp.dps = 50
    l = [mp.mpf(float(v)) for v in logits]
    m = max(l)
    w = [mp.exp(v - m) for v in l]
    rad = mp.pi / 180
    R = mp.mpf(6378137) / 1000
    d = []
    for c in range(len(l)):
        lng1, lat1, lng2, lat2 = (mp.mpf(float(v)) * rad for v in (pt[0], pt[1], cen[c, 0], cen[c, 1]))
        a = mp.sin((lat1 - lat2) / 2) ** 2 + mp.cos(lat1) * mp.cos(lat2) * mp.sin((lng1 - lng2) / 2) ** 2
        d.append(2 * R * mp.asin(mp.sqrt(a)))
    Z = mp.fsum(w)
    ek = mp.fsum(wc * dc for wc, dc in zip(w, d)) / Z
    es = mp.fsum(wc * 5000 * mp.exp(-dc / mp.mpf("1492.7")) for wc, dc in zip(w, d)) / Z
    key = [dc + mp.mpf(float(e)) for dc, e in zip(d, ext)]
    order = sorted(range(len(l)), key=lambda c: (key[c], c))
    ans = []
    for q in qs:
        acc = mp.mpf(0)
        for c in order:
            acc += w[c]
            if acc >= mp.mpf(q) * Z:
                ans.append((c, key[c]))
                break
    return ek, es, ans


@pytest.mark.parametrize("C_cells,seed", [(3, 0), (17, 1), (64, 2), (257, 3)])
def test_restatement_against_mpmath(C_cells, seed):
    logits = S.gaussian_logits(2, C_cells, seed)
    cen, pts, ext = S.centroids_of(C_cells, seed), S.points_of(2, 1, seed), S.extents_of(C_cells, seed)
    t = S.truth(logits, cen, pts, (0.5, 0.9), ext)
    for b in range(2):
        ek, es, ans = _mp_case(logits[b], cen, pts[b, 0], ext, (0.5, 0.9))
        assert abs(float(ek) - t["expected_km"][b, 0]) <= 4 * G.EPS * float(ek)
        assert abs(float(es) - t["expected_score"][b, 0]) <= 4 * G.EPS * float(es)
        for j, (cell, key) in enumerate(ans):
            assert t["cell"][b, 0, j] == cell
            assert abs(float(key) - t["key"][b, 0, j]) <= 4 * G.EPS * float(key)
            assert t["tight"][b, 0, j]


def test_restatement_masked_cells_ties_and_nan_rules():
    cen = S.centroids_of(6, 9)
    cen[3] = cen[1]                                                  # two cells of one key: M(key) takes both
    logits = np.zeros((4, 6), dtype=np.float32)
    logits[0, 0] = -np.inf                                           # a masked cell
    logits[1, 2] = np.nan
    logits[2, :] = -np.inf
    logits[3, 4] = np.inf
    pts = S.points_of(4, 1, 9)
    t = S.truth(logits, cen, pts, (0.35, 1.0))
    assert not np.isnan(t["expected_km"][0, 0]) and np.isnan(t["expected_km"][1:, 0]).all()
    d, _ = G.haversine_truth(pts[0], cen)
    d = d.astype(np.float64)
    live = np.argsort(np.where(np.arange(6) == 0, np.inf, d), kind="stable")
    # five live cells of weight 1: q = 0.35 needs 1.75 -> the second key, unless the first two share theirs
    keys = np.sort(d[1:])
    assert t["key"][0, 0, 0] == keys[1] and t["key"][0, 0, 1] == keys[-1]
    assert t["cell"][0, 0, 1] == live[4]
    pts[0, 0, 1] = np.inf
    assert np.isnan(S.truth(logits, cen, pts, (0.5,))["expected_km"][0, 0])
    e = np.zeros(6); e[5] = np.nan
    assert np.isnan(S.truth(logits[:1], cen, S.points_of(1, 1, 9), (0.5,), e)["expected_km"]).all()


@pytest.mark.parametrize("C_cells", GRID_C)
def test_plain_implementation_passes_and_nothing_is_loose(C_cells):
    """the inputs the GPU tests use: 0 loose quantiles in the restatement alone, and a straightforward fp64 implementation inside
    every bound"""
    for seed in range(2):
        B = 5
        logits, cen = S.gaussian_logits(B, C_cells, seed), S.centroids_of(C_cells, seed)
        pts, ext = S.points_of(B, 2, seed), S.extents_of(C_cells, seed)
        for extent in (None, ext):
            t = S.truth(logits, cen, pts, QS, extent)
            assert t["tight"].all(), (t["mass_margin"].min(), t["key_gap"].min())
            errors, loose, worst = S.compare(t, *S.plain(logits, cen, pts, QS, extent))
            assert not errors and loose == 0 and worst < 1, errors[:3]


def test_uniform_weights_quantile_is_never_on_a_step():
    for C_cells in GRID_C + (9600, 9601):
        q = S.uniform_quantile(C_cells)
        assert 0 < q <= 1 and abs(q * C_cells - round(q * C_cells)) > 0.2


# ================================================================================================================ planted mistakes
RADIUS_MISTAKES = ("strict_greater", "unsorted_cumsum", "extent_left_out", "lnglat_swapped", "neighbour_row_point")


@pytest.mark.parametrize("mistake", S.MISTAKES)
def test_comparator_rejects(mistake):
    B, C_cells = 3, 65
    logits, cen = S.gaussian_logits(B, C_cells, 5), S.centroids_of(C_cells, 5)
    pts, ext = S.points_of(B, 2, 5), S.extents_of(C_cells, 5) + 50.0
    if mistake == "no_max_shift":
        logits = logits + np.float32(1000)
    t = S.truth(logits, cen, pts, QS, ext)
    ok, _, _ = S.compare(t, *S.plain(logits, cen, pts, QS, ext))
    assert not ok, ok[:3]
    errors, _, _ = S.compare(t, *S.plain(logits, cen, pts, QS, ext, mistake=mistake))
    assert errors, f"{mistake} went through"
    named = [e for e in errors if re.match(r"row \d+ point \d+ (quantile \d+ \(q = [0-9.]+|expected_km|expected_score)", e)]
    assert named == errors, errors[:3]
    if mistake in RADIUS_MISTAKES:
        assert any(" quantile " in e for e in errors), errors[:3]
    if mistake == "strict_greater":                                  # only q = 1 sits on a step of these inputs
        assert all("quantile 2 (q = 1.0" in e for e in errors), errors[:3]


def test_comparator_accepts_a_neighbour_only_where_loose():
    C_cells = 9
    cen = S.centroids_of(C_cells, 3)
    logits = np.zeros((1, C_cells), dtype=np.float32)
    pts = S.points_of(1, 1, 3)
    t = S.truth(logits, cen, pts, (3 / 9,))                          # q C is an integer: on a step, loose
    assert not t["tight"].any()
    ek, es, rk = S.plain(logits, cen, pts, (3 / 9,))
    for k in (t["lo_key"], t["key"], t["hi_key"]):
        errors, loose, _ = S.compare(t, ek, es, k)
        assert not errors and loose == 1
    errors, _, _ = S.compare(t, ek, es, t["hi_key"] + 1.0)
    assert errors and "loose" in errors[0]
    assert S.loose_allowed(t) == 0                                   # one loose of one quantile is over the 1 % cap
    t = S.truth(logits, cen, pts, (S.uniform_quantile(C_cells),))
    assert t["tight"].all()
    errors, _, _ = S.compare(t, ek, es, t["hi_key"])
    assert errors


# ================================================================================================================ coverage metrics
def test_spread_metrics_on_planted_arrays():
    from pigeon_amd.evaluate import spread_metrics
    radius = np.array([[10.0, 100.0], [10.0, 100.0], [10.0, 100.0], [np.nan, 100.0]])
    dist = np.array([10.0, 10.5, 5.0, 1.0])                          # on the radius counts as covered; a NaN radius covers nothing
    m = spread_metrics(radius, (0.5, 0.9), dist, expected_km=[1.0, 2.0, 3.0, 6.0], expected_score=[5000.0, 0.0, 0.0, 0.0])
    assert m["Radius_50_coverage"] == 0.5 and m["Radius_90_coverage"] == 1.0
    assert m["Median_radius_90_km"] == 100.0 and np.isnan(m["Median_radius_50_km"])
    assert m["Mean_expected_km"] == 3.0 and m["Mean_expected_score"] == 1250.0
    assert S.coverage_np(radius[:, 0], dist) == m["Radius_50_coverage"]
    assert set(spread_metrics(radius[:, :1], (0.75,), dist)) == {"Radius_75_coverage", "Median_radius_75_km"}
    with pytest.raises(ValueError):
        spread_metrics(radius, (0.5,), dist)


def test_cell_extents_from_polygons():
    from pigeon_amd.regions import RegionBank, cell_extents_km
    bank = RegionBank.from_wkt(["POLYGON ((0 0, 2 0, 2 1, 0 1, 0 0))",
                                "MULTIPOLYGON (((179 10, 180 10, 180 11, 179 10)), ((-180 10, -178 10, -178 12, -180 10)))"])
    cen = np.array([[0.5, 0.5], [179.5, 10.5]])
    got = cell_extents_km(bank, cen)
    for r in range(2):
        d, a = G.haversine_truth(cen[r], bank.xy[bank.ring_off[bank.region_off[r]]:bank.ring_off[bank.region_off[r + 1]]])
        assert abs(got[r] - float(d.max())) <= 16 * G.U(a).max()
    assert got[1] < 400                                              # across the antimeridian, not around the globe
    with pytest.raises(ValueError):
        cell_extents_km(bank, cen[:1])


# ================================================================================================================ the library, no GPU
FAKE = C.c_void_p(0x1000)                                            # never dereferenced: every call below returns before any HIP call
NULL = C.c_void_p(0)


def _call(lib, B=2, Cn=8, G_pts=1, q=(0.5, 0.9), nq=None, logits=FAKE, cen=FAKE, ext=NULL, pts=FAKE, ek=FAKE, es=FAKE, rk=FAKE,
          qnull=False):
    arr = (C.c_double * max(len(q), 1))(*q)
    rc = lib.pg_guess_spread(logits, B, Cn, cen, ext, pts, G_pts, None if qnull else arr, len(q) if nq is None else nq, ek, es, rk, NULL)
    return rc, lib.pg_last_error().decode()


def test_refusals_before_any_hip_call(hip_lib):
    for kw, word in ((dict(Cn=0), "C must be"), (dict(Cn=-3), "C must be"), (dict(nq=0), "nq must be"), (dict(q=(0.1,) * 5), "nq must be"),
                     (dict(q=(0.5, 0.0)), "quantiles[1]"), (dict(q=(1.5,)), "quantiles[0]"), (dict(q=(-0.1,)), "quantiles[0]"),
                     (dict(q=(0.5, 0.9, float("nan"))), "quantiles[2]"), (dict(q=(float("inf"),)), "quantiles[0]"),
                     (dict(qnull=True), "quantiles"), (dict(B=-1), "B ="), (dict(G_pts=-1), "G ="),
                     (dict(logits=NULL), "logits"), (dict(cen=NULL), "centroids"), (dict(pts=NULL), "points"),
                     (dict(ek=NULL), "expected_km"), (dict(es=NULL), "expected_score"), (dict(rk=NULL), "radius_km"),
                     (dict(B=70000, G_pts=70000), "B * G")):
        rc, msg = _call(hip_lib, **kw)
        assert rc == -1 and msg.startswith("guess_spread") and word in msg, (kw, rc, msg)


def test_empty_batches_are_noops(hip_lib):
    every_null = dict(logits=NULL, cen=NULL, pts=NULL, ek=NULL, es=NULL, rk=NULL)
    assert _call(hip_lib, B=0, **every_null)[0] == 0
    assert _call(hip_lib, G_pts=0, **every_null)[0] == 0
    assert _call(hip_lib, B=0, G_pts=0, q=(1.0,), **every_null)[0] == 0
    assert _call(hip_lib, B=0, Cn=0, **every_null)[0] == -1           # the scalars are checked first, whatever the batch


def test_plan(hip_lib):
    from pigeon_amd import hip_ops
    one = hip_ops.guess_spread_plan(1)
    assert one == {"form": 0, "lds_bytes": 16, "lds_cells": one["lds_cells"], "threads": 256}
    top = one["lds_cells"]
    assert 2076 < top and 16 * top <= 160 * 1024 - 1024             # a CU's 160 KB of LDS, less the kernel's static arrays
    assert hip_ops.guess_spread_plan(top) == {"form": 0, "lds_bytes": 16 * top, "lds_cells": top, "threads": 256}
    assert hip_ops.guess_spread_plan(top + 1) == {"form": 1, "lds_bytes": 0, "lds_cells": top, "threads": 256}
    assert hip_ops.guess_spread_plan(2 ** 31 - 1)["form"] == 1
    out = (C.c_int32 * 4)()
    assert hip_lib.pg_guess_spread_plan(0, out) == -1 and "C must be" in hip_lib.pg_last_error().decode()
    assert hip_lib.pg_guess_spread_plan(5, None) == -1 and "out" in hip_lib.pg_last_error().decode()


def test_front_end_refuses_by_name(hip_lib):
    from pigeon_amd import hip_ops, _lib
    with pytest.raises(_lib.PigeonHipError, match="device tensor"):
        hip_ops.guess_spread(torch.zeros(2, 8), torch.zeros(8, 2, dtype=torch.float64), torch.zeros(2, 2, dtype=torch.float64))


# ================================================================================================================ serving keys
TopK = namedtuple("TopK", ["values", "indices"])
Spread = namedtuple("Spread", "expected_km expected_score radius_km quantiles")


class StubModel:
    def __call__(self, pixel_values=None):
        llh = torch.tensor([[12.5, -33.25]], dtype=torch.float64)
        return llh, TopK(torch.ones(1, 5), torch.arange(5)[None]), torch.zeros(1, 4, 1024)


class StubSpreadModel(StubModel):
    def __init__(self):
        self.asked = None

    def spread(self, points=None, quantiles=(0.5, 0.9), state=None):
        self.asked = (points.clone(), tuple(quantiles))
        return Spread(torch.tensor([321.5], dtype=torch.float64), torch.tensor([4100.25], dtype=torch.float64),
                      torch.tensor([[40.0, 900.0]], dtype=torch.float64), tuple(quantiles))


class StubRefiner:
    def __call__(self, embedding=None, initial_preds=None, candidate_cells=None, candidate_probs=None):
        return None, initial_preds.to(torch.float32) + torch.tensor([[1.0, 2.0]]), torch.zeros(1, dtype=torch.int64)


def _body():
    from PIL import Image
    img = Image.fromarray(np.random.default_rng(1).integers(0, 255, (60, 80, 3), dtype=np.uint8))
    buf = io.BytesIO()
    img.save(buf, format="PNG")
    return {"gameID": "g", "roundID": 1, "image": "data:image/png;base64," + base64.b64encode(buf.getvalue()).decode()}


def test_serving_keys_with_stub_models():
    from starlette.testclient import TestClient
    from pigeon_amd import serve
    from pigeon_amd.clip_embedder import clip_preprocess
    model = StubSpreadModel()
    plain = TestClient(serve.make_app(model, preprocess=clip_preprocess)).post("/api/v1/predict", json=_body()).json()["results"]
    assert set(plain) == {"lat", "lng"} and model.asked is None      # nothing is computed unless asked for
    res = TestClient(serve.make_app(model, StubRefiner(), preprocess=clip_preprocess, spread=True)).post("/api/v1/predict", json=_body())
    assert res.status_code == 200
    r = res.json()["results"]
    assert (r["lat"], r["lng"]) == (-31.25, 13.5)                    # what the extension reads: unchanged
    assert r["expected_km"] == 321.5 and r["expected_score"] == 4100.25 and r["radius_km"] == {"0.5": 40.0, "0.9": 900.0}
    pts, qs = model.asked
    assert qs == serve.SPREAD_QUANTILES == (0.5, 0.9)
    assert pts.dtype == torch.float64 and pts.tolist() == [[13.5, -31.25]]       # the REFINED point
    with pytest.raises(ValueError, match="spread"):
        serve.make_app(StubModel(), preprocess=clip_preprocess, spread=True)
    with pytest.raises(ValueError, match="spread"):
        serve.predict_panorama([None] * 4, StubModel(), spread=True)
    assert serve._arg_parser().parse_args(["--spread"]).spread and not serve._arg_parser().parse_args([]).spread
