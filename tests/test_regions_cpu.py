"""The host half of the point-in-region lookup (no GPU): the three loaders of pigeon_amd.regions.RegionBank on the synthetic fixtures
tests/golden/regions_* (tools/make_regions_golden.py), every refusal and its message, the rational fallback `exact_state` against the
independent reference tests/_regionref.py, the C side's checks of a bank (pg_region_plan runs them without a GPU), and that
compute_geoguessr_metrics without `countries` returns exactly the keys it returned before."""
import json
import os
import sys

import numpy as np
import pytest

import _regionref as ref
from _regionref import BOUNDARY, INSIDE, OUTSIDE, box, star, to_wkt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rg():
    from pigeon_amd import regions
    return regions


# ------------------------------------------------------------------------------------------------ loaders
def test_geojson_loader(rg, golden_dir):
    bank = rg.RegionBank.from_geojson(os.path.join(golden_dir, "regions_countries.geojson"))
    assert len(bank) == 6 and [p["ADMIN"] for p in bank.names] == ["Holed", "Lakeisle", "Dateline", "Plug", "Overlap", "Star"]
    assert bank.region_off.tolist() == [0, 2, 6, 8, 9, 10, 11]
    assert bank.ring_off.tolist() == [0, 5, 10, 15, 20, 25, 33, 38, 43, 48, 53, 87]
    assert bank.xy.shape == (87, 2) and bank.xy.dtype == np.float64
    for r in range(11):                                                          # closure stored, boxes exact
        ring = bank.xy[bank.ring_off[r]:bank.ring_off[r + 1]]
        assert (ring[0] == ring[-1]).all()
        assert bank.ring_bbox[r].tolist() == [ring[:, 0].min(), ring[:, 1].min(), ring[:, 0].max(), ring[:, 1].max()]
    assert bank.region_bbox[0].tolist() == [-10, -10, 10, 10] and bank.region_bbox[2].tolist() == [-180, -20, 180, 20]
    assert np.array_equal(bank.rings(5)[0], star(33, -60.0, 30.0, 3.0, 8.0))     # every float survives the file
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_regions_golden as tool
    for g, (_, polys) in enumerate(tool.countries()):
        want = [ring for poly in polys for ring in poly]
        assert len(bank.rings(g)) == len(want) and all(np.array_equal(a, b) for a, b in zip(bank.rings(g), want))


def test_wkt_and_geocell_csv_loaders(rg, golden_dir):
    cells = rg.RegionBank.from_geocell_csv(os.path.join(golden_dir, "regions_geocells.csv"))
    assert len(cells) == 24 and cells.names[0] == "cell_0_0" and cells.names[-1] == "cell_3_5"
    assert cells.region_off.tolist() == list(range(9)) + list(range(10, 26))     # cell 8 = (ix 2, iy 1) is a MULTIPOLYGON of two rings
    assert np.array_equal(cells.rings(0)[0], box(-30, -20, -20, -10)) and np.array_equal(cells.rings(23)[0], box(20, 10, 30, 20))
    assert np.array_equal(cells.rings(8)[0], box(-10, -10, -5, 0)) and np.array_equal(cells.rings(8)[1], box(-5, -10, 0, 0))
    shell, hole, isle = star(9, 1.0, 2.0, 0.5, 1.5), box(0.9, 1.9, 1.1, 2.1)[::-1], box(5, 5, 6, 6)
    bank = rg.RegionBank.from_wkt([to_wkt([[shell, hole]]), to_wkt([[shell, hole], [isle]]), "  polygon((0 0,1 0 , 1 1,0 0))  ",
                                   "MULTIPOLYGON (((1e-3 -2.5E+1, 2 3, 4 -5, 1e-3 -2.5E+1)))"], names=["a", "b", "c", "d"])
    assert bank.region_off.tolist() == [0, 2, 5, 6, 7] and bank.names == ["a", "b", "c", "d"]
    assert np.array_equal(bank.rings(0)[0], shell) and np.array_equal(bank.rings(1)[1], hole) and np.array_equal(bank.rings(1)[2], isle)
    assert bank.rings(3)[0].tolist() == [[0.001, -25.0], [2.0, 3.0], [4.0, -5.0], [0.001, -25.0]]
    direct = rg.RegionBank([[shell, hole], []])                                  # a region without rings covers nothing
    assert direct.region_off.tolist() == [0, 2, 2] and direct.region_bbox[1, 0] > direct.region_bbox[1, 2]


@pytest.mark.parametrize("text, message", [
    ("POINT (1 2)", "region 0: not a POLYGON / MULTIPOLYGON WKT string"),
    ("POLYGON EMPTY", "region 0: not a POLYGON / MULTIPOLYGON WKT string"),
    ("POLYGON (((0 0, 1 0, 1 1, 0 0)))", "region 0: unbalanced or wrongly nested parentheses for a POLYGON"),
    ("MULTIPOLYGON ((0 0, 1 0, 1 1, 0 0))", "wrongly nested parentheses for a MULTIPOLYGON"),
    ("POLYGON ((0 0, 1 0, 1 1, 0 0)", "unbalanced or wrongly nested parentheses for a POLYGON"),
    ("POLYGON (0 0, 1 0, 1 1, 0 0", "not a POLYGON / MULTIPOLYGON WKT string"),
    ("POLYGON ((0 0, 1 0), 1 1, 0 0))", "unbalanced or wrongly nested"),
    ("POLYGON ((0 0, 1 x, 1 1, 0 0))", "region 0, ring 0: a coordinate is not a number"),
    ("POLYGON ((0 0 5, 1 0 5, 1 1 5, 0 0 5))", "region 0, ring 0: every position must be two numbers"),
    ("POLYGON ((0 0, 1 0, 0 0))", "region 0, ring 0: 3 positions; a closed ring needs at least 4"),
    ("POLYGON ((0 0, 1 0, 1 1, 0 1))", r"region 0, ring 0: not closed \(first position \(0.0, 0.0\), last \(0.0, 1.0\)\)"),
    ("POLYGON ((0 0, 2 0, 2 2, 0 0), (1 0.5, 1.5 0.5, nan 1, 1 0.5))", "region 0, ring 1: position 2 is not finite"),
    ("POLYGON ((0 0, 181 0, 1 1, 0 0))", r"region 0, ring 0: position 1 = \(181.0, 0.0\) is outside \|lng\| <= 180, \|lat\| <= 90"),
    ("POLYGON ((0 0, 1 0, 1 -90.5, 0 0))", r"position 2 = \(1.0, -90.5\) is outside"),
])
def test_loader_refusals(rg, text, message):
    with pytest.raises(ValueError, match=message):
        rg.RegionBank.from_wkt([text])
    with pytest.raises(ValueError, match=message.replace("region 0", "region 1")):
        rg.RegionBank.from_wkt(["POLYGON ((0 0, 1 0, 1 1, 0 0))", text])


def test_file_refusals(rg, tmp_path):
    path = os.path.join(str(tmp_path), "x.geojson")
    feature = lambda geom: {"type": "Feature", "properties": {}, "geometry": geom}       # noqa: E731
    cases = [({"type": "Feature"}, "not a GeoJSON FeatureCollection"),
             ({"type": "FeatureCollection", "features": [feature({"type": "Polygon", "coordinates": [box(0, 0, 1, 1).tolist()]}),
                                                         feature({"type": "LineString", "coordinates": [[0, 0], [1, 1]]})]},
              "feature 1 has geometry type 'LineString'; only Polygon and MultiPolygon are regions"),
             ({"type": "FeatureCollection", "features": [feature(None)]}, "feature 0 has geometry type None"),
             ({"type": "FeatureCollection", "features": [feature({"type": "Polygon", "coordinates": [[[0, 0], [1], [1, 1], [0, 0]]]})]},
              "feature 0: malformed coordinates"),
             ({"type": "FeatureCollection", "features": [feature({"type": "Polygon", "coordinates": [[[0, 0], [1, 0], [1, 1], [0, 1]]]})]},
              "region 0, ring 0: not closed")]
    for doc, message in cases:
        with open(path, "w") as f:
            json.dump(doc, f)
        with pytest.raises(ValueError, match=message):
            rg.RegionBank.from_geojson(path)
    csv = os.path.join(str(tmp_path), "cells.csv")
    with open(csv, "w") as f:
        f.write("name,lng,lat\na,0,0\n")
    with pytest.raises(ValueError, match="no `polygon` column"):
        rg.RegionBank.from_geocell_csv(csv)
    # a position's third number (an altitude) is dropped, as GeoJSON allows it
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "features": [feature({"type": "Polygon", "coordinates": [[[0, 0, 9], [1, 0, 9], [1, 1, 9], [0, 0, 9]]]})]}, f)
    assert rg.RegionBank.from_geojson(path).xy.tolist() == [[0, 0], [1, 0], [1, 1], [0, 0]]


def test_point_refusals_and_no_gpu(rg, golden_dir):
    bank = rg.RegionBank.from_geojson(os.path.join(golden_dir, "regions_countries.geojson"))
    with pytest.raises(ValueError, match=r"find_regions: expected \(N, 2\) \[lng, lat\] points, got shape \(3,\)"):
        rg.find_regions(bank, np.zeros(3))
    with pytest.raises(ValueError, match="find_regions: point 1 is not finite"):
        rg.find_regions(bank, np.array([[0.0, 0.0], [np.nan, 1.0]]))
    with pytest.raises(ValueError, match="the bank has no regions"):
        rg.find_regions(rg.RegionBank([]), np.zeros((1, 2)))
    idx, info = rg.find_regions(bank, np.zeros((0, 2)))
    assert idx.shape == (0,) and info == dict(ambiguous=0, nearest=0)
    import torch
    if not torch.cuda.is_available():                                            # no host fallback for the device part
        from pigeon_amd._lib import PigeonHipError
        for call in (lambda: rg.find_regions(bank, np.zeros((1, 2))), lambda: rg.country_accuracy(np.zeros((1, 2)), np.zeros((1, 2)), bank),
                     lambda: rg.assign_geocells(np.zeros((1, 2)), bank), lambda: rg.contains(bank, np.zeros((1, 2)), [0])):
            with pytest.raises(PigeonHipError):
                call()


# ------------------------------------------------------------------------------------------------ the rational fallback
def test_exact_state_matches_the_reference(rg, golden_dir):
    bank = rg.RegionBank.from_geojson(os.path.join(golden_dir, "regions_countries.geojson"))
    regions = [bank.rings(g) for g in range(len(bank))]
    rng = np.random.default_rng(0)
    generic = np.concatenate([np.stack([rng.uniform(-12, 42, 250), rng.uniform(-12, 22, 250)], axis=1),
                              np.stack([rng.uniform(-70, -50, 60), rng.uniform(20, 40, 60)], axis=1)])
    special = np.array([[4, 4], [0, 4], [-4, 0], [10, -10], [30, 10], [28, 9], [24, 10], [36, 16], [32, 12], [180, 0], [-180, 3], [170, 20], [6, 6], [0, 0],
                        [3, 0], [6, 3], [np.nextafter(4.0, 5.0), 1.0], [np.nextafter(4.0, 0.0), 1.0], [1.0, np.nextafter(-4.0, -5.0)],
                        [np.nextafter(180.0, 0.0), 7.0], [28, 8], [30, 4], [2 ** -1074, 0.0], [-4.0, 2 ** -1074]], dtype=np.float64)
    seen = set()
    for p in np.concatenate([generic, special]):
        for g in range(len(bank)):
            want = ref.state(regions[g], p)
            assert rg.exact_state(bank, p, g) == want, (p, g)
            seen.add(want)
    assert seen == {OUTSIDE, INSIDE, BOUNDARY}
    for rings, first in zip(regions, bank.xy[bank.ring_off[bank.region_off[:-1]]]):       # every region's first vertex is on its boundary
        assert ref.state(rings, first) == BOUNDARY
    # a point on a long diagonal edge, where fp64 determinants round: exact either way
    tri = rg.RegionBank([[np.array([[0.1, 0.1], [0.7, 0.3], [0.2, 0.9], [0.1, 0.1]])]])
    a, b = tri.xy[0], tri.xy[1]
    for t in (0.25, 0.5, 0.3):
        p = a + t * (b - a)                                                      # rounded: near the edge, rarely on it
        assert rg.exact_state(tri, p, 0) == ref.state(tri.rings(0), p)


# ------------------------------------------------------------------------------------------------ the C side's checks, without a GPU
def test_bank_checks_and_plan(rg, hip_lib):
    from pigeon_amd import hip_ops
    from pigeon_amd._lib import PigeonHipError
    bank = rg.RegionBank([[star(128)], [box(0, 0, 1, 1), box(0.2, 0.2, 0.4, 0.4)[::-1]]])
    try:
        assert hip_ops.region_plan(bank.handle) == {"form": 0, "threads": 64, "max_ring_edges": 128, "wave_edges": 128}
        hip_ops.tune_region_wave_edges(127)
        assert hip_ops.region_plan(bank.handle) == {"form": 1, "threads": 256, "max_ring_edges": 128, "wave_edges": 127}
        hip_ops.tune_region_wave_edges(0)
        assert hip_ops.region_plan(rg.RegionBank([[box(0, 0, 1, 1)]]).handle)["form"] == 1
        hip_ops.tune_region_wave_edges(2 ** 31 - 1)
        assert hip_ops.region_plan(rg.RegionBank([[star(1025)]]).handle)["form"] == 0
    finally:
        hip_ops.tune_region_wave_edges(-1)
    assert hip_ops.region_plan(rg.RegionBank([]).handle) == {"form": 0, "threads": 64, "max_ring_edges": 0, "wave_edges": 128}
    h = bank.handle
    saved = (h.region_off.copy(), h.ring_off.copy())
    for array, at, value, message in [
            (h.region_off, 0, 1, r"region_off\[0\] is 1, not 0"),
            (h.region_off, 1, 4, r"region 0: region_off goes from 0 to 4 \(the bank has 3 rings\)"),
            (h.region_off, 1, -1, r"region 0: region_off goes from 0 to -1"),
            (h.region_off, 2, 2, r"region_off ends at 2, the bank has 3 rings"),
            (h.ring_off, 0, 2, r"ring_off\[0\] is 2, not 0"),
            (h.ring_off, 1, 500, r"ring 0: ring_off goes from 0 to 500 \(a ring needs at least 2 vertices; the bank has 139\)"),
            (h.ring_off, 2, 130, r"ring 1: ring_off goes from 129 to 130"),
            (h.ring_off, 3, 138, r"ring_off ends at 138, the bank has 139 vertices")]:
        array[at] = value
        with pytest.raises(PigeonHipError, match="region_plan: " + message):
            hip_ops.region_plan(h)
        h.region_off[:], h.ring_off[:] = saved
    assert hip_ops.region_plan(h)["max_ring_edges"] == 128


def test_region_kernels_have_no_spills_and_no_waterfall_loops(hip_lib):
    """the six kernels of csrc/regions.hip (three entry points, two forms each) in the built library's ISA"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import asm_audit
    res = {k: v for k, v in asm_audit.audit(os.path.join(ROOT, "pigeon_amd", "libpigeon_hip.so")).items() if "region_" in k and "_kernel" in k}
    assert len(res) == 6 and sum("locate" in k for k in res) == 2 and sum("classify" in k for k in res) == 2 and sum("nearest" in k for k in res) == 2, sorted(res)
    for name, v in res.items():
        assert v["scratch"] == 0 and v["waterfall"] == 0 and 0 < v["vgpr"] <= 64 and v["agpr"] == 0, (name, v)


# ------------------------------------------------------------------------------------------------ the metrics dict
def test_metrics_without_countries_keep_their_keys():
    from oracle import geo_oracle
    from pigeon_amd.evaluate import compute_geoguessr_metrics
    import inspect
    rng = np.random.default_rng(1)
    n = 40
    preds = np.stack([rng.uniform(-180, 180, n), rng.uniform(-90, 90, n)], axis=1).astype(np.float32)
    labels = np.stack([rng.uniform(-180, 180, n), rng.uniform(-90, 90, n)], axis=1)
    cell_preds, cell_labels = rng.integers(0, 50, n), rng.integers(0, 50, n)
    top5 = rng.integers(0, 50, (n, 5))
    got = compute_geoguessr_metrics((preds, cell_preds, None, None, None, top5, labels, cell_labels, None, None, None))
    want = geo_oracle.geoguessr_metrics(preds, labels, cell_preds, cell_labels, top5)
    assert list(got) == list(want) and "Country_accuracy" not in got
    for k in want:
        assert got[k] == want[k], k
    sig = inspect.signature(compute_geoguessr_metrics)
    assert list(sig.parameters) == ["results", "scaler", "countries"] and sig.parameters["countries"].default is None
    from pigeon_amd.evaluate import evaluate
    assert inspect.signature(evaluate).parameters["country_path"].default is None
