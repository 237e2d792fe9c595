"""Writes the synthetic fixtures of the point-in-region tests (tests/test_regions_cpu.py, tests/test_gpu_regions.py):

  tests/golden/regions_countries.geojson   six "countries": a hole, an island inside a lake plus a far part, a region touching
                                           lng = +-180, a region that fills another one's hole (shared boundary), an overlapping
                                           region, a 33-edge star
  tests/golden/regions_geocells.csv        a 6 x 4 grid of 10-degree geocells in the columns of the reference's geocell table
                                           (name, lng, lat, polygon as WKT); one cell is written as a MULTIPOLYGON of two halves
  tests/golden/regions_metadata.csv        48 points (lng, lat): inside cells, on shared edges and corners, outside the grid

Deterministic; run from the repository root:  python tools/make_regions_golden.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from _regionref import box, star, to_wkt  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def countries():
    """name -> list of polygons, each a list of rings (shell first, then holes)"""
    return [
        ("Holed", [[box(-10, -10, 10, 10), box(-4, -4, 4, 4)[::-1]]]),
        ("Lakeisle", [[box(20, 0, 40, 20), box(24, 4, 36, 16)[::-1]], [box(28, 8, 32, 12)], [star(7, 60.0, 40.0, 2.0, 5.0)]]),
        ("Dateline", [[box(170, -20, 180, 20)], [box(-180, -20, -170, 20)]]),
        ("Plug", [[box(-4, -4, 4, 4)]]),
        ("Overlap", [[box(0, 0, 6, 6)]]),
        ("Star", [[star(33, -60.0, 30.0, 3.0, 8.0)]]),
    ]


def geocells():
    rows = []
    for iy in range(4):
        for ix in range(6):
            x0, y0 = -30.0 + 10 * ix, -20.0 + 10 * iy
            polys = [[box(x0, y0, x0 + 10, y0 + 10)]]
            if (ix, iy) == (2, 1):                                          # the same cell as two halves
                polys = [[box(x0, y0, x0 + 5, y0 + 10)], [box(x0 + 5, y0, x0 + 10, y0 + 10)]]
            rows.append((f"cell_{iy}_{ix}", x0 + 5, y0 + 5, to_wkt(polys)))
    return rows


def metadata():
    rng = np.random.default_rng(7)
    inside = np.stack([rng.uniform(-30, 30, 30), rng.uniform(-20, 20, 30)], axis=1)
    edges = np.array([[-20.0, 3.5], [0.0, 0.0], [10.0, -10.0], [7.25, 10.0], [-30.0, -20.0], [30.0, 20.0], [-15.0, -5.0], [12.5, 20.0]])
    outside = np.array([[35.0, 0.0], [-31.0, 19.0], [0.0, 25.0], [0.0, -20.5], [100.0, 60.0], [-30.0, 45.0], [30.0, -20.0 - 2.0 ** -40],
                        [44.0, 31.0], [-33.0, -24.0], [5.0, 20.0 + 2.0 ** -45]])
    return np.concatenate([inside, edges, outside])


def main():
    os.makedirs(GOLDEN, exist_ok=True)
    feats = []
    for name, polys in countries():
        coords = [[[[float(x), float(y)] for x, y in ring] for ring in poly] for poly in polys]
        geom = {"type": "Polygon", "coordinates": coords[0]} if len(coords) == 1 else {"type": "MultiPolygon", "coordinates": coords}
        feats.append({"type": "Feature", "properties": {"ADMIN": name}, "geometry": geom})
    with open(os.path.join(GOLDEN, "regions_countries.geojson"), "w") as f:
        json.dump({"type": "FeatureCollection", "features": feats}, f, indent=0)
        f.write("\n")
    with open(os.path.join(GOLDEN, "regions_geocells.csv"), "w") as f:
        f.write("name,lng,lat,polygon\n")
        for name, lng, lat, wkt in geocells():
            f.write(f'{name},{lng!r},{lat!r},"{wkt}"\n')
    with open(os.path.join(GOLDEN, "regions_metadata.csv"), "w") as f:
        f.write("id,lng,lat\n")
        for i, (x, y) in enumerate(metadata()):
            f.write(f"{i},{float(x)!r},{float(y)!r}\n")
    print("written:", ", ".join(sorted(n for n in os.listdir(GOLDEN) if n.startswith("regions_"))))


if __name__ == "__main__":
    main()
