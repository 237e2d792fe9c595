"""Exact point-in-region lookup: `Country_accuracy` and the geocell labels without geopandas / shapely.

Reference semantics (the device half is csrc/regions.hip):
  find_country          evaluation/metrics.py:56-72                      the first region that covers the point -- interior or boundary,
  generate_cell_labels  preprocessing/dataset_preprocessing.py:60-94     `covered_by` -- else the nearest one (planar distance in degrees
                                                                         to the region's boundary, as GEOS computes it on EPSG:4326)
  country_accuracy      evaluation/metrics.py:74-88                      correct iff the label's country `contains` the prediction:
                                                                         strictly interior, a prediction on the boundary is wrong
Two stated deviations: where several regions cover a point the LOWEST index is returned (the reference returns
whatever order its STRtree yields), and `buffer(0)` (metrics.py:19) is not reproduced -- the loaders check the rings and a region is
the even-odd set of all its rings, the same set for valid polygons.

The device classifies every (point, region) pair as certainly OUTSIDE, certainly INSIDE or AMBIGUOUS and never guesses; the ambiguous
pairs -- every point on a ring among them -- are settled here in `fractions.Fraction` (floats are exact rationals, so there is no
tolerance anywhere).  There is no host fallback for the device part: without a GPU the lookups raise PigeonHipError.

  python -m pigeon_amd.regions --geocells data/geocells_2203.csv --metadata data/metadata.csv -o data/metadata_labeled.csv
"""
from __future__ import annotations

import json
import re
from fractions import Fraction
from typing import List, Optional, Sequence, Tuple

import numpy as np

OUTSIDE, INSIDE, AMBIGUOUS, BOUNDARY = 0, 1, 2, 3       # 0..2: the device's states (PG_REGION_*); BOUNDARY: exact_state only

_WKT_HEAD = re.compile(r"^\s*(MULTIPOLYGON|POLYGON)\s*(\(.*\))\s*$", re.I | re.S)
_WKT_RING = re.compile(r"\(([^()]*)\)")


class RegionBank:
    """R regions, each a list of closed rings (all polygons' shells and holes of a multipolygon, in any order: the region is their
    even-odd set), in the CSR form of pg_region_bank: region_off (R+1), ring_off (n_rings+1), xy (n_vertices, 2) fp64 [lng, lat] with
    the closure vertex stored, ring_bbox (n_rings, 4) and region_bbox (R, 4) as [min lng, min lat, max lng, max lat]."""

    def __init__(self, regions: Sequence[Sequence[np.ndarray]], names: Optional[Sequence] = None):
        region_off, ring_off, xy, ring_bbox, region_bbox = [0], [0], [], [], []
        for g, rings in enumerate(regions):
            for k, ring in enumerate(rings):
                ring = _check_ring(ring, g, k)
                xy.append(ring)
                ring_off.append(ring_off[-1] + ring.shape[0])
                ring_bbox.append([ring[:, 0].min(), ring[:, 1].min(), ring[:, 0].max(), ring[:, 1].max()])
            region_off.append(len(ring_bbox))
            mine = np.asarray(ring_bbox[region_off[-2]:], dtype=np.float64).reshape(-1, 4)
            # a region without rings covers nothing: an empty box (min > max) that no point is in
            region_bbox.append([mine[:, 0].min(), mine[:, 1].min(), mine[:, 2].max(), mine[:, 3].max()] if len(mine) else [1.0, 1.0, 0.0, 0.0])
        self.region_off = np.asarray(region_off, dtype=np.int64)
        self.ring_off = np.asarray(ring_off, dtype=np.int64)
        self.xy = np.concatenate(xy, axis=0) if xy else np.zeros((0, 2))
        self.ring_bbox = np.asarray(ring_bbox, dtype=np.float64).reshape(-1, 4)
        self.region_bbox = np.asarray(region_bbox, dtype=np.float64).reshape(-1, 4)
        self.names = list(names) if names is not None else None
        self._handle = None

    def __len__(self) -> int:
        return self.region_off.size - 1

    def rings(self, region: int) -> List[np.ndarray]:
        return [self.xy[self.ring_off[r]:self.ring_off[r + 1]] for r in range(self.region_off[region], self.region_off[region + 1])]

    @property
    def handle(self):
        """The pg_region_bank of this bank (pigeon_amd.hip_ops.RegionBankHandle); the device copies are made at the first lookup."""
        if self._handle is None:
            from . import hip_ops
            self._handle = hip_ops.RegionBankHandle(self.region_off, self.ring_off, self.xy, self.ring_bbox, self.region_bbox)
        return self._handle

    # ------------------------------------------------------------------------------------------------ loaders
    @classmethod
    def from_wkt(cls, strings: Sequence[str], names: Optional[Sequence] = None) -> "RegionBank":
        """One region per string: `POLYGON ((x y, ...), (hole), ...)` or `MULTIPOLYGON (((...)), ((...), (...)))`."""
        return cls([_parse_wkt(s, g) for g, s in enumerate(strings)], names)

    @classmethod
    def from_geojson(cls, path: str) -> "RegionBank":
        """A FeatureCollection of Polygon / MultiPolygon features (the file config.COUNTRY_PATH names: reference metrics.py:17);
        `names` are the features' property dicts."""
        with open(path) as f:
            doc = json.load(f)
        if not isinstance(doc, dict) or doc.get("type") != "FeatureCollection" or not isinstance(doc.get("features"), list):
            raise ValueError(f"{path}: not a GeoJSON FeatureCollection")
        regions, names = [], []
        for g, feat in enumerate(doc["features"]):
            geom = (feat or {}).get("geometry") or {}
            kind, coords = geom.get("type"), geom.get("coordinates")
            if kind == "Polygon":
                polys = [coords]
            elif kind == "MultiPolygon":
                polys = coords
            else:
                raise ValueError(f"{path}: feature {g} has geometry type {kind!r}; only Polygon and MultiPolygon are regions")
            try:
                rings = [np.asarray([pos[:2] for pos in ring], dtype=np.float64).reshape(-1, 2) for poly in polys for ring in poly]
            except (TypeError, ValueError, IndexError) as why:
                raise ValueError(f"{path}: feature {g}: malformed coordinates ({why})") from None
            regions.append(rings)
            names.append(feat.get("properties"))
        return cls(regions, names)

    @classmethod
    def from_geocell_csv(cls, path: str) -> "RegionBank":
        """The `polygon` WKT column of a geocell CSV, row order = geocell index (reference dataset_preprocessing.py:48-58 load_geocell_df)."""
        import pandas as pd
        df = pd.read_csv(path)
        if "polygon" not in df.columns:
            raise ValueError(f"{path}: no `polygon` column (columns: {list(df.columns)})")
        return cls.from_wkt([str(s) for s in df["polygon"]], list(df["name"]) if "name" in df.columns else None)


def _check_ring(ring, g: int, k: int) -> np.ndarray:
    ring = np.ascontiguousarray(ring, dtype=np.float64)
    where = f"region {g}, ring {k}"
    if ring.ndim != 2 or ring.shape[1] != 2:
        raise ValueError(f"{where}: expected (n, 2) positions, got shape {ring.shape}")
    if ring.shape[0] < 4:
        raise ValueError(f"{where}: {ring.shape[0]} positions; a closed ring needs at least 4")
    if not np.isfinite(ring).all():
        raise ValueError(f"{where}: position {int(np.argwhere(~np.isfinite(ring).all(axis=1))[0, 0])} is not finite")
    if (np.abs(ring[:, 0]) > 180).any() or (np.abs(ring[:, 1]) > 90).any():
        j = int(np.argwhere((np.abs(ring[:, 0]) > 180) | (np.abs(ring[:, 1]) > 90))[0, 0])
        raise ValueError(f"{where}: position {j} = ({float(ring[j, 0])!r}, {float(ring[j, 1])!r}) is outside |lng| <= 180, |lat| <= 90")
    if not (ring[0] == ring[-1]).all():
        raise ValueError(f"{where}: not closed (first position {tuple(ring[0].tolist())}, last {tuple(ring[-1].tolist())})")
    return ring


def _parse_wkt(text: str, g: int) -> List[np.ndarray]:
    m = _WKT_HEAD.match(text)
    if not m:
        raise ValueError(f"region {g}: not a POLYGON / MULTIPOLYGON WKT string: {text[:60]!r}")
    kind, body = m.group(1).upper(), m.group(2)
    depth = most = 0
    for ch in body:
        depth += (ch == "(") - (ch == ")")
        most = max(most, depth)
        if depth < 0:
            break
    if depth != 0 or most != (2 if kind == "POLYGON" else 3):
        raise ValueError(f"region {g}: unbalanced or wrongly nested parentheses for a {kind}")
    rings = []
    for k, inner in enumerate(_WKT_RING.findall(body)):
        try:
            pos = [[float(v) for v in p.split()] for p in inner.split(",")]
        except ValueError:
            raise ValueError(f"region {g}, ring {k}: a coordinate is not a number") from None
        if any(len(p) != 2 for p in pos):
            raise ValueError(f"region {g}, ring {k}: every position must be two numbers `lng lat`")
        rings.append(np.asarray(pos, dtype=np.float64))
    return rings


# ---------------------------------------------------------------------------------------------------- the exact fallback
def exact_state(bank: RegionBank, point, region: int) -> int:
    """OUTSIDE, BOUNDARY or INSIDE of `point` against region `region`, without a tolerance: the classification of csrc/regions.hip
    (crossing number, half-open rule, even-odd over all rings) with every determinant in `fractions.Fraction`.  The comparisons that
    pick the straddling edges are exact in floating point already; only those edges' determinants need rationals."""
    px, py = float(point[0]), float(point[1])
    parity = 0
    for ring in bank.rings(region):
        ax, ay, bx, by = ring[:-1, 0], ring[:-1, 1], ring[1:, 0], ring[1:, 1]
        if ((ring[:, 0] == px) & (ring[:, 1] == py)).any():
            return BOUNDARY
        flat = (ay == py) & (by == py) & (np.minimum(ax, bx) <= px) & (px <= np.maximum(ax, bx))
        if flat.any():
            return BOUNDARY
        fpx, fpy = Fraction(px), Fraction(py)
        for j in np.nonzero((ay <= py) != (by <= py))[0]:
            det = (Fraction(ax[j]) - fpx) * (Fraction(by[j]) - fpy) - (Fraction(ay[j]) - fpy) * (Fraction(bx[j]) - fpx)
            if det == 0:
                return BOUNDARY
            if (det > 0) == bool(ay[j] <= py):            # an upward edge crosses the ray towards +x iff det > 0, a downward one iff det < 0
                parity ^= 1
    return INSIDE if parity else OUTSIDE


# ---------------------------------------------------------------------------------------------------- cell extents
def cell_extents_km(bank: RegionBank, centroids) -> np.ndarray:
    """(R,) fp64 km: the haversine distance (reference preprocessing/geo_utils.py:58-74, R = 6378.137 km) from region r's centroid
    -- `centroids` (R, 2) [lng, lat] -- to the farthest vertex of its rings; 0 for a region without rings.  Host arithmetic, run once
    per geocell table: what `SuperGuessr.spread` adds to a cell's distance so that a radius holds the cell whole."""
    cen = np.ascontiguousarray(np.asarray(centroids), dtype=np.float64)
    if cen.shape != (len(bank), 2):
        raise ValueError(f"cell_extents_km: expected ({len(bank)}, 2) centroids, got shape {cen.shape}")
    out = np.zeros((len(bank),), dtype=np.float64)
    for r in range(len(bank)):
        lo, hi = bank.ring_off[bank.region_off[r]], bank.ring_off[bank.region_off[r + 1]]
        if hi == lo:
            continue
        v = np.deg2rad(bank.xy[lo:hi])
        c = np.deg2rad(cen[r])
        a = np.sin((c[1] - v[:, 1]) / 2) ** 2 + np.cos(c[1]) * np.cos(v[:, 1]) * np.sin((c[0] - v[:, 0]) / 2) ** 2
        out[r] = (6378137.0 * (2 * np.arcsin(np.sqrt(np.minimum(a, 1.0))))).max() / 1000
    return out


# ---------------------------------------------------------------------------------------------------- lookups
def _points(who: str, lnglat, finite: bool) -> np.ndarray:
    pts = np.ascontiguousarray(np.asarray(lnglat), dtype=np.float64)           # fp32 predictions widen exactly
    if pts.ndim != 2 or pts.shape[1] != 2:
        raise ValueError(f"{who}: expected (N, 2) [lng, lat] points, got shape {pts.shape}")
    if finite and not np.isfinite(pts).all():
        raise ValueError(f"{who}: point {int(np.argwhere(~np.isfinite(pts).all(axis=1))[0, 0])} is not finite")
    return pts


def _device_points(pts: np.ndarray):
    import torch
    from . import _lib
    _lib.require_gpu()
    return torch.from_numpy(pts).to("cuda")


def find_regions(bank: RegionBank, lnglat) -> Tuple[np.ndarray, dict]:
    """The region of every point as find_country / generate_cell_labels assign it: the lowest-index region that covers the point
    (interior or boundary), else the nearest one.  Returns (indices (N,) int64, info) with info = dict(ambiguous: points the device
    could not decide for at least one region and that were settled exactly, nearest: points no region covers)."""
    import torch
    from . import hip_ops
    pts = _points("find_regions", lnglat, finite=True)
    n = pts.shape[0]
    out = np.full((n,), -1, dtype=np.int64)
    if n == 0:
        return out, dict(ambiguous=0, nearest=0)
    if len(bank) == 0:
        raise ValueError("find_regions: the bank has no regions")
    d_pts = _device_points(pts)
    pending = np.arange(n)
    start = np.zeros((n,), dtype=np.int64)
    was_ambiguous = np.zeros((n,), dtype=bool)
    uncovered = []
    pick = lambda rows: d_pts if rows.size == n else d_pts[torch.from_numpy(rows).to(d_pts.device)]     # noqa: E731
    while pending.size:                                    # ends: every pass settles a point or raises its `start`
        cover, state = hip_ops.region_locate(bank.handle, pick(pending), start[pending])
        cover, state = cover.cpu().numpy().astype(np.int64), state.cpu().numpy()
        settled = state != AMBIGUOUS
        for k in np.nonzero(~settled)[0]:
            i = pending[k]
            was_ambiguous[i] = True
            if exact_state(bank, pts[i], int(cover[k])) == OUTSIDE:
                start[i] = cover[k] + 1                    # re-enters behind the region that does not cover it after all
            else:
                settled[k] = True
        covered = settled & (cover >= 0)
        out[pending[covered]] = cover[covered]
        uncovered.append(pending[settled & (cover < 0)])
        pending = pending[~settled]
    uncovered = np.concatenate(uncovered)
    if uncovered.size:
        idx, _ = hip_ops.region_nearest(bank.handle, pick(uncovered))
        out[uncovered] = idx.cpu().numpy()
        if (out[uncovered] < 0).any():
            raise ValueError("find_regions: the bank has no edges, nothing is nearest")
    return out, dict(ambiguous=int(was_ambiguous.sum()), nearest=int(uncovered.size))


def contains(bank: RegionBank, lnglat, region) -> np.ndarray:
    """shapely's `region.contains(point)` per row: True iff the point is STRICTLY inside region[i] (a point on the boundary is not
    contained; region -1 contains nothing).  Non-finite points are contained nowhere."""
    from . import hip_ops
    pts = _points("contains", lnglat, finite=False)
    region = np.asarray(region, dtype=np.int64)
    if pts.shape[0] == 0:
        return np.zeros((0,), dtype=bool)
    state = hip_ops.region_classify(bank.handle, _device_points(pts), region).cpu().numpy()
    inside = state == INSIDE
    for i in np.nonzero(state == AMBIGUOUS)[0]:
        inside[i] = exact_state(bank, pts[i], int(region[i])) == INSIDE
    return inside


def country_accuracy(predictions, labels, bank: RegionBank) -> float:
    """reference evaluation/metrics.py:74-88: the label's country is find_country(label); the prediction is correct iff that country
    `contains` it.  The mean over the samples."""
    return float(np.mean(country_hits(predictions, labels, bank)))


def country_hits(predictions, labels, bank: RegionBank) -> np.ndarray:
    """The per-sample hit (0 / 1) whose mean is `country_accuracy`: the column a bootstrap resamples."""
    countries, _ = find_regions(bank, labels)
    return contains(bank, predictions, countries).astype(int)


def assign_geocells(lnglat, bank: RegionBank) -> Tuple[np.ndarray, dict]:
    """reference preprocessing/dataset_preprocessing.py:60-94 (one_hot=False) for every row: the `labels_clf` column."""
    return find_regions(bank, lnglat)


def main(argv=None) -> int:
    import argparse
    import pandas as pd
    ap = argparse.ArgumentParser(prog="python -m pigeon_amd.regions", description="Write the geocell label column `labels_clf` of a metadata CSV.")
    ap.add_argument("--geocells", required=True, metavar="CSV", help="geocell table with a `polygon` WKT column (row = geocell index)")
    ap.add_argument("--metadata", required=True, metavar="CSV", help="table with `lng` and `lat` columns")
    ap.add_argument("-o", "--output", required=True, metavar="CSV")
    args = ap.parse_args(argv)
    bank = RegionBank.from_geocell_csv(args.geocells)
    meta = pd.read_csv(args.metadata, float_precision="round_trip")          # the default parser may be an ulp off: a point ON an edge must stay there
    missing = [c for c in ("lng", "lat") if c not in meta.columns]
    if missing:
        raise SystemExit(f"{args.metadata}: no column {missing} (columns: {list(meta.columns)})")
    cells, info = assign_geocells(meta[["lng", "lat"]].to_numpy(dtype=np.float64), bank)
    meta["labels_clf"] = cells
    meta.to_csv(args.output, index=False)
    print(f"{len(meta)} points into {len(bank)} geocells: {info['ambiguous']} ambiguous on the device (settled exactly), "
          f"{info['nearest']} covered by no geocell (assigned to the nearest); written to {args.output}")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
