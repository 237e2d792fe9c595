"""Exact reference of the point-in-region lookup (csrc/regions.hip, pigeon_amd/regions.py), written independently of both: the
classification walks WINDING NUMBERS (Sunday's signed crossings) where the product counts crossing parity, and every determinant
and every squared distance is a `fractions.Fraction` -- floats are exact rationals, so no comparison here has a tolerance.

A region is a list of closed rings, (n, 2) float64 arrays with ring[0] == ring[-1]; it is the even-odd set of its rings: a ring
"holds" a point when its winding number around it is not zero, the region holds it when an odd number of rings do; a point on any
ring is on the boundary.  numpy is used only for comparisons that are exact in floating point (which edges can matter at all)."""
from fractions import Fraction

import numpy as np

OUTSIDE, INSIDE, AMBIGUOUS, BOUNDARY = 0, 1, 2, 3          # AMBIGUOUS: the device's "cannot certify", never returned here


def _cross(ax, ay, bx, by, px, py):
    """(b - a) x (p - a), exact: > 0 iff p is to the left of a -> b"""
    ax, ay, bx, by, px, py = (Fraction(float(v)) for v in (ax, ay, bx, by, px, py))
    return (bx - ax) * (py - ay) - (px - ax) * (by - ay)


def ring_winding(ring, p):
    """(winding number of the ring around p, p lies on the ring)"""
    px, py = float(p[0]), float(p[1])
    ax, ay, bx, by = ring[:-1, 0], ring[:-1, 1], ring[1:, 0], ring[1:, 1]
    # on the ring: inside the edge's closed box (exact comparisons) and collinear (exact rational)
    box = (np.minimum(ax, bx) <= px) & (px <= np.maximum(ax, bx)) & (np.minimum(ay, by) <= py) & (py <= np.maximum(ay, by))
    for j in np.nonzero(box)[0]:
        if _cross(ax[j], ay[j], bx[j], by[j], px, py) == 0:
            return 0, True
    wn = 0
    for j in np.nonzero((ay <= py) & (by > py))[0]:          # upward crossings with p strictly left
        if _cross(ax[j], ay[j], bx[j], by[j], px, py) > 0:
            wn += 1
    for j in np.nonzero((ay > py) & (by <= py))[0]:          # downward crossings with p strictly right
        if _cross(ax[j], ay[j], bx[j], by[j], px, py) < 0:
            wn -= 1
    return wn, False


def state(rings, p):
    """OUTSIDE, BOUNDARY or INSIDE of p against the region made of `rings`"""
    held = 0
    for ring in rings:
        wn, on = ring_winding(ring, p)
        if on:
            return BOUNDARY
        held += wn != 0
    return INSIDE if held % 2 else OUTSIDE


def covers(rings, p):
    """GEOS `covered_by`: interior or boundary"""
    return state(rings, p) != OUTSIDE


def contains(rings, p):
    """GEOS `contains`: strictly interior"""
    return state(rings, p) == INSIDE


def _box(rings):
    xy = np.concatenate(rings)
    return xy[:, 0].min(), xy[:, 1].min(), xy[:, 0].max(), xy[:, 1].max()


def first_cover(regions, p, start=0):
    """the lowest region index >= start that covers p, or -1"""
    for g in range(start, len(regions)):
        if not regions[g]:                                                         # a region without rings covers nothing
            continue
        x0, y0, x1, y1 = _box(regions[g])
        if x0 <= p[0] <= x1 and y0 <= p[1] <= y1 and covers(regions[g], p):        # closed box, exact
            return g
    return -1


def segment_d2(a, b, p):
    """squared distance from p to the segment a-b, exact"""
    ax, ay, bx, by, px, py = (Fraction(float(v)) for v in (a[0], a[1], b[0], b[1], p[0], p[1]))
    dx, dy, wx, wy = bx - ax, by - ay, px - ax, py - ay
    len2, dot = dx * dx + dy * dy, wx * dx + wy * dy
    if len2 == 0 or dot <= 0:
        return wx * wx + wy * wy
    if dot >= len2:
        return (px - bx) ** 2 + (py - by) ** 2
    return (wx * dy - wy * dx) ** 2 / len2


def region_d2(regions, p, slack=1e-6):
    """per region the exact squared distance from p to its boundary (None for a region without edges).  Edges whose float distance is
    more than `slack` degrees above the region's float minimum cannot be the minimum (float error here is below 1e-11 for |coordinates|
    <= 360) and are not evaluated exactly."""
    out = []
    p = np.asarray(p, dtype=np.float64)
    for rings in regions:
        if not rings:
            out.append(None)
            continue
        a = np.concatenate([r[:-1] for r in rings])
        b = np.concatenate([r[1:] for r in rings])
        d, w = b - a, p - a
        len2 = (d * d).sum(1)
        t = np.clip((w * d).sum(1) / np.where(len2 == 0, 1, len2), 0, 1)
        approx = np.sqrt(((w - t[:, None] * d) ** 2).sum(1))
        out.append(min(segment_d2(a[j], b[j], p) for j in np.nonzero(approx <= approx.min() + slack)[0]))
    return out


def nearest(regions, p):
    """(index of the nearest region, ties to the lowest; its exact squared distance; the smallest squared distance among the OTHER regions or None)"""
    d2 = region_d2(regions, p)
    have = [(v, g) for g, v in enumerate(d2) if v is not None]
    best, g = min(have)
    others = [v for v, h in have if h != g]
    return g, best, (min(others) if others else None)


def find_region(regions, p):
    """find_country / generate_cell_labels: (index, covered): the lowest covering region, else the nearest"""
    g = first_cover(regions, p)
    return (g, True) if g >= 0 else (nearest(regions, p)[0], False)


def country_correct(regions, prediction, label):
    """one sample of country_accuracy: the label's region strictly contains the prediction"""
    return contains(regions[find_region(regions, label)[0]], prediction)


# ------------------------------------------------------------------------------------------------ shapes the tests share
def star(n, cx=0.0, cy=0.0, r0=1.0, r1=2.0, phase=0.1):
    """a closed star-shaped ring of n edges (n + 1 positions) around (cx, cy), radii alternating between r0 and r1"""
    ang = phase + 2 * np.pi * np.arange(n) / n
    rad = np.where(np.arange(n) % 2 == 0, r1, r0) if n >= 6 else np.full(n, r1)
    ring = np.stack([cx + rad * np.cos(ang), cy + rad * np.sin(ang)], axis=1)
    return np.concatenate([ring, ring[:1]])


def box(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1], [x0, y0]], dtype=np.float64)


def to_wkt(rings_by_polygon):
    """WKT of a multipolygon given as a list of polygons, each a list of rings; repr() keeps every float exact"""
    ring = lambda r: "(" + ", ".join(f"{float(x)!r} {float(y)!r}" for x, y in r) + ")"      # noqa: E731
    polys = ["(" + ", ".join(ring(r) for r in poly) + ")" for poly in rings_by_polygon]
    return ("POLYGON " + polys[0]) if len(polys) == 1 else ("MULTIPOLYGON (" + ", ".join(polys) + ")")
