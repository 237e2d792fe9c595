"""Pins tests/_regionref.py, the exact reference the GPU tests of the point-in-region lookup compare against (no GPU):
on generic points against matplotlib's `Path.contains_points` (an independent implementation), on enumerated boundary truths, and by
showing that seven planted mistakes -- made in a numpy restatement of the device's filter (csrc/regions.hip's header) -- are each
reported at the point built for them, while the unplanted restatement disagrees nowhere."""
import numpy as np
import pytest

import _regionref as ref
from _regionref import AMBIGUOUS, BOUNDARY, INSIDE, OUTSIDE, box, star

EPS = 2.0 ** -53
ERRBOUND = (3.0 + 16.0 * EPS) * EPS
MIN_SUM = 2.0 ** -960


# ------------------------------------------------------------------------------------------------ _regionref against matplotlib
@pytest.mark.parametrize("n", [3, 4, 5, 63, 64, 65, 257, 1025])
def test_reference_matches_matplotlib_on_generic_points(n):
    from matplotlib.path import Path
    rng = np.random.default_rng(n)
    shell, hole = star(n, 0.0, 0.0, 1.0, 2.0), star(max(3, n // 3), 0.1, -0.1, 0.2, 0.4)[::-1]
    pts = rng.uniform(-2.2, 2.2, (400, 2))
    in_shell, in_hole = Path(shell).contains_points(pts), Path(hole).contains_points(pts)
    want = np.where(in_shell & ~in_hole, INSIDE, OUTSIDE)
    got = np.array([ref.state([shell, hole], p) for p in pts])
    assert np.array_equal(got, want)
    assert {INSIDE, OUTSIDE} <= set(got.tolist())


def test_reference_on_enumerated_boundary_truths():
    holed = [box(0, 0, 10, 10), box(3, 3, 7, 7)[::-1]]
    island = holed + [box(4, 4, 6, 6)]                                          # an island inside the lake
    tri = [np.array([[0.0, 0.0], [8.0, 0.0], [0.0, 8.0], [0.0, 0.0]])]           # hypotenuse x + y = 8: representable on-line points
    truths = [
        (holed, (0, 0), BOUNDARY), (holed, (10, 10), BOUNDARY), (holed, (5, 0), BOUNDARY), (holed, (10, 2.5), BOUNDARY),
        (holed, (3, 5), BOUNDARY), (holed, (7, 7), BOUNDARY), (holed, (5, 3), BOUNDARY),            # on the hole's ring
        (holed, (5, 5), OUTSIDE), (holed, (1, 5), INSIDE), (holed, (1, 3), INSIDE), (holed, (1, 7), INSIDE),   # ray through hole vertices / along hole edges
        (holed, (8, 3), INSIDE), (holed, (1, 10), BOUNDARY), (holed, (-1, 10), OUTSIDE), (holed, (11, 0), OUTSIDE), (holed, (-1, 0), OUTSIDE),
        (holed, (np.nextafter(10.0, 11.0), 5), OUTSIDE), (holed, (np.nextafter(10.0, 0.0), 5), INSIDE),
        (holed, (np.nextafter(3.0, 4.0), 5), OUTSIDE), (holed, (np.nextafter(3.0, 0.0), 5), INSIDE),
        (island, (5, 5), INSIDE), (island, (4, 5), BOUNDARY), (island, (3.5, 5), OUTSIDE), (island, (6.5, 6.5), OUTSIDE),
        (tri, (4, 4), BOUNDARY), (tri, (1, 7), BOUNDARY), (tri, (np.nextafter(4.0, 0.0), 4), INSIDE), (tri, (np.nextafter(4.0, 5.0), 4), OUTSIDE),
        (tri, (0, 8), BOUNDARY), (tri, (0, 4), BOUNDARY), (tri, (2, 0), BOUNDARY), (tri, (3, 3), INSIDE), (tri, (5, 5), OUTSIDE),
    ]
    for rings, p, want in truths:
        assert ref.state(rings, np.array(p, dtype=np.float64)) == want, (p, want)
    assert ref.covers(holed, (0.0, 0.0)) and not ref.contains(holed, (0.0, 0.0))


def test_reference_nearest_and_lowest_cover():
    regions = [[box(0, 0, 1, 1)], [box(1, 0, 2, 1)], [box(0.5, 0, 1.5, 1)], []]
    assert ref.first_cover(regions, (1.0, 0.5)) == 0 and ref.first_cover(regions, (1.0, 0.5), start=1) == 1      # shared edge: both cover
    assert ref.first_cover(regions, (1.25, 0.5)) == 1 and ref.first_cover(regions, (1.25, 0.5), start=2) == 2
    assert ref.first_cover(regions, (3.0, 0.5)) == -1
    g, d2, other = ref.nearest(regions, (1.0, 2.0))                              # the corner (1, 1) belongs to regions 0 and 1: a tie
    assert (g, d2, other) == (0, 1, 1)
    g, d2, other = ref.nearest(regions, (4.0, 0.5))
    assert (g, d2, other) == (1, 4, 6.25)
    g, d2, _ = ref.nearest([[np.array([[0.0, 0.0], [4.0, 4.0], [0.0, 4.0], [0.0, 0.0]])]], (3.0, 1.0))   # the foot is inside the diagonal
    assert g == 0 and d2 == 2
    assert ref.find_region(regions, (4.0, 0.5)) == (1, False) and ref.find_region(regions, (0.75, 0.5)) == (0, True)


# ------------------------------------------------------------------------------------------------ the device's filter, in numpy
class Flat:
    """regions -> the CSR arrays of pg_region_bank"""

    def __init__(self, regions):
        self.regions = regions
        self.region_off = np.cumsum([0] + [len(r) for r in regions])
        rings = [ring for r in regions for ring in r]
        self.ring_off = np.cumsum([0] + [len(ring) for ring in rings])
        self.xy = np.concatenate(rings)
        self.ring_bbox = np.array([[r[:, 0].min(), r[:, 1].min(), r[:, 0].max(), r[:, 1].max()] for r in rings])
        self.region_bbox = np.array([[self.ring_bbox[a:b, 0].min(), self.ring_bbox[a:b, 1].min(), self.ring_bbox[a:b, 2].max(), self.ring_bbox[a:b, 3].max()]
                                     for a, b in zip(self.region_off[:-1], self.region_off[1:])])


def model_state(bank, g, p, mistake=None):
    """csrc/regions.hip's classification of p against region g in numpy fp64, operation for operation; `mistake` plants one error"""
    px, py = float(p[0]), float(p[1])
    if mistake == "open_boxes":
        in_box = lambda b: b[0] < px < b[2] and b[1] < py < b[3]                # noqa: E731
    else:
        in_box = lambda b: b[0] <= px <= b[2] and b[1] <= py <= b[3]            # noqa: E731
    if not in_box(bank.region_bbox[g]):
        return OUTSIDE
    parity, amb = 0, False
    for k, r in enumerate(range(bank.region_off[g], bank.region_off[g + 1])):
        if (mistake == "hole_ignored" and k > 0) or not in_box(bank.ring_bbox[r]):
            continue
        v0, last = bank.ring_off[r], bank.ring_off[r + 1] - 1                   # edges start at v0 .. last - 1
        if mistake == "last_edge_dropped":
            last -= 1
        if mistake == "closure_edge" and last + 1 < len(bank.xy):               # the closure vertex starts one more edge: into the next ring
            last += 1
        a, b = bank.xy[v0:last], bank.xy[v0 + 1:last + 1]
        ax, ay, bx, by = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
        vertex = ((ax == px) & (ay == py)) | ((bx == px) & (by == py))
        au, bu = ay <= py, by <= py
        flat = (ay == py) & (by == py) & (np.minimum(ax, bx) <= px) & (px <= np.maximum(ax, bx))
        straddle = (au != bu) if mistake != "closed_straddle" else ((np.minimum(ay, by) <= py) & (py <= np.maximum(ay, by)) & (ay != by))
        up = au if mistake != "closed_straddle" else ay < by
        with np.errstate(all="ignore"):
            left, right = (ax - px) * (by - py), (ay - py) * (bx - px)
            det = left - right
            total = np.abs(left) + np.abs(right)
            certified = (total >= MIN_SUM) & (np.abs(det) > ERRBOUND * total)
        amb = amb or bool((vertex | flat | (straddle & ~vertex & ~certified)).any())
        parity ^= int((straddle & ~vertex & certified & np.where(up, det > 0, det < 0)).sum()) & 1
    return AMBIGUOUS if amb else parity


def agrees(device, truth):
    """what the product guarantees: never a wrong certain answer, and every boundary point flagged"""
    return device == AMBIGUOUS or (device == truth and truth != BOUNDARY)


@pytest.fixture(scope="module")
def probe_bank():
    # region 0: a pentagon whose LAST edge is the upper right one and whose vertex (12, 5) lies on the rays of y = 5, with a square hole
    shell = np.array([[10.0, 10.0], [0.0, 10.0], [0.0, 0.0], [10.0, 0.0], [12.0, 5.0], [10.0, 10.0]])
    return Flat([[shell, box(3, 3, 7, 7)[::-1]], [box(20, 0, 30, 10)], [box(25, 5, 35, 15)]])


PROBES = {
    "closed_straddle": (8.0, 5.0),        # the ray passes through the vertex (12, 5): counted once, not twice
    "hole_ignored": (6.0, 5.5),           # in the hole
    "last_edge_dropped": (8.5, 8.0),      # the ray crosses only the shell's last edge
    "closure_edge": (8.0, 9.0),           # the ray crosses the phantom edge from the shell's closure vertex to the hole's first vertex
    "open_boxes": (12.0, 5.0),            # a vertex on the region's bounding box
}
OTHERS = [(1.0, 1.0), (11.0, 4.0), (11.5, 8.0), (2.0, 9.5), (22.0, 3.0), (28.0, 8.0), (33.0, 12.0), (0.0, 5.0), (5.0, 3.0), (40.0, 40.0)]


def test_unplanted_model_agrees_everywhere(probe_bank):
    for p in list(PROBES.values()) + OTHERS:
        for g in range(3):
            assert agrees(model_state(probe_bank, g, p), ref.state(probe_bank.regions[g], p)), (p, g)


@pytest.mark.parametrize("mistake", sorted(PROBES))
def test_planted_classification_mistake_is_reported_at_its_point(probe_bank, mistake):
    p = PROBES[mistake]
    truth = ref.state(probe_bank.regions[0], p)
    assert agrees(model_state(probe_bank, 0, p), truth)
    assert not agrees(model_state(probe_bank, 0, p, mistake), truth), (mistake, p)
    # and a mistake is not reported where it does not act: the plain interior / exterior probes keep agreeing
    for q in [(1.0, 1.0), (40.0, 40.0), (22.0, 7.0)]:
        for g in range(3):
            assert agrees(model_state(probe_bank, g, q, mistake), ref.state(probe_bank.regions[g], q)), (mistake, q, g)


def test_planted_contains_and_order_mistakes_are_reported(probe_bank):
    regions = probe_bank.regions
    on_edge = (0.0, 5.0)                                                         # on region 0's left edge
    assert ref.state(regions[0], on_edge) == BOUNDARY and model_state(probe_bank, 0, on_edge) == AMBIGUOUS
    boundary_is_inside = lambda rings, p: ref.state(rings, p) != OUTSIDE         # noqa: E731  -- the planted `contains`
    assert boundary_is_inside(regions[0], on_edge) != ref.contains(regions[0], on_edge)
    assert boundary_is_inside(regions[0], (1.0, 1.0)) == ref.contains(regions[0], (1.0, 1.0))
    overlap = (28.0, 8.0)                                                        # regions 1 and 2 both cover it
    first_found = lambda p: next(g for g in (2, 1, 0) if ref.covers(regions[g], p))      # noqa: E731  -- the planted order
    assert ref.first_cover(regions, overlap) == 1 and first_found(overlap) == 2
    assert ref.first_cover(regions, (22.0, 3.0)) == first_found((22.0, 3.0)) == 1


def test_filter_certifies_every_generic_point():
    """The cap the GPU test asserts (no uniformly drawn point is ambiguous) is a property of the filter: under it, in numpy fp64, stars
    of 3 to 1 025 edges decide every one of these points, and decide it as matplotlib does."""
    from matplotlib.path import Path
    rng = np.random.default_rng(5)
    for n in (3, 4, 5, 63, 64, 65, 255, 256, 257, 1025):
        ring = star(n)
        bank = Flat([[ring]])
        pts = rng.uniform(-2.2, 2.2, (300, 2))
        got = np.array([model_state(bank, 0, p) for p in pts])
        assert not (got == AMBIGUOUS).any(), n
        assert np.array_equal(got == INSIDE, Path(ring).contains_points(pts)), n
