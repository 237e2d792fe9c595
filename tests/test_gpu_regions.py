"""The point-in-region lookup on the GPU (run with -m gpu on an MI355X): pg_region_locate / _classify / _nearest and the functions on
top of them (pigeon_amd/regions.py) against the exact rational reference tests/_regionref.py, point by point.

What is asserted about the device's three states:
  * a certain answer (OUTSIDE, INSIDE) is never wrong;
  * every point that lies ON a ring comes back AMBIGUOUS;
  * uniformly drawn points are never AMBIGUOUS (a condition, not a measurement: tests/test_regionref_cpu.py shows it for the filter);
  * `find_regions` / `contains` are exact for every point, ambiguous or not.
The boundary family also holds points that are near the boundary but not on it (the y of a vertex, the y of a horizontal edge outside
its x-range, `nextafter` neighbours).  The filter of csrc/regions.hip decides many of those exactly -- a determinant with an exact zero
factor is certified -- so for them the assertion is "AMBIGUOUS or right", and exact after the host fallback.

Both mappings (one wave / one workgroup per point) are forced through pg_tune_region_wave_edges and checked by pg_region_plan."""
import ctypes
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

import _regionref as ref
from _regionref import AMBIGUOUS, BOUNDARY, INSIDE, OUTSIDE, box, star

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING_EDGES = (3, 4, 5, 63, 64, 65, 255, 256, 257, 1025)
FORMS = (0, 1)
U = 2.0 ** -53


@pytest.fixture(scope="module")
def ops():
    from pigeon_amd import _lib, hip_ops
    _lib.require_gpu()
    yield hip_ops
    hip_ops.tune_region_wave_edges(-1)


@pytest.fixture()
def form(request, ops):
    """0: one wave per point, 1: one workgroup per point -- whatever the bank"""
    ops.tune_region_wave_edges(2 ** 31 - 1 if request.param == 0 else 0)
    yield request.param
    ops.tune_region_wave_edges(-1)


both_forms = pytest.mark.parametrize("form", FORMS, indirect=True)


def bank_of(regions):
    from pigeon_amd.regions import RegionBank
    return RegionBank(regions)


def dev(pts):
    return torch.from_numpy(np.ascontiguousarray(pts, dtype=np.float64)).to(DEV)


def classify(ops, bank, pts, region):
    return ops.region_classify(bank.handle, dev(pts), np.full(len(pts), region) if np.isscalar(region) else region).cpu().numpy()


def check_states(got, truth, what):
    """never a wrong certain answer; every boundary point flagged"""
    for k, (g, t) in enumerate(zip(got, truth)):
        assert g == AMBIGUOUS or (g == t and t != BOUNDARY), f"{what}: point {k}: device state {g}, exact state {t}"


def neighbours(pts):
    """the points and their `nextafter` neighbours in the four axis directions"""
    pts = np.asarray(pts, dtype=np.float64)
    out = [pts]
    for axis in (0, 1):
        for toward in (-np.inf, np.inf):
            q = pts.copy()
            q[:, axis] = np.nextafter(q[:, axis], toward)
            out.append(q)
    return np.concatenate(out)


# ------------------------------------------------------------------------------------------------ ring sizes
@functools.lru_cache(maxsize=None)
def ring_case(n):
    """a star of n edges with a small hole; 150 uniform points; a boundary family on its vertices; the exact states of both"""
    rng = np.random.default_rng(100 + n)
    rings = [star(n, 3.0, -2.0, 1.0, 2.0), star(max(3, n // 4), 3.1, -2.1, 0.2, 0.4)[::-1]]
    generic = np.stack([rng.uniform(0.8, 5.2, 150), rng.uniform(-4.2, 0.2, 150)], axis=1)
    verts = rings[0][rng.choice(n, min(n, 6), replace=False)]
    at_vertex_y = np.stack([verts[:, 0] - rng.uniform(0.05, 3.0, len(verts)), verts[:, 1]], axis=1)     # the ray passes through the vertex
    family = neighbours(np.concatenate([verts, at_vertex_y, rings[1][:2]]))
    return rings, generic, np.array([ref.state(rings, p) for p in generic]), family, np.array([ref.state(rings, p) for p in family])


@both_forms
@pytest.mark.parametrize("n", RING_EDGES)
def test_ring_sizes(ops, form, n):
    rings, generic, generic_truth, family, family_truth = ring_case(n)
    bank = bank_of([rings])
    plan = ops.region_plan(bank.handle)
    assert plan["form"] == form and plan["threads"] == (256 if form else 64) and plan["max_ring_edges"] == n
    got = classify(ops, bank, generic, 0)
    assert not (got == AMBIGUOUS).any(), f"{int((got == AMBIGUOUS).sum())} uniformly drawn points came back ambiguous"
    assert np.array_equal(got, generic_truth)
    assert {INSIDE, OUTSIDE} <= set(generic_truth.tolist())
    got = classify(ops, bank, family, 0)
    check_states(got, family_truth, f"{n} edges")
    assert (family_truth == BOUNDARY).sum() >= min(n, 6) + 2 and (got[family_truth == BOUNDARY] == AMBIGUOUS).all()


def test_default_plan_follows_the_largest_ring(ops):
    ops.tune_region_wave_edges(-1)
    small, large = bank_of([[star(128)], [box(0, 0, 1, 1)]]), bank_of([[box(0, 0, 1, 1)], [star(129)]])
    assert ops.region_plan(small.handle) == {"form": 0, "threads": 64, "max_ring_edges": 128, "wave_edges": 128}
    assert ops.region_plan(large.handle) == {"form": 1, "threads": 256, "max_ring_edges": 129, "wave_edges": 128}
    pts = np.array([[0.5, 0.5], [1.5, 0.1], [3.0, 3.0]])
    for bank in (small, large):                                   # the forms as the plan picks them
        cover, state = ops.region_locate(bank.handle, dev(pts))
        regions = [bank.rings(g) for g in range(2)]
        assert cover.cpu().tolist() == [ref.first_cover(regions, p) for p in pts]
        assert state.cpu().tolist() == [INSIDE if c >= 0 else OUTSIDE for c in cover.cpu().tolist()]


# ------------------------------------------------------------------------------------------------ the boundary family on exact shapes
def exact_shapes():
    holed = [box(0, 0, 10, 10), box(3, 3, 7, 7)[::-1], box(4, 4, 6, 6)]          # a lake with an island
    tri = [np.array([[20.0, 0.0], [28.0, 0.0], [20.0, 8.0], [20.0, 0.0]])]       # hypotenuse x + y = 28: representable on-line points
    date = [box(170, -20, 180, 20), box(-180, -20, -170, 20)]                    # touches lng = +-180
    return [holed, tri, date]


def boundary_family():
    pts = [(0, 0), (10, 10), (3, 3), (7, 3), (4, 6), (20, 8), (28, 0), (180, 20), (-180, -20),          # vertices
           (5, 0), (10, 2.5), (0, 7.75), (3, 5), (5, 7), (6, 4.5), (24, 0), (20, 3), (180, 1.5), (-180, 0), (175, 20),     # axis-aligned edges
           (24, 4), (21, 7), (27.5, 0.5), (22.25, 5.75),                                                 # the diagonal x + y = 28
           (1, 3), (8, 7), (1, 4), (9, 6), (-1, 0), (21, 8), (19, 8), (5, 5),                             # the y of a vertex: the ray passes through it
           (1, 10), (11, 10), (-1, 10), (2, 7), (8, 3), (12, 0), (29, 0), (19, 0), (160, 20), (-160, -20)]    # the y of a horizontal edge, in and out of its range
    return neighbours(np.array(pts, dtype=np.float64))


@both_forms
def test_boundary_family(ops, form):
    from pigeon_amd.regions import contains, find_regions
    regions = exact_shapes()
    bank = bank_of(regions)
    pts = boundary_family()
    on_ring = 0
    for g, rings in enumerate(regions):
        truth = np.array([ref.state(rings, p) for p in pts])
        got = classify(ops, bank, pts, g)
        check_states(got, truth, f"region {g}")
        on_ring += int((truth == BOUNDARY).sum())
        assert np.array_equal(contains(bank, pts, np.full(len(pts), g)), truth == INSIDE)       # exact after the fallback: a boundary point is not contained
    assert on_ring >= 24
    idx, info = find_regions(bank, pts)
    want = [ref.find_region(regions, p) for p in pts]
    assert idx.tolist() == [g for g, _ in want]
    assert info["nearest"] == sum(not c for _, c in want) and info["ambiguous"] >= on_ring


# ------------------------------------------------------------------------------------------------ R and N
@functools.lru_cache(maxsize=None)
def row_case(R):
    """R regions in a row, every third one overlapping its left neighbour, shapes of 4 to 40 edges; 1000 points over and around them"""
    rng = np.random.default_rng(R)
    regions = []
    for g in range(R):
        cx = -96.0 + 3.0 * g - (1.2 if g % 3 == 2 else 0.0)
        regions.append([star(4 + (g * 7) % 37, cx, 0.0, 0.9, 1.6)] if g % 2 else [box(cx - 1.5, -1.5, cx + 1.5, 1.5), star(5, cx, 0.0, 0.3, 0.6)[::-1]])
    pts = np.stack([rng.uniform(-99.0, -96.0 + 3.0 * R, 1000), rng.uniform(-2.2, 2.2, 1000)], axis=1)
    return regions, pts, np.array([ref.first_cover(regions, p) for p in pts])


@both_forms
@pytest.mark.parametrize("R", [1, 2, 65])
def test_locate_over_R_and_N(ops, form, R):
    regions, pts, want = row_case(R)
    bank = bank_of(regions)
    assert (want >= 0).sum() > 100 and (want < 0).sum() > 20
    for N in (1, 63, 64, 65, 1000):
        cover, state = ops.region_locate(bank.handle, dev(pts[:N]))
        cover, state = cover.cpu().numpy(), state.cpu().numpy()
        assert not (state == AMBIGUOUS).any()
        assert np.array_equal(cover, want[:N]), f"R = {R}, N = {N}"
        assert np.array_equal(state, np.where(want[:N] >= 0, INSIDE, OUTSIDE))


@both_forms
def test_grid_bank_of_2000_regions(ops, form):
    """50 x 40 one-degree cells, the geocell shape of bank: uniform points have their cell by arithmetic; points on shared edges and
    corners go to the lowest index, points off the grid to the nearest cell (exact reference)."""
    from pigeon_amd.regions import assign_geocells
    regions = [[box(-25.0 + ix, -20.0 + iy, -24.0 + ix, -19.0 + iy)] for iy in range(40) for ix in range(50)]
    bank = bank_of(regions)
    rng = np.random.default_rng(3)
    inside = np.stack([rng.uniform(-25, 25, 960), rng.uniform(-20, 20, 960)], axis=1)
    special = np.array([[0.0, 0.0], [-25.0, -20.0], [25.0, 20.0], [3.0, 7.5], [3.5, 7.0], [-10.0, 20.0], [25.0, -3.25], [np.nextafter(4.0, 5.0), 4.0],
                        [26.0, 0.5], [-25.5, 19.25], [0.75, 21.0], [30.0, 30.0], [-26.0, -21.0], [10.5, -20.0 - 2.0 ** -40]])
    cells, info = assign_geocells(np.concatenate([inside, special]), bank)
    want_inside = (np.floor(inside[:, 1] + 20).astype(int) * 50 + np.floor(inside[:, 0] + 25).astype(int))
    assert np.array_equal(cells[:960], want_inside)
    want = [ref.find_region(regions, p) for p in special]
    assert cells[960:].tolist() == [g for g, _ in want]
    assert info["nearest"] == sum(not c for _, c in want) == 6 and info["ambiguous"] >= 7


# ------------------------------------------------------------------------------------------------ start, region -1, refusals, guards, streams
def test_start_reentry_region_minus_one_and_refusals(ops):
    from pigeon_amd._lib import PigeonHipError
    regions = [[box(0, 0, 10, 10)], [box(5, 5, 15, 15)], [box(7, 7, 9, 9)], [box(20, 20, 21, 21)]]
    bank = bank_of(regions)
    p = dev(np.array([[8.0, 8.0]] * 5 + [[12.0, 12.0], [8.0, 8.0]]))
    cover, state = ops.region_locate(bank.handle, p, np.array([0, 1, 2, 3, 4, 0, 4]))
    assert cover.cpu().tolist() == [0, 1, 2, -1, -1, 1, -1] and state.cpu().tolist() == [1, 1, 1, 0, 0, 1, 0]
    st = ops.region_classify(bank.handle, p, np.array([0, 1, 2, 3, -1, -1, 0]))
    assert st.cpu().tolist() == [1, 1, 1, 0, 0, 0, 1]
    with pytest.raises(PigeonHipError, match=r"start\[2\] = 5 is outside 0 \.\. 4"):
        ops.region_locate(bank.handle, p, np.array([0, 1, 5, 3, 4, 0, 4]))
    with pytest.raises(PigeonHipError, match=r"start\[0\] = -1"):
        ops.region_locate(bank.handle, p, np.array([-1, 1, 2, 3, 4, 0, 4]))
    with pytest.raises(PigeonHipError, match=r"region\[6\] = 4 is outside -1 \.\. 3"):
        ops.region_classify(bank.handle, p, np.array([0, 1, 2, 3, -1, -1, 4]))
    with pytest.raises(PigeonHipError, match=r"region\[1\] = -2"):
        ops.region_classify(bank.handle, p, np.array([0, -2, 2, 3, -1, -1, 0]))
    # N = 0 and an empty bank are no-ops
    cover, state = ops.region_locate(bank.handle, dev(np.zeros((0, 2))))
    assert cover.numel() == 0 and state.numel() == 0
    empty = bank_of([])
    cover, state = ops.region_locate(empty.handle, p)
    idx, dist = ops.region_nearest(empty.handle, p)
    assert cover.cpu().tolist() == [-1] * 7 and state.cpu().tolist() == [0] * 7
    assert idx.cpu().tolist() == [-1] * 7 and torch.isinf(dist).all()
    # a bank whose host offsets do not describe its arrays is refused by name before anything is launched
    broken = bank_of(regions)
    broken.handle.on_device(DEV).ring_off[2] = 99
    with pytest.raises(PigeonHipError, match=r"ring 1: ring_off goes from 5 to 99"):
        ops.region_locate(broken.handle, p)
    broken.handle.ring_off[2] = 6
    with pytest.raises(PigeonHipError, match=r"ring 1: ring_off goes from 5 to 6 \(a ring needs at least 2"):
        ops.region_nearest(broken.handle, p)


@both_forms
def test_outputs_stay_inside_their_arrays(ops, form):
    """guard regions behind every output: N = 65 results, 64 sentinel elements each"""
    from pigeon_amd import _lib
    regions, pts, want = row_case(65)
    bank = bank_of(regions)
    N, G = 65, 64
    d_pts = dev(pts[:N])
    cover = torch.full((N + G,), 0x5a5a5a5a, dtype=torch.int32, device=DEV)
    idx = cover.clone()
    state = torch.full((N + G,), 0xa5, dtype=torch.uint8, device=DEV)
    state2 = state.clone()
    dist = torch.full((N + G,), -7.0, dtype=torch.float64, device=DEV)
    h, lib, stream = bank.handle.on_device(DEV), _lib.load(), ops._stream()
    region = np.ascontiguousarray(np.maximum(want[:N], 0), dtype=np.int32)
    _lib.check(lib.pg_region_locate(ctypes.byref(h.struct), ops._p(d_pts), None, N, ops._p(cover), ops._p(state), stream), "pg_region_locate")
    _lib.check(lib.pg_region_classify(ctypes.byref(h.struct), ops._p(d_pts), region.ctypes.data, N, ops._p(state2), stream), "pg_region_classify")
    _lib.check(lib.pg_region_nearest(ctypes.byref(h.struct), ops._p(d_pts), N, ops._p(idx), ops._p(dist), stream), "pg_region_nearest")
    torch.cuda.synchronize()
    assert np.array_equal(cover[:N].cpu().numpy(), want[:N])
    assert (cover[N:] == 0x5a5a5a5a).all() and (idx[N:] == 0x5a5a5a5a).all() and (state[N:] == 0xa5).all() and (state2[N:] == 0xa5).all()
    assert (dist[N:] == -7.0).all() and (dist[:N] >= 0).all() and ((idx[:N] >= 0) & (idx[:N] < 65)).all()


def test_side_stream(ops):
    regions, pts, want = row_case(65)
    bank = bank_of(regions)
    d_pts = dev(pts[:300])
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        cover, state = ops.region_locate(bank.handle, d_pts)
        cover2, _ = ops.region_locate(bank.handle, d_pts, np.zeros(300, dtype=np.int64))
        st = ops.region_classify(bank.handle, d_pts, np.maximum(want[:300], 0))
        idx, dist = ops.region_nearest(bank.handle, d_pts)
    side.synchronize()
    assert np.array_equal(cover.cpu().numpy(), want[:300]) and torch.equal(cover, cover2)
    assert np.array_equal(st.cpu().numpy() == INSIDE, want[:300] >= 0)
    idx0, dist0 = ops.region_nearest(bank.handle, d_pts)
    assert torch.equal(idx, idx0) and torch.equal(dist, dist0)


# ------------------------------------------------------------------------------------------------ nearest
@both_forms
def test_nearest(ops, form):
    """The index where the exact reference alone decides it (nearest and runner-up at least 1e-9 apart, relative), exact ties to the
    lower index, and the distance within a bound derived from the kernel's stated operations (csrc/regions.hip's header).  With
    u = 2^-53, w = p - a, d = b - a: the four differences carry (1 + u) each; an end-point distance sqrt(wx^2 + wy^2) is then within
    3u relative; the interior form |cr| / |d| has |cr^ - cr| <= 3u |w||d| + u |cr| (Cauchy-Schwarz on the two products), len2 within
    4u, so the distance is within 3u |w| + 5u dist <= 8u |w|; where rounding picks the other branch of `dot <= 0` / `dot >= len2`
    than exact arithmetic would, |dot^ - dot| <= 4u |w||d| and |len2^ - len2| <= 4u |d|^2 bound the foot's distance from the end point
    by 4u (|w| + |d|), which is also the most the two forms differ by.  In all: at most 12u |w| + 4u |d| + 3u |p - b| per edge, taken
    as 16u (|p - a| + |p - b| + |b - a|) for the second-order terms; the minimum over edges is off by at most the largest such bound
    among the edges within that bound of the minimum -- here simply the largest over all edges -- plus 4u dist for the reference's
    own square root in floating point."""
    regions = [[star(1025, 0.0, 0.0, 1.0, 2.0)], [box(4, -1, 6, 1), box(4.5, -0.5, 5.5, 0.5)[::-1]], [box(6, -1, 8, 1)], [star(7, 3.0, 5.0, 0.5, 1.0)],
               [np.array([[-6.0, -6.0], [-2.0, -2.0], [-6.0, -2.0], [-6.0, -6.0]])], [box(170, 0, 180, 10)]]
    bank = bank_of(regions)
    rng = np.random.default_rng(9)
    pts = np.concatenate([np.stack([rng.uniform(-9, 11, 120), rng.uniform(-8, 8, 120)], axis=1),
                          [[6.0, 2.0], [6.0, -3.0], [5.0, 0.0], [-3.0, -5.0], [175.0, 5.0], [-179.0, 5.0]]])     # ties, a hole, a diagonal's foot, inside, across the date line
    idx, dist = ops.region_nearest(bank.handle, dev(pts))
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    a = np.concatenate([r[:-1] for rings in regions for r in rings])
    b = np.concatenate([r[1:] for rings in regions for r in rings])
    worst, decided = 0.0, 0
    for k, p in enumerate(pts):
        g, d2, other = ref.nearest(regions, p)
        true = math.sqrt(d2)
        if other == d2:
            assert idx[k] == g, f"point {k}: an exact tie goes to the lower index"
        if math.sqrt(other) - true >= 1e-9 * true:
            assert idx[k] == g, f"point {k}: nearest region {idx[k]}, exact {g}"
            decided += 1
        bound = 16 * U * float((np.hypot(*(p - a).T) + np.hypot(*(p - b).T) + np.hypot(*(b - a).T)).max()) + 4 * U * true
        err = abs(dist[k] - true)
        print(f"nearest point {k}: dist {dist[k]!r} exact {true!r} error {err:.3e} = {err / bound:.4f} of the bound")
        assert err <= bound, f"point {k}: {dist[k]!r} against {true!r}: {err:.3e} exceeds {bound:.3e}"
        worst = max(worst, err / bound)
    print(f"nearest (form {form}): worst distance error {worst:.4f} of the derived bound over {len(pts)} points; index decided by the reference alone at {decided}")
    assert decided >= 100 and idx[120] == 1 and idx[121] == 1 and dist[120] == 1.0 and dist[122] == 0.5 and dist[124] == 5.0


# ------------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def fixtures(golden_dir):
    from pigeon_amd.regions import RegionBank
    countries = RegionBank.from_geojson(os.path.join(golden_dir, "regions_countries.geojson"))
    cells = RegionBank.from_geocell_csv(os.path.join(golden_dir, "regions_geocells.csv"))
    meta = np.loadtxt(os.path.join(golden_dir, "regions_metadata.csv"), delimiter=",", skiprows=1)[:, 1:]
    return countries, cells, meta


def country_points():
    rng = np.random.default_rng(21)
    spread = np.stack([rng.uniform(-180, 180, 150), rng.uniform(-30, 50, 150)], axis=1)
    near = np.array([[0, 0], [4, 4], [0, 4], [-4, 0], [5, 5], [6, 6], [3, 3], [30, 10], [28, 9], [25, 5], [24, 10], [22, 2], [180, 0], [-180, 3],
                     [175, 0], [-175, 19], [10, 10], [-60, 30], [60, 40], [-7, 7], [1, 1], [5.5, 2]], dtype=np.float64)
    return np.concatenate([spread, near])


@both_forms
def test_country_accuracy_and_geocell_labels_on_the_fixtures(ops, form, fixtures, tmp_path, golden_dir, capsys):
    from pigeon_amd import regions as rg
    countries, cells, meta = fixtures
    c_regions = [countries.rings(g) for g in range(len(countries))]
    labels = country_points()
    preds = (labels + 0.01).astype(np.float32)                       # predictions as evaluate_model collects them: fp32
    preds[::3] = np.roll(labels, 7, axis=0)[::3].astype(np.float32)
    idx, info = rg.find_regions(countries, labels)
    want = [ref.find_region(c_regions, p) for p in labels]
    assert idx.tolist() == [g for g, _ in want] and info["nearest"] == sum(not c for _, c in want) > 50
    correct = [ref.country_correct(c_regions, p.astype(np.float64), l) for p, l in zip(preds, labels)]
    assert 5 <= sum(correct) < len(correct)
    assert rg.country_accuracy(preds, labels, countries) == float(np.mean(np.array(correct, dtype=int)))
    # the geocell labels, through the command line
    g_regions = [cells.rings(g) for g in range(len(cells))]
    out = os.path.join(str(tmp_path), "labeled.csv")
    assert rg.main(["--geocells", os.path.join(golden_dir, "regions_geocells.csv"), "--metadata", os.path.join(golden_dir, "regions_metadata.csv"), "-o", out]) == 0
    want = [ref.find_region(g_regions, p) for p in meta]
    written = np.loadtxt(out, delimiter=",", skiprows=1)
    assert written[:, 3].astype(int).tolist() == [g for g, _ in want] and np.array_equal(written[:, 1:3], meta)
    n_near = sum(not c for _, c in want)
    assert n_near == 10 and f"{n_near} covered by no geocell" in capsys.readouterr().out
    cells_idx, info = rg.assign_geocells(meta, cells)
    assert cells_idx.tolist() == [g for g, _ in want] and info["nearest"] == n_near and info["ambiguous"] >= 7


def test_evaluate_model_reports_country_accuracy(ops, fixtures, tmp_path):
    """evaluate_model(..., metrics=compute_geoguessr_metrics with the country bank): `Country_accuracy` equals the exact reference's
    count on the predictions the run itself collected; without the bank the key is absent and every other key is unchanged."""
    from pigeon_amd import synthetic as syn
    from pigeon_amd.evaluate import compute_geoguessr_metrics, evaluate_model
    from pigeon_amd.super_guessr import SuperGuessr
    countries = fixtures[0]
    c_regions = [countries.rings(g) for g in range(len(countries))]
    C, n = 120, 24
    rng = np.random.default_rng(4)
    cen = np.stack([rng.uniform(-9.5, 9.5, C), rng.uniform(-9.5, 9.5, C)], axis=1)      # centroids over `Holed` and the `Plug` in its hole
    geo = os.path.join(str(tmp_path), "geocells.csv")
    syn.write_geocell_csv(geo, cen)
    model = SuperGuessr(None, panorama=True, num_candidates=10, geocell_path=geo)
    W, b = syn.make_head_weights(C, seed=3)
    with torch.no_grad():
        model.cell_layer.weight.copy_(W * 8); model.cell_layer.bias.copy_(b)
    model.to(DEV)
    gen = torch.Generator().manual_seed(2)
    emb = torch.randn((n, 4, 1024), generator=gen)
    labels = torch.from_numpy(cen[rng.integers(0, C, n)] + rng.normal(0, 1.0, (n, 2)))
    labels_clf = torch.randint(0, C, (n,), generator=gen)

    class DS(torch.utils.data.Dataset):
        def __len__(self): return n
        def __getitem__(self, i):
            if isinstance(i, str):
                return {"labels": labels.numpy(), "labels_clf": labels_clf.numpy()}[i]
            return {"embedding": emb[i], "labels": labels[i], "labels_clf": labels_clf[i]}

    plain = evaluate_model(model, DS(), compute_geoguessr_metrics, None, None, batch_size=16)
    res = evaluate_model(model, DS(), functools.partial(compute_geoguessr_metrics, countries=countries), None, None, batch_size=16)
    correct = [ref.country_correct(c_regions, p.astype(np.float64), l) for p, l in zip(res["preds"], labels.numpy())]
    assert 0 < sum(correct) < n
    assert res["Country_accuracy"] == float(np.mean(np.array(correct, dtype=int)))
    assert "Country_accuracy" not in plain and set(res) - set(plain) == {"Country_accuracy"}
    for k in ("Mean_km_error", "Geoguessr_score", "Geocell_accuracy", "Under_25_km"):
        assert plain[k] == res[k]


def test_run_py_evaluate_countries(ops, fixtures, golden_dir, monkeypatch):
    """`run.py evaluate none --synthetic 8 --countries FILE`: the entry point reports `Country_accuracy`, the exact reference's count on
    the predictions it collected (the synthetic labels are all (0, 0): inside the fixture's `Plug`)."""
    import importlib
    sys.path.insert(0, ROOT)
    path = os.path.join(golden_dir, "regions_countries.geojson")
    monkeypatch.setattr(sys, "argv", ["run.py", "evaluate", "none", "--synthetic", "8", "--layers", "2", "--geocells", "300", "--countries", path])
    import run
    importlib.reload(run)
    torch.manual_seed(0)
    results = run.main()
    countries = fixtures[0]
    c_regions = [countries.rings(g) for g in range(len(countries))]
    assert ref.find_region(c_regions, np.zeros(2)) == (3, True)
    correct = [ref.country_correct(c_regions, p.astype(np.float64), np.zeros(2)) for p in results["preds"]]
    assert results["Country_accuracy"] == float(np.mean(np.array(correct, dtype=int)))
    with pytest.raises(FileNotFoundError, match="country polygons"):
        from pigeon_amd.evaluate import evaluate
        evaluate("none", None, yfcc=False, landmarks=False, country_path=os.path.join(golden_dir, "no_such_file.geojson"))
