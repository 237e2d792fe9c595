"""The prototype cluster table on the GPU (run with -m gpu on an MI355X): pg_haversine_blocks against pg_haversine_matrix (bits) and
numpy (1e-12), pg_optics_graph against the numpy restatement tests/_opticsref.py on the device's own matrix and against sklearn's
recorded arrays (array_equal on ordering, core distances, reachability, predecessors), both forms of the ordering kernel at every
thread count, cells packed from a non-zero base, empty cells, a side stream, the batching of prototypes.optics_graph_cells, and
ProtoDataset.generate against the CSV the reference wrote."""
import os

import numpy as np
import pytest
import torch

import _opticsref as ref
from _opticsref import assert_same_table, frame_of as _frame

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAMES = ("ordering", "core", "reach", "pred")


@pytest.fixture(scope="module")
def ops():
    from pigeon_amd import _lib, hip_ops
    _lib.require_gpu()
    return hip_ops


def quantised(rng, n, side=None):
    """points on a coarse 1e-3 degree lattice: many exactly equal distances and exact duplicates"""
    side = side or max(2, int(np.sqrt(n) * 0.6))
    return np.stack([11.0 + 1e-3 * rng.integers(0, side, n), 47.0 + 1e-3 * rng.integers(0, side, n)], axis=1)


def offsets(sizes):
    return torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64))


def run_graph(ops, dist, cell_off, mat_off, ms):
    g = ops.optics_graph(dist, cell_off, mat_off, ms)
    return {k: v.cpu().numpy() for k, v in g.items()}


def check_cells(g, dist_host, cell_off, mat_off, ms, what=""):
    co, mo = cell_off.numpy(), mat_off.numpy()
    for c in range(len(co) - 1):
        n = int(co[c + 1] - co[c])
        D = dist_host[mo[c]:mo[c] + n * n].reshape(n, n)
        want = ref.graph(D, ms)
        for name, w in zip(NAMES, want):
            got = g[name][co[c]:co[c + 1]]
            assert got.dtype == w.dtype and np.array_equal(got, w), f"{what} cell {c} (n = {n}, min_samples = {ms}): {name}"


# ------------------------------------------------------------------------------------------------ distances
def test_haversine_blocks(ops):
    """Cells of 1, 2, 65 and 300 points in one launch.  The upper triangle (i <= j) of every block is pg_haversine_matrix's value bit for
    bit; the block is exactly symmetric (the lower triangle mirrors the upper one, as numpy's matrix is symmetric and the matrix
    kernel's is not); zeros and identical points -- the diagonal, the exact duplicates -- are 1e-5, where the matrix kernel's fused
    longitude difference leaves ~1e-13 km; all of it within rtol 1e-12 / atol 1e-9 of the reference's numpy matrix."""
    rng = np.random.default_rng(0)
    sizes = [1, 2, 65, 300]
    pts = np.concatenate([np.array([rng.uniform(-170, 170), rng.uniform(-70, 70)]) + rng.normal(0, 0.3, (n, 2)) for n in sizes])
    pts[10] = pts[40]; pts[100] = pts[101] = pts[300]               # exact duplicates inside the 65- and the 300-point cell
    cell_off = offsets(sizes)
    d_pts = torch.from_numpy(pts).to(DEV)
    dist, mat_off = ops.haversine_blocks(d_pts, cell_off, 1e-5)
    torch.cuda.synchronize()
    assert mat_off.tolist() == np.concatenate([[0], np.cumsum(np.square(sizes))]).tolist() and dist.numel() == int(mat_off[-1])
    for c, n in enumerate(sizes):
        s = int(cell_off[c])
        block = dist[int(mat_off[c]):int(mat_off[c + 1])].reshape(n, n)
        cell = d_pts[s:s + n].contiguous()
        m = ops.haversine_matrix(cell, cell)
        same = (cell[:, None, :] == cell[None, :, :]).all(dim=2)
        m = torch.where((m == 0) | same, torch.full_like(m, 1e-5), m)
        assert torch.equal(torch.triu(block), torch.triu(m)), f"cell {c}: upper triangle differs from pg_haversine_matrix"
        assert torch.equal(block, block.t()), f"cell {c}: not symmetric"
        assert torch.equal(torch.diagonal(block), torch.full((n,), 1e-5, dtype=torch.float64, device=DEV))
        np.testing.assert_allclose(block.cpu().numpy(), ref.cell_distances(pts[s:s + n]), rtol=1e-12, atol=1e-9)
    assert float(dist[int(mat_off[2]) + (10 - 3) * 65 + (40 - 3)]) == 1e-5   # the duplicate pair of the 65-point cell (it starts at row 3)


# ------------------------------------------------------------------------------------------------ graphs
CASES = {2: [3, 4, 63, 64, 65, 257], 3: [3, 4, 63, 64, 65, 257, 1025], 100: [100, 257, 1025]}


@pytest.mark.parametrize("ms", [2, 3, 100])
def test_graph_equals_restatement(ops, ms):
    """quantised tie-heavy cells, every size of one min_samples in one call, on the device's own distance matrix"""
    rng = np.random.default_rng(ms)
    sizes = CASES[ms]
    pts = np.concatenate([quantised(rng, n) for n in sizes])
    cell_off = offsets(sizes)
    dist, mat_off = ops.haversine_blocks(torch.from_numpy(pts).to(DEV), cell_off)
    g = run_graph(ops, dist, cell_off, mat_off, ms)
    check_cells(g, dist.cpu().numpy(), cell_off, mat_off, ms, "quantised")


@pytest.mark.parametrize("n", [4, 64, 65, 257])
def test_graph_min_samples_equal_to_n(ops, n):
    rng = np.random.default_rng(n)
    cell_off = offsets([n])
    dist, mat_off = ops.haversine_blocks(torch.from_numpy(quantised(rng, n)).to(DEV), cell_off)
    check_cells(run_graph(ops, dist, cell_off, mat_off, n), dist.cpu().numpy(), cell_off, mat_off, n, "min_samples = n")


def test_graph_all_points_identical(ops):
    sizes = [3, 65, 257]
    pts = np.tile(np.array([[12.3456789, 45.6789012]]), (sum(sizes), 1))
    cell_off = offsets(sizes)
    dist, mat_off = ops.haversine_blocks(torch.from_numpy(pts).to(DEV), cell_off)
    host = dist.cpu().numpy()
    assert (host == 1e-5).all()
    g = run_graph(ops, dist, cell_off, mat_off, 3)
    check_cells(g, host, cell_off, mat_off, 3, "identical points")
    assert g["ordering"][:3].tolist() == [0, 1, 2] and g["pred"][:3].tolist() == [-1, 0, 0]


def test_graph_row_of_inf(ops):
    """a matrix given directly as `dist`: one row of +inf (its point reaches nothing and has an infinite core distance)"""
    rng = np.random.default_rng(9)
    sizes = [7, 65, 257]
    mats = []
    for n in sizes:
        D = ref.cell_distances(quantised(rng, n))
        D[n // 2, :] = np.inf
        mats.append(D.reshape(-1))
    host = np.concatenate(mats)
    cell_off = offsets(sizes)
    mat_off = offsets(np.square(sizes))
    g = run_graph(ops, torch.from_numpy(host).to(DEV), cell_off, mat_off, 3)
    check_cells(g, host, cell_off, mat_off, 3, "inf row")
    assert np.isinf(g["core"][7 + 32])


def test_graph_200_mixed_cells(ops):
    rng = np.random.default_rng(200)
    sizes = np.concatenate([rng.integers(3, 140, 190), rng.integers(129, 300, 9), [1030]]).tolist()
    rng.shuffle(sizes)
    pts = np.concatenate([quantised(rng, n) if i % 2 else np.array([5.0, 50.0]) + rng.normal(0, 0.01, (n, 2)) for i, n in enumerate(sizes)])
    cell_off = offsets(sizes)
    dist, mat_off = ops.haversine_blocks(torch.from_numpy(pts).to(DEV), cell_off)
    g = run_graph(ops, dist, cell_off, mat_off, 3)
    check_cells(g, dist.cpu().numpy(), cell_off, mat_off, 3, "200 cells")


def test_graph_global_form_equals_lds_form(ops):
    """pg_tune_optics_lds_points(64): the cells of 65 and 257 points keep their state in global memory (form 1), the same bits"""
    rng = np.random.default_rng(64)
    sizes = [64, 65, 257]
    pts = np.concatenate([quantised(rng, n) for n in sizes])
    cell_off = offsets(sizes)
    dist, mat_off = ops.haversine_blocks(torch.from_numpy(pts).to(DEV), cell_off)
    lds = run_graph(ops, dist, cell_off, mat_off, 3)
    assert [ops.optics_plan(n, 3)["form"] for n in sizes] == [0, 0, 0]
    try:
        ops.tune_optics_lds_points(64)
        assert [ops.optics_plan(n, 3)["form"] for n in sizes] == [0, 1, 1]
        glob = run_graph(ops, dist, cell_off, mat_off, 3)
    finally:
        ops.tune_optics_lds_points(0)
    for name in NAMES:
        assert np.array_equal(lds[name], glob[name]), name
    check_cells(glob, dist.cpu().numpy(), cell_off, mat_off, 3, "form 1")


def test_graph_largest_lds_cell(ops):
    """one cell of exactly pg_optics_plan's out[2] points, the most LDS any launch asks for, next to a small one"""
    n = ops.optics_plan(2, 2)["lds_points"]
    assert ops.optics_plan(n, 100)["form"] == 0 and ops.optics_plan(n + 1, 100)["form"] == 1
    rng = np.random.default_rng(8192)
    sizes = [130, n]
    pts = np.concatenate([np.array([5.0, 50.0]) + rng.normal(0, 0.05, (m, 2)) for m in sizes])
    cell_off = offsets(sizes)
    dist, mat_off = ops.haversine_blocks(torch.from_numpy(pts).to(DEV), cell_off)
    g = run_graph(ops, dist, cell_off, mat_off, 100)
    check_cells(g, dist.cpu().numpy(), cell_off, mat_off, 100, "largest LDS cell")


def test_graph_equals_recorded_sklearn(ops, golden_dir):
    """the file's numpy matrices uploaded as `dist`: sklearn's own four arrays"""
    z = np.load(os.path.join(golden_dir, "optics_graph.npz"))
    for n, ms in z["cases"]:
        D = z[f"dist_{n}"]
        cell_off, mat_off = offsets([int(n)]), offsets([int(n) * int(n)])
        g = run_graph(ops, torch.from_numpy(D.reshape(-1).copy()).to(DEV), cell_off, mat_off, int(ms))
        for name in NAMES:
            assert np.array_equal(g[name], z[f"{name}_{n}"]), (int(n), name)


# ------------------------------------------------------------------------------------------------ device paths off the beaten track
SENTINEL, GUARD = -7, 64                                            # exact in int64 and in fp64


def guarded(n, dtype):
    return torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=DEV)


def raw_cells(ops, pts, cell_off, ms, stream=None):
    """pg_haversine_blocks and pg_optics_graph through the C ABI, which (unlike the wrappers) takes a cell_off that does not start at 0:
    pts is indexed by the packed row itself, the outputs are packed from the first cell on.  -> (dist, {ordering, core, reach, pred})
    as numpy, every output in front of sentinel elements that must stay untouched."""
    from pigeon_amd import _lib
    L = _lib.load()
    off = cell_off.contiguous()
    n = off[1:] - off[:-1]
    mo = torch.zeros_like(off)
    torch.cumsum(n * n, 0, out=mo[1:])
    N, C, total = int(off[-1] - off[0]), off.numel() - 1, int(mo[-1])
    host = lambda t: ops._p(t)
    dist = guarded(total, torch.float64)
    before = pts.clone()
    _lib.check(L.pg_haversine_blocks(ops._p(pts), host(off), host(mo), C, 1e-5, ops._p(dist), ops._stream()), "pg_haversine_blocks")
    out = {"ordering": guarded(N, torch.int64), "core": guarded(N, torch.float64), "reach": guarded(N, torch.float64),
           "pred": guarded(N, torch.int64)}
    _lib.check(L.pg_optics_graph(ops._p(dist), host(off), host(mo), C, ms, ops._p(out["ordering"]), ops._p(out["core"]),
                                 ops._p(out["reach"]), ops._p(out["pred"]), ops._stream()), "pg_optics_graph")
    torch.cuda.synchronize()
    assert torch.equal(pts.view(torch.int64), before.view(torch.int64)), "pts changed"
    for name, t in [("dist", dist)] + list(out.items()):
        assert bool((t[(total if name == "dist" else N):] == SENTINEL).all()), f"{name}: wrote past its end"
    return dist[:total].cpu().numpy(), {k: v[:N].cpu().numpy() for k, v in out.items()}


def test_cells_packed_from_a_nonzero_base(ops):
    """cell_off[0] = 7: the first 7 rows of pts belong to nobody (NaN) and all three kernels index from the first cell on.  The
    matrices and the four graph arrays are those of the same cells run from 0, bit for bit."""
    rng = np.random.default_rng(7)
    sizes = [3, 65, 257]
    pts = np.concatenate([quantised(rng, n) for n in sizes])
    shifted = torch.from_numpy(np.concatenate([np.full((7, 2), np.nan), pts])).to(DEV)
    d7, g7 = raw_cells(ops, shifted, offsets(sizes) + 7, 3)
    d0, g0 = raw_cells(ops, torch.from_numpy(pts).to(DEV), offsets(sizes), 3)
    assert not np.isnan(d7).any() and np.array_equal(d7, d0)
    for name in NAMES:
        assert np.array_equal(g7[name], g0[name]), name
    check_cells(g7, d7, offsets(sizes), offsets(np.square(sizes)), 3, "base 7")


def test_haversine_blocks_with_empty_cells(ops):
    """cells of 0, 3, 0, 0, 65 and 0 points: the rows are found across the empty cells, mat_off repeats where a cell is empty"""
    rng = np.random.default_rng(65)
    pts = torch.from_numpy(np.concatenate([quantised(rng, n) for n in (3, 65)])).to(DEV)
    sizes = [0, 3, 0, 0, 65, 0]
    dist, mat_off = ops.haversine_blocks(pts, offsets(sizes))
    want, want_off = ops.haversine_blocks(pts, offsets([3, 65]))
    torch.cuda.synchronize()
    assert mat_off.tolist() == [0, 0, 9, 9, 9, 9 + 65 * 65, 9 + 65 * 65] and want_off.tolist() == [0, 9, 9 + 65 * 65]
    assert dist.numel() == 9 + 65 * 65 and torch.equal(dist, want)
    np.testing.assert_allclose(dist[9:].reshape(65, 65).cpu().numpy(), ref.cell_distances(pts[3:].cpu().numpy()), rtol=1e-12, atol=1e-9)


def test_graph_global_form_1024_threads(ops):
    """pg_tune_optics_lds_points(64) with cells of 1025 and 300 points: the 1024-thread and the 256-thread ordering kernel with their
    state in global memory, the same bits as the LDS form and as the restatement"""
    rng = np.random.default_rng(1025)
    sizes = [1025, 300]
    pts = np.concatenate([quantised(rng, n) for n in sizes])
    cell_off = offsets(sizes)
    dist, mat_off = ops.haversine_blocks(torch.from_numpy(pts).to(DEV), cell_off)
    lds = run_graph(ops, dist, cell_off, mat_off, 3)
    assert [(ops.optics_plan(n, 3)["form"], ops.optics_plan(n, 3)["threads"]) for n in sizes] == [(0, 1024), (0, 256)]
    try:
        ops.tune_optics_lds_points(64)
        assert [(ops.optics_plan(n, 3)["form"], ops.optics_plan(n, 3)["threads"]) for n in sizes] == [(1, 1024), (1, 256)]
        glob = run_graph(ops, dist, cell_off, mat_off, 3)
    finally:
        ops.tune_optics_lds_points(0)
    for name in NAMES:
        assert np.array_equal(lds[name], glob[name]), name
    check_cells(glob, dist.cpu().numpy(), cell_off, mat_off, 3, "form 1, 1024 threads")


def test_graph_global_form_by_size(ops):
    """under the default knobs: one cell of pg_optics_plan's out[2] + 1 points -- the route every large geocell takes -- next to a
    130-point cell"""
    n = ops.optics_plan(2, 2)["lds_points"] + 1
    plan = ops.optics_plan(n, 100)
    assert plan["form"] == 1 and plan["threads"] == 1024 and n <= plan["max_points"]
    rng = np.random.default_rng(8193)
    sizes = [n, 130]
    pts = np.concatenate([np.array([5.0, 50.0]) + rng.normal(0, 0.05, (m, 2)) for m in sizes])
    cell_off = offsets(sizes)
    dist, mat_off = ops.haversine_blocks(torch.from_numpy(pts).to(DEV), cell_off)
    g = run_graph(ops, dist, cell_off, mat_off, 100)
    check_cells(g, dist.cpu().numpy(), cell_off, mat_off, 100, "global form by size")


def test_graph_on_a_side_stream(ops):
    """both calls take torch's current stream and order their scratch on it: a side stream gives the default stream's bits"""
    rng = np.random.default_rng(11)
    sizes = [64, 65, 257, 1025]
    pts = torch.from_numpy(np.concatenate([quantised(rng, n) for n in sizes])).to(DEV)
    cell_off = offsets(sizes)
    dist, mat_off = ops.haversine_blocks(pts, cell_off)
    want = run_graph(ops, dist, cell_off, mat_off, 3)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
    with torch.cuda.stream(side):
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream
        dist2, mat_off2 = ops.haversine_blocks(pts, cell_off)
        got = run_graph(ops, dist2, cell_off, mat_off2, 3)
    torch.cuda.synchronize()
    assert torch.equal(mat_off, mat_off2) and torch.equal(dist, dist2)
    for name in NAMES:
        assert np.array_equal(got[name], want[name]), name


def test_optics_graph_cells_batches(ops):
    """prototypes.optics_graph_cells on interleaved rows with unsorted string labels, cells of 5, 40, 3, 130 and 70 rows at min_samples 4:
    with the default memory budget (one batch) and with 8 * 70^2 bytes (four: the 130-row cell is over budget and goes alone) the
    same arrays per cell; the 3-row cell is left out; `rows` are in row order; every cell's arrays are the restatement's on the cell's
    own device matrix."""
    from pigeon_amd import prototypes
    rng = np.random.default_rng(4)
    sizes = {"delta": 5, "alpha": 40, "echo": 3, "charlie": 130, "bravo": 70}
    labels = rng.permutation(np.concatenate([[k] * n for k, n in sizes.items()]))
    lnglat = quantised(rng, len(labels), side=12)
    one = prototypes.optics_graph_cells(lnglat, labels, 4)
    many = prototypes.optics_graph_cells(lnglat, labels, 4, memory_bytes=8 * 70 * 70)
    assert sorted(one) == sorted(many) == ["alpha", "bravo", "charlie", "delta"]
    for cell, n in sizes.items():
        if cell == "echo":
            continue
        rows = np.flatnonzero(labels == cell)
        assert len(rows) == n and np.array_equal(one[cell]["rows"], rows) and np.array_equal(many[cell]["rows"], rows)
        D, _ = ops.haversine_blocks(torch.from_numpy(lnglat[rows]).to(DEV), offsets([n]), prototypes.ZERO_AS)
        want = ref.graph(D.cpu().numpy().reshape(n, n), 4)
        for name, w in zip(NAMES, want):
            assert one[cell][name].dtype == w.dtype and np.array_equal(one[cell][name], w), (cell, name)
            assert np.array_equal(many[cell][name], w), (cell, name, "small budget")


def test_wrapper_refusals(ops):
    d = torch.zeros(16, dtype=torch.float64, device=DEV)
    from pigeon_amd._lib import PigeonHipError
    with pytest.raises(PigeonHipError, match="min_samples must be at least 2"):
        ops.optics_graph(d, offsets([4]), offsets([16]), 1)
    with pytest.raises(PigeonHipError, match="fewer than min_samples"):
        ops.optics_graph(d, offsets([4]), offsets([16]), 5)
    with pytest.raises(PigeonHipError, match="room for its n x n"):
        ops.optics_graph(d, offsets([4]), offsets([15]), 2)
    with pytest.raises(PigeonHipError, match="dist has 16 elements"):
        ops.optics_graph(d, offsets([4, 4]), offsets([16, 16]), 2)
    with pytest.raises(PigeonHipError, match="device tensor"):
        ops.haversine_blocks(torch.zeros(4, 2, dtype=torch.float64), offsets([4]))


# ------------------------------------------------------------------------------------------------ end to end
def test_protodataset_end_to_end(ops, golden_dir, tmp_path):
    """ProtoDataset.generate on the GPU writes the reference's CSV (both cluster_args of the fixture); the CSV and a tiny embedding
    set then go through build_bank and ProtoRefiner.forward."""
    pytest.importorskip("sklearn")
    import datasets
    from pigeon_amd.prototypes import ProtoDataset
    from pigeon_amd.proto_refiner import ProtoRefiner
    proto = np.load(os.path.join(golden_dir, "proto_csv.npz"))
    df = _frame(proto)
    outs = []
    for which in (0, 1):
        ms, xi = proto["cluster_args"][which]
        out = tmp_path / f"protos_{which}.csv"
        ds = ProtoDataset(df, None, str(out), cluster_args=(int(ms), float(xi)))
        ds.generate()
        assert np.array_equal(ds.df["cluster"].values, proto[f"labels_{which}"])
        assert_same_table(out.read_text(), str(proto[f"csv_{which}"]))
        outs.append(str(out))
    train = df[df["selection"] == "train"].reset_index(drop=True)
    g = torch.Generator().manual_seed(3)
    emb = torch.nn.functional.normalize(torch.randn((len(train), 1024), generator=g), dim=1).numpy()
    hf = datasets.Dataset.from_dict({"embedding": emb, "labels": train[["lng", "lat"]].values.astype(np.float32)})
    hf.set_format("torch")
    ds_dir = str(tmp_path / "emb")
    datasets.DatasetDict(train=hf).save_to_disk(ds_dir)
    refiner = ProtoRefiner(topk=3, max_refinement=1000, temperature=1.6, proto_path=outs[0], dataset_path=ds_dir).eval()
    assert refiner.num_geocells == 6
    B = 4
    cand = torch.tensor([[5, 4, 3], [2, 3, 4], [0, 1, 2], [4, 5, 2]], dtype=torch.int64)
    probs = torch.tensor([[0.5, 0.3, 0.2]] * B, dtype=torch.float32)
    init = torch.from_numpy(train[["lng", "lat"]].values[:B].astype(np.float64))
    _, llh, cell = refiner(torch.from_numpy(emb[:B]).to(DEV), initial_preds=init, candidate_cells=cand, candidate_probs=probs, quiet=True)
    torch.cuda.synchronize()
    assert llh.shape == (B, 2) and cell.shape == (B,) and bool(torch.isfinite(llh).all())
