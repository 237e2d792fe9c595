"""The prototype cluster table on the GPU (run with -m gpu on an MI355X): pg_haversine_blocks against pg_haversine_matrix (bits) and
numpy (1e-12), pg_optics_graph against the numpy restatement tests/_opticsref.py on the device's own matrix and against sklearn's
recorded arrays (array_equal on ordering, core distances, reachability, predecessors), both forms of the ordering kernel, and
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
