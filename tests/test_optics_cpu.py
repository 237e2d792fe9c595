"""The prototype cluster table without a GPU: the host restatement of the OPTICS graph against sklearn's recorded arrays (and a live
sklearn), the table writer against the reference's recorded CSV with the restatement injected for the device, and the host side of the
C ABI (symbols, plan, refusals)."""
import ctypes as C
import io
import os

import numpy as np
import pytest

import _opticsref as ref
from _opticsref import assert_same_table, frame_of as _frame, parse_csv

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def graphs():
    return np.load(os.path.join(GOLDEN, "optics_graph.npz"))


@pytest.fixture(scope="module")
def proto():
    return np.load(os.path.join(GOLDEN, "proto_csv.npz"))


def _case(g, n):
    return g[f"dist_{n}"], tuple(g[f"{k}_{n}"] for k in ("ordering", "core", "reach", "pred"))


def test_restatement_equals_recorded_sklearn(graphs):
    for n, ms in graphs["cases"]:
        D, want = _case(graphs, n)
        np.testing.assert_allclose(ref.cell_distances(graphs[f"pts_{n}"]), D, rtol=1e-12, atol=1e-9)   # the recorded matrix is the input
        got = ref.graph(D, int(ms))
        for name, a, b in zip(("ordering", "core", "reach", "pred"), got, want):
            assert a.dtype == b.dtype and np.array_equal(a, b), (int(n), name)


def test_restatement_equals_live_sklearn(graphs):
    pytest.importorskip("sklearn")
    from sklearn.cluster._optics import compute_optics_graph
    rng = np.random.default_rng(5)
    cases = [(graphs[f"dist_{n}"], int(ms)) for n, ms in graphs["cases"]]
    pts = np.stack([2.0 + 1e-3 * rng.integers(0, 9, 120), 40.0 + 1e-3 * rng.integers(0, 9, 120)], axis=1)
    cases.append((ref.cell_distances(pts), 5))
    for D, ms in cases:
        want = compute_optics_graph(X=D, min_samples=ms, max_eps=np.inf, metric="precomputed", p=2, metric_params=None, algorithm="auto",
                                    leaf_size=30, n_jobs=None)
        for a, b in zip(ref.graph(D, ms), want):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("mistake", ["rounding", "tie_smallest", "core_with_self", "skip_processed"])
def test_recorded_graphs_reject_a_mistake(graphs, mistake):
    """no rounding / ties to the larger index / core distance without the point itself / updating processed points: each must differ
    from sklearn's recorded arrays on at least one fixture cell"""
    differs = False
    for n, ms in graphs["cases"]:
        D, want = _case(graphs, n)
        got = ref.graph(D, int(ms), **{mistake: False})
        differs = differs or any(not np.array_equal(a, b) for a, b in zip(got, want))
    assert differs, mistake


def _host_graph(points, min_samples):
    return ref.graph(ref.cell_distances(points), min_samples)


@pytest.mark.parametrize("which", [0, 1])
def test_protodataset_reproduces_the_reference_csv(proto, tmp_path, which):
    """ProtoDataset.generate with the numpy restatement in the device's place against the CSV the reference's own generate() wrote."""
    pytest.importorskip("sklearn")
    from pigeon_amd.prototypes import ProtoDataset
    ms, xi = proto["cluster_args"][which]
    out = tmp_path / "protos.csv"
    ds = ProtoDataset(_frame(proto), None, str(out), cluster_args=(int(ms), float(xi)), graph_fn=_host_graph)
    ds.generate()
    assert np.array_equal(ds.df["cluster"].values, proto[f"labels_{which}"])
    assert_same_table(out.read_text(), str(proto[f"csv_{which}"]))
    table = parse_csv(out.read_text())
    sizes = ds.df.groupby("geocell_idx").size()
    small = sizes[sizes < int(ms)].index.tolist()
    assert small, "the fixture has cells below min_samples"
    for c in small:                                               # reference prototype.py:144-145: one cluster 0 holding every row
        rows = table[table["geocell_idx"] == c]
        assert rows["cluster"].tolist() == [0] and rows["count"].tolist() == [int(sizes[c])]
    assert not os.path.exists(tmp_path / "tmp")
    assert all(isinstance(l, list) and l for l in table["indices"])


def test_protodataset_needs_cells_or_embeddings(proto):
    from pigeon_amd.prototypes import ProtoDataset
    with pytest.raises(ValueError, match="geocell_idx"):
        ProtoDataset(_frame(proto).drop(columns=["geocell_idx"]), None, "unused.csv")


def test_cluster_cells_refuses_fractional_min_samples():
    from pigeon_amd.prototypes import cluster_cells
    with pytest.raises(ValueError, match="min_samples"):
        cluster_cells(np.zeros((4, 2)), np.zeros(4, dtype=np.int64), (0.5, 0.1), graph_fn=_host_graph)


NEW_SYMBOLS = ("pg_haversine_blocks", "pg_optics_graph", "pg_optics_plan", "pg_tune_optics_lds_points")


def test_library_exports_the_new_symbols(hip_lib):
    from pigeon_amd import _lib
    for s in NEW_SYMBOLS:
        assert hasattr(hip_lib, s) and s in _lib.SIGNATURES, s
    assert hip_lib.pg_abi_version() == 7


def _plan(lib, n, ms):
    out = (C.c_int32 * 4)()
    rc = lib.pg_optics_plan(n, ms, out)
    return rc, [int(v) for v in out]


def test_plan_is_monotone_and_consistent(hip_lib):
    from pigeon_amd import hip_ops
    try:
        rc, top = _plan(hip_lib, 2, 2)
        assert rc == 0
        lds_default, n_max = top[2], top[3]
        assert n_max == 32768 and 64 <= lds_default <= n_max
        assert lds_default * 13 + 1024 <= 160 * 1024              # the state of the largest LDS-resident cell fits a CU's LDS
        prev = None
        for n in [2, 3, 63, 64, 65, 128, 129, 1024, 1025, lds_default - 1, lds_default, lds_default + 1, n_max]:
            rc, p = _plan(hip_lib, n, 2)
            assert rc == 0 and p[2] == lds_default and p[3] == n_max
            assert p[0] == (1 if n > lds_default else 0)
            assert p[1] in (64, 256, 1024)
            if prev is not None:
                assert p[0] >= prev[0] and p[1] >= prev[1]
            prev = p
        assert hip_ops.optics_plan(65, 3) == {"form": 0, "threads": 64, "lds_points": lds_default, "max_points": n_max}
        hip_ops.tune_optics_lds_points(64)
        assert _plan(hip_lib, 64, 2)[1][0] == 0 and _plan(hip_lib, 65, 2)[1][0] == 1 and _plan(hip_lib, 65, 2)[1][2] == 64
        assert _plan(hip_lib, 65, 2)[1][1] == 64                  # the tune moves the state, not the threads
        assert hip_lib.pg_tune_optics_lds_points(lds_default + 1) != 0 and hip_lib.pg_tune_optics_lds_points(-1) != 0
    finally:
        hip_lib.pg_tune_optics_lds_points(0)
    assert _plan(hip_lib, 65, 2)[1][0] == 0


def test_refusals_are_named(hip_lib):
    """min_samples < 2, a cell below min_samples, a cell above 32768 points: PG_EINVAL with the reason, before any device call (there
    is no device here; the pointers are never followed)."""
    dummy = C.c_void_p(8)

    def call(sizes, ms):
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        mat = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64) ** 2)]).astype(np.int64)
        rc = hip_lib.pg_optics_graph(dummy, C.c_void_p(off.ctypes.data), C.c_void_p(mat.ctypes.data), len(sizes), ms, dummy, dummy, dummy,
                                     dummy, None)
        return rc, hip_lib.pg_last_error().decode()

    rc, msg = call([5, 6], 1)
    assert rc == -1 and "min_samples must be at least 2" in msg
    rc, msg = call([5, 3, 6], 4)
    assert rc == -1 and "cell 1 has 3 points, fewer than min_samples = 4" in msg
    rc, msg = call([5, 32769], 2)
    assert rc == -1 and "cell 1 has 32769 points, more than the 32768" in msg
    out = (C.c_int32 * 4)()
    assert hip_lib.pg_optics_plan(1, 1, out) == -1 and "min_samples" in hip_lib.pg_last_error().decode()
    assert hip_lib.pg_optics_plan(3, 4, out) == -1 and "fewer than min_samples" in hip_lib.pg_last_error().decode()
    assert hip_lib.pg_optics_plan(32769, 4, out) == -1 and "more than the 32768" in hip_lib.pg_last_error().decode()


def test_cli_parser():
    from pigeon_amd import prototypes
    a = prototypes._arg_parser().parse_args(["--metadata", "m.csv", "-o", "o.csv"])
    assert (a.min_samples, a.xi, a.embeddings) == (100, 0.1, None)
