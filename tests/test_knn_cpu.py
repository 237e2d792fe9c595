"""What the nearest-neighbour entry points decide on the host (no GPU): every PG_EINVAL that precedes a HIP call, pg_knn_plan's
arithmetic, the command line of pigeon_amd.neighbours, and the refusals of evaluate_model / serve, with stubs."""
import ctypes as C

import numpy as np
import pytest

PG_EINVAL = -1


@pytest.fixture(scope="module")
def L(hip_lib):
    from pigeon_amd import _lib
    lib = _lib.load()
    lib.pg_tune_knn_spans(0)
    yield lib
    lib.pg_tune_knn_spans(0)


def last(L):
    return L.pg_last_error().decode()


def bank_struct(n=1000, x=4096, x16=8192, hn=12288, stats=16384):
    from pigeon_amd import _lib
    return _lib.KnnBank(x=x, x16=x16, hn=hn, stats=stats, n=n)


def call(L, bank=None, q=4096, B=4, k=10, exclude=None, mode=0, idx=4096, d2=4096, cert=None, ws=256 * 1024, ws_bytes=1 << 40):
    """pg_knn_search with fake, aligned, never-dereferenced pointers: every path taken here must return before a HIP call"""
    b = bank_struct() if bank is None else bank
    return L.pg_knn_search(C.byref(b) if b is not False else None, q, B, k, exclude, mode, idx, d2, cert, ws, ws_bytes, None)


# ---------------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("kw,needle", [
    (dict(bank=False), "bank"),
    (dict(q=None), "q"),
    (dict(idx=None), "idx"),
    (dict(d2=None), "d2"),
    (dict(ws=None), "workspace"),
    (dict(ws=256 * 1024 + 16), "256-byte aligned"),
    (dict(ws_bytes=1024), "workspace_bytes"),
    (dict(k=0), "k = 0"),
    (dict(k=65), "k = 65"),
    (dict(B=-1), "B = -1"),
    (dict(mode=3), "mode = 3"),
    (dict(mode=-1), "mode = -1"),
    (dict(q=4100), "q must be 16-byte aligned"),
    (dict(bank=dict(n=-1)), "n = -1"),
    (dict(bank=dict(n=1 << 31)), "n = "),
    (dict(bank=dict(x=None)), "bank->x"),
    (dict(bank=dict(x16=None)), "bank->x16"),
    (dict(bank=dict(hn=None)), "bank->hn"),
    (dict(bank=dict(stats=None)), "bank->stats"),
    (dict(bank=dict(x=4100)), "bank->x must be 16-byte aligned"),
    (dict(bank=dict(x16=8200), mode=2), "bank->x16 must be 16-byte aligned"),
])
def test_search_refuses_by_name_before_any_hip_call(L, kw, needle):
    kw = dict(kw)
    if isinstance(kw.get("bank"), dict):
        kw["bank"] = bank_struct(**kw["bank"])
    assert call(L, **kw) == PG_EINVAL
    assert needle in last(L), last(L)


def test_search_empty_batch_is_a_no_op(L):
    assert call(L, B=0, q=None, idx=None, d2=None, ws=None, ws_bytes=0) == 0


def test_exact_mode_needs_the_fp32_bank_only(L):
    # mode 1 with the prepared arrays missing passes the pointer checks and stops at the short workspace
    assert call(L, bank=bank_struct(x16=None, hn=None, stats=None), mode=1, ws_bytes=16) == PG_EINVAL
    assert "workspace_bytes" in last(L)


def test_prepare_and_workspace_refusals(L):
    out = C.c_size_t(0)
    assert L.pg_knn_workspace_bytes(1000, 4, 10, None) == PG_EINVAL and "bytes" in last(L)
    assert L.pg_knn_workspace_bytes(1000, 4, 0, C.byref(out)) == PG_EINVAL and "k = 0" in last(L)
    assert L.pg_knn_workspace_bytes(-5, 4, 1, C.byref(out)) == PG_EINVAL and "n = -5" in last(L)
    assert L.pg_knn_workspace_bytes(1000, -2, 1, C.byref(out)) == PG_EINVAL and "B = -2" in last(L)
    assert L.pg_knn_prepare(4096, -1, 4096, 4096, 4096, None) == PG_EINVAL and "n = -1" in last(L)
    assert L.pg_knn_prepare(4096, 5, 4096, 4096, None, None) == PG_EINVAL and "stats" in last(L)
    assert L.pg_knn_prepare(None, 5, 4096, 4096, 4096, None) == PG_EINVAL and "x" in last(L)
    assert L.pg_knn_prepare(4096, 5, None, 4096, 4096, None) == PG_EINVAL and "x16" in last(L)
    assert L.pg_knn_prepare(4096, 5, 4096, None, 4096, None) == PG_EINVAL and "hn" in last(L)
    assert L.pg_knn_prepare(4100, 5, 4096, 4096, 4096, None) == PG_EINVAL and "16-byte aligned" in last(L)
    assert L.pg_tune_knn_spans(-1) == PG_EINVAL and L.pg_tune_knn_spans(5000) == PG_EINVAL and "spans" in last(L)
    assert L.pg_knn_plan(10, 1, 1, None) == PG_EINVAL and "out" in last(L)


# ---------------------------------------------------------------------------------------------------------------------- the plan
def test_plan_arithmetic(L):
    from pigeon_amd import hip_ops
    p = hip_ops.knn_plan(4099, 64, 16)
    assert p["candidates"] == 128 and p["rows_per_tile"] == 128 and p["queries_per_tile"] == 32 and p["exact_rows_per_tile"] == 256
    assert p["spans"] == 33 and p["tiles_per_span"] == 1 and p["exact_spans"] == 17          # one span per tile while there are few
    assert p["lds_bytes"] <= 160 * 1024
    big = hip_ops.knn_plan(1 << 20, 128, 10)
    assert big["spans"] == 256 and big["tiles_per_span"] == 32 and big["exact_spans"] == 512
    assert big["spans"] * big["tiles_per_span"] * big["rows_per_tile"] >= 1 << 20
    assert hip_ops.knn_plan(0, 0, 1)["spans"] == 1
    try:
        hip_ops.tune_knn_spans(3)
        p3 = hip_ops.knn_plan(4099, 64, 16)
        assert p3["spans"] == 3 and p3["tiles_per_span"] == 11 and p3["exact_spans"] == 3
        few = hip_ops.knn_plan(100, 1, 1)                                                   # more spans than tiles
        assert few["spans"] == 3 and few["tiles_per_span"] == 1
        w3 = hip_ops.knn_workspace_bytes(4099, 64, 16)
    finally:
        hip_ops.tune_knn_spans(0)
    w = hip_ops.knn_workspace_bytes(4099, 64, 16)
    assert w % 256 == 0 and w3 % 256 == 0 and w3 < w
    assert w >= 64 * 33 * 128 * 8 + 64 * 128 * 8 + 64 * 17 * 16 * 8


# ---------------------------------------------------------------------------------------------------------------------- wrappers
def test_wrappers_refuse_by_name_without_a_gpu():
    import torch
    from pigeon_amd import _lib, hip_ops
    with pytest.raises(_lib.PigeonHipError, match="device tensor"):
        hip_ops.knn_prepare(torch.zeros(3, 1024))
    with pytest.raises(_lib.PigeonHipError, match="KnnBank"):
        hip_ops.knn_search(torch.zeros(3, 1024), torch.zeros(1, 1024), 1)
    with pytest.raises(_lib.PigeonHipError, match="mode"):
        hip_ops.knn_search(hip_ops.KnnBank(torch.zeros(3, 1024), None, None, None), torch.zeros(1, 1024), 1, mode="fast")


# ---------------------------------------------------------------------------------------------------------------------- the command line
def test_cli_arguments(capsys):
    from pigeon_amd import neighbours as nb
    a = nb.parse_args(["--bank", "d", "--queries", "q.npy", "-o", "o.npz"])
    assert (a.bank, a.queries, a.k, a.output, a.self_search, a.exact) == ("d", "q.npy", 10, "o.npz", False, False)
    a = nb.parse_args(["--bank", "d", "--self", "-k", "5", "-o", "o.npz", "--exact"])
    assert a.self_search and a.k == 5 and a.exact and a.queries is None
    for bad in (["--bank", "d", "-o", "o.npz"],                                            # neither --queries nor --self
                ["--bank", "d", "--self", "--queries", "q.npy", "-o", "o.npz"],            # both
                ["--bank", "d", "--self", "-k", "0", "-o", "o.npz"],
                ["--bank", "d", "--self", "-k", "65", "-o", "o.npz"],
                ["--bank", "d", "--self", "-o", "o.npz", "--batch", "0"],
                ["--queries", "q.npy", "-o", "o.npz"],                                     # no bank
                ["--bank", "d", "--self"]):                                                # no output
        with pytest.raises(SystemExit):
            nb.parse_args(bad)
    capsys.readouterr()


def test_check_k():
    from pigeon_amd.neighbours import check_k
    assert check_k(1) == 1 and check_k(np.int64(64)) == 64
    for bad in (0, 65, -1, 2.0, True, "3", None):
        with pytest.raises(ValueError, match="1..64"):
            check_k(bad)


# ---------------------------------------------------------------------------------------------------------------------- evaluate / serve
def test_evaluate_model_refuses_neighbours_without_a_refiner():
    from pigeon_amd.evaluate import evaluate_model

    class Stub:                                                                             # never reached: refused before the model is touched
        def __getattr__(self, name):
            raise AssertionError(f"model.{name} was read")

    with pytest.raises(ValueError, match="refiner"):
        evaluate_model(Stub(), [], refiner=None, neighbours=5)
    with pytest.raises(ValueError, match="1..64"):
        evaluate_model(Stub(), [], refiner=object(), neighbours=0)
    with pytest.raises(ValueError, match="1..64"):
        evaluate_model(Stub(), [], refiner=object(), neighbours=65)


def test_serve_refuses_neighbours_without_a_refiner_bank():
    from pigeon_amd import serve

    class Model:
        pass

    with pytest.raises(ValueError, match="refiner"):
        serve.make_app(Model(), None, neighbours=3)
    with pytest.raises(ValueError, match="refiner"):
        serve.make_app(Model(), object(), neighbours=3)                                    # a refiner without a bank
    with pytest.raises(ValueError, match="1..64"):
        serve.make_app(Model(), None, neighbours=0)
    with pytest.raises(ValueError, match="refiner"):
        serve.predict_panorama([], Model(), None, neighbours=3)
    with pytest.raises(SystemExit):
        serve.main(["--neighbours", "3"])                                                  # no --protos: refused at start-up
    with pytest.raises(SystemExit):
        serve.main(["--neighbours", "99", "--protos", "p.csv", "--dataset", "d"])


def test_neighbour_metrics():
    from pigeon_amd.evaluate import neighbour_metrics
    from pigeon_amd.geo_utils import haversine_np
    labels = np.array([[0.0, 0.0], [10.0, 10.0], [20.0, -5.0]])
    nn = np.array([[[0.0, 0.0], [5.0, 5.0]], [[10.0, 11.0], [0.0, 0.0]], [[50.0, 50.0], [20.0, -5.0]]])
    preds = np.array([[1.0, 0.0], [10.0, 10.0], [21.0, -5.0]])
    m = neighbour_metrics(nn, haversine_np, labels, preds)
    d = haversine_np(nn[:, 0, :], labels)
    assert m["Mean_km_error_nn"] == pytest.approx(np.mean(d)) and m["Median_km_error_nn"] == pytest.approx(np.median(d))
    assert m["NN_beats_model"] == pytest.approx(1 / 3) and 0 <= m["Geoguessr_score_nn"] <= 5000
