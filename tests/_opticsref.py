"""Host restatements the OPTICS tests compare against (numpy only; no sklearn, no GPU).

`graph` restates sklearn.cluster._optics.compute_optics_graph(metric='precomputed', max_eps=inf) (sklearn 1.7.2, _optics.py):
  * core distances (_compute_core_distances_ :406-441, :627-631): the min_samples-th smallest entry of each row of the matrix, the point itself included
    (NearestNeighbors on a precomputed matrix does not skip the diagonal), rounded with np.around(., finfo(float64).precision = 15);
  * the main loop (:640-660, :643): the next point is `index[np.argmin(reachability_[index])]` over the unprocessed `index` -- the first
    minimum, so ties (inf included) go to the smallest index;
  * _set_reach_dist (:672-720): over the unprocessed points only, rdists = np.maximum(dists, core[p]) (:711) rounded the same way
    (:712), `improved = rdists < reachability_` (:713, strict).
tests/golden/optics_graph.npz holds sklearn's own four arrays for tie-heavy inputs; tests/test_optics_cpu.py checks this
restatement against them (and against a live sklearn where one is installed) and that four deliberate mistakes are told apart.

`haversine_matrix_np` is the numpy distance matrix of reference preprocessing/geo_utils.py:77-93, `cell_distances` the
reference's use of it in dataset_creation/prototype/prototype.py:130-133 (zeros -> 1e-5).
"""
import io

import numpy as np

RAD = np.float64(6378137.0)


def haversine_matrix_np(x: np.ndarray, y: np.ndarray) -> np.ndarray:
    """x (N,2), y (2,M) [lng,lat] degrees -> (N,M) km (reference preprocessing/geo_utils.py:77-93)"""
    x_rad, y_rad = np.deg2rad(x), np.deg2rad(y)
    delta = np.expand_dims(x_rad, axis=2) - y_rad
    p = np.expand_dims(np.cos(x_rad[:, 1]), axis=1) * np.expand_dims(np.cos(y_rad[1, :]), axis=0)
    a = np.sin(delta[:, 1, :] / 2) ** 2 + p * np.sin(delta[:, 0, :] / 2) ** 2
    c = 2 * np.arcsin(np.sqrt(a))
    return (RAD * c) / 1000


def cell_distances(points: np.ndarray, zero_as: float = 1e-5) -> np.ndarray:
    """reference dataset_creation/prototype/prototype.py:130-133"""
    d = haversine_matrix_np(points, points.T)
    return np.where(d == 0, zero_as, d)


def graph(D: np.ndarray, min_samples: int, rounding: bool = True, tie_smallest: bool = True, core_with_self: bool = True,
          skip_processed: bool = True):
    """(ordering int64, core fp64, reach fp64, pred int64) of one cell's n x n matrix D.  The four keyword switches turn on one
    deliberate mistake each (the tests check that every one of them is caught)."""
    D = np.asarray(D, dtype=np.float64)
    n = D.shape[0]
    R = (lambda v: np.around(v, 15)) if rounding else (lambda v: v)
    if core_with_self:
        core = R(np.partition(D, min_samples - 1, axis=1)[:, min_samples - 1])
    else:
        off = D.copy()
        off[np.arange(n), np.arange(n)] = np.inf
        core = R(np.partition(off, min_samples - 1, axis=1)[:, min_samples - 1])
    reach = np.full(n, np.inf)
    pred = np.full(n, -1, dtype=np.int64)
    done = np.zeros(n, dtype=bool)
    ordering = np.empty(n, dtype=np.int64)
    for t in range(n):
        idx = np.flatnonzero(~done)
        r = reach[idx]
        p = idx[np.argmin(r)] if tie_smallest else idx[len(r) - 1 - np.argmin(r[::-1])]
        done[p] = True
        ordering[t] = p
        js = np.flatnonzero(~done) if skip_processed else np.delete(np.arange(n), p)
        rd = R(np.maximum(D[p, js], core[p]))
        better = rd < reach[js]
        reach[js[better]] = rd[better]
        pred[js[better]] = p
    return ordering, core, reach, pred


# ---- the prototype table of tests/golden/proto_csv.npz (shared by the CPU and the GPU test of ProtoDataset.generate)
def frame_of(proto):
    """the metadata frame of tests/golden/proto_csv.npz"""
    import pandas as pd
    sel = np.where(proto["selection_is_train"], "train", "val")
    return pd.DataFrame({"selection": sel, "lng": proto["lng"], "lat": proto["lat"], "geocell_idx": proto["geocell_idx"]})


def parse_csv(text):
    """a prototype CSV as the existing bank builder reads it (pigeon_amd.proto_refiner.build_bank: read_csv + _load_indices)"""
    import pandas as pd
    from pigeon_amd.proto_refiner import _load_indices
    df = pd.read_csv(io.StringIO(text))
    df["indices"] = df["indices"].apply(_load_indices)
    return df


def assert_same_table(got_text, want_text):
    """columns, dtypes and `indices` lists equal, lng and lat == exactly"""
    got, want = parse_csv(got_text), parse_csv(want_text)
    assert list(got.columns) == list(want.columns) == ["geocell_idx", "cluster", "lng", "lat", "count", "indices"]
    assert list(got.dtypes) == list(want.dtypes)
    assert len(got) == len(want)
    for col in ("geocell_idx", "cluster", "count", "indices"):
        assert got[col].tolist() == want[col].tolist(), col
    assert (got["lng"].values == want["lng"].values).all() and (got["lat"].values == want["lat"].values).all()
