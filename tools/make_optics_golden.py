"""Write the fixtures of the prototype-table tests (CPU only; not a test; needs the reference tree and scikit-learn):

    python tools/make_optics_golden.py            ->  tests/golden/proto_csv.npz, tests/golden/optics_graph.npz

proto_csv.npz     a tiny seeded metadata frame (six geocells of 2, 3, 40, 64, 65 and 150 training rows, rows of all cells interleaved,
                  a few non-training rows, clumped points with exact duplicates, coordinates not quantised), and what the REFERENCE's
                  own `ProtoDataset(...).generate()` (dataset_creation/prototype/prototype.py:38-95) writes for it with cluster_args
                  (3, 0.15) and (20, 0.1): the CSV text and the per-row cluster labels.  The reference file is executed as it is, read at
                  run time; its two imports that are not installed get stand-ins -- a `pandarallel` whose `parallel_apply` is `apply`, an
                  empty `geopandas` -- and it runs in a temporary working directory with a `tmp/` folder (it saves an array there).
                  Before anything is written the fixture is checked to be STABLE: the reference is re-run 20 times with every computed
                  distance multiplied by 1 + u, u uniform in +-1e-11 (ten times the 1e-12 the device's haversine is held to against
                  numpy), and every draw must give the same labels; the seed is advanced until that holds.  u is drawn per unordered pair
                  of distinct COORDINATES, not per matrix element: the device's distance is a function of the two points' coordinates
                  and pg_haversine_blocks mirrors the upper triangle, so its matrix is symmetric as numpy's is and exact duplicates
                  keep equal rows and columns (the 1e-5 the reference writes for a zero distance, which the device writes as a
                  constant for identical points, stays 1e-5).  Those exact ties decide the graph at min_samples = 3: with u drawn per
                  element, or per ORDERED pair, no seed of ten kept its labels -- which is why the device matrix is mirrored.
optics_graph.npz  quantised, tie-heavy cells of 3, 7, 64, 65 and 257 points: the points, their numpy distance matrix
                  (tests/_opticsref.py cell_distances), min_samples and the four arrays of sklearn's compute_optics_graph.
"""
import io
import os
import sys
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CELL_SIZES = (2, 3, 40, 64, 65, 150)
CLUSTER_ARGS = ((3, 0.15), (20, 0.1))
GRAPH_CASES = ((3, 3), (7, 3), (64, 3), (65, 3), (257, 100))      # (points, min_samples)
DRAWS, PERTURB = 20, 1e-11


def load_reference_protodataset():
    """The reference's ProtoDataset class, its file executed unmodified next to stand-ins for what is not installed."""
    import pandas as pd
    from pandas.core.groupby import DataFrameGroupBy
    from oracle import reference_loader as rl
    if not rl.available():
        raise SystemExit("the reference tree is needed to make these fixtures")
    pandarallel_mod = types.ModuleType("pandarallel")

    class _Pandarallel:
        @staticmethod
        def initialize(**kw):
            DataFrameGroupBy.parallel_apply = DataFrameGroupBy.apply

    pandarallel_mod.pandarallel = _Pandarallel
    sys.modules["pandarallel"] = pandarallel_mod
    sys.modules["geopandas"] = types.ModuleType("geopandas")
    with open(os.path.join(rl.REFERENCE_ROOT, "config.py")) as f:
        cfg_src = f.read().split("# Training arguments")[0].replace("from transformers import TrainingArguments", "")
    config = types.ModuleType("config")
    exec(compile(cfg_src, "config.py", "exec"), config.__dict__)
    sys.modules["config"] = config
    prep = types.ModuleType("preprocessing")
    prep.__path__ = []
    sys.modules["preprocessing"] = prep
    geo = rl._load_file_as("preprocessing.geo_utils", os.path.join(rl.REFERENCE_ROOT, "preprocessing", "geo_utils.py"))
    prep.haversine_matrix_np = geo.haversine_matrix_np
    mod = rl._load_file_as("ref_prototype", os.path.join(rl.REFERENCE_ROOT, "dataset_creation", "prototype", "prototype.py"))
    return mod.ProtoDataset


def make_frame(seed: int):
    import pandas as pd
    rng = np.random.default_rng(seed)
    lng, lat, cell = [], [], []
    for c, n in enumerate(CELL_SIZES):
        centre = np.array([rng.uniform(-150, 150), rng.uniform(-60, 60)])
        pts = []
        clumps = max(1, min(4, n // 12))
        for k in range(clumps):                                   # clumps of different spread around the cell's centre
            m = n // clumps if k < clumps - 1 else n - (n // clumps) * (clumps - 1)
            pts.append(centre + rng.normal(0, 0.4, 2) + rng.normal(0, 0.002 * 4 ** k, (m, 2)))
        pts = np.concatenate(pts)
        if n >= 40:                                               # background noise and exact duplicates
            far = rng.choice(n, n // 10, replace=False)
            pts[far] = centre + rng.uniform(-1.5, 1.5, (len(far), 2))
            dup = rng.choice(n, n // 8, replace=False)
            pts[dup] = pts[rng.choice(n, len(dup))]
        lng += pts[:, 0].tolist(); lat += pts[:, 1].tolist(); cell += [c] * n
    extra = 9                                                     # rows of other splits, in cells that exist
    lng += rng.uniform(-150, 150, extra).tolist(); lat += rng.uniform(-60, 60, extra).tolist(); cell += rng.integers(0, len(CELL_SIZES), extra).tolist()
    selection = ['train'] * sum(CELL_SIZES) + ['val'] * extra
    perm = rng.permutation(len(lng))                              # rows of all cells interleaved
    df = pd.DataFrame({'selection': np.array(selection)[perm], 'lng': np.array(lng)[perm], 'lat': np.array(lat)[perm],
                       'geocell_idx': np.array(cell, dtype=np.int64)[perm]})
    return df


def run_reference(Ref, df, emb_dir, args, perturb_rng=None):
    """-> (csv text, labels of the training rows)"""
    orig = Ref._compute_distances
    if perturb_rng is not None:
        def perturbed(self, frame):
            d = orig(self, frame)
            _, ids = np.unique(frame[['lng', 'lat']].values, axis=0, return_inverse=True)
            ids = ids.reshape(-1)
            u = perturb_rng.uniform(-PERTURB, PERTURB, (ids.max() + 1, ids.max() + 1))
            u = np.triu(u) + np.triu(u, 1).T
            return np.where(d == 1e-5, d, d * (1 + u[ids][:, ids]))
        Ref._compute_distances = perturbed
    try:
        with tempfile.TemporaryDirectory() as work:
            os.makedirs(os.path.join(work, "tmp"))
            out = os.path.join(work, "protos.csv")
            cwd = os.getcwd()
            os.chdir(work)
            stdout = sys.stdout
            sys.stdout = io.StringIO()
            try:
                ds = Ref(df, emb_dir, out, cluster_args=args)
                ds.generate()
            finally:
                sys.stdout = stdout
                os.chdir(cwd)
            with open(out) as f:
                text = f.read()
            return text, np.asarray(ds.df['cluster'].values, dtype=np.int64)
    finally:
        Ref._compute_distances = orig


def make_proto_csv(path: str):
    import datasets
    Ref = load_reference_protodataset()
    datasets.disable_progress_bar()
    seed = 20260
    while True:
        df = make_frame(seed)
        n_train = int((df['selection'] == 'train').sum())
        with tempfile.TemporaryDirectory() as emb_dir:
            datasets.DatasetDict({'train': datasets.Dataset.from_dict({
                'embedding': np.zeros((n_train, 4), np.float32), 'labels_clf': df.loc[df['selection'] == 'train', 'geocell_idx'].values})}).save_to_disk(emb_dir)
            results, stable = [], True
            for args in CLUSTER_ARGS:
                text, labels = run_reference(Ref, df, emb_dir, args)
                prng = np.random.default_rng(seed + 1)
                for _ in range(DRAWS):
                    _, lab2 = run_reference(Ref, df, emb_dir, args, perturb_rng=prng)
                    if not np.array_equal(labels, lab2):
                        stable = False
                        break
                if not stable:
                    break
                results.append((text, labels))
        if stable:
            break
        print(f"seed {seed}: labels move under a {PERTURB:g} perturbation of the distances, trying the next")
        seed += 1
    for (text, labels), args in zip(results, CLUSTER_ARGS):
        print(f"seed {seed} cluster_args {args}: {len(text.splitlines()) - 1} prototypes, labels {np.unique(labels).tolist()}, "
              f"stable over {DRAWS} draws")
    np.savez_compressed(path, seed=seed, selection_is_train=(df['selection'] == 'train').values, lng=df['lng'].values, lat=df['lat'].values,
                        geocell_idx=df['geocell_idx'].values, cluster_args=np.array(CLUSTER_ARGS, dtype=np.float64),
                        csv_0=np.array(results[0][0]), csv_1=np.array(results[1][0]), labels_0=results[0][1], labels_1=results[1][1])


def make_graphs(path: str):
    from sklearn.cluster._optics import compute_optics_graph
    import _opticsref
    rng = np.random.default_rng(7)
    out = {'cases': np.array(GRAPH_CASES, dtype=np.int64)}
    for n, ms in GRAPH_CASES:
        # a coarse 1e-3 degree lattice with repeated sites: many exactly equal distances, many exact duplicates
        side = max(2, int(np.sqrt(n) * 0.6))
        pts = np.stack([11.0 + 1e-3 * rng.integers(0, side, n), 47.0 + 1e-3 * rng.integers(0, side, n)], axis=1)
        D = _opticsref.cell_distances(pts)
        ordering, core, reach, pred = compute_optics_graph(X=D, min_samples=ms, max_eps=np.inf, metric='precomputed', p=2, metric_params=None,
                                                           algorithm='auto', leaf_size=30, n_jobs=None)
        mine = _opticsref.graph(D, ms)
        for a, b in zip((ordering, core, reach, pred), mine):
            assert np.array_equal(a, b), f"the restatement differs from sklearn at n = {n}"
        out.update({f'pts_{n}': pts, f'dist_{n}': D, f'ordering_{n}': ordering.astype(np.int64), f'core_{n}': core, f'reach_{n}': reach,
                    f'pred_{n}': pred.astype(np.int64)})
        print(f"n = {n} min_samples = {ms}: {len(np.unique(D))} distinct distances among {n * n}")
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    golden = os.path.join(ROOT, "tests", "golden")
    make_graphs(os.path.join(golden, "optics_graph.npz"))
    make_proto_csv(os.path.join(golden, "proto_csv.npz"))
    for f in ("optics_graph.npz", "proto_csv.npz"):
        print(f, os.path.getsize(os.path.join(golden, f)), "bytes")
