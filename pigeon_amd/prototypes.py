"""The prototype cluster table: training metadata -> the CSV `build_bank` / `ProtoRefiner` read
(`geocell_idx, cluster, lng, lat, count, indices`), with the clustering on the GPU.

    python -m pigeon_amd.prototypes --metadata META.csv [--embeddings DIR] -o OUT.csv --min-samples 100 --xi 0.1

Mirrors reference dataset_creation/prototype/prototype.py: `ProtoDataset(df, embedding_path, output_file, cluster_args, sample)` and
`.generate()` (:38-95).  The reference clusters one geocell at a time in 64 worker processes -- OPTICS over a precomputed haversine
matrix (:121-149).  Here the distance matrices (pg_haversine_blocks) and the OPTICS graphs (pg_optics_graph: ordering, core
distances, reachability, predecessors -- sklearn's `compute_optics_graph`, bit for bit) of many cells are computed per launch in
libpigeon_hip.so (csrc/optics.hip); the xi extraction that turns a graph into labels is O(n) and runs on the host through
`sklearn.cluster.cluster_optics_xi`.  The reference's per-row cluster lookup (:151-174) is one vectorised assignment, and
`tmp/clusters_100.npy` is not written.  There is no host fallback for the graphs: without a GPU `generate()` raises.
"""
from __future__ import annotations

import argparse
import sys
from typing import Callable, Dict, Optional, Tuple

import numpy as np

DEFAULT_CLUSTER_ARGS = (100, 0.1)                                  # reference prototype.py:35
ZERO_AS = 1e-5                                                     # reference prototype.py:132

# (points (n,2) float64 [lng,lat], min_samples) -> (ordering, core, reach, pred) of one cell: what the tests inject in place of the GPU
GraphFn = Callable[[np.ndarray, int], Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]]


def _group_rows(cell_of_row: np.ndarray):
    """-> (the distinct cells ascending, the rows of each in row order)"""
    cells = np.asarray(cell_of_row)
    uniq, inv = np.unique(cells, return_inverse=True)
    order = np.argsort(inv.reshape(-1), kind='stable')            # keeps the row order inside a cell
    bounds = np.concatenate([[0], np.cumsum(np.bincount(inv.reshape(-1), minlength=len(uniq)))])
    return uniq, [order[bounds[i]:bounds[i + 1]] for i in range(len(uniq))]


def optics_graph_cells(lnglat: np.ndarray, cell_of_row: np.ndarray, min_samples: int, memory_bytes: int = 4 << 30) -> Dict:
    """The OPTICS graph of every cell that has at least `min_samples` rows, on the GPU.

    lnglat (N,2) [lng,lat] degrees, cell_of_row (N,) any sortable labels.  Cells are packed into batches whose distance matrices fit
    `memory_bytes` (a cell larger than that goes alone); a batch is one pg_haversine_blocks and one pg_optics_graph call.  Returns
    {cell: {'rows': its row numbers in row order, 'ordering', 'core', 'reach', 'pred'}} with numpy arrays local to the cell -- the
    arrays sklearn's compute_optics_graph(metric='precomputed', max_eps=inf) returns for that cell's matrix.  Cells with fewer rows
    are left out; a cell of more than 32768 rows is refused by name."""
    import torch
    from . import _lib, hip_ops
    _lib.require_gpu()
    min_samples = int(min_samples)
    lnglat = np.ascontiguousarray(np.asarray(lnglat, dtype=np.float64))
    if lnglat.ndim != 2 or lnglat.shape[1] != 2 or lnglat.shape[0] != len(cell_of_row):
        raise ValueError('optics_graph_cells: lnglat (N,2) and cell_of_row (N,) expected')
    uniq, rows = _group_rows(cell_of_row)
    todo = [i for i in range(len(uniq)) if len(rows[i]) >= min_samples]
    batches, cur, cur_bytes = [], [], 0
    for i in todo:
        b = 8 * len(rows[i]) ** 2
        if cur and cur_bytes + b > memory_bytes:
            batches.append(cur)
            cur, cur_bytes = [], 0
        cur.append(i)
        cur_bytes += b
    if cur:
        batches.append(cur)
    out = {}
    for batch in batches:
        sizes = np.array([len(rows[i]) for i in batch], dtype=np.int64)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        pts = torch.from_numpy(lnglat[np.concatenate([rows[i] for i in batch])]).to('cuda')
        cell_off = torch.from_numpy(off)
        dist, mat_off = hip_ops.haversine_blocks(pts, cell_off, ZERO_AS)
        g = {k: v.cpu().numpy() for k, v in hip_ops.optics_graph(dist, cell_off, mat_off, min_samples).items()}
        del dist
        for j, i in enumerate(batch):
            s, e = int(off[j]), int(off[j + 1])
            out[uniq[i].item() if hasattr(uniq[i], 'item') else uniq[i]] = {
                'rows': rows[i], 'ordering': g['ordering'][s:e], 'core': g['core'][s:e], 'reach': g['reach'][s:e], 'pred': g['pred'][s:e]}
    return out


def _xi():
    try:
        from sklearn.cluster import cluster_optics_xi
    except ImportError as e:
        raise ImportError('pigeon_amd.prototypes needs scikit-learn (sklearn.cluster.cluster_optics_xi) for the xi cluster extraction; '
                          'it is not installed') from e
    return cluster_optics_xi


def cluster_cells(lnglat: np.ndarray, cell_of_row: np.ndarray, cluster_args: Tuple[int, float] = DEFAULT_CLUSTER_ARGS,
                  graph_fn: Optional[GraphFn] = None, memory_bytes: int = 4 << 30) -> np.ndarray:
    """A cluster label per row: what `OPTICS(min_samples, xi, metric='precomputed').fit_predict` gives on each cell's haversine matrix
    (reference :135-149); a cell with fewer than `min_samples` rows gets 0 on every row (:144-145); -1 is noise.
    `graph_fn` replaces the GPU graphs (tests)."""
    min_samples, xi = int(cluster_args[0]), float(cluster_args[1])
    if min_samples != cluster_args[0] or min_samples < 2:
        raise ValueError(f'cluster_cells: min_samples must be an integer of at least 2 (got {cluster_args[0]!r}); fractional values are not supported')
    lnglat = np.asarray(lnglat, dtype=np.float64)
    labels = np.zeros(len(cell_of_row), dtype=np.int64)
    if graph_fn is None:
        graphs = optics_graph_cells(lnglat, cell_of_row, min_samples, memory_bytes)
    else:
        uniq, rows = _group_rows(cell_of_row)
        graphs = {}
        for i in range(len(uniq)):
            if len(rows[i]) >= min_samples:
                o, c, r, p = graph_fn(np.ascontiguousarray(lnglat[rows[i]]), min_samples)
                graphs[i] = {'rows': rows[i], 'ordering': o, 'core': c, 'reach': r, 'pred': p}
    if graphs:
        cluster_optics_xi = _xi()
    for g in graphs.values():
        lab, _ = cluster_optics_xi(reachability=g['reach'], predecessor=g['pred'], ordering=g['ordering'], min_samples=min_samples, xi=xi)
        labels[g['rows']] = lab
    return labels


class ProtoDataset:
    def __init__(self, df, embedding_path: Optional[str], output_file: str, cluster_args: Tuple[int, float] = DEFAULT_CLUSTER_ARGS,
                 sample: Optional[int] = None, seed: Optional[int] = None, graph_fn: Optional[GraphFn] = None):
        """A prototype dataset for in-cell refinement (reference prototype.py:38-67).

        df: the metadata (`selection`, `lng`, `lat`, optionally `geocell_idx`); embedding_path: the Huggingface dataset with the
        embeddings, read only for its `labels_clf` when `geocell_idx` is absent (None is allowed otherwise); output_file: the CSV;
        cluster_args: (min_samples, xi); sample / seed: cluster a seeded sample of the rows."""
        self.df = df[df['selection'] == 'train'].copy().reset_index(drop=True)
        self.output = output_file
        self.cluster_args = cluster_args
        self._sample = sample
        self._seed = seed
        self._graph_fn = graph_fn
        if 'geocell_idx' not in self.df.columns:                  # :63-67
            if embedding_path is None:
                raise ValueError('ProtoDataset: the metadata has no geocell_idx column, so embedding_path (labels_clf) is needed')
            try:
                import datasets
            except ImportError as e:
                raise ImportError('ProtoDataset needs the `datasets` package to read labels_clf from the embeddings') from e
            train = datasets.DatasetDict.load_from_disk(embedding_path)['train'].with_format('numpy')
            cell_idx = np.asarray(train['labels_clf'][:])
            if len(cell_idx) != len(self.df):
                raise ValueError(f'ProtoDataset: {len(cell_idx)} embeddings for {len(self.df)} training rows')
            self.df['geocell_idx'] = cell_idx

    def generate(self):
        """Clusters every geocell and writes the prototypes (:69-95)."""
        if self._sample:
            self.df = self.df.sample(self._sample, random_state=self._seed).copy()
        self.df['cluster'] = cluster_cells(self.df[['lng', 'lat']].values, self.df['geocell_idx'].values, self.cluster_args,
                                           graph_fn=self._graph_fn)
        centroids = self.df.groupby(['geocell_idx', 'cluster']).agg(lng=('lng', 'mean'), lat=('lat', 'mean'), count=('lng', len),
                                                                    indices=('lng', lambda s: s.index.values.tolist()))
        centroids = centroids.reset_index(drop=False)
        centroids = centroids.loc[centroids['cluster'] != -1].copy()
        centroids.to_csv(self.output, index=False)
        return centroids


def _arg_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog='python -m pigeon_amd.prototypes', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--metadata', required=True, metavar='META.csv', help='training metadata: selection, lng, lat and optionally geocell_idx')
    ap.add_argument('--embeddings', default=None, metavar='DIR', help='Huggingface dataset of the embeddings (labels_clf), needed when the metadata has no geocell_idx')
    ap.add_argument('-o', '--output', required=True, metavar='OUT.csv')
    ap.add_argument('--min-samples', type=int, default=DEFAULT_CLUSTER_ARGS[0])
    ap.add_argument('--xi', type=float, default=DEFAULT_CLUSTER_ARGS[1])
    ap.add_argument('--sample', type=int, default=None, help='cluster a sample of this many training rows')
    ap.add_argument('--seed', type=int, default=None, help='seed of --sample')
    return ap


def main(argv=None) -> int:
    ap = _arg_parser()
    args = ap.parse_args(argv)
    if args.min_samples < 2:
        ap.error('--min-samples must be at least 2')
    import pandas as pd
    ds = ProtoDataset(pd.read_csv(args.metadata), args.embeddings, args.output, (args.min_samples, args.xi), args.sample, args.seed)
    table = ds.generate()
    print(f'{len(table)} prototypes in {table["geocell_idx"].nunique()} geocells written to {args.output}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
