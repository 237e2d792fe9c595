"""Paired bootstrap intervals of evaluation statistics (pg_bootstrap_means / pg_bootstrap_quantiles, csrc/bootstrap.hip).

Every metric `evaluate` prints is the mean of a per-item column or the median of one.  `bootstrap` resamples the items with
replacement R times -- the same items for every column of a replicate, so that differences of statistics are paired -- recomputes
every statistic on each resample on the GPU and reports percentile intervals.  `metric_columns` builds the per-item columns behind
the metrics of `compute_geoguessr_metrics`, `best_guess_metrics` and `neighbour_metrics` under the metrics' own keys.

    python -m pigeon_amd.bootstrap --columns FILE.npz --mean km --median km --diff km_best km -R 10000

The resampling is a pure function of (seed, replicate): see include/pigeon_hip.h for the contract.
"""
from __future__ import annotations

import argparse
from typing import Dict, Mapping, Optional, Sequence, Tuple

import numpy as np

KINDS = {'mean': 1, 'median': 1, 'quantile': 1, 'mean_diff': 2, 'median_diff': 2}     # kind -> columns it names
MAX_QUANTILES = 16
MAX_ITEMS = 1 << 24                                  # pg_bootstrap_plan's out[6]
DIFF_KEY = '{} - {}'


def _normalise(columns, stats, R, seed, level) -> Tuple[Dict[str, np.ndarray], Dict[str, tuple], int]:
    """Every argument check of `bootstrap`, before anything touches the GPU.  Returns (columns as 1-D arrays, key -> stat, N)."""
    if not isinstance(columns, Mapping) or not columns:
        raise ValueError('bootstrap: columns must be a non-empty mapping of names to per-item arrays')
    cols = {}
    for name, v in columns.items():
        a = np.asarray(v)
        if a.ndim != 1:
            raise ValueError(f'bootstrap: column {name!r} must be one-dimensional, got shape {a.shape}')
        if a.dtype == object or not (np.issubdtype(a.dtype, np.number) or a.dtype == bool):
            raise ValueError(f'bootstrap: column {name!r} is not numeric ({a.dtype})')
        cols[name] = a
    lengths = {len(a) for a in cols.values()}
    if len(lengths) != 1:
        raise ValueError(f'bootstrap: columns must have one length, got {({k: len(a) for k, a in cols.items()})}')
    N = lengths.pop()
    if not 1 <= N <= MAX_ITEMS:
        raise ValueError(f'bootstrap: the columns hold {N} items; 1 .. {MAX_ITEMS} are supported')
    if isinstance(R, bool) or int(R) != R or int(R) < 1:
        raise ValueError(f'bootstrap: R must be a positive integer, got {R!r}')
    if isinstance(seed, bool) or int(seed) != seed or not 0 <= int(seed) < 2 ** 64:
        raise ValueError(f'bootstrap: seed must be an integer in 0 .. 2^64 - 1, got {seed!r}')
    if not 0.0 < float(level) < 1.0:
        raise ValueError(f'bootstrap: level must lie strictly between 0 and 1, got {level!r}')
    if not isinstance(stats, Mapping):
        stats = {(DIFF_KEY.format(s[1], s[2]) + f' ({s[0]})' if len(s) == 3 and s[0].endswith('_diff') else ' '.join(str(p) for p in s)): s
                 for s in stats}
    if not stats:
        raise ValueError('bootstrap: stats names no statistic')
    out = {}
    for key, s in stats.items():
        s = tuple(s)
        if not s or s[0] not in KINDS:
            raise ValueError(f'bootstrap: statistic {key!r}: unknown kind {s[0] if s else None!r} (one of {sorted(KINDS)})')
        want = 1 + KINDS[s[0]] + (s[0] == 'quantile')
        if len(s) != want:
            raise ValueError(f'bootstrap: statistic {key!r}: {s[0]!r} takes {want - 1} arguments, got {len(s) - 1}')
        for name in s[1:1 + KINDS[s[0]]]:
            if name not in cols:
                raise ValueError(f'bootstrap: statistic {key!r} names the column {name!r}, which is not among {sorted(cols)}')
        if s[0] == 'quantile':
            if not 0.0 <= float(s[2]) <= 1.0:                       # NaN fails both comparisons
                raise ValueError(f'bootstrap: statistic {key!r}: the quantile {s[2]!r} is not in [0, 1]')
            s = (s[0], s[1], float(s[2]))
        if s[0] in ('median', 'quantile', 'median_diff'):
            for name in s[1:1 + KINDS[s[0]]]:
                if np.issubdtype(cols[name].dtype, np.floating) and np.isnan(cols[name]).any():
                    raise ValueError(f'bootstrap: column {name!r} holds a NaN; statistic {key!r} takes a quantile of it')
        out[key] = s
    qs = sorted({0.5 if s[0] != 'quantile' else s[2] for s in out.values() if s[0] in ('median', 'quantile', 'median_diff')})
    if len(qs) > MAX_QUANTILES:
        raise ValueError(f'bootstrap: {len(qs)} distinct quantiles; one call takes {MAX_QUANTILES}')
    return cols, out, N


def _estimate(cols, s) -> float:
    """The statistic on the data itself, computed as pigeon_amd.evaluate computes it."""
    if s[0] == 'mean':
        return float(np.mean(cols[s[1]]))
    if s[0] == 'median':
        return float(np.median(cols[s[1]]))
    if s[0] == 'quantile':
        return float(np.quantile(cols[s[1]], s[2]))
    one = 'mean' if s[0] == 'mean_diff' else 'median'
    return _estimate(cols, (one, s[1])) - _estimate(cols, (one, s[2]))


def replicates(columns, stats, R: int = 2000, seed: int = 0, device='cuda') -> Dict[str, np.ndarray]:
    """key -> the statistic on each of the R resamples, (R,) float64: one pg_bootstrap_means call over the columns that means are
    taken of, one stable device sort and one pg_bootstrap_quantiles call over the columns that quantiles are taken of."""
    cols, stats, N = _normalise(columns, stats, R, seed, 0.5)
    import torch
    from . import hip_ops
    mean_names = list(dict.fromkeys(n for s in stats.values() if s[0] in ('mean', 'mean_diff') for n in s[1:1 + KINDS[s[0]]]))
    q_names = list(dict.fromkeys(n for s in stats.values() if s[0] in ('median', 'quantile', 'median_diff') for n in s[1:1 + KINDS[s[0]]]))
    qs = sorted({0.5 if s[0] != 'quantile' else s[2] for s in stats.values() if s[0] in ('median', 'quantile', 'median_diff')})
    dev = hip_ops.indexed_device(device)

    def matrix(names):
        return torch.from_numpy(np.stack([cols[n].astype(np.float64) for n in names])).to(dev).contiguous()

    means = quants = None
    if mean_names:
        means = hip_ops.bootstrap_means(matrix(mean_names), int(R), int(seed))
    if q_names:
        # + 0.0: a -0.0 is a 0.0 to a quantile, and to the sort one key, so that ties go by item index as the contract says
        srt, order = torch.sort(matrix(q_names) + 0.0, dim=1, stable=True)
        rank = torch.empty(order.shape, dtype=torch.int32, device=dev)
        rank.scatter_(1, order, torch.arange(N, dtype=torch.int32, device=dev).expand_as(order))
        quants = hip_ops.bootstrap_quantiles(rank, srt.contiguous(), int(R), qs, int(seed))
    means = means.cpu().numpy() if means is not None else None
    quants = quants.cpu().numpy() if quants is not None else None

    def one(s):
        if s[0] == 'mean':
            return means[:, mean_names.index(s[1])]
        if s[0] == 'mean_diff':
            return means[:, mean_names.index(s[1])] - means[:, mean_names.index(s[2])]
        if s[0] == 'median_diff':
            return quants[:, q_names.index(s[1]), qs.index(0.5)] - quants[:, q_names.index(s[2]), qs.index(0.5)]
        return quants[:, q_names.index(s[1]), qs.index(0.5 if s[0] == 'median' else s[2])]

    return {key: np.ascontiguousarray(one(s)) for key, s in stats.items()}


def summarise(cols, stats, reps: Dict[str, np.ndarray], level: float) -> Dict[str, dict]:
    """Per statistic: estimate (on the data itself), se (the replicates' standard deviation, ddof = 1; 0 for R = 1 and for equal replicates), lo and hi (the
    percentile interval: numpy's linear quantiles (1 - level) / 2 and (1 + level) / 2 of the replicates) and, for differences,
    share_le_zero: the share of replicates in which the difference is at most 0."""
    out = {}
    for key, s in stats.items():
        v = reps[key]
        lo, hi = np.quantile(v, [(1.0 - level) / 2.0, (1.0 + level) / 2.0]) if not np.isnan(v).any() else (np.nan, np.nan)
        # equal replicates have no spread: numpy's std of R equal values is a few ulps of them, not 0 (its mean is rounded)
        se = float(np.std(v, ddof=1)) if len(v) > 1 and v.min() != v.max() else 0.0
        row = dict(estimate=_estimate(cols, s), se=se, lo=float(lo), hi=float(hi))
        if s[0].endswith('_diff'):
            row['share_le_zero'] = float(np.mean(v <= 0))
        out[key] = row
    return out


def bootstrap(columns, stats, R: int = 2000, seed: int = 0, level: float = 0.95, device='cuda') -> Dict[str, dict]:
    """`columns`: names -> per-item arrays of one length N.  `stats`: key -> statistic (or a list of statistics), each one of
    ('mean', col), ('median', col), ('quantile', col, q), ('mean_diff', a, b), ('median_diff', a, b).  A column with a NaN is refused by
    name for quantile statistics.  Returns key -> dict(estimate, se, lo, hi[, share_le_zero]) (`summarise`)."""
    cols, norm, _ = _normalise(columns, stats, R, seed, level)
    return summarise(cols, norm, replicates(cols, norm, R, seed, device), float(level))


# ------------------------------------------------------------------------------------------------------- the metrics' columns
def metric_columns(results, scaler=None, countries=None, best_LLH=None, best_taken=None, nn_lnglat=None):
    """The per-item columns behind every metric of `pigeon_amd.evaluate`.  `results`: the 11-tuple `evaluate_model` hands to
    `compute_geoguessr_metrics` (`scaler`, `countries` as there).  `best_LLH` (N,2) / `best_taken` (N,): the guesses by expectation;
    `nn_lnglat` (N,K,2): the nearest training rows.  Returns (columns, stats): stats maps every metric's existing key to the statistic
    that reproduces it -- ('mean', column) or ('median', column) -- plus the paired differences '<key>_best - <key>' and
    '<key>_nn - <key>' of the km error's mean and median and of the GeoGuessr score."""
    from .config import DECAY_CONSTANT
    from .evaluate import _class_labels, load_scaler, recover_regression_values
    from .geo_utils import haversine_np
    predictions, cell_preds, preds_mt, preds_climate, preds_month, top5_geocells, labels, cell_labels, labels_mt, labels_climate, \
        labels_month = results
    cols, stats = {}, {}

    def hit(key, name, values):
        cols[name] = np.asarray(values).astype(np.float64)
        stats[key] = ('mean', name)

    def guess(suffix, km):
        cols['km' + suffix] = km
        cols['score' + suffix] = np.round(5000 * np.exp(-km / DECAY_CONSTANT))
        stats['Mean_km_error' + suffix] = ('mean', 'km' + suffix)
        stats['Median_km_error' + suffix] = ('median', 'km' + suffix)
        stats['Geoguessr_score' + suffix] = ('mean', 'score' + suffix)
        if suffix:
            stats[DIFF_KEY.format('Mean_km_error' + suffix, 'Mean_km_error')] = ('mean_diff', 'km' + suffix, 'km')
            stats[DIFF_KEY.format('Median_km_error' + suffix, 'Median_km_error')] = ('median_diff', 'km' + suffix, 'km')
            stats[DIFF_KEY.format('Geoguessr_score' + suffix, 'Geoguessr_score')] = ('mean_diff', 'score' + suffix, 'score')

    cell_labels = np.asarray(cell_labels)
    if cell_labels.ndim > 1:
        cell_labels = np.argmax(cell_labels, axis=-1)
    labels = np.asarray(labels)
    distances = haversine_np(np.asarray(predictions), labels)
    guess('', distances)
    for km in (1, 5, 10, 25, 50, 100, 200, 750, 1000, 2500):
        hit(f'Under_{km}_km', f'under_{km}_km', distances < km)
    if countries is not None:
        from .regions import country_hits
        hit('Country_accuracy', 'country_hit', country_hits(np.asarray(predictions), labels, countries))
    hit('Geocell_accuracy', 'geocell_hit', cell_labels == np.asarray(cell_preds))
    hit('Geocell_top5_accuracy', 'geocell_top5_hit', [label in top5 for label, top5 in zip(cell_labels, top5_geocells)])
    if labels_mt is not None:
        yfcc = labels_month is None
        if scaler is None:
            scaler = load_scaler(yfcc)
        if scaler is not None:
            p_mt = recover_regression_values(np.asarray(preds_mt), yfcc, scaler)
            l_mt = recover_regression_values(np.asarray(labels_mt), False, scaler)
            for i, name in enumerate(('elevation', 'population', 'temperature', 'temp_diff', 'precipitation', 'prec_diff')):
                cols[f'{name}_abs_error'] = np.abs(l_mt[:, i] - p_mt[:, i])
                stats[f'Mean_{name}_error'] = ('mean', f'{name}_abs_error')
        hit('Climate_accuracy', 'climate_hit', _class_labels(labels_climate) == np.argmax(np.asarray(preds_climate), axis=-1))
        if not yfcc:
            hit('Month_accuracy', 'month_hit', _class_labels(labels_month) == np.argmax(np.asarray(preds_month), axis=-1))
    if best_LLH is not None:
        guess('_best', haversine_np(np.asarray(best_LLH), labels))
        if best_taken is not None:
            hit('Best_guess_changed', 'best_taken', np.asarray(best_taken, dtype=bool))
    if nn_lnglat is not None:
        d_nn = haversine_np(np.asarray(nn_lnglat)[:, 0, :].astype(np.float64), labels)
        guess('_nn', d_nn)
        hit('NN_beats_model', 'nn_beats_model', d_nn < distances)
    return cols, stats


def format_value(row: dict) -> str:
    return f"{row['estimate']:.6g} [{row['lo']:.6g}, {row['hi']:.6g}]"


def report(table: Dict[str, dict], level: float) -> str:
    """The metrics as `value [lo, hi]`, the paired differences below them."""
    plain = [k for k, row in table.items() if 'share_le_zero' not in row]
    diffs = [k for k in table if k not in plain]
    lines = [f'bootstrap: {100 * level:g} % percentile intervals']
    lines += [f'  {k}: {format_value(table[k])}' for k in plain]
    if diffs:
        lines.append('  paired differences (the same resample on both sides):')
        lines += [f"  {k}: {format_value(table[k])}, at most 0 in {table[k]['share_le_zero']:.1%} of the replicates" for k in diffs]
    return '\n'.join(lines)


def main(argv: Optional[Sequence[str]] = None) -> Dict[str, dict]:
    ap = argparse.ArgumentParser(prog='python -m pigeon_amd.bootstrap',
                                 description='Paired bootstrap intervals of statistics of per-item columns (an .npz of 1-D arrays).')
    ap.add_argument('--columns', required=True, metavar='FILE.npz')
    ap.add_argument('--mean', action='append', default=[], metavar='COL')
    ap.add_argument('--median', action='append', default=[], metavar='COL')
    ap.add_argument('--quantile', action='append', nargs=2, default=[], metavar=('COL', 'Q'))
    ap.add_argument('--diff', action='append', nargs=2, default=[], metavar=('A', 'B'), help='mean and median of A minus those of B, paired')
    ap.add_argument('-R', '--replicates', type=int, default=2000)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--level', type=float, default=0.95)
    args = ap.parse_args(argv)
    try:
        with np.load(args.columns) as f:
            columns = {k: f[k] for k in f.files}
    except OSError as e:
        ap.error(f'--columns: {e}')
    stats = {}
    for c in args.mean:
        stats[f'mean {c}'] = ('mean', c)
    for c in args.median:
        stats[f'median {c}'] = ('median', c)
    for c, q in args.quantile:
        stats[f'quantile {q} {c}'] = ('quantile', c, float(q))
    for a, b in args.diff:
        stats[f'mean {a} - {b}'] = ('mean_diff', a, b)
        stats[f'median {a} - {b}'] = ('median_diff', a, b)
    if not stats:
        ap.error('name at least one statistic: --mean, --median, --quantile or --diff')
    try:
        table = bootstrap(columns, stats, R=args.replicates, seed=args.seed, level=args.level)
    except ValueError as e:
        ap.error(str(e))
    print(report(table, args.level))
    return table


if __name__ == '__main__':
    main()
