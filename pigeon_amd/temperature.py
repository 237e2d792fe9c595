"""One scalar that calibrates the geocell head's probabilities: fit a temperature T on held-out embeddings, keep it next to the head,
apply it wherever probabilities are integrated (`SuperGuessr.temperature`: `spread`, `best_guess`, `serve`'s `confidence`).

`pigeon_amd.train` trains against haversine-smoothed targets whose row sum is not 1, so softmax(logits) is mis-scaled by construction.
With beta = 1 / T the negative log-likelihood of the true cells under softmax(beta * logits) is convex in beta; pg_temper_stats
(csrc/temper.hip, contract: include/pigeon_hip.h) gives its total and its first and second derivative for up to 16 betas a pass.

  fit_beta(stats_fn)                    the minimiser, pure host code on a callable betas -> totals (K,3): testable without a GPU
  fit_temperature(model, emb, labels)   logits by hip_ops.head_forward in chunks, pg_temper_stats per chunk, one host synchronisation
                                        a pass; a last pass at [1, beta*] for the NLL, the accuracy, the ECE and the reliability table
  save / load                           the JSON sidecar, keyed by the head's fingerprint (hip_ops.fingerprint of cell_layer.weight
                                        and .bias): a temperature fitted on another head is refused
  python -m pigeon_amd.temperature --head head.model -l DATASET [--split val] [--yfcc] -o head.temperature.json
  python -m pigeon_amd.temperature --synthetic N --geocells C --seed S -o t.json

What stays uncalibrated on purpose: the argmax, the top-k indices, `topk_values`, the refiner's inputs and every certainty
computation read the head's own logits -- they are the reference's outputs, and a positive scale changes no order.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import time
from dataclasses import asdict, dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

BETA_LO, BETA_HI = 1.0 / 64, 64.0
MAX_BETAS = 16                                   # pg_temper_stats takes up to 16 betas a pass
MAX_PASSES = 16
BRACKET_REL = 2.0 ** -40                          # fit_beta stops at hi / lo - 1 <= 2^-40
ECE_BINS = 15
LOGITS_BUDGET = 4 << 30                           # bytes of (N,C) fp32 logits kept on the device between passes; above: recomputed


class FitError(RuntimeError):
    pass


def _log_grid(lo: float, hi: float, n: int, ends: bool) -> List[float]:
    """n log-spaced points: lo and hi themselves and n - 2 between them (ends), or n strictly between them"""
    a, b = math.log(lo), math.log(hi)
    if ends:
        pts = [lo] + [math.exp(a + (b - a) * i / (n - 1)) for i in range(1, n - 1)] + [hi]
    else:
        pts = [math.exp(a + (b - a) * i / (n + 1)) for i in range(1, n + 1)]
    return [p for p in pts if lo <= p <= hi]


def fit_beta(stats_fn: Callable[[Sequence[float]], np.ndarray], lo: float = BETA_LO, hi: float = BETA_HI) -> Tuple[float, int, bool]:
    """The beta in [lo, hi] that minimises the total NLL -> (beta, passes, clamped).  `stats_fn(betas)` (up to 16 betas) returns the
    totals (K,3): NLL, first and second derivative in beta; only the sign of the first derivative steers the search, which makes it
    as robust as a bisection: the total is convex, so its derivative changes sign once.  Pass 1 is a 16-point log-spaced grid over
    [lo, hi], ends included; every later pass puts 16 log-spaced points strictly inside the bracket where the derivative changes
    sign, which shrinks the log-bracket 17-fold.  It stops when hi / lo - 1 <= 2^-40 and returns the bracket's geometric mean: from
    [1/64, 64] that is 11 passes; more than 16 raises FitError.  A beta whose derivative is exactly 0 is the answer.  Where the
    derivative has one sign on [lo, hi] the result is the end it points at and clamped=True (a perfectly separable set: hi; a set
    whose every row is wrong: lo); a derivative of 0 everywhere (every logit equal) gives 1 clipped to [lo, hi], not clamped."""
    if not (0 < lo < hi < math.inf):
        raise ValueError(f'fit_beta: need 0 < lo < hi, got [{lo}, {hi}]')
    passes = 0
    ends = True
    while True:
        if passes == MAX_PASSES:
            raise FitError(f'fit_beta: the bracket [{lo!r}, {hi!r}] is still wider than 2^-40 after {MAX_PASSES} passes')
        betas = _log_grid(lo, hi, MAX_BETAS, ends)
        betas = sorted(set(betas))
        if not ends and (not betas or betas[0] <= lo or betas[-1] >= hi):      # fp64 has no 16 numbers left inside: as narrow as it gets
            return math.sqrt(lo * hi), passes, False
        totals = np.asarray(stats_fn(betas), dtype=np.float64).reshape(len(betas), 3)
        passes += 1
        d1 = totals[:, 1]
        if not np.isfinite(d1).all():
            raise FitError(f'fit_beta: a non-finite total first derivative at betas {betas}')
        if ends:
            if (d1 == 0).all():
                return min(max(1.0, lo), hi), passes, False
            if (d1 >= 0).all():                                 # rising from lo on: the minimum is at or below lo
                return lo, passes, bool(d1[0] > 0)
            if (d1 <= 0).all():
                return hi, passes, bool(d1[-1] < 0)
            pts, ds = betas, d1
        else:
            pts, ds = [lo] + betas + [hi], np.concatenate([[-1.0], d1, [1.0]])
        j = int(np.argmax(ds >= 0))                             # the first point that is not falling any more; ds[j - 1] < 0
        if ds[j] == 0:
            return pts[j], passes, False
        lo, hi = pts[j - 1], pts[j]
        ends = False
        if hi / lo - 1 <= BRACKET_REL:
            return math.sqrt(lo * hi), passes, False


# ------------------------------------------------------------------------------------------------ reliability
def reliability_table(conf, correct, bins: int = ECE_BINS) -> List[dict]:
    """`bins` equal-width confidence bins (j / bins, (j + 1) / bins] -> per bin {lo, hi, n, accuracy, confidence} (None where empty)"""
    conf, correct = np.asarray(conf, dtype=np.float64), np.asarray(correct, dtype=np.float64)
    idx = np.clip(np.ceil(conf * bins).astype(np.int64) - 1, 0, bins - 1)
    rows = []
    for j in range(bins):
        sel = idx == j
        n = int(sel.sum())
        rows.append({'lo': j / bins, 'hi': (j + 1) / bins, 'n': n, 'accuracy': float(correct[sel].mean()) if n else None,
                     'confidence': float(conf[sel].mean()) if n else None})
    return rows


def ece_of_table(table: List[dict]) -> float:
    """ECE = sum_j n_j / N |acc_j - conf_j| over the bins of `reliability_table`"""
    total = sum(r['n'] for r in table)
    if total == 0:
        return float('nan')
    return float(sum(r['n'] / total * abs(r['accuracy'] - r['confidence']) for r in table if r['n']))


def expected_calibration_error(conf, correct, bins: int = ECE_BINS) -> float:
    return ece_of_table(reliability_table(conf, correct, bins))


@dataclass
class TemperatureFit:
    temperature: float
    beta: float
    n: int                      # valid rows the fit used
    skipped: int                # rows pg_temper_stats calls invalid (label outside the head, non-finite logits)
    passes: int                 # passes of fit_beta (the reporting pass at [1, beta] not counted)
    clamped: bool
    nll_before: float           # mean per valid row at beta = 1
    nll_after: float
    ece_before: float
    ece_after: float
    reliability: dict = field(default_factory=dict)        # {'accuracy', 'before': [bins], 'after': [bins]}


# ------------------------------------------------------------------------------------------------ the fit on the device
def _head_logits(model, emb):
    import torch
    from . import hip_ops
    dev = model.cell_layer.weight.device
    head_in = model._head_rows(emb.to(dev, torch.float32).contiguous())
    return hip_ops.head_forward(head_in, model.cell_layer.weight.data, model.cell_layer.bias.data, model.lla_geocells.data, 1)['logits']


def fit_temperature(model, embedding, labels_clf, chunk: int = 8192, logits_budget: int = LOGITS_BUDGET,
                    lo: float = BETA_LO, hi: float = BETA_HI, pass_seconds: Optional[list] = None) -> TemperatureFit:
    """Fit the temperature of `model`'s geocell head on held-out embeddings (N,1024) or (N,P,1024) with their true cells (N,).
    Logits come from hip_ops.head_forward in chunks of `chunk` rows; they stay on the device while N * C * 4 bytes fit
    `logits_budget` (default 4 GiB) and are recomputed every pass otherwise -- the same kernel on the same rows: the same bits.
    Chunk totals are added on the device in chunk order; a pass ends in one host synchronisation.  `pass_seconds`, a list, receives
    the wall time of every pass (the reporting pass last)."""
    import torch
    from . import hip_ops
    dev = model.cell_layer.weight.device
    emb = torch.as_tensor(embedding)
    labels = torch.as_tensor(labels_clf).to(dev, torch.int64).contiguous()
    N = int(emb.shape[0])
    if labels.shape != (N,):
        raise ValueError(f'fit_temperature: labels_clf must have shape ({N},), got {tuple(labels.shape)}')
    if N == 0:
        raise ValueError('fit_temperature: no rows to fit on')
    chunk = max(1, int(chunk))
    spans = [(i, min(i + chunk, N)) for i in range(0, N, chunk)]
    keep = N * int(model.num_cells) * 4 <= int(logits_budget)
    kept = {}

    def logits_of(span):
        if span in kept:
            return kept[span]
        lg = _head_logits(model, emb[span[0]:span[1]])
        if keep:
            kept[span] = lg
        return lg

    def run_pass(betas, extras: bool = False):
        t0 = time.perf_counter()
        totals = torch.zeros((len(betas), 3), dtype=torch.float64, device=dev)
        counts = torch.zeros((2,), dtype=torch.int64, device=dev)
        confs, states = [], []
        for span in spans:
            r = hip_ops.temper_stats(logits_of(span), labels[span[0]:span[1]], betas, conf=extras, state=extras)
            totals += r['totals']
            counts += r['counts']
            if extras:
                confs.append(r['conf']); states.append(r['state'])
        packed = [totals.flatten(), counts.to(torch.float64)]          # counts below 2^53: exact
        if extras:
            packed += [torch.cat(confs).flatten(), torch.cat(states).to(torch.float64)]
        host = torch.cat(packed).cpu().numpy()                         # the pass's one host synchronisation
        if pass_seconds is not None:
            pass_seconds.append(time.perf_counter() - t0)
        K = len(betas)
        out = {'totals': host[:3 * K].reshape(K, 3), 'counts': host[3 * K:3 * K + 2].astype(np.int64)}
        if extras:
            out['conf'] = host[3 * K + 2:3 * K + 2 + N * K].reshape(N, K)
            out['state'] = host[3 * K + 2 + N * K:].astype(np.uint8)
        return out

    valid = {}

    def stats_fn(betas):
        r = run_pass(betas)
        valid['n'] = int(r['counts'][0])
        if valid['n'] == 0:
            raise FitError(f'fit_temperature: none of the {N} rows is valid (labels outside [0, {model.num_cells}) or non-finite logits)')
        return r['totals']

    beta, passes, clamped = fit_beta(stats_fn, lo, hi)
    r = run_pass([1.0, beta], extras=True)
    nv = int(r['counts'][0])
    ok = r['state'] != 2
    correct = (r['state'][ok] == 1).astype(np.float64)
    before, after = reliability_table(r['conf'][ok, 0], correct), reliability_table(r['conf'][ok, 1], correct)
    return TemperatureFit(temperature=1.0 / beta, beta=beta, n=nv, skipped=N - nv, passes=passes, clamped=clamped,
                          nll_before=float(r['totals'][0, 0] / nv), nll_after=float(r['totals'][1, 0] / nv),
                          ece_before=ece_of_table(before), ece_after=ece_of_table(after),
                          reliability={'accuracy': float(r['counts'][1] / nv), 'before': before, 'after': after})


# ------------------------------------------------------------------------------------------------ the sidecar
def head_fingerprint(model, fingerprint: Optional[Callable] = None) -> dict:
    """{'weight', 'bias'}: the 128-bit digests (hip_ops.fingerprint) of cell_layer.weight and .bias, as hex strings"""
    if fingerprint is None:
        from . import hip_ops
        fingerprint = hip_ops.fingerprint
    hexed = lambda t: '%016x%016x' % tuple(fingerprint(t.data.contiguous()))
    return {'weight': hexed(model.cell_layer.weight), 'bias': hexed(model.cell_layer.bias)}


def save(path: str, fit: TemperatureFit, model, fingerprint: Optional[Callable] = None) -> str:
    """Write the sidecar: the fit's fields plus the head's fingerprint, JSON."""
    obj = {'format': 'pigeon_amd.temperature/1', **asdict(fit), 'head_fingerprint': head_fingerprint(model, fingerprint)}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(obj, f, indent=1)
        f.write('\n')
    return path


def load(path: str, model, fingerprint: Optional[Callable] = None) -> TemperatureFit:
    """Read a sidecar for `model`'s head.  ValueError, naming both fingerprints, when it was fitted on another head -- as the
    encoder calibration file refuses weights it was not measured on."""
    with open(path) as f:
        obj = json.load(f)
    if obj.get('format') != 'pigeon_amd.temperature/1':
        raise ValueError(f'{path}: not a temperature sidecar (format {obj.get("format")!r})')
    theirs, ours = obj.get('head_fingerprint'), head_fingerprint(model, fingerprint)
    if theirs != ours:
        raise ValueError(f'{path}: fitted on a head with fingerprint {theirs}, this head has {ours}; fit it again '
                         f'(python -m pigeon_amd.temperature)')
    fit = TemperatureFit(**{k: obj[k] for k in TemperatureFit.__dataclass_fields__})
    _check_temperature(fit.temperature, path)
    return fit


def _check_temperature(t, where: str = 'temperature') -> float:
    t = float(t)
    if not (math.isfinite(t) and t > 0):
        raise ValueError(f'{where}: a temperature must be a finite positive number, got {t!r}')
    return t


def resolve(path_or_number, model, fingerprint: Optional[Callable] = None) -> float:
    """`--temperature FILE|NUMBER`: a number as it is, a path through `load` (keyed to `model`'s head)"""
    if isinstance(path_or_number, (int, float)):
        return _check_temperature(path_or_number)
    try:
        return _check_temperature(float(path_or_number))
    except (TypeError, ValueError):
        pass
    if isinstance(path_or_number, str) and not os.path.exists(path_or_number):
        raise ValueError(f'--temperature: {path_or_number!r} is neither a positive number nor an existing file')
    return load(path_or_number, model, fingerprint).temperature


# ------------------------------------------------------------------------------------------------ command line
def planted_head(model, seed: int, gain: float = 0.05, noise: float = 10.0) -> None:
    """A head for `train.synthetic_dataset(.., seed)` without training: cell c's weight row is gain * (the direction the synthetic
    samples of cell c scatter around + noise * a seeded Gaussian row), bias 0.  The noise makes the head err on a share of the
    samples; the gain decides how sure it claims to be -- what the fit has to undo."""
    import torch
    from . import hip_ops
    C = int(model.num_cells)
    protos = torch.randn((C, hip_ops.HIDDEN), generator=torch.Generator().manual_seed(seed + 4711))      # synthetic_dataset's first draw
    rows = torch.randn((C, hip_ops.HIDDEN), generator=torch.Generator().manual_seed(seed + 4712))
    with torch.no_grad():
        model.cell_layer.weight.copy_((gain * (protos + noise * rows)).to(model.cell_layer.weight.device))
        model.cell_layer.bias.zero_()


def format_fit(fit: TemperatureFit) -> str:
    lines = [f'temperature {fit.temperature:.6f} (beta {fit.beta:.6f}){" -- CLAMPED to the end of the search interval" if fit.clamped else ""}',
             f'rows {fit.n} (+ {fit.skipped} skipped), accuracy {fit.reliability.get("accuracy", float("nan")):.4f}, passes {fit.passes}',
             f'NLL {fit.nll_before:.6f} -> {fit.nll_after:.6f}    ECE {fit.ece_before:.6f} -> {fit.ece_after:.6f}',
             'confidence bin        before: n  accuracy  confidence        after: n  accuracy  confidence']
    cell = lambda r: f'{r["n"]:9d}  {"-":>8}  {"-":>10}' if not r['n'] else f'{r["n"]:9d}  {r["accuracy"]:8.4f}  {r["confidence"]:10.4f}'
    for b, a in zip(fit.reliability.get('before', []), fit.reliability.get('after', [])):
        lines.append(f'({b["lo"]:.3f}, {b["hi"]:.3f}]   {cell(b)}    {cell(a)}')
    return '\n'.join(lines)


def parser() -> argparse.ArgumentParser:
    argp = argparse.ArgumentParser(prog='python -m pigeon_amd.temperature',
                                   description='Fit the temperature of a geocell head on held-out embeddings (one GPU).')
    argp.add_argument('--head', default=None, help='saved head (state dict, as pigeon_amd.train writes it)')
    argp.add_argument('-l', '--load', default=None, help='dataset directory (datasets.DatasetDict; the split holds embedding, labels_clf)')
    argp.add_argument('--split', default='val')
    argp.add_argument('--yfcc', action='store_true', default=False)
    argp.add_argument('-o', '--out', required=True, help='where the sidecar is written, e.g. head.temperature.json')
    argp.add_argument('--chunk', type=int, default=8192)
    argp.add_argument('--synthetic', type=int, default=0, help='fit on N seeded synthetic samples and a planted head instead of a dataset')
    argp.add_argument('--geocells', type=int, default=10000, help='synthetic geocell count')
    argp.add_argument('--seed', type=int, default=0)
    argp.add_argument('--save-head', default=None, help='with --synthetic: also save the planted head and its geocell table '
                                                        '(<path> and <path>.geocells.csv), for `run.py evaluate`')
    return argp


def main(argv=None) -> TemperatureFit:
    argp = parser()
    args = argp.parse_args(argv)
    if args.synthetic < 0 or args.chunk < 1 or (args.synthetic and args.geocells < 1):
        argp.error('--synthetic, --chunk and --geocells take positive numbers')
    if args.synthetic and (args.head or args.load):
        argp.error('--synthetic takes neither --head nor -l')
    if not args.synthetic and not (args.head and args.load):
        argp.error('both --head HEAD and -l DATASET are needed (or --synthetic N)')
    if args.save_head and not args.synthetic:
        argp.error('--save-head goes with --synthetic')
    import torch
    from . import hip_ops
    from .super_guessr import SuperGuessr
    if args.synthetic:
        import tempfile
        from . import synthetic
        from .train import synthetic_dataset
        dataset, cen = synthetic_dataset(args.synthetic, args.geocells, seed=args.seed, panorama=not args.yfcc)
        geocell_path = (args.save_head + '.geocells.csv') if args.save_head else os.path.join(tempfile.mkdtemp(prefix='pigeon_temperature_'), 'geocells.csv')
        synthetic.write_geocell_csv(geocell_path, cen)
        model = SuperGuessr(base_model=None, panorama=not args.yfcc, yfcc=args.yfcc, geocell_path=geocell_path).to('cuda')
        planted_head(model, args.seed)
        if args.save_head:
            torch.save(model.state_dict(), args.save_head)
        emb, cells = (torch.cat([dataset[k].columns[c] for k in ('train', 'val')]) for c in ('embedding', 'labels_clf'))
    else:
        from datasets import DatasetDict
        dataset = DatasetDict.load_from_disk(args.load)
        dataset.set_format('torch')
        if args.split not in dataset:
            argp.error(f'--split {args.split}: the dataset has {list(dataset)}')
        model = SuperGuessr(base_model=None, panorama=not args.yfcc, yfcc=args.yfcc).to('cuda')
        model.load_state(args.head)
        emb, cells = dataset[args.split]['embedding'], dataset[args.split]['labels_clf']
    seconds: list = []
    t0 = time.perf_counter()
    fit = fit_temperature(model, emb, cells, chunk=args.chunk, pass_seconds=seconds)
    wall = time.perf_counter() - t0
    # the yardstick: one head_forward over the same rows
    torch.cuda.synchronize(); t1 = time.perf_counter()
    for i in range(0, len(emb), args.chunk):
        _head_logits(model, emb[i:i + args.chunk])
    torch.cuda.synchronize(); head_s = time.perf_counter() - t1
    print(format_fit(fit))
    print(f'wall time {wall:.3f} s; per pass ' + ' '.join(f'{s:.3f}' for s in seconds) + f' s; head_forward over the same rows {head_s:.3f} s')
    print(f'written to {save(args.out, fit, model)}')
    return fit


if __name__ == '__main__':
    main()
