"""Fit the refiner's three settings -- `topk`, `temperature`, `max_refinement` -- on held-out embeddings, keep them next to the head and
the prototype bank, apply them in `run.py evaluate --refiner` and `python -m pigeon_amd.serve --refiner`.

Finding the nearest prototype and the farthest member of every candidate is the expensive part of the refinement and depends on none
of the three settings: ONE `hip_ops.refine_forward` at topk = max(topks) leaves the records, and pg_refine_sweep (csrc/refine_sweep.hip,
contract: include/pigeon_hip.h) does the selection of every grid point from them, bit-identical to a `refine_forward` call with that
point's settings.  pg_refine_sweep_totals sums the metrics' per-row columns of every point in one fixed order.

  choose(totals, grid, objective, current)   pure host code on the totals: testable without a GPU
  fit_refiner(model, refiner, emb, labels)   candidates from the head, even rows fit, odd rows held out, two passes over a grid
  save / load                                the JSON sidecar, keyed by the fingerprints of the head and of the bank
  python -m pigeon_amd.refiner_fit --head H --protos P --dataset D -l DATA [--split val] [--objective score|km|under:R] [--bootstrap R] -o head.refiner.json
  python -m pigeon_amd.refiner_fit --synthetic N --geocells C --seed S -o r.json
"""
from __future__ import annotations

import argparse
import json
import math
import os
from dataclasses import asdict, dataclass, field
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

UNDER_KM = (1, 5, 10, 25, 50, 100, 200, 750, 1000, 2500)
COLUMNS = ('km', 'score') + tuple(f'under_{r}_km' for r in UNDER_KM)                     # the values table's V = 12 columns
METRICS = ('Mean_km_error', 'Geoguessr_score') + tuple(f'Under_{r}_km' for r in UNDER_KM) + ('Changed', 'Vetoed')
MAX_TOPK = 64
PASS1_TEMPS, PASS1_T_LO, PASS1_T_HI = 24, 0.05, 20.0
PASS2_TEMPS, PASS2_TOPK_SPAN = 16, 3
MAX_KMS = (25.0, 50.0, 100.0, 200.0, 500.0, 1000.0, 2500.0, 5000.0, 1e5)
FORMAT = 'pigeon_amd.refiner_fit/1'


def f32(t) -> float:
    """the float32 the kernel sees, as a Python float"""
    return float(np.float32(t))


# ------------------------------------------------------------------------------------------------ settings
def check_settings(topk, temperature, max_refinement, num_candidates: Optional[int] = None, where: str = 'refiner settings'):
    """(topk, temperature, max_refinement) validated: topk an integer in 1 .. 64 (and at most `num_candidates` when given), the
    temperature finite and positive, max_refinement a number >= 0 that is not NaN (+inf: never veto).  ValueError otherwise."""
    if isinstance(topk, bool) or not isinstance(topk, (int, np.integer)) and not (isinstance(topk, float) and topk == int(topk)):
        raise ValueError(f'{where}: topk must be an integer, got {topk!r}')
    topk = int(topk)
    if not 1 <= topk <= MAX_TOPK:
        raise ValueError(f'{where}: topk must be in 1 .. {MAX_TOPK}, got {topk}')
    if num_candidates is not None and topk > int(num_candidates):
        raise ValueError(f'{where}: topk = {topk} exceeds the {int(num_candidates)} candidates the head supplies (num_candidates)')
    try:
        temperature, max_refinement = float(temperature), float(max_refinement)
    except (TypeError, ValueError):
        raise ValueError(f'{where}: temperature and max_refinement must be numbers, got {temperature!r} and {max_refinement!r}') from None
    if not (math.isfinite(temperature) and temperature > 0):
        raise ValueError(f'{where}: the temperature must be a finite positive number, got {temperature!r}')
    if not max_refinement >= 0:
        raise ValueError(f'{where}: max_refinement must be a number >= 0 (inf: never veto), got {max_refinement!r}')
    return topk, temperature, max_refinement


def parse_settings(text: str) -> Tuple[int, float, float]:
    """`TOPK,TEMPERATURE,MAX_KM`, e.g. `5,1.6,1000` (MAX_KM may be `inf`) -> the validated triple"""
    parts = [p.strip() for p in str(text).split(',')]
    if len(parts) != 3:
        raise ValueError(f'--refiner: expected TOPK,TEMPERATURE,MAX_KM, got {text!r}')
    try:
        topk = int(parts[0])
        temperature, max_km = float(parts[1]), float(parts[2])
    except ValueError:
        raise ValueError(f'--refiner: expected TOPK,TEMPERATURE,MAX_KM as an integer and two numbers, got {text!r}') from None
    return check_settings(topk, temperature, max_km, where='--refiner')


def apply_settings(refiner, topk, temperature, max_refinement, num_candidates: Optional[int] = None):
    """`ProtoRefiner.apply_settings`: validate, then set the three.  The temperature Parameter is written through `.data`, which is what
    `_temperature_value` reads on every forward."""
    topk, temperature, max_refinement = check_settings(topk, temperature, max_refinement, num_candidates, 'ProtoRefiner.apply_settings')
    refiner.topk = topk
    refiner.max_refinement = int(max_refinement) if math.isfinite(max_refinement) and max_refinement == int(max_refinement) else max_refinement
    refiner.temperature.data.fill_(temperature)
    return refiner


def current_settings(refiner) -> Tuple[int, float, float]:
    return int(refiner.topk), float(refiner.temperature.data), float(refiner.max_refinement)


# ------------------------------------------------------------------------------------------------ the grids
def _log_space(lo: float, hi: float, n: int, inside: bool) -> List[float]:
    a, b = math.log(lo), math.log(hi)
    if inside:
        return [math.exp(a + (b - a) * i / (n + 1)) for i in range(1, n + 1)]
    return [lo] + [math.exp(a + (b - a) * i / (n - 1)) for i in range(1, n - 1)] + [hi]


def _temps(values) -> List[float]:
    """sorted, distinct, as the float32 values the kernel sees"""
    return sorted({f32(v) for v in values})


def pass1_grid(kmax: int, current) -> Tuple[List[int], List[float], List[float]]:
    """Every topk in 1 .. kmax, 24 log-spaced T in [0.05, 20], the nine max_km -- and the CURRENT settings' three values, so the current
    point is in the grid and the fit can never be worse than it on the fit rows.  Each axis sorted ascending."""
    topk, temperature, max_km = current
    if not 1 <= int(topk) <= int(kmax):
        raise ValueError(f'pass1_grid: the current topk = {topk} is outside 1 .. {kmax}')
    topks = list(range(1, int(kmax) + 1))
    temps = _temps(_log_space(PASS1_T_LO, PASS1_T_HI, PASS1_TEMPS, False) + [temperature])
    max_kms = sorted(set(MAX_KMS) | {float(max_km)})
    return topks, temps, max_kms


def pass2_temps(best_t: float, temps: Sequence[float], n: int = PASS2_TEMPS) -> Tuple[List[float], Tuple[float, float]]:
    """n log-spaced T strictly between the neighbours of `best_t` in the sorted `temps` (at an end of `temps`: best_t itself is that
    end of the bracket) -> (temps, (lo, hi)).  Values that float32 cannot tell from an end of the bracket are dropped."""
    ts = sorted(temps)
    i = ts.index(best_t)
    lo, hi = ts[max(i - 1, 0)], ts[min(i + 1, len(ts) - 1)]
    if not lo < hi:
        return [], (lo, hi)
    return [t for t in _temps(_log_space(lo, hi, n, True)) if lo < t < hi], (lo, hi)


def pass2_grid(best, grid1, kmax: int) -> Tuple[List[int], List[float], List[float]]:
    """Around pass 1's best point: topk within +-3, 16 T strictly inside the bracket of its neighbours plus the best T itself (so pass
    1's best point is a point of pass 2), every max_km of pass 1."""
    topk, temperature, _ = best
    inside, _ = pass2_temps(temperature, grid1[1])
    topks = [k for k in range(int(topk) - PASS2_TOPK_SPAN, int(topk) + PASS2_TOPK_SPAN + 1) if 1 <= k <= int(kmax)]
    return topks, _temps(inside + [temperature]), list(grid1[2])


# ------------------------------------------------------------------------------------------------ the choice
def objective_column(objective: str) -> Tuple[str, bool]:
    """objective -> (metric key, maximise)"""
    if objective == 'score':
        return 'Geoguessr_score', True
    if objective == 'km':
        return 'Mean_km_error', False
    if isinstance(objective, str) and objective.startswith('under:'):
        try:
            r = float(objective[len('under:'):])
        except ValueError:
            r = None
        if r is not None and r == int(r) and int(r) in UNDER_KM:
            return f'Under_{int(r)}_km', True
        raise ValueError(f'objective {objective!r}: under:R takes R from {UNDER_KM}')
    raise ValueError(f'objective {objective!r}: one of score, km, under:R')


def choose(totals: Dict[str, np.ndarray], grid, objective: str = 'score', current=None) -> Tuple[int, int, int]:
    """The grid point (iK, iT, iR) with the best objective.  `totals`: metric key -> (nK,nT,nR) array; `grid` = (topks, temps, max_kms).
    Objectives: 'score' (largest mean GeoGuessr score), 'km' (smallest mean km), 'under:R' (largest share under R km).  Ties go to the
    smallest topk, then to the T nearest in log to the current one (`current` = (topk, T, max_km); without it: to 1), then to the
    largest max_km.  A NaN objective never wins; all NaN is a ValueError."""
    key, maximise = objective_column(objective)
    topks, temps, max_kms = grid
    v = np.asarray(totals[key], dtype=np.float64)
    if v.shape != (len(topks), len(temps), len(max_kms)):
        raise ValueError(f'choose: totals[{key!r}] has shape {v.shape}, the grid {(len(topks), len(temps), len(max_kms))}')
    ok = ~np.isnan(v)
    if not ok.any():
        raise ValueError(f'choose: every grid point\'s {key} is NaN')
    best = (v[ok].max() if maximise else v[ok].min())
    t_ref = math.log(float(current[1])) if current is not None else 0.0
    ties = [(topks[i], abs(math.log(temps[j]) - t_ref), -max_kms[r], i, j, r) for i, j, r in zip(*np.nonzero(ok & (v == best)))]
    _, _, _, i, j, r = min(ties)
    return int(i), int(j), int(r)


# ------------------------------------------------------------------------------------------------ the sweep on the device
class Prepared:
    """The records of one `refine_forward` at topk = n_eval over a set of rows, and the values table (B,n_eval,12) of the metrics'
    per-row columns for every candidate: `totals(topks, temps, max_kms)` is then the sweep alone."""

    def __init__(self, refiner, embedding, initial_preds, candidate_cells, candidate_probs, labels, n_eval: int):
        import torch
        from . import hip_ops
        from .config import DECAY_CONSTANT
        dev = embedding.device if embedding.is_cuda else torch.device(refiner._device)
        if dev.type != 'cuda':
            raise RuntimeError('pigeon_amd.refiner_fit runs on the GPU only (no CPU fallback)')
        n_eval = int(n_eval)
        if not 1 <= n_eval <= min(MAX_TOPK, int(candidate_cells.shape[1])):
            raise ValueError(f'sweep: max(topks) = {n_eval} is outside 1 .. min({MAX_TOPK}, {int(candidate_cells.shape[1])} candidates)')
        with torch.no_grad():
            q = self.q = embedding.to(dev, torch.float32).contiguous()
            self.init = initial_preds.to(dev, torch.float64).contiguous()
            cand = self.cand = candidate_cells.to(dev, torch.int64).contiguous()
            self.probs = None if candidate_probs is None else candidate_probs.to(dev, torch.float32).contiguous()
            lab = torch.as_tensor(labels).to(dev, torch.float64).contiguous()
            B = int(q.shape[0])
            if lab.shape != (B, 2):
                raise ValueError(f'sweep: labels must have shape ({B}, 2) [lng, lat], got {tuple(lab.shape)}')
            self.bank = refiner._device_bank(dev)
            # the candidates, once: the records do not depend on the three settings (temperature 1 and no veto: only the records are used)
            _, _, _, self.scratch = hip_ops.refine_forward(self.bank, q, self.init, cand, self.probs, n_eval, 1.0, float('inf'),
                                                           return_scratch=True)
            points = self.scratch[:, :, 1:3].reshape(B * n_eval, 2).contiguous()
            km = hip_ops.haversine_pairs(lab[:, None, :].expand(B, n_eval, 2).reshape(B * n_eval, 2).contiguous(), points).reshape(B, n_eval)
            cols = [km, torch.round(5000 * torch.exp(-km / DECAY_CONSTANT))] + [(km < r).to(torch.float64) for r in UNDER_KM]
            self.values = torch.stack(cols, dim=2).contiguous()
        self.labels, self.rows, self.n_eval = lab, B, n_eval

    def raw_totals(self, topks, temps, max_kms, max_choice_bytes: Optional[int] = None):
        from . import hip_ops
        kw = {} if max_choice_bytes is None else {'max_choice_bytes': int(max_choice_bytes)}
        return hip_ops.refine_sweep(self.scratch, self.probs, self.init, self.values, topks, temps, max_kms, **kw)

    def totals(self, topks, temps, max_kms) -> Dict[str, np.ndarray]:
        """metric key -> (nK,nT,nR) float64: the mean over the rows of every column, the changed share and the veto share.  One host
        synchronisation."""
        shape = (len(topks), len(temps), len(max_kms))
        t = self.raw_totals(topks, temps, max_kms).cpu().numpy()
        return {key: (t[:, i] / self.rows).reshape(shape) for i, key in enumerate(METRICS)}

    def metrics_at(self, settings) -> Dict[str, float]:
        """every metric at one (topk, T, max_km), from the sweep"""
        topk, temperature, max_km = settings
        return {k: float(v[0, 0, 0]) for k, v in self.totals([int(topk)], [float(temperature)], [float(max_km)]).items()}

    def report_at(self, settings) -> Dict[str, float]:
        """Every metric at one (topk, T, max_km) as `evaluate` would print it: one `refine_forward` with these settings and the host
        metric functions of pigeon_amd.evaluate on its guesses (numpy's haversine: its fp32 cosine may sit one ulp from the device's,
        which moves a mean km by ~1e-10 relative -- irrelevant to the choice, visible in a report); Changed and Vetoed are the sweep's
        counts, which are exact."""
        from . import hip_ops
        from .evaluate import geoguessr_score, percentage_within_radius
        from .geo_utils import haversine_np
        topk, temperature, max_km = settings
        out = self.metrics_at(settings)
        llh, _, _ = hip_ops.refine_forward(self.bank, self.q, self.init, self.cand, self.probs, int(topk), float(temperature), float(max_km))
        d = haversine_np(llh.cpu().numpy(), self.labels.cpu().numpy())
        out.update(Mean_km_error=float(np.mean(d)), Geoguessr_score=float(geoguessr_score(d)))
        out.update({f'Under_{r}_km': float(percentage_within_radius(d, r)) for r in UNDER_KM})
        return out


def sweep(refiner, embedding, initial_preds, candidate_cells, candidate_probs, labels, topks, temps, max_kms) -> Dict[str, np.ndarray]:
    """`ProtoRefiner.sweep`: the metrics of every point of the grid topks x temps x max_kms as (nK,nT,nR) arrays -- Mean_km_error,
    Geoguessr_score, the ten Under_*_km, Changed (share of rows whose choice is not candidate 0) and Vetoed.  The candidates are
    evaluated once, by refine_forward at topk = max(topks); `labels` (B,2) are the true [lng, lat]."""
    topks = [int(k) for k in topks]
    if not topks:
        raise ValueError('sweep: topks is empty')
    prep = Prepared(refiner, embedding, initial_preds, candidate_cells, candidate_probs, labels, max(topks))
    return prep.totals(topks, list(temps), list(max_kms))


@dataclass
class RefinerFit:
    topk: int
    temperature: float           # the float32 value the kernel saw
    max_refinement: float
    objective: str
    current: dict                # the settings the refiner had: {topk, temperature, max_refinement}
    rows_fit: int
    rows_heldout: int
    fit_metrics: dict = field(default_factory=dict)          # {'current': {metric: value}, 'fitted': {...}} on the fit rows
    heldout_metrics: dict = field(default_factory=dict)      # the same on the held-out rows
    grid_points: list = field(default_factory=list)          # points of pass 1 and pass 2

    @property
    def settings(self) -> Tuple[int, float, float]:
        return self.topk, self.temperature, self.max_refinement


def holdout_mask(n: int, holdout: float) -> np.ndarray:
    """Row i is held out when floor((i + 1) h) > floor(i h): deterministic, and for h = 0.5 the odd rows (the even rows fit)."""
    if not 0.0 <= float(holdout) < 1.0:
        raise ValueError(f'holdout must be in [0, 1), got {holdout!r}')
    i = np.arange(n + 1, dtype=np.float64)
    f = np.floor(i * float(holdout))
    return f[1:] > f[:-1]


def head_candidates(model, embedding):
    """What `evaluate_model` feeds the refiner: the head's initial prediction and its `num_candidates` (at most 64) most probable cells
    with their softmax probabilities -> (embedding on the device, preds_LLH (N,2) f64, cells (N,k) i64, probs (N,k) f32)."""
    import torch
    from . import hip_ops
    dev = model.cell_layer.weight.device
    emb = torch.as_tensor(embedding).to(dev, torch.float32).contiguous()
    k = min(int(model.num_candidates), MAX_TOPK, int(model.num_cells))
    o = hip_ops.head_forward(model._head_rows(emb), model.cell_layer.weight.data, model.cell_layer.bias.data, model.lla_geocells.data, k)
    return emb, o['preds_LLH'], o['topk_indices'], o['topk_values']


def fit_with(prep, current, objective: str = 'score', log: Optional[Callable] = None):
    """The two passes over `prep.totals` (a Prepared, or any object with .n_eval and .totals: the stub of the CPU tests) ->
    ((topk, T, max_km), [points of pass 1, of pass 2], the pass-1 grid and its totals)."""
    kmax = int(prep.n_eval)
    g1 = pass1_grid(kmax, current)
    t1 = prep.totals(*g1)
    i, j, r = choose(t1, g1, objective, current)
    best1 = (g1[0][i], g1[1][j], g1[2][r])
    g2 = pass2_grid(best1, g1, kmax)
    t2 = prep.totals(*g2)
    i, j, r = choose(t2, g2, objective, current)
    best = (g2[0][i], g2[1][j], g2[2][r])
    if log:
        key, _ = objective_column(objective)
        log(f'pass 1: {len(g1[0])} x {len(g1[1])} x {len(g1[2])} points, best {best1}; pass 2: {len(g2[0])} x {len(g2[1])} x {len(g2[2])} '
            f'points, best {best} ({key} {float(t2[key][i, j, r]):.6g})')
    sizes = [len(g[0]) * len(g[1]) * len(g[2]) for g in (g1, g2)]
    return best, sizes, g1, t1


def fit_refiner(model, refiner, embedding, labels, objective: str = 'score', holdout: float = 0.5, log: Optional[Callable] = None) -> RefinerFit:
    """Fit (topk, temperature, max_refinement) of `refiner` for `model`'s head on embeddings (N,1024) / (N,P,1024) with their true
    [lng, lat] `labels` (N,2).  Candidates and probabilities come from the head (`head_candidates`).  Even rows fit, odd rows are held
    out (`holdout_mask`).  Pass 1: every topk in 1 .. Kmax x 24 log-spaced T in [0.05, 20] x nine max_km, plus the refiner's current
    settings; pass 2: 16 T strictly between the best T's neighbours, topk within +-3, every max_km.  The refiner is not changed:
    `refiner.apply_settings(*fit.settings)` does that."""
    import torch
    objective_column(objective)
    emb, init, cells, probs = head_candidates(model, embedding)
    lab = torch.as_tensor(labels).to(emb.device, torch.float64)
    N = int(emb.shape[0])
    held = holdout_mask(N, holdout)
    fit_rows = torch.from_numpy(np.nonzero(~held)[0]).to(emb.device)
    held_rows = torch.from_numpy(np.nonzero(held)[0]).to(emb.device)
    if fit_rows.numel() == 0:
        raise ValueError('fit_refiner: no rows to fit on')
    kmax = int(cells.shape[1])
    current = current_settings(refiner)
    current = (current[0], f32(current[1]), current[2])
    if current[0] > kmax:
        raise ValueError(f'fit_refiner: the refiner\'s topk = {current[0]} exceeds the {kmax} candidates the head supplies')
    take = lambda rows: (emb[rows], init[rows], cells[rows], probs[rows], lab[rows])
    prep = Prepared(refiner, *take(fit_rows), n_eval=kmax)
    best, sizes, _, _ = fit_with(prep, current, objective, log)
    tables = {'fit': {'current': prep.report_at(current), 'fitted': prep.report_at(best)}, 'heldout': {}}
    if held_rows.numel():
        hp = Prepared(refiner, *take(held_rows), n_eval=max(best[0], current[0]))
        tables['heldout'] = {'current': hp.report_at(current), 'fitted': hp.report_at(best)}
    return RefinerFit(topk=int(best[0]), temperature=float(best[1]), max_refinement=float(best[2]), objective=objective,
                      current=dict(topk=current[0], temperature=current[1], max_refinement=current[2]), rows_fit=int(fit_rows.numel()),
                      rows_heldout=int(held_rows.numel()), fit_metrics=tables['fit'], heldout_metrics=tables['heldout'], grid_points=sizes)


# ------------------------------------------------------------------------------------------------ the sidecar
def fingerprints(model, refiner, fingerprint: Optional[Callable] = None) -> dict:
    """{'head': {'weight', 'bias'}, 'bank': {'proto_emb', 'cell_off', 'member_idx'}}: 128-bit digests (hip_ops.fingerprint) as hex"""
    from .temperature import head_fingerprint
    if fingerprint is None:
        from . import hip_ops
        fingerprint = hip_ops.fingerprint
    bank = refiner._device_bank(model.cell_layer.weight.device)
    return {'head': head_fingerprint(model, fingerprint),
            'bank': {name: '%016x%016x' % tuple(fingerprint(bank.t[name])) for name in ('proto_emb', 'cell_off', 'member_idx')}}


def _json_number(v):
    return v if math.isfinite(v) else repr(v)          # 'inf': JSON has no infinity


def save(path: str, fit: RefinerFit, model, refiner, fingerprint: Optional[Callable] = None) -> str:
    """Write the sidecar: the settings, the objective, both metric tables, the row counts and the fingerprints of head and bank."""
    obj = {'format': FORMAT, **asdict(fit), 'fingerprints': fingerprints(model, refiner, fingerprint)}
    obj['max_refinement'] = _json_number(fit.max_refinement)
    obj['current'] = dict(fit.current, max_refinement=_json_number(float(fit.current['max_refinement'])))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'w') as f:
        json.dump(obj, f, indent=1)
        f.write('\n')
    return path


def load(path: str, model, refiner, fingerprint: Optional[Callable] = None) -> RefinerFit:
    """Read a sidecar for `model`'s head and `refiner`'s bank.  ValueError, naming both fingerprints, when it was fitted for another
    head or another bank -- as `temperature.load` refuses another head's temperature."""
    with open(path) as f:
        obj = json.load(f)
    if obj.get('format') != FORMAT:
        raise ValueError(f'{path}: not a refiner-fit sidecar (format {obj.get("format")!r})')
    theirs, ours = obj.get('fingerprints') or {}, fingerprints(model, refiner, fingerprint)
    for part in ('head', 'bank'):
        if theirs.get(part) != ours[part]:
            raise ValueError(f'{path}: fitted for a {part} with fingerprint {theirs.get(part)}, this {part} has {ours[part]}; fit it again '
                             f'(python -m pigeon_amd.refiner_fit)')
    kw = {k: obj[k] for k in RefinerFit.__dataclass_fields__}
    kw['max_refinement'] = float(kw['max_refinement'])
    kw['current'] = dict(kw['current'], max_refinement=float(kw['current']['max_refinement']))
    fit = RefinerFit(**kw)
    check_settings(fit.topk, fit.temperature, fit.max_refinement, where=path)
    return fit


def resolve(spec, model, refiner, fingerprint: Optional[Callable] = None) -> Tuple[int, float, float]:
    """`--refiner FILE|TOPK,TEMPERATURE,MAX_KM` (or a triple) -> the validated triple; a path goes through `load` (keyed to head and
    bank).  topk above the head's `num_candidates` is refused."""
    if isinstance(spec, (tuple, list)):
        triple = check_settings(*spec, where='refiner settings')
    elif isinstance(spec, str) and os.path.exists(spec):
        triple = load(spec, model, refiner, fingerprint).settings
    elif isinstance(spec, str) and ',' in spec:
        triple = parse_settings(spec)
    else:
        raise ValueError(f'--refiner: {spec!r} is neither TOPK,TEMPERATURE,MAX_KM nor an existing file')
    return check_settings(*triple, num_candidates=min(int(model.num_candidates), int(model.num_cells)), where='--refiner')


def apply_to(refiner, spec, model, fingerprint: Optional[Callable] = None, prefix: str = '') -> Tuple[int, float, float]:
    """What `evaluate(refiner_settings=...)` and `serve --refiner` do after the refiner is built: resolve, apply, print."""
    triple = resolve(spec, model, refiner, fingerprint)
    refiner.apply_settings(*triple)
    print(f'{prefix}Refiner settings: topk {triple[0]}, temperature {triple[1]:.6g}, max_refinement {triple[2]:g} km')
    return triple


# ------------------------------------------------------------------------------------------------ command line
def format_fit(fit: RefinerFit) -> str:
    cur = fit.current
    lines = [f'objective {fit.objective}: topk {cur["topk"]} -> {fit.topk}, temperature {cur["temperature"]:.6g} -> {fit.temperature:.6g}, '
             f'max_refinement {cur["max_refinement"]:g} -> {fit.max_refinement:g} km',
             f'rows: {fit.rows_fit} fit, {fit.rows_heldout} held out; grid points {fit.grid_points}',
             f'{"metric":<18}{"fit: current":>14}{"fitted":>12}{"held out: current":>20}{"fitted":>12}']
    for key in METRICS:
        cell = lambda table, which: f'{table.get(which, {}).get(key, float("nan")):.6g}'
        lines.append(f'{key:<18}{cell(fit.fit_metrics, "current"):>14}{cell(fit.fit_metrics, "fitted"):>12}'
                     f'{cell(fit.heldout_metrics, "current"):>20}{cell(fit.heldout_metrics, "fitted"):>12}')
    return '\n'.join(lines)


def heldout_columns(model, refiner, embedding, labels, fit: RefinerFit, holdout: float = 0.5) -> Dict[str, np.ndarray]:
    """Per held-out row: km and score under the current and under the fitted settings (one `refine_forward` per setting), for the
    paired bootstrap."""
    import torch
    from . import hip_ops
    from .config import DECAY_CONSTANT
    emb, init, cells, probs = head_candidates(model, embedding)
    rows = torch.from_numpy(np.nonzero(holdout_mask(int(emb.shape[0]), holdout))[0]).to(emb.device)
    lab = torch.as_tensor(labels).to(emb.device, torch.float64)[rows].contiguous()
    cols = {}
    cur = fit.current
    for name, (topk, temperature, max_km) in (('current', (cur['topk'], cur['temperature'], cur['max_refinement'])), ('fitted', fit.settings)):
        llh, _, _ = hip_ops.refine_forward(refiner._device_bank(emb.device), emb[rows].contiguous(), init[rows].contiguous(),
                                           cells[rows].contiguous(), probs[rows].contiguous(), int(topk), float(temperature), float(max_km))
        km = hip_ops.haversine_pairs(lab, llh).cpu().numpy()
        cols[f'km_{name}'] = km
        cols[f'score_{name}'] = np.round(5000 * np.exp(-km / DECAY_CONSTANT))
    return cols


def parser() -> argparse.ArgumentParser:
    argp = argparse.ArgumentParser(prog='python -m pigeon_amd.refiner_fit',
                                   description="Fit the refiner's topk, temperature and max_refinement on held-out embeddings (one GPU).")
    argp.add_argument('--head', default=None, help='saved head (state dict, as pigeon_amd.train writes it)')
    argp.add_argument('--protos', default=None, help='prototype CSV (pigeon_amd.prototypes), or a packed .npz bank')
    argp.add_argument('--dataset', default=None, help='the training dataset the prototypes index (not needed for a packed bank)')
    argp.add_argument('--geocells', type=str, default=None, help='geocell CSV of the head; with --synthetic: the synthetic geocell count')
    argp.add_argument('-l', '--load', default=None, help='dataset directory (datasets.DatasetDict; the split holds embedding, labels)')
    argp.add_argument('--split', default='val')
    argp.add_argument('--yfcc', action='store_true', default=False)
    argp.add_argument('--objective', default='score', help='score (default) | km | under:R')
    argp.add_argument('--bootstrap', type=int, default=None, metavar='R',
                      help='R paired bootstrap replicates of the held-out difference fitted - current of km and score')
    argp.add_argument('-o', '--out', required=True, help='where the sidecar is written, e.g. head.refiner.json')
    argp.add_argument('--synthetic', type=int, default=0, help='fit on N seeded synthetic samples, a planted head and a synthetic bank')
    argp.add_argument('--seed', type=int, default=0)
    return argp


def synthetic_bank(num_cells: int, seed: int, centroids, protos_per_cell: int = 4, empty_frac: float = 0.05):
    """A prototype bank for `train.synthetic_dataset(.., num_cells, seed)`: cell c's training rows scatter around the direction its
    samples scatter around and lie next to its centroid, so the nearest prototype of the true cell is near and refining towards it
    helps where the head errs.  About `empty_frac` of the cells have no prototypes; clusters have 1 .. 3 members."""
    import torch
    from . import hip_ops, synthetic
    rng = np.random.default_rng(seed + 77)
    dirs = torch.randn((num_cells, hip_ops.HIDDEN), generator=torch.Generator().manual_seed(seed + 4711)).numpy()      # synthetic_dataset's first draw
    empty = rng.random(num_cells) < empty_frac
    empty[-1] = False
    cell_off = np.concatenate([[0], np.cumsum(np.where(empty, 0, protos_per_cell))]).astype(np.int64)
    P = int(cell_off[-1])
    cell_of = np.repeat(np.arange(num_cells), np.diff(cell_off))
    count = rng.integers(1, 4, size=P).astype(np.int32)
    member_off = np.concatenate([[0], np.cumsum(count)]).astype(np.int64)
    n_train = int(member_off[-1])
    member_idx = rng.permutation(n_train).astype(np.int64)
    row_cell = np.empty(n_train, dtype=np.int64)
    row_cell[member_idx] = np.repeat(cell_of, count)
    train_emb = (dirs[row_cell] + 0.5 * rng.standard_normal((n_train, hip_ops.HIDDEN))).astype(np.float32)
    train_lnglat = (np.asarray(centroids)[row_cell] + rng.uniform(-0.5, 0.5, (n_train, 2))).astype(np.float32)
    train_lnglat[:, 1] = np.clip(train_lnglat[:, 1], -89.5, 89.5)
    proto_emb = np.stack([train_emb[member_idx[member_off[p]:member_off[p + 1]]].mean(axis=0, dtype=np.float32) for p in range(P)])
    proto_lnglat = np.stack([train_lnglat[member_idx[member_off[p]:member_off[p + 1]]].astype(np.float64).mean(axis=0) for p in range(P)])
    return synthetic.SyntheticBank(proto_emb=proto_emb.astype(np.float32), cell_off=cell_off, proto_lnglat=proto_lnglat.astype(np.float32),
                                   proto_count=count, member_off=member_off, member_idx=member_idx, train_emb=train_emb,
                                   train_lnglat=train_lnglat)


def synthetic_setup(n: int, num_cells: int, seed: int, panorama: bool = True, geocell_path: Optional[str] = None):
    """A seeded model, refiner, embeddings and labels with no data: `train.synthetic_dataset`, `temperature.planted_head` and a
    `synthetic_bank`."""
    import tempfile
    import torch
    from . import synthetic
    from .proto_refiner import ProtoRefiner
    from .super_guessr import SuperGuessr
    from .temperature import planted_head
    from .train import synthetic_dataset
    dataset, cen = synthetic_dataset(n, num_cells, seed=seed, panorama=panorama)
    geocell_path = geocell_path or os.path.join(tempfile.mkdtemp(prefix='pigeon_refiner_fit_'), 'geocells.csv')
    synthetic.write_geocell_csv(geocell_path, cen)
    model = SuperGuessr(base_model=None, panorama=panorama, yfcc=not panorama, geocell_path=geocell_path,
                        num_candidates=min(50, num_cells)).to('cuda')
    planted_head(model, seed)
    emb, labels = (torch.cat([dataset[k].columns[c] for k in ('train', 'val')]) for c in ('embedding', 'labels'))
    bank = synthetic_bank(num_cells, seed, cen)
    refiner = ProtoRefiner(topk=min(5, model.num_candidates), bank=bank)
    return model, refiner, emb, labels


def main(argv=None) -> RefinerFit:
    argp = parser()
    args = argp.parse_args(argv)
    try:
        objective_column(args.objective)
    except ValueError as e:
        argp.error(str(e))
    if args.synthetic < 0:
        argp.error('--synthetic takes a positive number')
    if args.synthetic and (args.head or args.load or args.protos):
        argp.error('--synthetic takes none of --head, --protos, -l')
    if not args.synthetic and not (args.head and args.load and args.protos):
        argp.error('--head HEAD, --protos PROTOS and -l DATASET are needed (or --synthetic N)')
    if args.bootstrap is not None and args.bootstrap < 1:
        argp.error('--bootstrap takes a positive number of replicates')
    if args.synthetic:
        try:
            cells = int(args.geocells) if args.geocells is not None else 1000
        except ValueError:
            argp.error('--geocells C: with --synthetic, the synthetic geocell count')
        model, refiner, emb, labels = synthetic_setup(args.synthetic, cells, args.seed, panorama=not args.yfcc)
    else:
        from datasets import DatasetDict
        from .proto_refiner import ProtoRefiner
        from .super_guessr import SuperGuessr
        dataset = DatasetDict.load_from_disk(args.load)
        dataset.set_format('torch')
        if args.split not in dataset:
            argp.error(f'--split {args.split}: the dataset has {list(dataset)}')
        kw = {'geocell_path': args.geocells} if args.geocells else {}
        model = SuperGuessr(base_model=None, panorama=not args.yfcc, yfcc=args.yfcc, num_candidates=50, **kw).to('cuda')
        model.load_state(args.head)
        emb, labels = dataset[args.split]['embedding'], dataset[args.split]['labels']
        labels = labels[:, :2]
        if args.protos.endswith('.npz'):
            refiner = ProtoRefiner(bank=args.protos)
        else:
            refiner = ProtoRefiner(proto_path=args.protos, dataset_path=args.dataset)
    fit = fit_refiner(model, refiner, emb, labels, objective=args.objective, log=print)
    print(format_fit(fit))
    if args.bootstrap is not None and fit.rows_heldout:
        from . import bootstrap as boot
        cols = heldout_columns(model, refiner, emb, labels, fit)
        stats = {'Mean_km_error fitted - current': ('mean_diff', 'km_fitted', 'km_current'),
                 'Geoguessr_score fitted - current': ('mean_diff', 'score_fitted', 'score_current')}
        print(boot.report(boot.bootstrap(cols, stats, R=args.bootstrap, seed=args.seed), 0.95))
    print(f'written to {save(args.out, fit, model, refiner)}')
    return fit


if __name__ == '__main__':
    main()
