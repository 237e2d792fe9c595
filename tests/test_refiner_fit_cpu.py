"""pigeon_amd/refiner_fit.py's host side with no GPU: `choose` on hand-made totals (every tie rule, every objective), the two grids,
the fit over a stub sweep, the sidecar and its refusals, `apply_settings`, the `--refiner` parser, what `evaluate` builds with and
without `refiner_settings`, and every PG_EINVAL of the sweep's entry points (raised before any HIP call)."""
import json
import math
import types

import numpy as np
import pytest
import torch

from pigeon_amd import refiner_fit as F


def table(grid, fill=0.0):
    shape = tuple(len(a) for a in grid)
    return {k: np.full(shape, fill, dtype=np.float64) for k in F.METRICS}


GRID = ([1, 2, 3], [0.5, 1.0, 2.0, 4.0], [100.0, 1000.0, 1e5])


# ------------------------------------------------------------------------------------------------ choose
def test_choose_objectives():
    t = table(GRID)
    t['Geoguessr_score'][1, 2, 0] = 10
    t['Mean_km_error'][:] = 50
    t['Mean_km_error'][2, 0, 1] = 3
    t['Under_25_km'][0, 3, 2] = 0.9
    assert F.choose(t, GRID) == (1, 2, 0)                                  # the default: the largest mean score
    assert F.choose(t, GRID, 'score') == (1, 2, 0)
    assert F.choose(t, GRID, 'km') == (2, 0, 1)                            # the smallest mean km
    assert F.choose(t, GRID, 'under:25') == (0, 3, 2)
    for bad in ('nearest', 'under:', 'under:26', 'under:x', None):
        with pytest.raises(ValueError, match='objective'):
            F.choose(t, GRID, bad)
    with pytest.raises(ValueError, match='shape'):
        F.choose({k: v[:2] for k, v in t.items()}, GRID)


def test_choose_tie_rules():
    t = table(GRID)                                                        # everything ties
    cur = (2, 2.0, 1000.0)
    assert F.choose(t, GRID, 'score', cur) == (0, 2, 2)                    # smallest topk, the current T, the largest max_km
    assert F.choose(t, GRID, 'score', (2, 1.5, 1000.0)) == (0, 2, 2)       # |log 2 - log 1.5| < |log 1 - log 1.5|
    assert F.choose(t, GRID, 'score', (2, 1.3, 1000.0)) == (0, 1, 2)       # nearer to 1 in log
    assert F.choose(t, GRID, 'score', (2, 0.01, 1000.0)) == (0, 0, 2)
    assert F.choose(t, GRID, 'score', None) == (0, 1, 2)                   # no current settings: nearest to T = 1
    # topk outranks T, T outranks max_km
    t['Geoguessr_score'][:] = -1
    t['Geoguessr_score'][2, 2, 0] = t['Geoguessr_score'][1, 0, 1] = t['Geoguessr_score'][1, 3, 2] = 7
    assert F.choose(t, GRID, 'score', cur) == (1, 3, 2)                    # topk 2 beats topk 3; T = 4 is nearer to the current 2 in log than 0.5 is
    t['Geoguessr_score'][1, 3, 2] = -1
    t['Geoguessr_score'][1, 0, 2] = 7
    assert F.choose(t, GRID, 'score', cur) == (1, 0, 2)                    # the same T: the largest max_km
    # a NaN never wins, all NaN is an error
    t['Geoguessr_score'][0, 0, 0] = np.nan
    assert F.choose(t, GRID, 'score', cur) == (1, 0, 2)
    t['Mean_km_error'][:] = np.nan
    with pytest.raises(ValueError, match='NaN'):
        F.choose(t, GRID, 'km', cur)
    t['Mean_km_error'][2, 1, 1] = 5.0
    assert F.choose(t, GRID, 'km', cur) == (2, 1, 1)


def test_choose_equal_log_distance_goes_to_the_larger_max_km_then_first():
    t = table(GRID, -1.0)
    t['Geoguessr_score'][0, 0, 1] = t['Geoguessr_score'][0, 2, 2] = 3       # T = 0.5 and T = 2 are equally far from 1 in log
    i, j, r = F.choose(t, GRID, 'score', (1, 1.0, 100.0))
    assert (i, j, r) == (0, 2, 2)                                          # the tie in T falls to the larger max_km


# ------------------------------------------------------------------------------------------------ the grids
def test_pass1_grid_holds_the_current_settings():
    for cur in ((5, 1.6, 1000), (40, 0.6, 100000), (20, 1.0, 10000), (3, 0.123456789, 77.0), (1, 30.0, float('inf'))):
        topks, temps, max_kms = F.pass1_grid(50, cur)
        assert topks == list(range(1, 51))
        assert cur[0] in topks and F.f32(cur[1]) in temps and float(cur[2]) in max_kms
        assert set(F.MAX_KMS) <= set(max_kms) and len(max_kms) in (9, 10)
        assert len(temps) in (24, 25) and temps == sorted(temps) and max_kms == sorted(max_kms)
        assert all(t == F.f32(t) for t in temps)                           # stored as the float32 the kernel sees
        assert min(temps) == F.f32(min(0.05, cur[1])) and max(temps) == F.f32(max(20.0, cur[1]))
        inner = [t for t in temps if t != F.f32(cur[1])] if len(temps) == 25 else temps
        ratios = np.diff(np.log(inner))
        assert np.allclose(ratios, ratios[0], rtol=1e-5)                   # log-spaced
    with pytest.raises(ValueError, match='topk'):
        F.pass1_grid(12, (20, 1.0, 1000))


def test_pass2_grid_lies_strictly_inside_the_bracket():
    g1 = F.pass1_grid(50, (5, 1.6, 1000))
    for j in (0, 1, 7, len(g1[1]) - 2, len(g1[1]) - 1):
        best_t = g1[1][j]
        inside, (lo, hi) = F.pass2_temps(best_t, g1[1])
        assert lo == g1[1][max(j - 1, 0)] and hi == g1[1][min(j + 1, len(g1[1]) - 1)]
        assert len(inside) == 16 and all(lo < t < hi for t in inside) and inside == sorted(set(inside))
        assert all(t == F.f32(t) for t in inside)
        topks, temps, max_kms = F.pass2_grid((7, best_t, 500.0), g1, 50)
        assert topks == [4, 5, 6, 7, 8, 9, 10] and max_kms == g1[2]
        assert set(temps) == set(inside) | {best_t}                        # pass 1's best point is a point of pass 2
    assert F.pass2_grid((1, g1[1][3], 25.0), g1, 50)[0] == [1, 2, 3, 4]
    assert F.pass2_grid((50, g1[1][3], 25.0), g1, 50)[0] == [47, 48, 49, 50]
    assert F.pass2_grid((2, g1[1][3], 25.0), g1, 2)[0] == [1, 2]
    # a bracket float32 cannot split: nothing inside, the best T alone
    one = np.float32(1.0)
    tight = [float(one), float(np.nextafter(one, np.float32(2)))]
    assert F.pass2_temps(tight[0], tight)[0] == []


class StubSweep:
    """totals of a made-up smooth objective with its optimum at topk 9, T 0.8, 200 km: the sweep's interface, no GPU"""
    n_eval = 30

    def __init__(self):
        self.calls = []

    def totals(self, topks, temps, max_kms):
        self.calls.append((list(topks), list(temps), list(max_kms)))
        K, T, R = np.meshgrid(topks, temps, max_kms, indexing='ij')
        score = 4000 - 3 * (K - 9) ** 2 - 500 * (np.log(T) - math.log(0.8)) ** 2 - 40 * (np.log(R) - math.log(200.0)) ** 2
        t = {k: np.zeros(K.shape) for k in F.METRICS}
        t['Geoguessr_score'] = score
        t['Mean_km_error'] = 5000 - score
        return t


def test_fit_over_a_stub_sweep():
    stub = StubSweep()
    current = (5, F.f32(1.6), 1000.0)
    best, sizes, g1, t1 = F.fit_with(stub, current, 'score')
    assert len(stub.calls) == 2 and sizes == [len(a) * len(b) * len(c) for a, b, c in stub.calls]
    assert list(stub.calls[0]) == [list(a) for a in g1]
    assert current[0] in g1[0] and current[1] in g1[1] and current[2] in g1[2]          # the current point is evaluated
    assert best[0] == 9 and best[2] == 200.0 and abs(math.log(best[1] / 0.8)) < 0.02
    assert best[1] == F.f32(best[1])
    # never worse than the current settings, and never worse than any point of pass 1
    at = lambda k, T, r: float(stub.totals([k], [T], [r])['Geoguessr_score'][0, 0, 0])
    assert at(*best) >= t1['Geoguessr_score'].max() >= at(*current)
    best_km, _, _, _ = F.fit_with(StubSweep(), current, 'km')
    assert best_km == best


# ------------------------------------------------------------------------------------------------ settings
class FakeRefiner:
    def __init__(self, topk=5, temperature=1.6, max_refinement=1000):
        self.topk, self.max_refinement = topk, max_refinement
        self.temperature = torch.nn.Parameter(torch.tensor(temperature), requires_grad=False)
        self._bank = types.SimpleNamespace(t={'proto_emb': torch.arange(8.0), 'cell_off': torch.arange(3), 'member_idx': torch.arange(5)})

    def apply_settings(self, *a, **kw):
        return F.apply_settings(self, *a, **kw)

    def _device_bank(self, device):
        return self._bank

    def _temperature_value(self):
        return float(self.temperature.data)


def test_apply_settings_validation():
    r = FakeRefiner()
    version = r.temperature._version
    r.apply_settings(7, 0.3, 250.0)
    assert (r.topk, r.max_refinement) == (7, 250) and r._temperature_value() == F.f32(0.3)
    assert r.temperature._version == version and not r.temperature.requires_grad         # written through .data
    r.apply_settings(64, 20, float('inf'))
    assert r.max_refinement == float('inf')
    for bad, word in (((0, 1.0, 10), 'topk'), ((65, 1.0, 10), 'topk'), ((2.5, 1.0, 10), 'topk'), ((True, 1.0, 10), 'topk'),
                      ((3, 0.0, 10), 'temperature'), ((3, -1.0, 10), 'temperature'), ((3, float('nan'), 10), 'temperature'),
                      ((3, float('inf'), 10), 'temperature'), ((3, 1.0, -1), 'max_refinement'), ((3, 1.0, float('nan')), 'max_refinement'),
                      ((3, 'x', 10), 'numbers')):
        with pytest.raises(ValueError, match=word):
            r.apply_settings(*bad)
    assert (r.topk, r.max_refinement) == (64, float('inf'))                               # a refused call changes nothing
    with pytest.raises(ValueError, match='candidates'):
        r.apply_settings(13, 1.0, 10, num_candidates=12)
    # the real class routes to the same function
    from pigeon_amd.proto_refiner import ProtoRefiner
    assert ProtoRefiner.apply_settings.__doc__ and ProtoRefiner.sweep.__doc__


def test_parse_refiner_flag():
    assert F.parse_settings('5,1.6,1000') == (5, 1.6, 1000.0)
    assert F.parse_settings(' 40 , 0.6 , inf ') == (40, 0.6, float('inf'))
    for bad in ('5,1.6', '5,1.6,1000,2', 'a,b,c', '5.5,1,1', '0,1,1', '5,0,1', '5,1,-3', '5,1,nan'):
        with pytest.raises(ValueError):
            F.parse_settings(bad)
    import run                                                             # the flag exists and defaults to nothing
    assert run.argp.parse_args(['evaluate', 'x']).refiner is None
    assert run.argp.parse_args(['evaluate', 'x', '--refiner', '5,1.6,1000']).refiner == '5,1.6,1000'


# ------------------------------------------------------------------------------------------------ the sidecar
def fake_model(scale=1.0, num_candidates=50):
    m = types.SimpleNamespace(num_candidates=num_candidates, num_cells=100)
    m.cell_layer = types.SimpleNamespace(weight=torch.nn.Parameter(scale * torch.arange(12.0).reshape(3, 4)), bias=torch.nn.Parameter(torch.zeros(3)))
    return m


def fake_fingerprint(t, seed=0):
    b = t.detach().cpu().contiguous().numpy().tobytes()
    return (hash(b) & 0xFFFFFFFFFFFFFFFF, len(b))


def a_fit(max_refinement=2500.0):
    m = {k: 0.5 for k in F.METRICS}
    return F.RefinerFit(topk=9, temperature=F.f32(0.8), max_refinement=max_refinement, objective='score',
                        current=dict(topk=5, temperature=F.f32(1.6), max_refinement=1000.0), rows_fit=256, rows_heldout=256,
                        fit_metrics={'current': m, 'fitted': m}, heldout_metrics={'current': m, 'fitted': m}, grid_points=[100, 50])


def test_sidecar_round_trip_and_refusals(tmp_path):
    model, refiner = fake_model(), FakeRefiner()
    for km in (2500.0, float('inf')):
        path = str(tmp_path / f'r{km}.json')
        fit = a_fit(km)
        F.save(path, fit, model, refiner, fake_fingerprint)
        obj = json.load(open(path))
        assert obj['format'] == F.FORMAT and set(obj['fingerprints']) == {'head', 'bank'}
        assert set(obj['fingerprints']['bank']) == {'proto_emb', 'cell_off', 'member_idx'} and set(obj['fingerprints']['head']) == {'weight', 'bias'}
        for key in ('topk', 'temperature', 'max_refinement', 'objective', 'fit_metrics', 'heldout_metrics', 'rows_fit', 'rows_heldout'):
            assert key in obj
        back = F.load(path, model, refiner, fake_fingerprint)
        assert back == fit and back.settings == (9, F.f32(0.8), km)
        assert F.resolve(path, model, refiner, fake_fingerprint) == back.settings
    # another head, another bank: refused, both fingerprints named
    other = fake_model(2.0)
    with pytest.raises(ValueError) as e:
        F.load(path, other, refiner, fake_fingerprint)
    theirs, ours = obj['fingerprints']['head'], F.fingerprints(other, refiner, fake_fingerprint)['head']
    assert 'head' in str(e.value) and theirs['weight'] in str(e.value) and ours['weight'] in str(e.value)
    other_bank = FakeRefiner()
    other_bank._bank.t['member_idx'] = torch.arange(6)
    with pytest.raises(ValueError, match='bank'):
        F.load(path, model, other_bank, fake_fingerprint)
    bad = str(tmp_path / 'bad.json')
    json.dump({'format': 'pigeon_amd.temperature/1'}, open(bad, 'w'))
    with pytest.raises(ValueError, match='not a refiner-fit sidecar'):
        F.load(bad, model, refiner, fake_fingerprint)
    # the flag's other form, and the candidates' limit
    assert F.resolve('5,1.6,1000', model, refiner) == (5, 1.6, 1000.0)
    assert F.resolve((5, 1.6, 1000), model, refiner) == (5, 1.6, 1000.0)
    with pytest.raises(ValueError, match='candidates'):
        F.resolve('51,1.6,1000', model, refiner)
    with pytest.raises(ValueError, match='candidates'):
        F.resolve(path, fake_model(num_candidates=8), refiner, fake_fingerprint)
    with pytest.raises(ValueError, match='neither'):
        F.resolve(str(tmp_path / 'missing.json'), model, refiner)
    r = FakeRefiner()
    assert F.apply_to(r, path, model, fake_fingerprint) == (9, F.f32(0.8), float('inf'))
    assert (r.topk, r._temperature_value(), r.max_refinement) == (9, F.f32(0.8), float('inf'))


def test_holdout_mask_is_deterministic():
    m = F.holdout_mask(9, 0.5)
    assert list(m) == [False, True] * 4 + [False]                          # even rows fit, odd rows are held out
    assert F.holdout_mask(100, 0.25).sum() == 25 and not F.holdout_mask(7, 0.0).any()
    with pytest.raises(ValueError):
        F.holdout_mask(5, 1.0)


# ------------------------------------------------------------------------------------------------ evaluate's refiner
@pytest.mark.parametrize("settings", [None, '7,0.3,250'])
def test_evaluate_builds_the_refiner_as_before(monkeypatch, tmp_path, settings, capsys):
    from pigeon_amd import evaluate as E
    built = []

    class StubRefiner(FakeRefiner):
        def __init__(self, *args, **kw):
            built.append((args, {k: v for k, v in kw.items() if k in ('temperature', 'bank')}))
            super().__init__(args[0], float(kw['temperature']), args[2])
            self.bank_rel_tol = 0.0

    class StubModel:
        num_candidates, num_cells = 50, 100

        def __init__(self, *a, **kw):
            self.kw = kw

        def to(self, *_):
            return self

        def load_state(self, *_):
            pass

    seen = {}

    def stub_evaluate_model(model, dataset, metrics, _, refiner, **kw):
        seen['refiner'] = refiner
        return {'Mean_km_error': 1.0}

    monkeypatch.setattr(E, 'ProtoRefiner', StubRefiner)
    monkeypatch.setattr(E, 'SuperGuessr', StubModel)
    monkeypatch.setattr(E, 'evaluate_model', stub_evaluate_model)
    monkeypatch.setattr(E, '_resolve_bank_rel_tol', lambda v, m: None)
    kw = {} if settings is None else {'refiner_settings': settings}
    res = E.evaluate('none', [], yfcc=False, landmarks=False, base_model=None, bank='a-bank', **kw)
    assert res == {'Mean_km_error': 1.0}
    assert built == [((40, False, 100000), {'temperature': 0.6, 'bank': 'a-bank'})]       # the same literals with and without the argument
    r = seen['refiner']
    out = capsys.readouterr().out
    if settings is None:
        assert (r.topk, r._temperature_value(), r.max_refinement) == (40, F.f32(0.6), 100000) and 'Refiner settings' not in out
    else:
        assert (r.topk, r._temperature_value(), r.max_refinement) == (7, F.f32(0.3), 250) and 'Refiner settings: topk 7' in out
    if settings is not None:
        with pytest.raises(ValueError, match='candidates'):
            E.evaluate('none', [], yfcc=False, landmarks=False, base_model=None, bank='a-bank', refiner_settings='51,1,10')


# ------------------------------------------------------------------------------------------------ the ABI's refusals
def test_sweep_refusals_without_a_gpu(hip_lib):
    import _sweep_refusals
    _sweep_refusals.check_refusals(hip_lib)
    from pigeon_amd import hip_ops
    assert hip_ops.refine_sweep_plan(8192, 50, 64 * 25 * 9, 12) == {"rows_per_workgroup": 64, "lds_bytes": 41600, "row_groups": 128,
                                                                     "choice_bytes": 64 * 25 * 9 * 8192}
