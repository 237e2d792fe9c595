"""The refiner fit at the entry points (run with -m gpu on an MI355X), on a seeded synthetic head, bank and 512 rows over 33 cells:
`fit_refiner` against an independent recomputation by `refine_forward` and the host metrics, the sidecar through `evaluate` and the
server's refiner builder, the refusal of another head's sidecar, and `run.py evaluate` with and without `--refiner`."""
import math
import os
import sys

import numpy as np
import pytest
import torch

import _refitref as R
from pigeon_amd.geo_utils import haversine_np

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
ROWS, CELLS, SEED = 512, 33, 4


@pytest.fixture(scope="module")
def fitted(tmp_path_factory):
    from pigeon_amd import _lib, refiner_fit as F
    _lib.require_gpu()
    tmp = tmp_path_factory.mktemp("refiner_fit")
    gp = str(tmp / "geocells.csv")
    model, refiner, emb, labels = F.synthetic_setup(ROWS, CELLS, SEED, geocell_path=gp)
    model.eval()
    assert emb.shape == (ROWS, 4, 1024) and labels.shape == (ROWS, 2) and model.num_candidates == CELLS
    calls = []
    real = F.Prepared.totals

    def spy(self, topks, temps, max_kms):
        out = real(self, topks, temps, max_kms)
        calls.append((self.rows, list(topks), list(temps), list(max_kms), out))
        return out

    F.Prepared.totals = spy
    try:
        fit = F.fit_refiner(model, refiner, emb, labels)
    finally:
        F.Prepared.totals = real
    head = str(tmp / "head.model")
    torch.save(model.state_dict(), head)
    sidecar = F.save(str(tmp / "head.refiner.json"), fit, model, refiner)
    emb_d, init, cells, probs = F.head_candidates(model, emb)
    held = F.holdout_mask(ROWS, 0.5)
    return dict(F=F, model=model, refiner=refiner, emb=emb, labels=labels, fit=fit, calls=calls, head=head, sidecar=sidecar, gp=gp, tmp=tmp,
                cand=(emb_d, init, cells, probs), held=held)


def forward_metrics(env, rows, settings):
    """one `refine_forward` over `rows` at `settings` and the host metric functions of pigeon_amd.evaluate -> (metrics, choice, preds)"""
    from pigeon_amd import hip_ops
    from pigeon_amd.evaluate import compute_geoguessr_metrics
    emb, init, cells, probs = env["cand"]
    idx = torch.from_numpy(np.nonzero(rows)[0]).to(DEV)
    topk, T, km = settings
    llh, cell, choice = hip_ops.refine_forward(env["refiner"]._device_bank(torch.device(DEV)), emb[idx].contiguous(), init[idx].contiguous(),
                                               cells[idx].contiguous(), probs[idx].contiguous(), int(topk), float(T), float(km))
    labels = env["labels"].numpy()[rows]
    n = int(rows.sum())
    collected = (llh.cpu().numpy(), cell.cpu().numpy(), None, None, None, np.zeros((n, 5), dtype=np.int64), labels, np.zeros(n, dtype=np.int64),
                 None, None, None)
    return compute_geoguessr_metrics(collected), choice.cpu().numpy(), llh


def close(a, b):
    return abs(a - b) <= 1e-12 * max(abs(a), abs(b))


def test_fit_is_at_least_every_sampled_grid_point_and_the_current_settings(fitted):
    F, fit = fitted["F"], fitted["fit"]
    assert fit.objective == "score" and fit.rows_fit == 256 and fit.rows_heldout == 256
    assert fit.temperature == F.f32(fit.temperature) and 1 <= fit.topk <= CELLS
    cur = (fit.current["topk"], fit.current["temperature"], fit.current["max_refinement"])
    assert cur == (5, F.f32(1.6), 1000.0)
    fit_rows = ~fitted["held"]
    best = fit.fit_metrics["fitted"]["Geoguessr_score"]
    mine, _, _ = forward_metrics(fitted, fit_rows, fit.settings)
    assert close(mine["Geoguessr_score"], best)
    at_current, _, _ = forward_metrics(fitted, fit_rows, cur)
    assert close(at_current["Geoguessr_score"], fit.fit_metrics["current"]["Geoguessr_score"])
    slack = 1e-12 * abs(best)
    assert best >= at_current["Geoguessr_score"] - slack
    # pass 1 as the fit ran it: 33 topks x 24 (+ the current) temperatures x 9 (the current 1000 km is one of them) radii
    rows, topks, temps, max_kms, totals = fitted["calls"][0]
    assert rows == 256 and topks == list(range(1, CELLS + 1)) and len(temps) == 25 and len(max_kms) == 9
    assert cur[0] in topks and cur[1] in temps and cur[2] in max_kms
    rng = np.random.default_rng(1)
    labels = fitted["labels"].numpy()[fit_rows]
    for _ in range(40):
        i, j, r = rng.integers(len(topks)), rng.integers(len(temps)), rng.integers(len(max_kms))
        m, choice, llh = forward_metrics(fitted, fit_rows, (topks[i], temps[j], max_kms[r]))
        assert best >= m["Geoguessr_score"] - slack, (topks[i], temps[j], max_kms[r])
        assert (choice != 0).sum() == round(totals["Changed"][i, j, r] * 256)
        # the sweep's own totals against the host metrics.  Its km column is the device's haversine, whose fp32 cos(lat) may sit one
        # fp32 ulp from numpy's: a row's distance d = R c moves by at most R 2^-23 tan(c / 2) (+ 1e-9 d for the fp64 rest), its
        # score by what that moves it across a rounding boundary
        d = haversine_np(llh.cpu().numpy(), labels)
        delta = 6378.137 * 2.0 ** -23 * np.tan(d / 6378.137 / 2) + 1e-9 * d
        assert abs(m["Mean_km_error"] - totals["Mean_km_error"][i, j, r]) <= delta.mean() + 1e-12 * d.mean(), (i, j, r)
        score = lambda km: np.round(5000 * np.exp(-km / 1492.7))
        assert abs(m["Geoguessr_score"] - totals["Geoguessr_score"][i, j, r]) <= (score(d - delta) - score(d + delta)).mean() + slack, (i, j, r)
    # pass 2 holds pass 1's best point, strictly finer temperatures and the +-3 topks
    _, topks2, temps2, max_kms2, _ = fitted["calls"][1]
    i, j, r = F.choose(totals, (topks, temps, max_kms), "score", cur)
    assert topks[i] in topks2 and temps[j] in temps2 and max_kms2 == max_kms and len(temps2) == 17 and len(topks2) <= 7


def test_reported_heldout_metrics_equal_a_fresh_forward(fitted):
    from pigeon_amd import hip_ops
    fit, held = fitted["fit"], fitted["held"]
    emb, init, cells, probs = fitted["cand"]
    assert list(held[:4]) == [False, True, False, True]
    for name, settings in (("fitted", fit.settings), ("current", (fit.current["topk"], fit.current["temperature"], fit.current["max_refinement"]))):
        reported = fit.heldout_metrics[name]
        m, choice, _ = forward_metrics(fitted, held, settings)
        for key in ("Mean_km_error", "Geoguessr_score"):
            assert close(float(m[key]), reported[key]), (name, key, m[key], reported[key])
        for km in (1, 5, 10, 25, 50, 100, 200, 750, 1000, 2500):
            assert round(float(m[f"Under_{km}_km"]) * 256) == round(reported[f"Under_{km}_km"] * 256), (name, km)
        assert (choice != 0).sum() == round(reported["Changed"] * 256)
        # the vetoed rows: the refined candidate of pg_refine_forward_ex, its distance by torch on the host
        idx = torch.from_numpy(np.nonzero(held)[0]).to(DEV)
        topk, T, km = settings
        _, _, _, refined, scratch = hip_ops.refine_forward_ex(fitted["refiner"]._device_bank(torch.device(DEV)), emb[idx].contiguous(),
                                                              init[idx].contiguous(), cells[idx].contiguous(), probs[idx].contiguous(),
                                                              int(topk), int(topk), float(T), float(km))
        d = R.veto_distances(init[idx].cpu().numpy(), scratch[:, :, 1:3].cpu().numpy())[np.arange(256), refined.cpu().numpy()]
        assert not (math.isfinite(km) and (np.abs(d - km) <= 1e-6 * km).any())   # no row sits on the threshold
        assert (d > km).sum() == round(reported["Vetoed"] * 256)


def build_model(gp, head):
    from pigeon_amd.super_guessr import SuperGuessr
    m = SuperGuessr(None, panorama=True, hierarchical=False, freeze_base=True, yfcc=False, num_candidates=50, geocell_path=gp)
    m.load_state(head)
    return m.to(DEV).eval()


def dataset_of(fitted):
    from pigeon_amd.train import ColumnDataset
    n = 96
    return ColumnDataset(embedding=fitted["emb"][:n].contiguous(), labels=fitted["labels"][:n].contiguous(),
                         labels_clf=torch.zeros(n, dtype=torch.int64))


def test_sidecar_through_evaluate_and_the_server_builder(fitted, monkeypatch, capsys):
    from pigeon_amd import evaluate as E, serve
    from pigeon_amd.proto_refiner import HostBank, ProtoRefiner
    fit, bank = fitted["fit"], fitted["refiner"].host_bank
    seen = {}
    real = E.evaluate_model

    def spy(model, dataset, metrics, train_args, refiner, **kw):
        seen["refiner"] = refiner
        return real(model, dataset, metrics, train_args, refiner, **kw)

    monkeypatch.setattr(E, "evaluate_model", spy)
    data = dataset_of(fitted)
    got = E.evaluate(fitted["head"], data, yfcc=False, landmarks=False, base_model=None, geocell_path=fitted["gp"], bank=bank,
                     refiner_settings=fitted["sidecar"])
    out = capsys.readouterr().out
    r = seen["refiner"]
    assert (r.topk, r._temperature_value(), float(r.max_refinement)) == fit.settings
    assert f"Refiner settings: topk {fit.topk}, temperature {fit.temperature:.6g}" in out
    hand = ProtoRefiner(fit.topk, False, fit.max_refinement, temperature=fit.temperature, bank=bank)
    want = real(build_model(fitted["gp"], fitted["head"]), data, E.compute_geoguessr_metrics, None, hand)
    assert torch.equal(torch.from_numpy(got["preds"]), torch.from_numpy(want["preds"]))
    assert torch.equal(torch.from_numpy(got["preds_geocells"]), torch.from_numpy(want["preds_geocells"]))
    assert got["Geoguessr_score"] == want["Geoguessr_score"]
    # the three numbers on the command line do the same
    spec = f"{fit.topk},{fit.temperature!r},{fit.max_refinement!r}"
    again = E.evaluate(fitted["head"], data, yfcc=False, landmarks=False, base_model=None, geocell_path=fitted["gp"], bank=bank, refiner_settings=spec)
    assert np.array_equal(again["preds"], got["preds"])
    with pytest.raises(ValueError, match="candidates"):
        E.evaluate(fitted["head"], data, yfcc=False, landmarks=False, base_model=None, geocell_path=fitted["gp"], bank=bank, refiner_settings="34,1,10")
    # the server's builder: a packed bank, the sidecar
    packed = str(fitted["tmp"] / "bank.npz")
    HostBank(**{f: getattr(bank, f) for f in HostBank.FIELDS}).save(packed)
    model = build_model(fitted["gp"], fitted["head"])
    args = serve._arg_parser().parse_args(["--protos", packed, "--refiner", fitted["sidecar"]])
    served = serve.build_refiner(args, model)
    assert (served.topk, served._temperature_value(), float(served.max_refinement)) == fit.settings
    emb, init, cells, probs = fitted["cand"]
    a = served(embedding=emb[:64], initial_preds=init[:64], candidate_cells=cells[:64], candidate_probs=probs[:64], quiet=True)
    b = hand(embedding=emb[:64], initial_preds=init[:64], candidate_cells=cells[:64], candidate_probs=probs[:64], quiet=True)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    plain = serve.build_refiner(serve._arg_parser().parse_args(["--protos", packed]), model)
    assert (plain.topk, plain._temperature_value(), plain.max_refinement) == (5, float(np.float32(1.6)), 1000)        # the constructor defaults
    assert serve.build_refiner(serve._arg_parser().parse_args([]), model) is None


def test_a_sidecar_for_another_head_is_refused(fitted):
    from pigeon_amd import evaluate as E, refiner_fit as F
    from pigeon_amd.temperature import planted_head
    other = build_model(fitted["gp"], fitted["head"])
    planted_head(other, SEED + 1)
    with pytest.raises(ValueError) as e:
        F.load(fitted["sidecar"], other, fitted["refiner"])
    ours = F.fingerprints(other, fitted["refiner"])["head"]["weight"]
    theirs = F.fingerprints(fitted["model"], fitted["refiner"])["head"]["weight"]
    assert ours != theirs and ours in str(e.value) and theirs in str(e.value)
    other_head = str(fitted["tmp"] / "other.model")
    torch.save(other.state_dict(), other_head)
    with pytest.raises(ValueError, match="fitted for a head"):
        E.evaluate(other_head, dataset_of(fitted), yfcc=False, landmarks=False, base_model=None, geocell_path=fitted["gp"],
                   bank=fitted["refiner"].host_bank, refiner_settings=fitted["sidecar"])
    assert F.load(fitted["sidecar"], fitted["model"], fitted["refiner"]) == fitted["fit"]


def run_main(argv):
    import contextlib
    import importlib
    import io
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    old, out = sys.argv, io.StringIO()
    sys.argv = ["run.py"] + argv
    try:
        import run
        importlib.reload(run)                                 # argparse is module level, as in the reference
        torch.manual_seed(0)
        with contextlib.redirect_stdout(out):
            results = run.main()
        return results, out.getvalue()
    finally:
        sys.argv = old


def same_value(a, b):
    if isinstance(b, (str, tuple, list, dict)) or b is None:
        return a == b
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def test_without_the_flag_evaluate_is_unchanged():
    """`run.py evaluate` without --refiner builds ProtoRefiner(40, False, 100000, temperature=0.6) over the synthetic bank, as it always
    did: no settings line, and the results equal those of the same literals given through the flag, key for key."""
    command = ["evaluate", "none", "--synthetic", "16", "--layers", "2", "--geocells", "300"]
    plain, plain_out = run_main(command)
    same, same_out = run_main(command + ["--refiner", "40,0.6,100000"])
    assert "Refiner settings" not in plain_out and "Refiner settings: topk 40, temperature 0.6, max_refinement 100000 km" in same_out
    assert "\ttopk\t\t= 40" in plain_out and "\ttemperature\t= 0.6" in plain_out and "\tmax_refinement\t= 100000" in plain_out
    assert set(plain) == set(same)
    for k, v in plain.items():
        if k != "exact_passes":
            assert same_value(same[k], v), k
