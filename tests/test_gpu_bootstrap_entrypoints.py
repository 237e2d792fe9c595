"""The bootstrap at the entry points (run with -m gpu on an MI355X): `run.py evaluate ... --bootstrap R --guess expected-score` against
the same command without the flag, `evaluate_model(bootstrap=R)` with a bank-backed `neighbours=K` on the embedding route, and the
standalone command line on an .npz.  The intervals are compared with tests/_bootref.py on the columns the entry point collected."""
import os
import sys

import numpy as np
import pytest
import torch

import _bootref as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
R = 200
COMMAND = ["evaluate", "none", "--synthetic", "64", "--layers", "2", "--guess", "expected-score"]


def reference_table(cols, stats, R, seed, level):
    """`pigeon_amd.bootstrap.summarise` fed with the restatement's replicates."""
    from pigeon_amd import bootstrap as boot
    names = list(cols)
    x = np.stack([np.asarray(cols[n], dtype=np.float64) for n in names])
    m = B.means(x, R, seed)
    q = B.quantiles(x, R, seed, (0.5,))[:, :, 0]
    reps = {}
    for key, s in stats.items():
        one = m if s[0].startswith("mean") else q
        reps[key] = one[:, names.index(s[1])] - (one[:, names.index(s[2])] if s[0].endswith("_diff") else 0.0)
    return boot.summarise({k: np.asarray(v) for k, v in cols.items()}, stats, reps, level)


def same_value(a, b):
    if isinstance(b, (str, tuple, list, dict)) or b is None:
        return a == b
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


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


@pytest.fixture(scope="module")
def runs():
    from pigeon_amd import _lib, bootstrap as boot
    _lib.require_gpu()
    seen = {}
    real = boot.metric_columns

    def spy(*a, **k):
        seen["columns"], seen["stats"] = real(*a, **k)
        return seen["columns"], seen["stats"]

    plain, plain_out = run_main(COMMAND)
    boot.metric_columns = spy
    try:
        got, got_out = run_main(COMMAND + ["--bootstrap", str(R)])
    finally:
        boot.metric_columns = real
    return dict(plain=plain, plain_out=plain_out, got=got, got_out=got_out, **seen)


def test_without_the_flag_nothing_changes(runs):
    plain, got = runs["plain"], runs["got"]
    assert "bootstrap" not in plain and "bootstrap_level" not in plain and "bootstrap" not in runs["plain_out"]
    assert set(got) == set(plain) | {"bootstrap", "bootstrap_level"}
    for k, v in plain.items():
        if k == "exact_passes":
            continue
        assert same_value(got[k], v), k
    # the metrics line is printed as before, bit for bit
    line = [l for l in runs["plain_out"].splitlines() if l.startswith("{'preds'")]
    assert len(line) == 1 and line[0] in runs["got_out"].splitlines()


def test_the_stored_intervals_equal_the_restatement(runs):
    got, cols, stats = runs["got"], runs["columns"], runs["stats"]
    table = got["bootstrap"]
    assert got["bootstrap_level"] == 0.95
    metrics = [k for k in stats if " - " not in k]
    assert set(metrics) == {k for k in got if k in stats} and "Mean_km_error_best" in metrics and "Best_guess_changed" in metrics
    assert {k for k in table if " - " in k} == {"Mean_km_error_best - Mean_km_error", "Median_km_error_best - Median_km_error",
                                                "Geoguessr_score_best - Geoguessr_score"}
    for k in metrics:
        kind, name = stats[k]
        assert (np.mean(cols[name]) if kind == "mean" else np.median(cols[name])) == got[k] == table[k]["estimate"], k
    want = reference_table(cols, {k: stats[k] for k in table}, R, 0, 0.95)
    assert table == want, {k: (table[k], want[k]) for k in table if table[k] != want[k]}
    constant = [k for k in metrics if np.ptp(np.asarray(cols[stats[k][1]], dtype=np.float64)) == 0]
    assert constant, "a random head is within 1 km of nothing: Under_1_km is a constant column"
    for k, row in table.items():
        assert row["lo"] <= row["hi"], k
        if k in constant:
            # 64 items: a thread adds at most one, and the butterfly of equal values only doubles, so every replicate is the constant
            # itself (numpy's own mean of 64 equal values, the estimate, may be an ulp off: its partial sums 3 x, 5 x, ... are rounded)
            assert row["lo"] == row["hi"] == float(np.asarray(cols[stats[k][1]], dtype=np.float64)[0]) and row["se"] == 0.0, k
            assert abs(row["estimate"] - row["lo"]) <= 2.0 ** -50 * abs(row["lo"]), k
    assert 0.0 <= table["Geoguessr_score_best - Geoguessr_score"]["share_le_zero"] <= 1.0


def test_the_intervals_are_printed_with_the_differences_below(runs):
    from pigeon_amd import bootstrap as boot
    out, table = runs["got_out"], runs["got"]["bootstrap"]
    assert boot.report(table, 0.95) in out
    lines = out.splitlines()
    at = lines.index("bootstrap: 95 % percentile intervals")
    row = table["Mean_km_error"]
    assert lines[at + 1] == f"  Mean_km_error: {row['estimate']:.6g} [{row['lo']:.6g}, {row['hi']:.6g}]"
    below = lines.index("  paired differences (the same resample on both sides):")
    assert below > at and any(l.startswith("  Median_km_error_best - Median_km_error: ") for l in lines[below:])


def test_evaluate_model_with_neighbours_and_another_seed():
    from pigeon_amd import synthetic
    from pigeon_amd.evaluate import compute_geoguessr_metrics, evaluate_model
    from pigeon_amd import bootstrap as boot
    from pigeon_amd.proto_refiner import ProtoRefiner
    from pigeon_amd.super_guessr import SuperGuessr
    import tempfile
    cells, n = 64, 40
    gp = os.path.join(tempfile.mkdtemp(prefix="pigeon_boot_"), "g.csv")
    synthetic.write_geocell_csv(gp, synthetic.make_geocells(cells, seed=0))
    bank = synthetic.make_bank(cells, 9, seed=5, empty_frac=0.1, max_members=6)
    ref = ProtoRefiner(topk=5, max_refinement=1000, temperature=1.6, bank=bank, device=DEV).eval()
    W, b = synthetic.make_head_weights(cells, seed=1)
    m = SuperGuessr(None, panorama=True, freeze_base=True, num_candidates=5, geocell_path=gp)
    with torch.no_grad():
        m.cell_layer.weight.copy_(W * 64.0); m.cell_layer.bias.copy_(b)
    m = m.to(DEV).eval()
    g = torch.Generator().manual_seed(3)
    te = torch.as_tensor(np.asarray(bank.train_emb))
    emb = (te[torch.randint(0, te.shape[0], (n,), generator=g)][:, None, :] + 0.05 * torch.randn((n, 4, 1024), generator=g)).contiguous()
    cen = m.lla_geocells.data.cpu().numpy()
    labels = np.stack([cen[(7 * i) % cells] + [0.3 * i, -0.2 * i] for i in range(n)])
    data = [dict(embedding=emb[i], labels=torch.from_numpy(labels[i]), labels_clf=torch.tensor((7 * i) % cells)) for i in range(n)]

    class Columns(list):
        def __getitem__(self, i):
            return np.stack([np.asarray(d[i]) for d in self]) if isinstance(i, str) else list.__getitem__(self, i)

    kw = dict(refiner=ref, batch_size=16, neighbours=3, best_guess="km")
    plain = evaluate_model(m, Columns(data), compute_geoguessr_metrics, **kw)
    got = evaluate_model(m, Columns(data), compute_geoguessr_metrics, bootstrap=50, bootstrap_seed=(9 << 32) | 1, bootstrap_level=0.8, **kw)
    assert set(got) == set(plain) | {"bootstrap", "bootstrap_level"} and got["bootstrap_level"] == 0.8
    for k, v in plain.items():
        if k != "exact_passes":
            assert same_value(got[k], v), k
    results = (got["preds"], got["preds_geocells"], None, None, None, got["top5_geocells"], labels, np.array([(7 * i) % cells for i in range(n)]),
               None, None, None)
    cols, stats = boot.metric_columns(results, best_LLH=got["best_LLH"], best_taken=got["best_taken"], nn_lnglat=got["nn_lnglat"])
    assert set(stats) == set(got["bootstrap"]) and "Mean_km_error_nn - Mean_km_error" in stats and "NN_beats_model" in stats
    assert got["bootstrap"] == reference_table(cols, stats, 50, (9 << 32) | 1, 0.8)
    for key in ("Mean_km_error_nn", "Median_km_error_best", "NN_beats_model", "Geocell_top5_accuracy"):
        assert got["bootstrap"][key]["estimate"] == got[key]
    with pytest.raises(ValueError, match="metrics"):
        evaluate_model(m, Columns(data), None, refiner=ref, bootstrap=10)
    with pytest.raises(ValueError, match="positive number of replicates"):
        evaluate_model(m, Columns(data), compute_geoguessr_metrics, refiner=ref, bootstrap=0)


def test_the_command_line_on_an_npz(tmp_path, capsys):
    from pigeon_amd import bootstrap as boot
    rng = np.random.default_rng(21)
    km, km_best = rng.gamma(2.0, 300.0, 500), rng.gamma(2.0, 250.0, 500)
    path = str(tmp_path / "columns.npz")
    np.savez(path, km=km, km_best=km_best)
    table = boot.main(["--columns", path, "--mean", "km", "--median", "km", "--diff", "km_best", "km", "--quantile", "km", "0.9", "-R", "300",
                       "--seed", "7", "--level", "0.9"])
    out = capsys.readouterr().out
    stats = {"mean km": ("mean", "km"), "median km": ("median", "km"), "mean km_best - km": ("mean_diff", "km_best", "km"),
             "median km_best - km": ("median_diff", "km_best", "km")}
    want = reference_table({"km": km, "km_best": km_best}, stats, 300, 7, 0.9)
    assert {k: table[k] for k in stats} == want
    q = B.quantiles(km[None, :], 300, 7, (0.9,))[:, 0, 0]
    assert (table["quantile 0.9 km"]["lo"], table["quantile 0.9 km"]["hi"]) == tuple(float(v) for v in np.quantile(q, [(1.0 - 0.9) / 2.0, (1.0 + 0.9) / 2.0]))
    assert table["quantile 0.9 km"]["estimate"] == float(np.quantile(km, 0.9))
    assert boot.report(table, 0.9) in out and "bootstrap: 90 % percentile intervals" in out
    with pytest.raises(SystemExit):
        boot.main(["--columns", path, "--mean", "nothing"])
    with pytest.raises(SystemExit):
        boot.main(["--columns", path])
