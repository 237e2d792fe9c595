"""pigeon_amd/temperature.py without a GPU: fit_beta on a numpy stats_fn (a planted beta recovered within 4 standard errors, the pass
budget, the clamped ends, a flat set), the sidecar round trip with an injected fingerprint, the ECE of a hand-made table and the
command line's argument errors."""
import json
import math
import types

import numpy as np
import pytest

import _tempref as T
from pigeon_amd import temperature as tmp

PLANTED = [(4096, 257, 3.0, 0.4), (4096, 257, 1.0, 2.5), (1024, 65, 2.0, 1.0), (300, 1025, 4.0, 0.25)]


def counting(fn):
    calls = []

    def wrapped(betas):
        assert 1 <= len(betas) <= 16 and all(math.isfinite(b) and b > 0 for b in betas)
        calls.append(list(betas))
        return fn(betas)
    return wrapped, calls


@pytest.mark.parametrize("seed", range(4))
def test_a_planted_beta_is_recovered_within_four_standard_errors(seed):
    N, C, scale, beta0 = PLANTED[seed]
    logits = (np.random.default_rng(seed).standard_normal((N, C)) * scale).astype(np.float32)
    labels = T.planted_labels(logits, beta0, seed)
    fn, calls = counting(T.stats_fn_np(logits, labels))
    beta, passes, clamped = tmp.fit_beta(fn)
    assert not clamped and passes == len(calls)
    assert passes <= 16, "the pass budget"
    se = 1.0 / math.sqrt(T.stats_fn_np(logits, labels)([beta])[0, 2])
    print(f"planted {beta0}: fitted {beta!r} in {passes} passes, {(beta - beta0) / se:+.2f} standard errors")
    assert abs(beta - beta0) <= 4 * se
    ref = T.bisect_beta(logits, labels)                              # the reference's own minimiser: plain bisection
    assert abs(beta / ref - 1) <= 2.0 ** -36
    d = T.stats_fn_np(logits, labels)([beta * (1 - 2.0 ** -30), beta * (1 + 2.0 ** -30)])[:, 1]
    assert d[0] < 0 < d[1], "the total first derivative changes sign at the fitted beta"


def test_a_pure_grid_needs_eleven_passes_and_stops_at_the_bracket():
    fn, calls = counting(lambda betas: np.array([[0.0, math.log(b / 0.777), 1.0] for b in betas]))
    beta, passes, clamped = tmp.fit_beta(fn)
    assert passes == 11 and not clamped
    assert abs(beta / 0.777 - 1) <= 2.0 ** -40
    assert calls[0][0] == 1 / 64 and calls[0][-1] == 64 and len(calls[0]) == 16


def test_budget_is_enforced(monkeypatch):
    monkeypatch.setattr(tmp, "MAX_BETAS", 2)                         # two betas a pass shrink the bracket 3-fold: 16 passes are not enough
    with pytest.raises(tmp.FitError, match="16 passes"):
        tmp.fit_beta(lambda betas: np.array([[0.0, math.log(b / 0.777), 1.0] for b in betas]))


def test_clamped_ends_and_flat_set():
    rng = np.random.default_rng(7)
    logits = rng.standard_normal((200, 17)).astype(np.float32)
    right = logits.argmax(axis=1)
    assert tmp.fit_beta(T.stats_fn_np(logits, right)) == (64.0, 1, True)              # separable: ever sharper
    wrong = logits.argmin(axis=1)
    assert tmp.fit_beta(T.stats_fn_np(logits, wrong)) == (1 / 64, 1, True)            # all wrong: ever flatter
    flat = np.full((50, 9), 0.25, dtype=np.float32)
    beta, passes, clamped = tmp.fit_beta(T.stats_fn_np(flat, np.zeros(50, dtype=np.int64)))
    assert (beta, passes, clamped) == (1.0, 1, False)
    assert tmp.fit_beta(T.stats_fn_np(flat, np.zeros(50, dtype=np.int64)), lo=2.0, hi=8.0)[0] == 2.0
    with pytest.raises(ValueError):
        tmp.fit_beta(T.stats_fn_np(flat, np.zeros(50, dtype=np.int64)), lo=2.0, hi=1.0)
    with pytest.raises(tmp.FitError, match="non-finite"):
        tmp.fit_beta(lambda betas: np.full((len(betas), 3), np.nan))


def fake_model(w=1.0):
    t = lambda v: types.SimpleNamespace(data=types.SimpleNamespace(contiguous=lambda: v))
    return types.SimpleNamespace(cell_layer=types.SimpleNamespace(weight=t(("w", w)), bias=t(("b", w))))


def stub_fingerprint(v):
    return (hash(v) & 0xFFFFFFFFFFFFFFFF, 7)


def a_fit():
    conf = np.array([0.65, 0.65, 1.0, 1.0])
    table = tmp.reliability_table(conf, [1, 0, 1, 1])
    return tmp.TemperatureFit(temperature=2.5, beta=0.4, n=4, skipped=1, passes=11, clamped=False, nll_before=1.5, nll_after=1.25,
                              ece_before=0.25, ece_after=tmp.ece_of_table(table), reliability={"accuracy": 0.75, "before": table, "after": table})


def test_sidecar_round_trip_and_refusal(tmp_path):
    path = str(tmp_path / "sub" / "head.temperature.json")
    fit = a_fit()
    assert tmp.save(path, fit, fake_model(), fingerprint=stub_fingerprint) == path
    obj = json.load(open(path))
    for k in ("temperature", "beta", "n", "skipped", "passes", "clamped", "nll_before", "nll_after", "ece_before", "ece_after",
              "reliability", "head_fingerprint"):
        assert k in obj
    assert set(obj["head_fingerprint"]) == {"weight", "bias"}
    assert tmp.load(path, fake_model(), fingerprint=stub_fingerprint) == fit
    assert tmp.resolve(path, fake_model(), fingerprint=stub_fingerprint) == 2.5
    other = fake_model(2.0)
    with pytest.raises(ValueError) as e:
        tmp.load(path, other, fingerprint=stub_fingerprint)
    mine, theirs = tmp.head_fingerprint(other, stub_fingerprint), obj["head_fingerprint"]
    assert mine["weight"] in str(e.value) and theirs["weight"] in str(e.value), "both fingerprints are named"
    assert tmp.resolve("2.5", None) == 2.5 and tmp.resolve(0.5, None) == 0.5
    for bad in ("0", "-1", "nan", "inf", str(tmp_path / "missing.json")):
        with pytest.raises(ValueError):
            tmp.resolve(bad, fake_model(), fingerprint=stub_fingerprint)
    obj["temperature"] = -1.0
    json.dump(obj, open(path, "w"))
    with pytest.raises(ValueError, match="finite positive"):
        tmp.load(path, fake_model(), fingerprint=stub_fingerprint)


def test_ece_of_a_hand_made_table():
    # (0.6, 0.667] holds confidence 0.65 twice at accuracy 0.5; (0.933, 1] holds confidence 1 twice at accuracy 1
    conf, correct = [0.65, 0.65, 1.0, 1.0], [1, 0, 1, 1]
    table = tmp.reliability_table(conf, correct)
    assert len(table) == 15 and [r["n"] for r in table] == [0] * 9 + [2] + [0] * 4 + [2]
    assert table[9]["accuracy"] == 0.5 and table[9]["confidence"] == pytest.approx(0.65) and table[0]["accuracy"] is None
    assert tmp.ece_of_table(table) == pytest.approx(0.5 * 0.15)
    assert tmp.expected_calibration_error(conf, correct) == pytest.approx(T.ece_np(conf, correct))
    # the bins are (j / 15, (j + 1) / 15]: an edge belongs to the bin below it
    assert [r["n"] for r in tmp.reliability_table([1 / 15, 2 / 15 + 1e-12, 0.0], [1, 1, 1])][:3] == [2, 0, 1]
    rng = np.random.default_rng(0)
    c, k = rng.random(1000), rng.random(1000) < 0.5
    assert tmp.expected_calibration_error(c, k) == pytest.approx(T.ece_np(c, k), abs=1e-15)
    assert "CLAMPED" not in tmp.format_fit(a_fit()) and "temperature 2.5" in tmp.format_fit(a_fit())


@pytest.mark.parametrize("argv", [[], ["-o", "t.json"], ["--head", "h.model", "-o", "t.json"], ["-l", "data", "-o", "t.json"],
                                  ["--head", "h.model", "-l", "data"], ["--synthetic", "64", "--head", "h.model", "-o", "t.json"],
                                  ["--synthetic", "-3", "-o", "t.json"], ["--synthetic", "64", "--geocells", "0", "-o", "t.json"],
                                  ["--head", "h.model", "-l", "data", "-o", "t.json", "--save-head", "x"],
                                  ["--synthetic", "64", "--chunk", "0", "-o", "t.json"]])
def test_cli_argument_errors(argv, capsys):
    with pytest.raises(SystemExit) as e:
        tmp.main(argv)
    assert e.value.code == 2
    assert "usage:" in capsys.readouterr().err
