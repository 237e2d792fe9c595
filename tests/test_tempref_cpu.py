"""tests/_tempref.py without a GPU: the restatement against mpmath on a handful of rows, the plain fp64 implementation inside the
derived bounds, and every planted mistake rejected at a named row and output."""
import numpy as np
import pytest

import _tempref as T

mpmath = pytest.importorskip("mpmath")

BETAS = [1.0, 1.0 / 64, 64.0, 0.37]


def mp_row(r32, y, beta):
    mp = mpmath.mp
    mp.prec = 200
    l = [mpmath.mpf(float(v)) for v in r32 if v > -np.inf]
    m = max(l)
    xs = [v - m for v in l]
    b = mpmath.mpf(beta)
    ws = [mpmath.exp(b * x) for x in xs]
    Z = mpmath.fsum(ws)
    A = mpmath.fsum(w * x for w, x in zip(ws, xs))
    Q = mpmath.fsum(w * x * x for w, x in zip(ws, xs))
    xy = mpmath.mpf(float(r32[y])) - m
    return {"nll": mpmath.log(Z) - b * xy, "d1": A / Z - xy, "d2": Q / Z - (A / Z) ** 2, "conf": 1 / Z}


def test_restatement_against_mpmath():
    l, y, kinds = T.make_rows(7, 65, seed=1)
    t = T.truth(l, y, BETAS)
    checked = 0
    for n in range(7):
        if t["state"][n] == 2:
            continue
        for k, beta in enumerate(BETAS):
            want = mp_row(l[n], int(y[n]), beta)
            for name in ("nll", "d1", "d2", "conf"):
                got = mpmath.mpf(float(t[name][n, k])) + mpmath.mpf(float(t[name][n, k] - np.longdouble(float(t[name][n, k]))))
                err = abs(got - want[name])
                # the truth's own error must be a small part of the bound it is published with
                assert err <= 0.05 * t[name + "_bound"][n, k] + mpmath.mpf(2) ** -780, (n, kinds[n], k, name, float(err))
                checked += 1
    assert checked >= 6 * len(BETAS) * 4


def test_states_and_nan_rows():
    l, y, kinds = T.make_rows(12, 65, seed=2)
    t = T.truth(l, y, BETAS)
    for n, kind in enumerate(kinds):
        assert (t["state"][n] == 2) == (kind in T.INVALID_KINDS), (n, kind)
        assert np.isnan(t["nll"][n]).all() == (kind in T.INVALID_KINDS)
    tie = kinds.index("tie")
    assert t["state"][tie] == (1 if y[tie] == int(np.argmax(l[tie])) else 0)
    const = kinds.index("constant")
    assert (t["d1"][const] == 0).all() and (t["d2"][const] == 0).all()
    assert np.allclose(t["conf"][const].astype(np.float64), 1 / 65, rtol=1e-15)


@pytest.mark.parametrize("C", [1, 2, 65, 257])
def test_plain_implementation_passes(C):
    l, y, _ = T.make_rows(12, C, seed=3)
    t = T.truth(l, y, BETAS)
    p = T.plain(l, y, BETAS)
    errors, worst = T.compare(t, p["row_stats"], p["conf"], p["state"])
    assert not errors, errors[:5]
    assert worst < 1
    errors, _ = T.compare_totals(t, p["totals"], p["counts"])
    assert not errors, errors[:5]


def mistake_rows():
    """24 rows of 65 cells in every kind, with a row of large logits in front: exp overflows there without the max shift"""
    l, y, kinds = T.make_rows(24, 65, seed=4)
    l[0] = l[0] * 3 + 900
    return l, y, kinds


WHERE = {"no_max_shift": ("row 0 ", " nll"), "temperature_for_beta": ("row 0 beta 1 ", " nll"),
         "beta_missing_in_label_term": ("row 1 beta 1 ", " nll"), "last_maximum": ("row 2 state", ""),
         "masked_weight_one": ("row 4 ", " conf"), "no_squared_mean": ("row 0 ", " d2"),
         "totals_include_invalid": ("totals beta 0 nll", ""), "conf_of_label": ("row 0 ", " conf")}


@pytest.mark.parametrize("mistake", T.MISTAKES)
def test_planted_mistake_is_rejected(mistake):
    l, y, kinds = mistake_rows()
    assert kinds[2] == "tie" and kinds[4] == "neginf_cells" and y[0] != int(np.argmax(l[0])) and y[1] != int(np.argmax(l[1]))
    t = T.truth(l, y, BETAS)
    p = T.plain(l, y, BETAS, mistake=mistake)
    errors, _ = T.compare(t, p["row_stats"], p["conf"], p["state"])
    errors += T.compare_totals(t, p["totals"], p["counts"])[0]
    assert errors, f"{mistake} passed"
    start, end = WHERE[mistake]
    assert any(e.startswith(start) and end in e.split(":")[0] + " " for e in errors), (mistake, errors[:6])


def test_totals_in_order_and_bisection():
    rng = np.random.default_rng(5)
    rs = rng.standard_normal((300, 3, 3))
    st = np.where(np.arange(300) % 3 == 0, 2, 0).astype(np.uint8)
    rs[st == 2] = np.nan
    got = T.totals_in_order(rs, st)
    want = np.where(np.isnan(rs), 0, rs).sum(axis=0)
    assert np.allclose(got, want, rtol=0, atol=1e-12) and np.isfinite(got).all()
    l = (rng.standard_normal((512, 33)) * 2).astype(np.float32)
    y = T.planted_labels(l, 0.7, seed=5)
    b = T.bisect_beta(l, y)
    assert 0.5 < b < 1.0
    assert T.accepts(l, y, b) and not T.accepts(l, y, b * 1.01)


def test_ece_of_a_hand_made_table():
    # two bins: (0.6, 0.667] holds conf 0.65 x 2 with accuracy 0.5; (0.933, 1] holds conf 1.0 x 2 with accuracy 1
    assert T.ece_np([0.65, 0.65, 1.0, 1.0], [1, 0, 1, 1]) == pytest.approx(0.5 * 0.15)
