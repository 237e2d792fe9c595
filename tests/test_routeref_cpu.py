"""tests/_routeref.py without a GPU: on embeddings drawn under the error model (a common part that dominates, as a tower's embeddings
have; an error of 5e-5 relative in a random direction) the planted head has the properties tests/test_gpu_embedding_route.py relies
on, in float64 on the fp32 weights -- and `check_preconditions` notices when it has not."""
import numpy as np

import _routeref as rr

N, D = 32, 1024


def _embeddings(seed=0, rho=5e-5):
    rng = np.random.default_rng(seed)
    exact = 8.8 * rng.standard_normal(D) / np.sqrt(D) + 0.9 * rng.standard_normal((N, D)) / np.sqrt(D)
    exact = exact.astype(np.float32).astype(np.float64)                       # what a device hands back
    eps = rng.standard_normal((N, D)) / np.sqrt(D) * rho * np.linalg.norm(exact, axis=1, keepdims=True)
    return exact, exact + eps, eps


def test_planted_head_has_the_stated_properties():
    exact, fast, eps = _embeddings()
    h = rr.plant_head(exact, eps, seed=0)
    assert h["W"].shape == (2 * N + 32, D) and h["W"].dtype == np.float32 and h["bias"].dtype == np.float32
    assert rr.check_preconditions(exact, fast, h) == []
    ref = rr.reference_top1(exact, h)
    assert ref.tolist() == h["a"].tolist()
    top_fast = np.argmax(rr.logits64(fast, h), axis=1)
    assert (top_fast == np.where(h["f"] < 1, h["b"], h["a"])).all() and (h["f"] < 1).sum() == 8
    # the margin of the ROUNDED weights is the planted one, f_i times what eps_i moves it by
    assert np.allclose(h["m"], h["m_planted"], rtol=1e-3) and np.allclose(h["m_planted"], h["f"] * h["shift"])
    moved = ((h["W"][h["b"]].astype(np.float64) - h["W"][h["a"]].astype(np.float64)) * eps).sum(axis=1)
    small = h["f"] <= 64                                                       # (the u_i term of D_i adds f_i * 1.5e-5 of it: visible from f = 1024)
    assert np.allclose(moved[small], h["shift"][small], rtol=2e-2) and (moved[small] > 0).all()   # towards b_i, by L |o_i . eps_i|
    # the directions: unit, orthogonal to EVERY exact embedding, typical draws against eps
    assert np.allclose(np.linalg.norm(h["o"], axis=1), 1.0) and np.abs(h["o"] @ exact.T).max() < 1e-9
    assert np.abs(h["u"] @ exact.T - np.diag(h["r"])).max() < 1e-9 and (h["r"] > 0).all()
    assert 1.5 < rr.random_direction_score(h, eps) < 4.0
    # fp32 can resolve every planted margin: at least 2^-14 of the row's top logit, and one A where the cap does not bind
    top = rr.logits64(exact, h)[np.arange(N), h["a"]]
    assert (h["m"] >= top * 2.0 ** -14 * (1 - 1e-2)).all() and np.abs(rr.logits64(exact, h)).max() < 1e3
    assert (h["A"] <= h["A"].max()).all() and (h["A"][h["f"] >= 65536] == h["A"].max()).all()


def test_preconditions_notice_a_head_that_is_not_the_planted_one():
    exact, fast, eps = _embeddings(seed=1)
    h = rr.plant_head(exact, eps, seed=3)
    assert rr.check_preconditions(exact, fast, h) == []
    # the error pushes AWAY from b_i: nothing flips
    bad = rr.check_preconditions(exact, exact - eps, h)
    assert len(bad) == 8 and all("fast top-1" in s for s in bad)
    # a and b swapped on one row
    g = dict(h, a=h["a"].copy(), b=h["b"].copy())
    g["a"][5], g["b"][5] = h["b"][5], h["a"][5]
    assert any(s.startswith("row 5 ") and "exact ranks" in s for s in rr.check_preconditions(exact, fast, g))
    # a background cell close below one row's pair
    g = dict(h, W=h["W"].copy(), bias=h["bias"].copy())
    g["W"][2 * N], g["bias"][2 * N] = h["W"][h["b"][12]] * np.float32(1 - 1e-3), h["bias"][h["b"][12]]      # 16 planted margins below b_12
    assert any(s.startswith("row 12 ") and "third cell" in s for s in rr.check_preconditions(exact, fast, g))
    # logits out of range
    g = dict(h, W=h["W"] * 64)
    assert any("logits reach" in s for s in rr.check_preconditions(exact, fast, g))
