"""The guess by expected score without a GPU: tests/_bestref.py is pinned against mpmath, its comparator is shown to reject the
mistakes it is for, and the built library's plan and refusals are checked (host arithmetic only: no HIP call is reached)."""
import base64
import ctypes as C
import io
import re
from collections import namedtuple

import numpy as np
import pytest
import torch

import _bestref as R
import _georef as G
import _spreadref as S


# ================================================================================================================ the restatement
def _mp_expectation(logits, cen, pt, objective):
    """one row, one candidate in mpmath at 50 digits"""
    import mpmath as mp
    mp.mp.dps = 50
    l = [mp.mpf(float(v)) for v in logits]
    m = max(l)
    w = [mp.exp(v - m) for v in l]
    rad = mp.pi / 180
    Rk = mp.mpf(6378137) / 1000
    terms = []
    for c in range(len(l)):
        lng1, lat1, lng2, lat2 = (mp.mpf(float(v)) * rad for v in (pt[0], pt[1], cen[c, 0], cen[c, 1]))
        a = mp.sin((lat1 - lat2) / 2) ** 2 + mp.cos(lat1) * mp.cos(lat2) * mp.sin((lng1 - lng2) / 2) ** 2
        d = 2 * Rk * mp.asin(mp.sqrt(a))
        terms.append(w[c] * (d if objective == "km" else 5000 * mp.exp(-d / mp.mpf("1492.7"))))
    return mp.fsum(terms) / mp.fsum(w)


@pytest.mark.parametrize("objective", R.OBJECTIVES)
@pytest.mark.parametrize("C_cells,M,seed", [(3, 9, 0), (65, 8, 1), (257, 10, 2)])
def test_restatement_against_mpmath(C_cells, M, seed, objective):
    logits, cen = S.gaussian_logits(2, C_cells, seed), S.centroids_of(C_cells, seed)
    cand = R.candidates_of(M, seed, cen)                             # poles, antimeridian, a centroid itself
    t = R.truth(logits, cen, cand, objective)
    want = np.array([[float(_mp_expectation(logits[b], cen, cand[j], objective)) for j in range(M)] for b in range(2)])
    assert (np.abs(want - t["E"]) <= 4 * G.EPS * np.abs(want) + 1e-11).all()       # (1e-11 km: a candidate ON a centroid, d ~ 0)
    for b in range(2):
        order = np.argsort(-want[b] if objective == "score" else want[b], kind="stable")
        assert t["best"][b] == order[0] and t["second"][b] == order[1] and t["tight"][b]


def test_restatement_nan_rules_and_ties():
    cen = S.centroids_of(6, 9)
    cand = R.candidates_of(8, 9, cen)
    logits = np.zeros((5, 6), dtype=np.float32)
    logits[1, 2] = np.nan
    logits[2, 0] = np.inf
    logits[3, :] = -np.inf
    logits[4, 1:] = -np.inf                                          # one cell of weight 1: E is the table's column
    cand[5] = (np.nan, 3.0)
    cand[7] = cand[6]                                                # an exact tie
    t = R.truth(logits, cen, cand, "score")
    assert np.isnan(t["E"][1:4]).all() and (t["best"][1:4] == -1).all() and (t["second"][1:4] == -1).all()
    assert np.isnan(t["E"][:, 5]).all() and not np.isnan(np.delete(t["E"][[0, 4]], 5, axis=1)).any()
    assert (t["best"][[0, 4]] >= 0).all() and (t["best"] != 5).all()
    want = R.table_np(cand, cen, "score")[:, 0]
    assert np.allclose(np.delete(t["E"][4], 5), np.delete(want, 5), rtol=1e-12, atol=0)
    assert t["E"][0, 6] == t["E"][0, 7]
    one = R.truth(logits[:1], cen, cand[:1], "km")                   # one candidate: nothing to confuse it with
    assert one["best"][0] == 0 and one["second"][0] == -1 and one["tight"][0] and one["gap"][0] == np.inf


@pytest.mark.parametrize("B,C_cells,M", [(5, 65, 97), (3, 97, 65), (4, 257, 33)])
def test_plain_implementation_passes_and_nothing_is_loose(B, C_cells, M):
    """Gaussian logits of scale 1, 3 and 6, both objectives: 0 loose rows in the restatement alone, and a straightforward fp64
    implementation of the table route inside every bound"""
    for seed, sigma in ((0, 1.0), (1, 3.0), (2, 6.0)):
        logits, cen = S.gaussian_logits(B, C_cells, seed, sigma), S.centroids_of(C_cells, seed)
        cand = R.candidates_of(M, seed, cen)
        for objective in R.OBJECTIVES:
            t = R.truth(logits, cen, cand, objective)
            assert t["tight"].all(), t["gap"].min()
            got = R.plain(logits, R.table_np(cand, cen, objective), maximize=objective == "score")
            errors, loose, worst = R.compare(t, *got)
            assert not errors and loose == 0 and worst < 1, errors[:3]
            assert loose <= R.loose_allowed(t)


# ================================================================================================================ planted mistakes
def _mistake_inputs():
    B, C_cells, M = 4, 96, 96                                        # square: a transposed table has the right shape
    cen = S.centroids_of(C_cells, 5)
    logits = S.gaussian_logits(B, C_cells, 5, 2.0)
    cand = R.candidates_of(M, 5, cen)
    cand[7] = cen[10]
    cand[40] = cand[7]                                               # an exact tie, in two different tiles of 32 candidates ...
    logits[0, 10] = 12.0                                             # ... and row 0's best
    cand[50] = (np.nan, 1.0)                                         # a candidate that may never win
    logits[2, 33] = np.nan                                           # a row that may poison nothing: row 3 is its neighbour
    return logits, cen, cand


@pytest.mark.parametrize("mistake", R.MISTAKES)
def test_comparator_rejects(mistake):
    logits, cen, cand = _mistake_inputs()
    t = R.truth(logits, cen, cand, "score")
    assert t["best"][0] == 7 and t["second"][0] == 40 and not t["tight"][0] and t["tight"][[1, 3]].all() and t["best"][2] == -1
    tab = R.table_np(cand, cen, "score")
    ok, loose, _ = R.compare(t, *R.plain(logits, tab))
    assert not ok and loose == 1, ok[:3]
    errors, _, _ = R.compare(t, *R.plain(logits, tab, mistake=mistake))
    assert errors, f"{mistake} went through"
    named = [e for e in errors if re.match(r"row \d+ candidate -?\d+ (expected|best_idx|best_value)", e)]
    assert named == errors, errors[:3]
    if mistake == "last_on_tie":
        assert errors == ["row 0 candidate 40 best_idx: the first best of the returned expected row is candidate 7"]
    if mistake == "nan_candidate_wins":
        assert all(" candidate 50 " in e for e in errors) and {int(e.split()[1]) for e in errors} == {0, 1, 3}
    if mistake == "poisoned_neighbour":
        assert {int(e.split()[1]) for e in errors} == {3}
    if mistake == "min_for_max":
        assert all("best_idx" in e for e in errors) and len(errors) >= 3
    if mistake in ("dropped_k_step", "doubled_k_step", "unnormalised_weights", "neighbour_row", "candidate_shifted_by_a_tile",
                   "transposed_table"):
        assert any(" expected: " in e for e in errors), errors[:3]


def test_comparator_accepts_the_runner_up_only_where_loose():
    logits, cen, cand = _mistake_inputs()
    t = R.truth(logits, cen, cand, "score")
    idx, val, exp = R.plain(logits, R.table_np(cand, cen, "score"))
    swapped = exp.copy()
    swapped[0, 7] = np.nextafter(exp[0, 7], 0.0)                     # one ulp: inside the bound, and candidate 40 is now the first best
    idx2 = idx.copy(); idx2[0] = 40
    val2 = val.copy(); val2[0] = swapped[0, 40]
    assert not R.compare(t, idx2, val2, swapped)[0]                  # row 0 is loose: the runner-up passes
    swapped[1, t["best"][1]] = np.nextafter(exp[1, t["best"][1]], 0.0)
    val2[1] = swapped[1, t["best"][1]]
    assert not R.compare(t, idx2, val2, swapped)[0]                  # row 1 is tight: one ulp moves nothing
    idx2[1] = t["second"][1]
    val2[1] = swapped[1, idx2[1]]
    errors = R.compare(t, idx2, val2, swapped)[0]
    assert errors and all(e.startswith("row 1 ") for e in errors)
    assert R.loose_allowed(t) == 0                                   # one loose row of four is over the 1 % cap


# ================================================================================================================ the library, no GPU
FAKE = C.c_void_p(0x1000)                                            # never dereferenced: every call below returns before any HIP call
NULL = C.c_void_p(0)


def _best(lib, B=2, Cn=8, M=5, logits=FAKE, table=FAKE, idx=FAKE, val=FAKE, exp=NULL):
    rc = lib.pg_guess_best(logits, B, Cn, table, M, 1, idx, val, exp, NULL)
    return rc, lib.pg_last_error().decode()


def _table(lib, M=5, Cn=8, kind=1, cand=FAKE, cen=FAKE, table=FAKE):
    rc = lib.pg_score_table(cand, M, cen, Cn, kind, table, NULL)
    return rc, lib.pg_last_error().decode()


def test_refusals_before_any_hip_call(hip_lib):
    for kw, word in ((dict(Cn=0), "C must be"), (dict(Cn=-3), "C must be"), (dict(B=-1), "B ="), (dict(M=-1), "M ="),
                     (dict(B=70000, M=70000), "B * M"), (dict(logits=NULL), "logits"), (dict(table=NULL), "table"),
                     (dict(idx=NULL), "best_idx"), (dict(val=NULL), "best_value")):
        rc, msg = _best(hip_lib, **kw)
        assert rc == -1 and msg.startswith("guess_best:") and word in msg, (kw, rc, msg)
    for kw, word in ((dict(Cn=0), "C must be"), (dict(M=-1), "M ="), (dict(kind=2), "kind"), (dict(kind=-1), "kind"),
                     (dict(cand=NULL), "candidates"), (dict(cen=NULL), "centroids"), (dict(table=NULL), "table")):
        rc, msg = _table(hip_lib, **kw)
        assert rc == -1 and msg.startswith("score_table:") and word in msg, (kw, rc, msg)


def test_empty_batches_are_noops(hip_lib):
    every_null = dict(logits=NULL, table=NULL, idx=NULL, val=NULL)
    assert _best(hip_lib, B=0, **every_null)[0] == 0
    assert _best(hip_lib, M=0, **every_null)[0] == 0
    assert _best(hip_lib, B=0, Cn=0, **every_null)[0] == -1          # the scalars are checked first, whatever the batch
    assert _table(hip_lib, M=0, cand=NULL, cen=NULL, table=NULL)[0] == 0


def test_plan(hip_lib):
    from pigeon_amd import hip_ops
    ceil = lambda a, b: -(-a // b)                                   # noqa: E731
    for B, Cn, M in ((1, 1, 1), (3, 65, 2), (17, 257, 257), (128, 2076, 2076), (128, 11000, 11000), (1, 5, 40000), (300, 9601, 2077)):
        p = hip_ops.guess_best_plan(B, Cn, M)
        rt, ct = p["rows_per_tile"], p["candidates_per_tile"]
        assert p["form"] == (1 if ceil(B, 64) * ceil(M, 64) >= 256 else 0)
        assert (rt, ct) == ((64, 64) if p["form"] else (32, 32))
        assert p["candidate_tiles"] == ceil(M, ct) and p["workgroups"] == ceil(B, rt) * ceil(M, ct)
        assert p["cells_per_step"] % 4 == 0 and p["threads"] == 256
        need = 8 * B * Cn + 8 * B + 12 * B * p["candidate_tiles"]    # weights, Z, one (value, index) partial per row and tile
        assert need <= p["scratch_bytes"] <= need + 4 * 256
    product = hip_ops.guess_best_plan(128, 2076, 2076)
    assert product["workgroups"] >= 256                              # the product's shape gives every CU of an MI355X a workgroup
    assert hip_ops.guess_best_plan(128, 2076, 2076)["form"] == 0 and hip_ops.guess_best_plan(128, 11000, 11000)["form"] == 1
    edge = 64 * 255                                                  # one row tile: the switch sits between 255 and 256 tiles of 64
    assert hip_ops.guess_best_plan(1, 7, edge)["form"] == 0 and hip_ops.guess_best_plan(1, 7, edge + 1)["form"] == 1
    assert hip_ops.guess_best_plan(0, 7, 5)["scratch_bytes"] == 0 and hip_ops.guess_best_plan(4, 7, 0)["scratch_bytes"] == 0
    assert hip_ops.guess_best_plan(2 ** 20, 2 ** 20, 2 ** 11 - 1)["scratch_bytes"] == 2 ** 31 - 1         # saturates
    out = (C.c_int32 * 8)()
    for args, word in (((2, 0, 5), "C must be"), ((-1, 3, 5), "B ="), ((2, 3, -5), "M ="), ((70000, 3, 70000), "B * M")):
        assert hip_lib.pg_guess_best_plan(*args, out) == -1
        msg = hip_lib.pg_last_error().decode()
        assert msg.startswith("guess_best_plan:") and word in msg
    assert hip_lib.pg_guess_best_plan(2, 3, 5, None) == -1 and "out" in hip_lib.pg_last_error().decode()


def test_front_end_refuses_by_name(hip_lib):
    from pigeon_amd import hip_ops, _lib
    f64 = dict(dtype=torch.float64)
    with pytest.raises(_lib.PigeonHipError, match="device tensor"):
        hip_ops.guess_best(torch.zeros(2, 8), torch.zeros(5, 8, **f64))
    with pytest.raises(_lib.PigeonHipError, match="device tensor"):
        hip_ops.score_table(torch.zeros(5, 2, **f64), torch.zeros(8, 2, **f64))
    with pytest.raises(_lib.PigeonHipError, match="kind"):
        hip_ops.score_table(torch.zeros(5, 2, **f64), torch.zeros(8, 2, **f64), kind="miles")


def test_best_guess_metrics_on_planted_arrays():
    from pigeon_amd.evaluate import best_guess_metrics, geoguessr_score, haversine_np
    best = np.array([[0.0, 0.0], [10.0, 10.0], [20.0, -5.0]])
    labels = np.array([[0.0, 0.0], [10.0, 11.0], [25.0, -5.0]])
    m = best_guess_metrics(best, haversine_np, labels, [True, False, False])
    d = haversine_np(best, labels)
    assert m["Mean_km_error_best"] == np.mean(d) and m["Median_km_error_best"] == np.median(d)
    assert m["Geoguessr_score_best"] == geoguessr_score(d) and m["Best_guess_changed"] == 1 / 3
    assert d[0] == 0 and 100 < d[1] < 120


# ================================================================================================================ serving keys
TopK = namedtuple("TopK", ["values", "indices"])
BestGuess = namedtuple("BestGuess", "index point expected incumbent_expected taken")


class StubModel:
    def __call__(self, pixel_values=None):
        llh = torch.tensor([[12.5, -33.25]], dtype=torch.float64)
        return llh, TopK(torch.ones(1, 5), torch.arange(5)[None]), torch.zeros(1, 4, 1024)


class StubBestModel(StubModel):
    def __init__(self, taken):
        self.asked, self.taken = None, taken

    def best_guess(self, candidates=None, objective="score", incumbent=None, state=None):
        self.asked = (objective, incumbent.clone())
        taken = torch.tensor([self.taken])
        point = torch.where(taken[:, None], torch.tensor([[100.0, 45.0]], dtype=torch.float64), incumbent)
        return BestGuess(torch.tensor([3]), point, torch.tensor([3000.5], dtype=torch.float64),
                         torch.tensor([2500.25], dtype=torch.float64) if self.taken else torch.tensor([3000.5], dtype=torch.float64), taken)


class StubRefiner:
    def __call__(self, embedding=None, initial_preds=None, candidate_cells=None, candidate_probs=None):
        return None, initial_preds.to(torch.float32) + torch.tensor([[1.0, 2.0]]), torch.zeros(1, dtype=torch.int64)


def _body():
    from PIL import Image
    img = Image.fromarray(np.random.default_rng(1).integers(0, 255, (60, 80, 3), dtype=np.uint8))
    buf = io.BytesIO()
    img.save(buf, format="PNG")
    return {"gameID": "g", "roundID": 1, "image": "data:image/png;base64," + base64.b64encode(buf.getvalue()).decode()}


def test_serving_keys_with_stub_models():
    from starlette.testclient import TestClient
    from pigeon_amd import serve
    from pigeon_amd.clip_embedder import clip_preprocess
    model = StubBestModel(taken=True)
    plain = TestClient(serve.make_app(model, preprocess=clip_preprocess)).post("/api/v1/predict", json=_body()).json()["results"]
    assert set(plain) == {"lat", "lng"} and model.asked is None      # nothing is computed unless asked for
    res = TestClient(serve.make_app(model, StubRefiner(), preprocess=clip_preprocess, best_guess=True)).post("/api/v1/predict", json=_body())
    assert res.status_code == 200
    r = res.json()["results"]
    assert (r["lat"], r["lng"]) == (45.0, 100.0)                     # what the extension reads: the chosen point
    assert (r["argmax_lat"], r["argmax_lng"]) == (-31.25, 13.5)      # the former answer: the REFINED point
    assert r["guess_expected_score"] == 3000.5 and r["guess_changed"] is True
    objective, inc = model.asked
    assert objective == "score" and inc.dtype == torch.float64 and inc.tolist() == [[13.5, -31.25]]
    kept = StubBestModel(taken=False)
    r = serve.predict_panorama(serve.panorama_from_request(_body(), False), kept, preprocess=clip_preprocess, best_guess=True)
    assert (r["lat"], r["lng"]) == (r["argmax_lat"], r["argmax_lng"]) == (-33.25, 12.5)
    assert r["guess_changed"] is False and r["guess_expected_score"] == 3000.5
    with pytest.raises(ValueError, match="best_guess"):
        serve.make_app(StubModel(), preprocess=clip_preprocess, best_guess=True)
    with pytest.raises(ValueError, match="best_guess"):
        serve.predict_panorama([None] * 4, StubModel(), best_guess=True)
