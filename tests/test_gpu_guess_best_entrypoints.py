"""The guess by expected score at the entry points (run with -m gpu on an MI355X), on a 2-layer synthetic tower:
`SuperGuessr.best_guess`, `certain_forward(best_guess=...)`, `evaluate_model(best_guess=...)` and `predict_panorama(best_guess=True)`.
The kernel itself is held to its contract in tests/test_gpu_guess_best.py; here every comparison is against
pigeon_amd.hip_ops.guess_best on the logits and table the entry point must have used, bit for bit."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CELLS = 64


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops, synthetic
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    _lib.require_gpu()
    vit = HipCLIPVisionModel(synthetic.make_vit_weights(seed=0, layers=2), layers=2).to(DEV)
    return dict(ops=hip_ops, syn=synthetic, vit=vit)


def model_of(env, tmp_path, cen=None, name="g.csv", exact_top1=True, gain=64.0, bias=None):
    from pigeon_amd.proto_refiner import ProtoRefiner
    from pigeon_amd.super_guessr import SuperGuessr
    syn = env["syn"]
    cen = syn.make_geocells(CELLS, seed=0) if cen is None else cen
    gp = os.path.join(str(tmp_path), name)
    syn.write_geocell_csv(gp, cen)
    W, b = syn.make_head_weights(CELLS, seed=1)
    m = SuperGuessr(env["vit"], panorama=True, freeze_base=True, num_candidates=5, geocell_path=gp, exact_top1=exact_top1, margin_kappa=3.6,
                    margin_autocalibrate=False, margin_rel_tol=1e-3)
    with torch.no_grad():
        m.cell_layer.weight.copy_(W * gain); m.cell_layer.bias.copy_(b if bias is None else bias)
    m = m.to(DEV).eval()
    ref = ProtoRefiner(topk=5, max_refinement=1000, temperature=1.6, bank=syn.make_bank(CELLS, 9, seed=5, empty_frac=0.1, max_members=6),
                       device=DEV).eval()
    return m, ref


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def want_guess(env, m, logits, incumbent, objective="score", candidates=None):
    """what `best_guess` must return, from the two kernels: (index, point, expected, incumbent_expected, taken)"""
    ops, cells = env["ops"], m.lla_geocells.data
    cand = cells if candidates is None else candidates
    idx, val = ops.guess_best(logits, ops.score_table(cand, cells, kind=objective), maximize=objective == "score")
    ek, es, _ = ops.guess_spread(logits, cells, incumbent, (1.0,), extent_km=m.cell_extent_km)
    inc = es if objective == "score" else ek
    taken = ((val > inc) if objective == "score" else (val < inc)) & (idx >= 0)
    return idx, torch.where(taken[:, None], cand[idx.clamp(min=0)], incumbent), val, inc, taken


def same_guess(bg, want):
    return (torch.equal(bg.index, want[0]) and same_bits(bg.point, want[1]) and same_bits(bg.expected, want[2])
            and same_bits(bg.incumbent_expected, want[3]) and torch.equal(bg.taken, want[4]))


def test_best_guess_is_the_kernel_on_the_last_state(env, tmp_path):
    m, _ = model_of(env, tmp_path)
    with pytest.raises(RuntimeError, match="no state"):
        m.best_guess()
    px = env["syn"].make_pixels(12, seed=3, panorama=True).to(DEV)
    out = m(pixel_values=px)
    with pytest.raises(ValueError, match="objective"):
        m.best_guess(objective="miles")
    st = m.last_state
    for objective in ("score", "km"):
        bg = m.best_guess(objective=objective)
        assert bg.index.dtype == torch.int64 and bg.point.shape == (3, 2) and bg.point.dtype == torch.float64 and bg.taken.dtype == torch.bool
        assert same_guess(bg, want_guess(env, m, st["logits"], out.preds_LLH, objective))
        strict = (bg.expected > bg.incumbent_expected) if objective == "score" else (bg.expected < bg.incumbent_expected)
        assert torch.equal(bg.taken, strict)
        # the argmax centroid is a candidate itself: the best candidate is never worse than it, to the two kernels' rounding
        slack = 1e-9 * bg.incumbent_expected.abs()
        assert bool(((bg.expected >= bg.incumbent_expected - slack) if objective == "score" else (bg.expected <= bg.incumbent_expected + slack)).all())
    # the table is built once per objective ...
    table = m._guess_tables["score"][3]
    m.best_guess()
    assert m._guess_tables["score"][3] is table
    # ... and again when the candidates change: another tensor, or the same one written in place
    grid = torch.stack(torch.meshgrid(torch.linspace(-170, 170, 12, dtype=torch.float64), torch.linspace(-80, 80, 9, dtype=torch.float64),
                                      indexing="ij"), dim=-1).reshape(-1, 2).to(DEV)
    inc = torch.tensor([[10.0, 20.0], [-60.0, 5.0], [100.0, -30.0]], dtype=torch.float64)
    bg = m.best_guess(candidates=grid, incumbent=inc.numpy(), state=dict(st))
    assert same_guess(bg, want_guess(env, m, st["logits"], inc.to(DEV), "score", grid))
    assert bool((bg.point[bg.taken] == grid[bg.index[bg.taken]]).all()) and bool((bg.point[~bg.taken] == inc.to(DEV)[~bg.taken]).all())
    t1 = m._guess_tables["score"][3]
    assert t1 is not table and t1.shape == (108, CELLS)
    m.best_guess(candidates=grid, incumbent=inc)
    assert m._guess_tables["score"][3] is t1
    grid[:, 0] += 3.0
    bg2 = m.best_guess(candidates=grid, incumbent=inc)
    assert m._guess_tables["score"][3] is not t1 and same_guess(bg2, want_guess(env, m, st["logits"], inc.to(DEV), "score", grid))
    # a NaN on either side keeps the incumbent
    poisoned = dict(st, logits=st["logits"].clone())
    poisoned["logits"][1, 5] = float("nan")
    bg3 = m.best_guess(state=poisoned)
    assert int(bg3.index[1]) == -1 and not bool(bg3.taken[1]) and same_bits(bg3.point[1], out.preds_LLH[1])
    assert bool(torch.isnan(bg3.expected[1])) and bool(torch.isnan(bg3.incumbent_expected[1]))
    keep = [0, 2]
    first = m.best_guess()
    assert torch.equal(bg3.index[keep], first.index[keep]) and same_bits(bg3.expected[keep], first.expected[keep])
    bad_inc = out.preds_LLH.clone(); bad_inc[2, 0] = float("nan")
    bg4 = m.best_guess(incumbent=bad_inc)
    assert not bool(bg4.taken[2]) and bool(torch.isnan(bg4.point[2, 0])) and int(bg4.index[2]) == int(first.index[2])


def test_certain_forward_takes_the_refined_point_as_the_incumbent(env, tmp_path):
    from pigeon_amd.evaluate import certain_forward
    m, ref = model_of(env, tmp_path)
    px = env["syn"].make_pixels(12, seed=4, panorama=True).to(DEV)
    out0, info0 = certain_forward(m, ref, pixel_values=px)
    assert "best_guess" not in info0
    for objective in ("score", "km"):
        out, info = certain_forward(m, ref, pixel_values=px, best_guess=objective)
        logits = m.last_state["logits"]
        assert same_guess(info["best_guess"], want_guess(env, m, logits, info["refined_LLH"].double(), objective))
        assert torch.equal(out.preds_LLH, out0.preds_LLH) and torch.equal(info["refined_LLH"], info0["refined_LLH"])
        assert torch.equal(out.preds_geocell, out0.preds_geocell) and torch.equal(info["certain"], info0["certain"])
    out2, info2 = certain_forward(m, None, pixel_values=px, best_guess="score")
    assert same_guess(info2["best_guess"], want_guess(env, m, m.last_state["logits"], out2.preds_LLH, "score"))


def test_evaluate_model_columns_and_metrics(env, tmp_path):
    from pigeon_amd.evaluate import certain_forward, compute_geoguessr_metrics, evaluate_model, geoguessr_score
    from pigeon_amd.geo_utils import haversine_np
    m, ref = model_of(env, tmp_path, exact_top1=False)               # (as the spread's columns test: compared with other batch sizes)
    px = env["syn"].make_pixels(24, seed=6, panorama=True)
    cen = m.lla_geocells.data.cpu().numpy()
    labels = np.stack([cen[(7 * i) % CELLS] + [0.3 * i, -0.2 * i] for i in range(6)])
    data = [dict(pixel_values=px[i], labels=torch.from_numpy(labels[i]), labels_clf=torch.tensor((7 * i) % CELLS)) for i in range(6)]

    class Columns(list):
        def __getitem__(self, i):
            return np.stack([np.asarray(d[i]) for d in self]) if isinstance(i, str) else list.__getitem__(self, i)

    new = {"best_LLH", "best_index", "best_expected", "best_taken", "Mean_km_error_best", "Median_km_error_best", "Geoguessr_score_best",
           "Best_guess_changed"}
    plain = evaluate_model(m, Columns(data), compute_geoguessr_metrics, refiner=ref, batch_size=4)
    assert not new & set(plain)
    got = evaluate_model(m, Columns(data), compute_geoguessr_metrics, refiner=ref, batch_size=4, best_guess="score")
    assert set(got) == set(plain) | new
    for k, v in plain.items():                                       # every existing key as before
        if k == "exact_passes":
            continue
        assert np.array_equal(np.asarray(got[k]), np.asarray(v), equal_nan=True) if not isinstance(v, (int, float)) else got[k] == v, k
    parts = [certain_forward(m, ref, pixel_values=px[s].to(DEV), best_guess="score")[1]["best_guess"] for s in (slice(0, 4), slice(4, 6))]
    for k, col in (("best_index", 0), ("best_LLH", 1), ("best_expected", 2), ("best_taken", 4)):
        assert np.array_equal(got[k], np.concatenate([p[col].cpu().numpy() for p in parts])), k
    assert got["best_LLH"].shape == (6, 2) and got["best_LLH"].dtype == np.float64 and got["best_taken"].dtype == np.bool_
    d = haversine_np(got["best_LLH"], labels)
    assert got["Mean_km_error_best"] == np.mean(d) and got["Median_km_error_best"] == np.median(d)
    assert got["Geoguessr_score_best"] == geoguessr_score(d) and got["Best_guess_changed"] == float(np.mean(got["best_taken"]))
    km = evaluate_model(m, [dict(pixel_values=x["pixel_values"]) for x in data], refiner=ref, batch_size=4, best_guess="km")
    assert "Mean_km_error_best" not in km and km["best_LLH"].shape == (6, 2)            # no labels: the four columns only
    parts = [certain_forward(m, ref, pixel_values=px[s].to(DEV), best_guess="km")[1]["best_guess"] for s in (slice(0, 4), slice(4, 6))]
    assert np.array_equal(km["best_expected"], np.concatenate([p.expected.cpu().numpy() for p in parts]))


def test_predict_panorama_answers_with_the_chosen_point(env, tmp_path):
    from pigeon_amd import serve
    from pigeon_amd.evaluate import certain_forward
    m, ref = model_of(env, tmp_path)
    px = env["syn"].make_pixels(4, seed=9, panorama=True).to(DEV).reshape(4, 3, 336, 336)
    plain = serve.predict_panorama([None] * 4, m, ref, preprocess=lambda views: px)
    res = serve.predict_panorama([None] * 4, m, ref, preprocess=lambda views: px, best_guess=True, spread=True)
    _, info = certain_forward(m, ref, pixel_values=px.reshape(1, 12, 336, 336), best_guess="score")
    bg = info["best_guess"]
    assert same_guess(bg, want_guess(env, m, m.last_state["logits"], info["refined_LLH"].double(), "score"))
    assert (res["lng"], res["lat"]) == tuple(bg.point[0].tolist())
    assert (res["argmax_lat"], res["argmax_lng"]) == (plain["lat"], plain["lng"])
    assert res["guess_changed"] == bool(bg.taken[0])
    assert res["guess_expected_score"] == float(bg.expected[0] if bg.taken[0] else bg.incumbent_expected[0])
    assert not {"argmax_lat", "argmax_lng", "guess_expected_score", "guess_changed"} & set(plain)
    assert {"expected_km", "expected_score", "radius_km"} <= set(res)
    for k in ("geocell_margin", "geocell_certain"):
        assert res[k] == plain[k]


def test_a_split_head_is_answered_between_its_cells(env, tmp_path):
    """Two regions, each a ring of six cells of 3 degrees radius around a centre cell of little mass: region A holds 0.55 of the
    probability and the argmax cell, region B 0.4.  No ring cell -- neither region's mode -- has the expected score of A's centre."""
    ring = lambda lng, lat: [(lng + 3 * np.cos(a), lat + 3 * np.sin(a)) for a in np.arange(6) * np.pi / 3]       # noqa: E731
    cen = env["syn"].make_geocells(CELLS, seed=0).copy()
    cen[:14] = [(10.0, 10.0)] + ring(10.0, 10.0) + [(70.0, -20.0)] + ring(70.0, -20.0)
    cen[14:] = np.stack([np.linspace(-170, -100, CELLS - 14), np.linspace(-60, 60, CELLS - 14)], axis=1)       # far away, no mass
    p = np.full(CELLS, 1e-9)
    p[0], p[1], p[2:7] = 0.02, 0.10, 0.086                           # A: centre, its mode, the rest of the ring
    p[7], p[8], p[9:14] = 0.01, 0.09, 0.06                           # B likewise
    bias = torch.from_numpy(np.log(p / p.sum())).float()
    m, _ = model_of(env, tmp_path, cen=cen, name="split.csv", exact_top1=False, gain=0.01, bias=bias)
    px = env["syn"].make_pixels(12, seed=2, panorama=True).to(DEV)
    out = m(pixel_values=px)
    assert bool((out.preds_geocell == 1).all())                      # the answer so far: A's mode
    bg = m.best_guess()
    _, _, E = env["ops"].guess_best(m.last_state["logits"], m._guess_tables["score"][3], return_expected=True)
    assert bool(bg.taken.all()) and bool((bg.index == 0).all()), bg.index.tolist()
    assert same_bits(bg.point, m.lla_geocells.data[:1].expand(3, 2).contiguous())
    assert bool((bg.expected > E[:, 1] + 50).all()) and bool((bg.expected > E[:, 8] + 50).all())        # points of score, not ulps
    assert bool((bg.expected - bg.incumbent_expected > 50).all())
    # (on the CPU, tests/_bestref.py: 2354 points at A's centre against 2262 at its mode and 1684 at B's)
