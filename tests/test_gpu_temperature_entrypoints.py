"""The temperature at the entry points (run with -m gpu on an MI355X), on the embedding-only route with a planted head: C = 257 cells,
N = 1024 rows.  Every cell has a direction p_c in embedding space; a row of cell y is p_y plus unit Gaussian noise (the mean of four
panels of noise 2), so the Bayes posterior is softmax(<e, p_c> - |p_c|^2 / 2).  The planted head is that times 2.5: over-confident
by a known factor, and beta = 0.4 is the true parameter the fit estimates.  A fitted beta is held to tests/_tempref.py's acceptance
rule -- the reference's total first derivative changes sign within beta (1 +- 2^-39), or is below the rows' derived bounds -- and
what `SuperGuessr` integrates over is compared, bit for bit, with the kernels on the logits it must have used."""
import json
import math
import os

import numpy as np
import pytest
import torch

import _tempref as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
CELLS, ROWS, GAIN = 257, 1024, 2.5
QS = (0.5, 0.9)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from pigeon_amd import _lib, hip_ops, synthetic
    from pigeon_amd.super_guessr import SuperGuessr
    from pigeon_amd.train import ColumnDataset
    _lib.require_gpu()
    root = tmp_path_factory.mktemp("temperature")
    cen = synthetic.make_geocells(CELLS, seed=3)
    geo = str(root / "geocells.csv")
    synthetic.write_geocell_csv(geo, cen)
    g = torch.Generator().manual_seed(77)
    protos = torch.randn((CELLS, 1024), generator=g) * (3.0 / 32)                     # |p_c|^2 about 9
    cells = torch.randint(0, CELLS, (ROWS,), generator=g)
    emb = (protos[cells][:, None, :] + 2 * torch.randn((ROWS, 4, 1024), generator=g)).contiguous()
    labels = torch.from_numpy(cen)[cells].contiguous()

    def model_of(gain=GAIN):
        m = SuperGuessr(None, panorama=True, geocell_path=geo, num_candidates=5).to(DEV).eval()
        with torch.no_grad():
            m.cell_layer.weight.copy_(gain * protos)
            m.cell_layer.bias.copy_(-0.5 * gain * (protos.double() ** 2).sum(dim=1).float())
        return m

    m = model_of()
    logits = hip_ops.head_forward(emb.to(DEV), m.cell_layer.weight.data, m.cell_layer.bias.data, m.lla_geocells.data, 1)["logits"]
    head_path = str(root / "head.model")
    torch.save(m.state_dict(), head_path)
    ds = ColumnDataset(embedding=emb, labels=labels, labels_clf=cells)
    return dict(ops=hip_ops, syn=synthetic, geo=geo, model_of=model_of, emb=emb, cells=cells, labels=labels, root=root,
                logits=logits.cpu().numpy(), clf=cells.numpy(), head=head_path, ds=ds, protos=protos)


@pytest.fixture(scope="module")
def fitted(world):
    from pigeon_amd import temperature
    return temperature.fit_temperature(world["model_of"](), world["emb"], world["cells"])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().flatten().view(torch.uint8), b.contiguous().flatten().view(torch.uint8))


def test_the_fit_is_accepted_by_the_reference(world, fitted, capsys):
    fit = fitted
    with capsys.disabled():
        print(f"\nfit_temperature: beta {fit.beta!r} (T {fit.temperature:.4f}) in {fit.passes} passes; NLL {fit.nll_before:.4f} -> "
              f"{fit.nll_after:.4f}, ECE {fit.ece_before:.4f} -> {fit.ece_after:.4f}, accuracy {fit.reliability['accuracy']:.3f}")
    assert T.accepts(world["logits"], world["clf"], fit.beta)
    assert fit.passes <= 16 and not fit.clamped and fit.n == ROWS and fit.skipped == 0
    assert fit.temperature == 1.0 / fit.beta
    # beta = 1 / GAIN is the true parameter of the planted set: the estimate lies within 4 standard errors of it
    t = T.truth(world["logits"], world["clf"], [fit.beta])
    se = 1.0 / math.sqrt(float(t["d2"][:, 0].sum()))
    assert abs(fit.beta - 1 / GAIN) <= 4 * se, (fit.beta, se)
    assert fit.nll_after <= fit.nll_before and fit.ece_after < fit.ece_before
    tot, bnd, _ = T.totals_truth(t)                                   # the mean is the total, one more rounded division
    assert abs(fit.nll_after - float(tot[0, 0]) / ROWS) <= (bnd[0, 0] + 2.0 ** -52 * float(tot[0, 0])) / ROWS
    st, _ = T.states(world["logits"], world["clf"])
    assert fit.reliability["accuracy"] == float((st == 1).mean())
    assert sum(r["n"] for r in fit.reliability["before"]) == ROWS == sum(r["n"] for r in fit.reliability["after"])
    conf1 = T.truth(world["logits"], world["clf"], [1.0])["conf"][:, 0].astype(np.float64)
    assert abs(fit.ece_before - T.ece_np(conf1, st == 1)) <= 1e-9


def test_chunked_recomputed_and_kept_logits(world, fitted):
    from pigeon_amd import temperature
    m = world["model_of"]()
    chunked = temperature.fit_temperature(m, world["emb"], world["cells"], chunk=100)
    assert T.accepts(world["logits"], world["clf"], chunked.beta) and T.accepts(world["logits"], world["clf"], fitted.beta)
    recomputed = temperature.fit_temperature(m, world["emb"], world["cells"], chunk=100, logits_budget=0)
    assert recomputed == chunked, "recomputed logits and kept logits give the same bits"
    # invalid rows are skipped, not fitted
    bad = world["cells"].clone()
    bad[::4] = CELLS + 5
    part = temperature.fit_temperature(m, world["emb"], bad)
    assert part.n == ROWS - ROWS // 4 and part.skipped == ROWS // 4
    assert T.accepts(world["logits"], bad.numpy(), part.beta)
    with pytest.raises(temperature.FitError, match="none of the"):
        temperature.fit_temperature(m, world["emb"][:8], torch.full((8,), -1))


def test_spread_and_best_guess_integrate_over_the_calibrated_logits(world):
    ops = world["ops"]
    m = world["model_of"]()
    e = world["emb"][:24].to(DEV)
    assert m.temperature == 1.0
    out = m(embedding=e)
    st = m.last_state
    # temperature 1.0: what it was before the attribute existed, and no calibrated copy in the state
    sp1, bg1 = m.spread(quantiles=QS), m.best_guess()
    want1 = ops.guess_spread(st["logits"], m.lla_geocells.data, out.preds_LLH, QS, extent_km=m.cell_extent_km)
    assert all(same_bits(a, b) for a, b in zip(sp1[:3], want1))
    table = ops.score_table(m.lla_geocells.data.to(DEV), m.lla_geocells.data.to(DEV), kind="score")
    idx1, val1 = ops.guess_best(st["logits"], table)
    assert same_bits(bg1.index, idx1) and same_bits(bg1.expected, val1)
    assert "calibrated_logits" not in st
    # temperature T: the kernels on temper_logits(logits, 1 / T)
    m.temperature = GAIN
    cal = ops.temper_logits(st["logits"], 1.0 / GAIN)
    assert torch.equal(cal, st["logits"] * torch.tensor(1.0 / GAIN).float())
    sp, bg = m.spread(quantiles=QS), m.best_guess()
    want = ops.guess_spread(cal, m.lla_geocells.data, out.preds_LLH, QS, extent_km=m.cell_extent_km)
    assert all(same_bits(a, b) for a, b in zip(sp[:3], want)) and not same_bits(sp.expected_km, sp1.expected_km)
    idx, val = ops.guess_best(cal, table)
    inc = ops.guess_spread(cal, m.lla_geocells.data, out.preds_LLH, (1.0,), extent_km=m.cell_extent_km)[1]
    assert same_bits(bg.index, idx) and same_bits(bg.expected, val) and same_bits(bg.incumbent_expected, inc)
    kept = st["calibrated_logits"][1]
    assert same_bits(kept, cal)
    m.spread(quantiles=(0.9,)); m.best_guess(objective="km")
    assert st["calibrated_logits"][1] is kept, "one launch per state and temperature"
    m.temperature = 1.7
    assert not same_bits(m.spread(quantiles=QS).expected_km, sp.expected_km) and st["calibrated_logits"][1] is not kept
    conf = m.confidence()
    want_conf = ops.temper_stats(st["logits"], st["preds_geocell"], [1 / 1.7], conf=True)["conf"][:, 0]
    assert same_bits(conf, want_conf) and bool(((conf > 0) & (conf <= 1)).all())
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite positive"):
            m.temperature = bad
    assert m.temperature == 1.7


def test_reference_parity_outputs_do_not_move(world):
    from pigeon_amd.evaluate import certain_forward
    from pigeon_amd.proto_refiner import ProtoRefiner
    m = world["model_of"]()
    ref = ProtoRefiner(topk=5, max_refinement=1000, temperature=1.6,
                       bank=world["syn"].make_bank(CELLS, 9, seed=5, empty_frac=0.1, max_members=6), device=DEV).eval()
    e = world["emb"][:24].to(DEV)
    runs = []
    for t in (1.0, GAIN):
        m.temperature = t
        out, info = certain_forward(m, ref, embedding=e, spread=QS, best_guess="score")
        st = m.last_state
        runs.append(dict(preds_geocell=out.preds_geocell.clone(), preds_LLH=out.preds_LLH.clone(), topk_idx=st["topk_indices"].clone(),
                         topk_values=st["topk_values"].clone(), out_topk_values=out.top5_geocells.values.clone(), out_topk_indices=out.top5_geocells.indices.clone(),
                         refined=info["refined_LLH"].clone(), refined_cell=info["refined_geocell"].clone(), tol=info["head_tol"].clone(),
                         certain=info["certain"].clone(), margin=st["margin"].clone(), logits=st["logits"].clone(),
                         spread=info["spread"].expected_km.clone()))
    a, b = runs
    for k in a:
        if k == "spread":
            continue
        assert same_bits(a[k], b[k]), k
    assert not same_bits(a["spread"], b["spread"])


def test_evaluate_prints_the_temperature_and_moves_the_coverage(world, fitted, capsys):
    from pigeon_amd import temperature
    from pigeon_amd.evaluate import evaluate
    side = str(world["root"] / "head.temperature.json")
    m = world["model_of"]()
    temperature.save(side, fitted, m)
    kw = dict(yfcc=False, landmarks=False, base_model=None, refine=False, geocell_path=world["geo"], spread=QS)
    plain = evaluate(world["head"], world["ds"], **kw)
    capsys.readouterr()
    cal = evaluate(world["head"], world["ds"], temperature=side, **kw)
    printed = capsys.readouterr().out
    assert "Temperature" in printed and cal["Temperature"] == fitted.temperature and "Temperature" not in plain
    assert np.array_equal(cal["preds"], plain["preds"]) and cal["Geocell_accuracy"] == plain["Geocell_accuracy"]
    print(f"Radius_90_coverage {plain['Radius_90_coverage']:.4f} -> {cal['Radius_90_coverage']:.4f}, "
          f"Radius_50_coverage {plain['Radius_50_coverage']:.4f} -> {cal['Radius_50_coverage']:.4f}")
    # the over-confident head's 90 % radius is too small; calibrated, its coverage moves towards 0.9
    assert plain["Radius_90_coverage"] < cal["Radius_90_coverage"]
    assert abs(cal["Radius_90_coverage"] - 0.9) < abs(plain["Radius_90_coverage"] - 0.9)
    by_number = evaluate(world["head"], world["ds"], temperature=str(fitted.temperature), **kw)
    assert np.array_equal(by_number["radius_km"], cal["radius_km"])
    other = world["model_of"](gain=1.0)
    other_path = str(world["root"] / "other.model")
    torch.save(other.state_dict(), other_path)
    with pytest.raises(ValueError, match="fingerprint"):
        evaluate(other_path, world["ds"], temperature=side, **kw)


def test_predict_panorama_carries_a_confidence(world):
    from pigeon_amd import serve
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    from pigeon_amd.super_guessr import SuperGuessr
    syn = world["syn"]
    vit = HipCLIPVisionModel(syn.make_vit_weights(seed=0, layers=2), layers=2).to(DEV)
    m = SuperGuessr(vit, panorama=True, serving=True, freeze_base=True, num_candidates=5, geocell_path=world["geo"], margin_autocalibrate=False)
    W, bias = syn.make_head_weights(CELLS, seed=1)
    with torch.no_grad():
        m.cell_layer.weight.copy_(W * 64); m.cell_layer.bias.copy_(bias)
    m = m.to(DEV).eval()
    px = syn.make_pixels(4, seed=9, panorama=True).to(DEV).reshape(4, 3, 336, 336)
    plain = serve.predict_panorama([None] * 4, m, None, preprocess=lambda views: px)
    assert "confidence" not in plain
    m.load_temperature(2.5)
    res = serve.predict_panorama([None] * 4, m, None, preprocess=lambda views: px, confidence=True, spread=True)
    assert isinstance(res["confidence"], float) and 0 < res["confidence"] <= 1
    st = m.last_state
    want = world["ops"].temper_stats(st["logits"], st["preds_geocell"], [1 / 2.5], conf=True)["conf"]
    assert res["confidence"] == float(want[0, 0])
    assert (res["lat"], res["lng"]) == (plain["lat"], plain["lng"])
    m.temperature = 1.0
    sharp = serve.predict_panorama([None] * 4, m, None, preprocess=lambda views: px, confidence=True)["confidence"]
    assert sharp >= res["confidence"], "a temperature above 1 flattens the probabilities"


def test_train_writes_a_sidecar_for_its_own_head(world, tmp_path):
    from pigeon_amd import temperature, train
    from pigeon_amd.super_guessr import SuperGuessr
    out = str(tmp_path / "head.model")
    model = train.main(["--synthetic", "512", "--geocells", "257", "--epochs", "1", "--temperature", "-o", out, "--batch", "64"])
    side = out + ".temperature.json"
    assert os.path.exists(side)
    fit = temperature.load(side, model)                               # the model train returns holds the reloaded best head
    obj = json.load(open(side))
    assert fit.temperature == obj["temperature"] > 0 and fit.n + fit.skipped == 128
    assert model.load_temperature(side) == fit.temperature and model.temperature_fit == fit
    with pytest.raises(ValueError) as e:
        temperature.load(side, world["model_of"]())
    assert obj["head_fingerprint"]["weight"] in str(e.value)
    plain = str(tmp_path / "plain.model")
    train.main(["--synthetic", "512", "--geocells", "257", "--epochs", "1", "-o", plain, "--batch", "64"])
    assert not os.path.exists(plain + ".temperature.json")
    assert torch.equal(torch.load(plain, map_location="cpu")["cell_layer.weight"], torch.load(out, map_location="cpu")["cell_layer.weight"])
