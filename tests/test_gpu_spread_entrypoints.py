"""The guess spread at the entry points (run with -m gpu on an MI355X), on a 2-layer synthetic tower: `SuperGuessr.spread`,
`certain_forward(spread=...)`, `evaluate_model(spread=...)` and the geocell CSV's polygons -> `cell_extent_km`.  The kernel itself is
held to its contract in tests/test_gpu_spread.py; here every comparison is against pigeon_amd.hip_ops.guess_spread on the logits,
point and extents the entry point must have used, bit for bit."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import _georef as G
import _spreadref as S

pytestmark = pytest.mark.gpu

DEV = "cuda"
CELLS = 64
QS = (0.5, 0.9)


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops, synthetic
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    _lib.require_gpu()
    vit = HipCLIPVisionModel(synthetic.make_vit_weights(seed=0, layers=2), layers=2).to(DEV)
    return dict(ops=hip_ops, syn=synthetic, vit=vit)


def square(lng, lat, half):
    x0, x1, y0, y1 = (float(v) for v in (lng - half, lng + half, max(lat - half, -90.0), min(lat + half, 90.0)))
    return f"POLYGON (({x0!r} {y0!r}, {x1!r} {y0!r}, {x1!r} {y1!r}, {x0!r} {y1!r}, {x0!r} {y0!r}))"


def model_of(env, tmp_path, polygons=False, name="g.csv", exact_top1=True):
    from pigeon_amd.proto_refiner import ProtoRefiner
    from pigeon_amd.super_guessr import SuperGuessr
    syn = env["syn"]
    cen = syn.make_geocells(CELLS, seed=0)
    gp = os.path.join(str(tmp_path), name)
    if polygons:
        cen = np.clip(cen, [-170.0, -80.0], [170.0, 80.0])
        pd.DataFrame({"lng": cen[:, 0], "lat": cen[:, 1],
                      "polygon": [square(x, y, 0.25 + 0.05 * (i % 7)) for i, (x, y) in enumerate(cen)]}).to_csv(gp, index=False)
    else:
        syn.write_geocell_csv(gp, cen)
    W, bias = syn.make_head_weights(CELLS, seed=1)
    m = SuperGuessr(env["vit"], panorama=True, freeze_base=True, num_candidates=5, geocell_path=gp, exact_top1=exact_top1, margin_kappa=3.6,
                    margin_autocalibrate=False, margin_rel_tol=1e-3)
    with torch.no_grad():
        m.cell_layer.weight.copy_(W * 64); m.cell_layer.bias.copy_(bias)
    m = m.to(DEV).eval()
    ref = ProtoRefiner(topk=5, max_refinement=1000, temperature=1.6, bank=syn.make_bank(CELLS, 9, seed=5, empty_frac=0.1, max_members=6),
                       device=DEV).eval()
    return m, ref


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def same_spread(sp, want):
    return all(same_bits(a, b) for a, b in zip(sp[:3], want))


def test_model_spread_is_the_kernel_on_the_last_state(env, tmp_path):
    m, _ = model_of(env, tmp_path)
    with pytest.raises(RuntimeError, match="no state"):
        m.spread()
    assert "cell_extent_km" not in m.state_dict() and m.cell_extent_km.device.type == "cuda"
    assert m.cell_extent_km.dtype == torch.float64 and not bool(m.cell_extent_km.any())              # no polygon column: zeros
    px = env["syn"].make_pixels(12, seed=3, panorama=True).to(DEV)
    out = m(pixel_values=px)
    st = m.last_state
    sp = m.spread()
    assert sp.quantiles == QS and sp.expected_km.shape == (3,) and sp.radius_km.shape == (3, 2)
    assert same_spread(sp, env["ops"].guess_spread(st["logits"], m.lla_geocells.data, out.preds_LLH, QS, extent_km=m.cell_extent_km))
    assert bool((sp.radius_km[:, 0] <= sp.radius_km[:, 1]).all()) and bool((sp.expected_score <= 5000).all())
    # candidate points (B, G, 2) as numpy, other quantiles, an explicit state
    pts = S.points_of(3, 2, 1)
    sp2 = m.spread(points=pts, quantiles=(0.25, 0.5, 0.75, 0.9), state=dict(st))
    want = env["ops"].guess_spread(st["logits"], m.lla_geocells.data, torch.from_numpy(pts).to(DEV), (0.25, 0.5, 0.75, 0.9))
    assert sp2.radius_km.shape == (3, 2, 4) and same_spread(sp2, want)
    errors, loose, _ = S.compare(S.truth(st["logits"].cpu().numpy(), m.lla_geocells.data.cpu().numpy(), pts, sp2.quantiles),
                                 *(t.cpu().numpy() for t in sp2[:3]))
    assert not errors and loose == 0, (errors[:3], loose)


def test_certain_forward_uses_the_refined_point_and_the_reencoded_logits(env, tmp_path):
    """A scripted near-tie: cells 0 and 1 lead every row, and W[1] - W[0] is orthogonal to row 0's head input, so row 0's top-1 cannot
    be settled by the 16-bit encoder and is re-encoded.  Its spread must come from the exact tier's logits, at the refined point."""
    from pigeon_amd.evaluate import certain_forward
    m, ref = model_of(env, tmp_path)
    px = env["syn"].make_pixels(12, seed=4, panorama=True).to(DEV)
    st0 = m.encode_head(px)
    e = st0["head_in"].mean(dim=1)                                    # (3, 1024): the mean over the panels the head sees
    g = torch.randn(1024, generator=torch.Generator().manual_seed(1)).to(DEV)
    g = g - (g @ e[0]) / (e[0] @ e[0]) * e[0]
    lift = 2 * float(st0["logits"].max() - st0["logits"].min()) + 10
    with torch.no_grad():
        W, b = m.cell_layer.weight, m.cell_layer.bias
        W[1] = W[0] + g * (0.05 / float(g.norm()))
        b[0] += lift; b[1] = b[0]
    m._wnorm, m._engines = {}, {}
    out, info = certain_forward(m, ref, pixel_values=px, spread=QS)
    re = info["reencoded"].tolist()
    assert 0 in re, f"row 0 was meant to be re-encoded (re-encoded: {re})"
    fast = m.encode_head(px)["logits"]
    exact = m.exact_rows([px[re].reshape(len(re), -1)])["logits"]
    logits = m.last_state["logits"]                                   # what the settled state carries: fast rows, re-encoded rows
    keep = [i for i in range(3) if i not in re]
    assert torch.equal(logits[keep], fast[keep]) and not torch.equal(logits[re], fast[re])
    # (the exact tier picks its GEMM split by batch size: a pass of its own reproduces the rows to its floor, not to the bit)
    assert float((logits[re] - exact).abs().max()) <= 1e-4 * float(exact.abs().max())
    assert float((fast[re] - exact).abs().max()) > float((logits[re] - exact).abs().max())
    refined = info["refined_LLH"]
    assert refined.dtype == torch.float32 and refined.shape == (3, 2)
    want = env["ops"].guess_spread(logits, m.lla_geocells.data, refined.double(), QS, extent_km=m.cell_extent_km)
    assert same_spread(info["spread"], want)
    moved = (refined.double() != out.preds_LLH).any(dim=1)            # rows whose guess the refiner moved: not the centroid's spread
    at_centroid = env["ops"].guess_spread(logits, m.lla_geocells.data, out.preds_LLH, QS, extent_km=m.cell_extent_km)
    assert bool((info["spread"].expected_km != at_centroid[0])[moved].all())
    stale = env["ops"].guess_spread(fast, m.lla_geocells.data, refined.double(), QS, extent_km=m.cell_extent_km)
    assert not same_bits(info["spread"].expected_km, stale[0]), "the spread ignores the re-encoded rows' logits"
    # without a refiner: the top-1 centroid; without the keyword: nothing
    out2, info2 = certain_forward(m, None, pixel_values=px, spread=(0.9,))
    assert same_spread(info2["spread"], env["ops"].guess_spread(m.last_state["logits"], m.lla_geocells.data, out2.preds_LLH, (0.9,)))
    assert "spread" not in certain_forward(m, None, pixel_values=px)[1]


def test_evaluate_model_columns_and_coverage(env, tmp_path):
    from pigeon_amd.evaluate import certain_forward, evaluate_model
    from pigeon_amd.geo_utils import haversine_np
    # the exact tier off: its GEMM split follows the batch size, so a row re-encoded in two differently sized passes is the same to its
    # floor, not to the bit -- and the columns below are compared bit for bit with the settle-before-return path
    m, ref = model_of(env, tmp_path, exact_top1=False)
    px = env["syn"].make_pixels(24, seed=6, panorama=True)           # 6 panoramas, on the host
    cen = m.lla_geocells.data.cpu().numpy()
    labels = np.stack([cen[(7 * i) % CELLS] + [0.3 * i, -0.2 * i] for i in range(6)])
    data = [dict(pixel_values=px[i], labels=torch.from_numpy(labels[i]), labels_clf=torch.tensor((7 * i) % CELLS)) for i in range(6)]

    class Columns(list):
        def __getitem__(self, i):
            return np.stack([np.asarray(d[i]) for d in self]) if isinstance(i, str) else list.__getitem__(self, i)

    plain = evaluate_model(m, Columns(data), refiner=ref, batch_size=4)
    assert not {"expected_km", "expected_score", "radius_km", "Radius_50_coverage"} & set(plain)
    got = evaluate_model(m, Columns(data), refiner=ref, batch_size=4, spread=QS)
    assert np.array_equal(got["preds"], plain["preds"]) and got["spread_quantiles"] == QS
    parts = [certain_forward(m, ref, pixel_values=px[s].to(DEV), spread=QS)[1]["spread"] for s in (slice(0, 4), slice(4, 6))]
    for k, col in (("expected_km", 0), ("expected_score", 1), ("radius_km", 2)):
        want = np.concatenate([p[col].cpu().numpy() for p in parts])
        assert got[k].dtype == np.float64 and np.array_equal(got[k], want), k
    true_km = haversine_np(got["preds"], labels)
    for j, tag in enumerate(("50", "90")):
        assert got[f"Radius_{tag}_coverage"] == float(np.mean(true_km <= got["radius_km"][:, j])) == S.coverage_np(got["radius_km"][:, j], true_km)
        assert got[f"Median_radius_{tag}_km"] == float(np.median(got["radius_km"][:, j]))
    assert got["Mean_expected_km"] == float(np.mean(got["expected_km"])) and got["Mean_expected_score"] == float(np.mean(got["expected_score"]))
    unlabelled = evaluate_model(m, [dict(pixel_values=d["pixel_values"]) for d in data], refiner=ref, batch_size=4, spread=QS)
    assert np.array_equal(unlabelled["radius_km"], got["radius_km"]) and "Radius_50_coverage" not in unlabelled


def test_extents_come_from_the_csv_polygons(env, tmp_path):
    from pigeon_amd.regions import RegionBank
    m, _ = model_of(env, tmp_path, polygons=True, name="gp.csv")
    cen = m.lla_geocells.data.cpu().numpy()
    bank = RegionBank.from_geocell_csv(os.path.join(str(tmp_path), "gp.csv"))
    ext = m.cell_extent_km.cpu().numpy()
    assert "cell_extent_km" not in m.state_dict() and ext.shape == (CELLS,)
    for c in range(CELLS):
        d, a = G.haversine_truth(cen[c], bank.rings(c)[0])
        assert abs(ext[c] - float(d.max())) <= 16 * G.U(a).max(), c
    assert 27 < ext.min() and ext.max() < 100                       # half-diagonals of 0.25 .. 0.55 degree squares, |lat| <= 80
    px = env["syn"].make_pixels(8, seed=8, panorama=True).to(DEV)
    out = m(pixel_values=px)
    sp = m.spread(quantiles=QS)
    logits = m.last_state["logits"]
    assert same_spread(sp, env["ops"].guess_spread(logits, m.lla_geocells.data, out.preds_LLH, sp.quantiles, extent_km=m.cell_extent_km))
    t = S.truth(logits.cpu().numpy(), cen, out.preds_LLH.cpu().numpy(), sp.quantiles, ext)
    errors, loose, _ = S.compare(t, *(x.cpu().numpy() for x in sp[:3]))
    assert not errors and loose <= S.loose_allowed(t), errors[:3]
    bare = env["ops"].guess_spread(logits, m.lla_geocells.data, out.preds_LLH, sp.quantiles)
    assert bool((sp.radius_km > bare[2]).all()) and same_bits(sp.expected_km, bare[0])              # the extent is in the key only
