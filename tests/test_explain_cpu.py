"""pigeon_amd/explain.py and the serving key "attribution" (no GPU): the token -> patch arrangement, the per-view shares, the overlay,
the JSON object the command line and the server write, and the HTTP contract with stub models."""
import json
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image
from starlette.testclient import TestClient

from pigeon_amd import explain, serve
from pigeon_amd.clip_embedder import clip_preprocess
from pigeon_amd.super_guessr import Attribution

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_serve_cpu import StubModel, _data_uri  # noqa: E402  (the stub and the payloads whose response that file pins)


def _planted(B=2, P=4, K=3):
    """maps[b,p,t,k] = 1000 b + 100 p + t + k / 10: every element names its place."""
    b, p, t, k = np.meshgrid(np.arange(B), np.arange(P), np.arange(577), np.arange(K), indexing="ij")
    return (1000.0 * b + 100.0 * p + t + k / 10.0).astype(np.float64)


def test_patch_grid_puts_token_1_plus_24y_plus_x_at_y_x():
    m = _planted()
    for maps in (m, torch.from_numpy(m)):
        grid, cls = explain.patch_grid(maps)
        assert grid.shape == (2, 4, 24, 24, 3) and cls.shape == (2, 4, 3)
        assert np.array_equal(cls, m[:, :, 0, :])
        for y, x in ((0, 0), (0, 23), (5, 7), (23, 0), (23, 23)):
            assert np.array_equal(grid[:, :, y, x, :], m[:, :, 1 + 24 * y + x, :]), (y, x)
        assert grid[1, 2, 23, 23, 1] == 1000 + 200 + 576 + 0.1
    with pytest.raises(ValueError, match="577"):
        explain.patch_grid(m[:, :, :576])


def test_view_share_sums_a_views_tokens():
    m = _planted()
    s = explain.view_share(m)
    assert s.shape == (2, 4, 3) and np.allclose(s, m.sum(axis=2), rtol=0, atol=1e-9)
    grid, cls = explain.patch_grid(m)
    assert np.allclose(s, grid.sum(axis=(2, 3)) + cls, rtol=0, atol=1e-6)
    one = np.zeros((1, 2, 577, 1), dtype=np.float32)
    one[0, 1, 576, 0] = 3.0
    assert explain.view_share(one).tolist() == [[[0.0], [3.0]]]


def test_overlay_keeps_the_crops_size_and_colours_by_sign():
    crop = np.full((336, 336, 3), 128, dtype=np.uint8)
    grid = np.zeros((24, 24))
    grid[2, 3], grid[20, 10] = 1.0, -0.5
    img = explain.overlay(crop, grid)
    assert isinstance(img, Image.Image) and img.size == (336, 336) and img.mode == "RGB"
    a = np.asarray(img).astype(int)
    r, g, b = a[2 * 14 + 7, 3 * 14 + 7]
    assert r > 128 > b                                                # speaks for the cell: red
    r, g, b = a[20 * 14 + 7, 10 * 14 + 7]
    assert b > 128 > r                                                # speaks against it: blue
    assert (a[300, 300] == 128).all()                                 # nothing to say: the crop itself
    assert np.array_equal(np.asarray(explain.overlay(crop, np.zeros((24, 24)))), crop)
    assert explain.overlay(torch.from_numpy(crop), torch.from_numpy(grid)).size == (336, 336)
    with pytest.raises(ValueError):
        explain.overlay(crop, np.zeros((577,)))
    with pytest.raises(ValueError):
        explain.overlay(crop.astype(np.float32), grid)


def _attribution(B=1, P=4, K=2, seed=0):
    rng = np.random.default_rng(seed)
    maps = (rng.standard_normal((B, P, 577, K)) * 1e-3).astype(np.float32)
    offset = rng.standard_normal((B, K)).astype(np.float32) * 0.01
    logits = (maps.astype(np.float64).sum(axis=(1, 2)) + offset).astype(np.float32)
    return Attribution(torch.from_numpy(maps), torch.from_numpy(offset), torch.tensor([[7, 3]] * B)[:, :K], torch.tensor([3] * B),
                       torch.from_numpy(logits))


def test_report_round_trips_through_json(tmp_path):
    att = _attribution()
    crops = np.random.default_rng(1).integers(0, 256, (4, 336, 336, 3), dtype=np.uint8)
    obj = explain.write_report(str(tmp_path / "out"), att, crops)
    back = json.load(open(tmp_path / "out" / "attribution.json"))
    assert back == obj == json.loads(json.dumps(explain.attribution_json(att)))
    assert sorted(os.listdir(tmp_path / "out")) == ["attribution.json", "view1.png", "view2.png", "view3.png", "view4.png"]
    assert all(Image.open(tmp_path / "out" / f"view{i}.png").size == (336, 336) for i in range(1, 5))
    assert set(back) == {"cells", "against", "logits", "offset", "token_sum", "view_share", "cls_share", "grids"}
    assert back["cells"] == [7, 3] and back["against"] == 3
    grids, cls = np.asarray(back["grids"]), np.asarray(back["cls_share"])
    assert grids.shape == (4, 24, 24, 2) and cls.shape == (4, 2) and np.asarray(back["view_share"]).shape == (4, 2)
    assert np.array_equal(grids.astype(np.float32), explain.patch_grid(att.maps)[0][0])                 # fp32 values survive the text
    # what the file holds adds up to its logits
    total = grids.sum(axis=(0, 1, 2)) + cls.sum(axis=0) + np.asarray(back["offset"])
    assert np.allclose(total, back["logits"], rtol=0, atol=1e-6)
    assert np.allclose(np.asarray(back["view_share"]).sum(axis=0), back["token_sum"], rtol=0, atol=1e-12)


def test_command_line_arguments():
    ap = explain._arg_parser()
    a = ap.parse_args(["-o", "out", "a.png"])
    assert (a.tier, a.against, a.layers, a.k, a.views, a.head, a.geocells) == ("fast", "runner_up", 24, 1, ["a.png"], None, None)
    a = ap.parse_args(["--head", "h", "--geocells", "g", "--layers", "2", "--tier", "exact", "--against", "none", "-o", "d", "1", "2", "3", "4"])
    assert (a.head, a.geocells, a.layers, a.tier, a.against, a.out, len(a.views)) == ("h", "g", 2, "exact", "none", "d", 4)
    with pytest.raises(SystemExit):
        ap.parse_args(["--tier", "double", "-o", "d", "x"])
    with pytest.raises(SystemExit):
        explain.main(["-o", "d", "a.png", "b.png"])                   # 1 or 4 views


# ---------------------------------------------------------------------------------------------- serving
class AttributingStub(StubModel):
    def __init__(self):
        super().__init__()
        self.asked = []

    def attribute(self, pixel_values=None, tier="fast", **kw):
        self.asked.append((tuple(pixel_values.shape), tier))
        return _attribution(seed=5)


BODY = {"gameID": "abc", "roundID": 3, "image": _data_uri(1), "image_2": _data_uri(2, fmt="JPEG"), "image_3": _data_uri(3),
        "image_4": _data_uri(4)}


def test_serving_adds_the_attribution_object_on_request():
    model = AttributingStub()
    c = TestClient(serve.make_app(model, preprocess=clip_preprocess))
    r = c.post("/api/v1/predict", json=dict(BODY, attribution=True))
    assert r.status_code == 200
    res = r.json()["results"]
    assert set(res) == {"lat", "lng", "attribution"} and res["lat"] == -33.25
    assert res["attribution"] == json.loads(json.dumps(explain.attribution_json(_attribution(seed=5))))
    assert model.asked == [((1, 12, 336, 336), "fast")]


def test_serving_without_attribute_answers_400():
    c = TestClient(serve.make_app(StubModel(), preprocess=clip_preprocess))
    r = c.post("/api/v1/predict", json=dict(BODY, attribution=True))
    assert r.status_code == 400 and "attribution" in r.json()["error"]


@pytest.mark.parametrize("extra", [{}, {"attribution": False}, {"attribution": None}])
def test_requests_without_the_key_get_todays_response(extra):
    plain, able = StubModel(), AttributingStub()
    want = TestClient(serve.make_app(plain, preprocess=clip_preprocess)).post("/api/v1/predict", json=BODY)
    got = TestClient(serve.make_app(able, preprocess=clip_preprocess)).post("/api/v1/predict", json=dict(BODY, **extra))
    assert got.status_code == 200 and got.content == want.content and able.asked == []
    out = got.json()                                                  # ... which is what tests/test_serve_cpu.py pins
    assert out["gameID"] == "abc" and out["roundID"] == 3 and set(out["results"]) == {"lat", "lng"} and out["results"]["lat"] == -33.25
    assert abs(out["results"]["lng"] - (12.5 + float(able.seen.mean()))) < 1e-9
