"""The entry points that take image FILES as bytes (pigeon_amd/jpeg.py EncodedImages), each on a 2-layer tower against the same entry
point fed with the pixels Pillow decodes from those files: embed_images, ImageEvalDataset through evaluate_model with worker
processes, run.py --raw-images --encoded, and a serving request.  The files are the fixtures of tests/golden/jpeg_fixtures.npz."""
import base64
import importlib
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VIEWS = ("image", "image_2", "image_3", "image_4")


@pytest.fixture(scope="module")
def env(golden_dir):
    from pigeon_amd import _lib, synthetic
    _lib.require_gpu()
    z = np.load(os.path.join(golden_dir, "jpeg_fixtures.npz"))
    off, shapes = z["file_off"], z["shapes"]
    po = np.cumsum([0] + [int(h) * int(w) * 3 for h, w in shapes])
    # the larger fixtures of every mode, restart and optimised files among them
    pick = [i for i, n in enumerate(z["names"]) if str(n).split("_")[0] in ("17x33", "37x53", "9x17") and not str(z["refused"][i])][:48]
    files = [z["files"][off[i]:off[i + 1]].tobytes() for i in pick]
    pixels = [z["pixels"][po[i]:po[i + 1]].reshape(int(shapes[i][0]), int(shapes[i][1]), 3).copy() for i in pick]
    return dict(syn=synthetic, files=files, pixels=pixels)


def _model(env, tmp_path, C_=64, **kw):
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    from pigeon_amd.proto_refiner import ProtoRefiner
    from pigeon_amd.super_guessr import SuperGuessr
    syn = env["syn"]
    gp = os.path.join(str(tmp_path), "g.csv")
    syn.write_geocell_csv(gp, syn.make_geocells(C_, seed=0))
    vit = HipCLIPVisionModel(syn.make_vit_weights(seed=0, layers=2), layers=2).to(DEV)
    W, bias = syn.make_head_weights(C_, seed=1)
    m = SuperGuessr(vit, panorama=True, freeze_base=True, num_candidates=5, geocell_path=gp, exact_top1=True, margin_kappa=3.6,
                    margin_autocalibrate=False, margin_rel_tol=1e-3, **kw)
    with torch.no_grad():
        m.cell_layer.weight.copy_(W * 64)
        m.cell_layer.bias.copy_(bias)
    m = m.to(DEV).eval()
    ref = ProtoRefiner(topk=5, max_refinement=1000, temperature=1.6, bank=syn.make_bank(C_, 9, seed=5, empty_frac=0.1, max_members=6),
                       device=DEV).eval()
    return m, ref


def test_evaluate_model_from_files_with_workers_equals_the_decoded_route(env, tmp_path):
    """ImageEvalDataset(encoded=True): two worker processes ship the files' bytes (one item as bytes, the next as the dict of a
    datasets.Image(decode=False) column, the next as a path), the main process decodes and resizes on the GPU; the result dict equals
    the one of ImageEvalDataset on the decoded pixels, key by key."""
    from pigeon_amd.evaluate import ImageEvalDataset, evaluate_model
    m, ref = _model(env, tmp_path)
    enc, dec = [], []
    for i in range(6):
        lab = {"labels": torch.tensor([10.0 * i, -5.0 * i], dtype=torch.float64), "labels_clf": torch.tensor(i)}
        e, d = dict(lab), dict(lab)
        for v, key in enumerate(VIEWS):
            k = (4 * i + v) % len(env["files"])
            data = env["files"][k]
            if i % 3 == 1:
                e[key] = {"bytes": data, "path": None}
            elif i % 3 == 2:
                path = os.path.join(str(tmp_path), f"{i}_{v}.jpg")
                with open(path, "wb") as f:
                    f.write(data)
                e[key] = {"bytes": None, "path": path} if v % 2 else path
            else:
                e[key] = data
            d[key] = env["pixels"][k]
        enc.append(e)
        dec.append(d)
    got = evaluate_model(m, ImageEvalDataset(enc, encoded=True), refiner=ref, batch_size=4, num_workers=2)
    want = evaluate_model(m, ImageEvalDataset(dec), refiner=ref, batch_size=4)
    assert set(got) == set(want)
    for k in want:
        a, b = got[k], want[k]
        if hasattr(b, "shape"):
            assert np.array_equal(a, b, equal_nan=True) if np.asarray(b).dtype.kind == "f" else np.array_equal(a, b), k
        elif k != "exact_passes":
            assert a == b or (a != a and b != b), k
    assert got["preds"].shape[0] == 6
    with pytest.raises(TypeError, match="encoded=True needs"):
        ImageEvalDataset(dec, encoded=True)[0]


def test_embed_images_encoded_equals_raw(env, tmp_path):
    from pigeon_amd import synthetic
    from pigeon_amd.clip_embedder import CLIPEmbedding, HipCLIPVisionModel
    from pigeon_amd.embed import embed_images
    sd = synthetic.make_vit_weights(seed=11, layers=2, affine_jitter=True)
    emb = CLIPEmbedding("synthetic", device=DEV, clip_model=HipCLIPVisionModel(sd, layers=2), contract_guard="off")
    n = 11
    files = [{"image": {"bytes": env["files"][i], "path": None}, "index": i} for i in range(n)]
    arrays = [{"image": env["pixels"][i], "index": i} for i in range(n)]

    def run(tag, items, **kw):
        out = os.path.join(str(tmp_path), tag)
        embed_images(emb, {"train": items}, batch_size=4, num_workers=0, out_dir=out, raw_images=True, **kw)
        return np.load(os.path.join(out, "train.npy")), np.load(os.path.join(out, "train_indices.npy"))

    e_raw, i_raw = run("raw", arrays)
    e_enc, i_enc = run("enc", files, encoded=True)
    assert e_enc.shape == (3, 4, 1024) and np.array_equal(i_enc, i_raw) and np.array_equal(e_enc, e_raw)
    with pytest.raises(ValueError, match="raw_images"):
        embed_images(emb, {"train": files}, raw_images=False, encoded=True)


def _run_main(monkeypatch, argv):
    sys.path.insert(0, ROOT)
    monkeypatch.setattr(sys, "argv", ["run.py"] + argv)
    import run
    importlib.reload(run)
    return run.main()


def test_run_py_encoded_smoke(env, monkeypatch, tmp_path, capsys):
    """`run.py evaluate ... --raw-images --encoded` and `run.py embed ... --raw-images --encoded` on synthetic JPEG files."""
    pytest.importorskip("PIL")
    torch.manual_seed(0)
    res = _run_main(monkeypatch, ["evaluate", "none", "--synthetic", "8", "--layers", "2", "--geocells", "300", "--raw-images", "--encoded"])
    assert res["preds"].shape == (8, 2) and "Geocell_accuracy" in res
    torch.manual_seed(0)
    plain = _run_main(monkeypatch, ["evaluate", "none", "--synthetic", "8", "--layers", "2", "--geocells", "300", "--raw-images"])
    assert plain["preds"].shape == (8, 2)                            # (other pixels: the JPEG files are lossy copies of these arrays)
    out_dir = os.path.join(str(tmp_path), "emb")
    _run_main(monkeypatch, ["embed", "random", "--synthetic", "6", "--layers", "2", "--out-dir", out_dir, "--yfcc", "--raw-images", "--encoded"])
    e = np.load(os.path.join(out_dir, "train.npy"))
    assert e.reshape(-1, 1024).shape[0] >= 6 and np.isfinite(e).all() and np.abs(e).max() > 0
    with pytest.raises(SystemExit):
        _run_main(monkeypatch, ["embed", "random", "--synthetic", "6", "--layers", "2", "--encoded"])


def test_serving_request_with_jpeg_payloads_equals_the_pillow_route(env, tmp_path):
    """One request through the Starlette app in its `encoded` mode equals the same request through the default app (Pillow decodes):
    the same JSON.  A payload no decoder can read is a 400 in both."""
    from starlette.testclient import TestClient
    from pigeon_amd import serve
    m, ref = _model(env, tmp_path, serving=True)
    body = {"gameID": "g", "roundID": 3}
    for v, key in enumerate(VIEWS):
        body[key] = "data:image/jpeg;base64," + base64.b64encode(env["files"][5 * v + 1]).decode()
    want = TestClient(serve.make_app(m, ref)).post("/api/v1/predict", json=body)
    got = TestClient(serve.make_app(m, ref, encoded=True)).post("/api/v1/predict", json=body)
    assert want.status_code == 200 and got.status_code == 200 and got.json() == want.json()
    assert set(got.json()["results"]) >= {"lat", "lng"}
    views = [env["files"][5 * v + 1] for v in range(4)]
    direct = serve.predict_panorama(views, m, ref)
    assert {k: direct[k] for k in ("lat", "lng")} == {k: got.json()["results"][k] for k in ("lat", "lng")}
    body["image_3"] = "data:image/jpeg;base64," + base64.b64encode(b"no image at all").decode()
    for app in (serve.make_app(m, ref), serve.make_app(m, ref, encoded=True)):
        assert TestClient(app).post("/api/v1/predict", json=body).status_code == 400
