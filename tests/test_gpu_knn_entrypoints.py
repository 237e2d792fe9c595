"""The nearest training embeddings at the entry points (run with -m gpu on an MI355X): `EmbeddingIndex`, `evaluate_model(neighbours=K)`
through the `embedding=` route, the command line's .npz and `--self`, and `predict_panorama(neighbours=K)` on a 2-layer synthetic
tower.  The kernels are held to their contract in tests/test_gpu_knn.py; here every comparison is against the exact tier on the
embeddings the entry point must have searched with."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CELLS = 64


@pytest.fixture(scope="module")
def env(tmp_path_factory):
    from pigeon_amd import _lib, hip_ops, synthetic
    from pigeon_amd.proto_refiner import ProtoRefiner
    _lib.require_gpu()
    tmp = str(tmp_path_factory.mktemp("knn"))
    gp = os.path.join(tmp, "g.csv")
    synthetic.write_geocell_csv(gp, synthetic.make_geocells(CELLS, seed=0))
    bank = synthetic.make_bank(CELLS, 9, seed=5, empty_frac=0.1, max_members=6)
    ref = ProtoRefiner(topk=5, max_refinement=1000, temperature=1.6, bank=bank, device=DEV).eval()
    return dict(ops=hip_ops, syn=synthetic, tmp=tmp, geocells=gp, bank=bank, ref=ref)


def model_of(env, base=None, **kw):
    from pigeon_amd.super_guessr import SuperGuessr
    W, b = env["syn"].make_head_weights(CELLS, seed=1)
    m = SuperGuessr(base, panorama=True, freeze_base=True, num_candidates=5, geocell_path=env["geocells"], **kw)
    with torch.no_grad():
        m.cell_layer.weight.copy_(W * 64.0); m.cell_layer.bias.copy_(b)
    return m.to(DEV).eval()


def queries(env, n, seed=0):
    """(n,4,1024) panel embeddings near bank rows"""
    g = torch.Generator().manual_seed(seed)
    te = torch.as_tensor(np.asarray(env["bank"].train_emb))
    rows = torch.randint(0, te.shape[0], (n,), generator=g)
    return (te[rows][:, None, :] + 0.05 * torch.randn((n, 4, 1024), generator=g)).contiguous()


def test_from_refiner_borrows_the_bank(env):
    from pigeon_amd.neighbours import EmbeddingIndex, index_of
    ref = env["ref"]
    index = EmbeddingIndex.from_refiner(ref)
    t = ref._device_bank(torch.device(DEV)).t
    assert index.embeddings.data_ptr() == t["train_emb"].data_ptr() and index.lnglat.data_ptr() == t["train_lnglat"].data_ptr()
    assert len(index) == t["train_emb"].shape[0] and index.bank.x16.shape == (len(index), 1024) and index.bank.bad_values == 0
    assert index_of(ref, 3) is index_of(ref, 5)                                 # built once, kept on the refiner
    q = queries(env, 9)
    nn = index.search(q, k=4)
    ex = index.search(q, k=4, exact=True)
    assert nn.rows.shape == (9, 4) and nn.rows.dtype == torch.int64 and nn.lnglat.shape == (9, 4, 2) and nn.certified.dtype == torch.bool
    assert torch.equal(nn.rows, ex.rows) and torch.equal(nn.d2.view(torch.int32), ex.d2.view(torch.int32)) and bool(ex.certified.all())
    assert torch.equal(nn.lnglat, t["train_lnglat"][nn.rows]) and torch.equal(nn.distance, nn.d2.sqrt())
    # against torch on the panel means
    qm = q.to(DEV).mean(dim=1)
    d = torch.cdist(qm.double(), t["train_emb"].double()) ** 2
    assert torch.equal(nn.rows[:, 0], d.argmin(dim=1))
    st = index.stats
    assert st["queries"] == 9 and st["certified"] + st["fallback"] == 9 and st["certified"] == int(nn.certified.sum())
    # a bank row against the bank, with and without itself
    own = index.search(t["train_emb"][:5], k=2)
    assert own.rows[:, 0].tolist() == [0, 1, 2, 3, 4] and bool((own.d2[:, 0] == 0).all())
    loo = index.search(t["train_emb"][:5], k=1, exclude=torch.arange(5))
    assert torch.equal(loo.rows[:, 0], own.rows[:, 1])


def test_evaluate_model_neighbours(env):
    from pigeon_amd.evaluate import compute_geoguessr_metrics, evaluate_model, geoguessr_score
    from pigeon_amd.geo_utils import haversine_np
    from pigeon_amd.neighbours import index_of
    m, ref = model_of(env), env["ref"]
    emb = queries(env, 10, seed=3)
    cen = m.lla_geocells.data.cpu().numpy()
    labels = np.stack([cen[(7 * i) % CELLS] + [0.3 * i, -0.2 * i] for i in range(10)])
    data = [dict(embedding=emb[i], labels=torch.from_numpy(labels[i]), labels_clf=torch.tensor((7 * i) % CELLS)) for i in range(10)]

    class Columns(list):
        def __getitem__(self, i):
            return np.stack([np.asarray(d[i]) for d in self]) if isinstance(i, str) else list.__getitem__(self, i)

    new = {"nn_rows", "nn_distance", "nn_lnglat", "nn_certified", "Mean_km_error_nn", "Median_km_error_nn", "Geoguessr_score_nn", "NN_beats_model"}
    plain = evaluate_model(m, Columns(data), compute_geoguessr_metrics, refiner=ref, batch_size=4)
    none = evaluate_model(m, Columns(data), compute_geoguessr_metrics, refiner=ref, batch_size=4, neighbours=None)
    got = evaluate_model(m, Columns(data), compute_geoguessr_metrics, refiner=ref, batch_size=4, neighbours=3)
    assert not new & set(plain) and set(none) == set(plain) and set(got) == set(plain) | new
    for k, v in plain.items():                                                  # every existing key as before
        if k == "exact_passes":
            continue
        for other in (none, got):
            assert np.array_equal(np.asarray(other[k]), np.asarray(v), equal_nan=True) if not isinstance(v, (int, float)) else other[k] == v, k
    want = index_of(ref, 3).search(emb, k=3, exact=True)
    assert np.array_equal(got["nn_rows"], want.rows.cpu().numpy()) and np.array_equal(got["nn_distance"], want.distance.cpu().numpy())
    assert got["nn_rows"].shape == (10, 3) and got["nn_lnglat"].shape == (10, 3, 2) and got["nn_certified"].shape == (10,)
    tl = np.asarray(env["bank"].train_lnglat, np.float32)
    assert np.array_equal(got["nn_lnglat"], tl[got["nn_rows"]])
    d = haversine_np(tl[got["nn_rows"][:, 0]].astype(np.float64), labels)
    assert got["Mean_km_error_nn"] == np.mean(d) and got["Median_km_error_nn"] == np.median(d) and got["Geoguessr_score_nn"] == geoguessr_score(d)
    assert got["NN_beats_model"] == float(np.mean(d < haversine_np(got["preds"], labels)))
    bare = evaluate_model(m, [dict(embedding=x["embedding"]) for x in data], refiner=ref, batch_size=4, neighbours=2)
    assert "Mean_km_error_nn" not in bare and bare["nn_rows"].shape == (10, 2)   # no labels: the columns only
    with pytest.raises(ValueError, match="refiner"):
        evaluate_model(m, Columns(data), refiner=None, neighbours=3)


def test_command_line(env, capsys):
    from pigeon_amd import neighbours as nb
    te = np.asarray(env["bank"].train_emb, np.float32).copy()
    tl = np.asarray(env["bank"].train_lnglat, np.float32)
    te[40] = te[17]                                                             # a planted duplicate
    bank = os.path.join(env["tmp"], "bank.npz")
    np.savez(bank, train_emb=te, train_lnglat=tl)
    q = queries(env, 6, seed=8).numpy()
    qp, out = os.path.join(env["tmp"], "q.npy"), os.path.join(env["tmp"], "nn.npz")
    np.save(qp, q)
    assert nb.main(["--bank", bank, "--queries", qp, "-k", "5", "-o", out, "--batch", "4"]) == 0
    z = np.load(out)
    index = nb.EmbeddingIndex(te, tl)
    want = index.search(q, k=5, exact=True)
    assert np.array_equal(z["rows"], want.rows.cpu().numpy()) and np.array_equal(z["d2"], want.d2.cpu().numpy())
    assert np.array_equal(z["distance"], np.sqrt(z["d2"])) and np.array_equal(z["lnglat"], tl[z["rows"]]) and z["certified"].shape == (6,)
    capsys.readouterr()
    dup = os.path.join(env["tmp"], "dup.npz")
    assert nb.main(["--bank", bank, "--self", "-k", "2", "-o", dup, "--batch", "100"]) == 0
    printed = capsys.readouterr().out
    z = np.load(dup)
    assert z["rows"].shape == (te.shape[0], 2) and not (z["rows"] == np.arange(te.shape[0])[:, None]).any()
    assert z["rows"][17, 0] == 40 and z["rows"][40, 0] == 17 and z["d2"][17, 0] == 0 and z["d2"][40, 0] == 0
    assert int((z["d2"][:, 0] == 0).sum()) == 2 and "2 rows have a neighbour at distance 0" in printed


def test_predict_panorama_neighbours(env):
    from pigeon_amd import serve
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    from pigeon_amd.neighbours import index_of
    vit = HipCLIPVisionModel(env["syn"].make_vit_weights(seed=0, layers=2), layers=2).to(DEV)
    m, ref = model_of(env, vit, exact_top1=False), env["ref"]
    px = env["syn"].make_pixels(4, seed=9, panorama=True).to(DEV).reshape(4, 3, 336, 336)
    plain = serve.predict_panorama([None] * 4, m, ref, preprocess=lambda views: px)
    res = serve.predict_panorama([None] * 4, m, ref, preprocess=lambda views: px, neighbours=3)
    assert "neighbours" not in plain and {k: v for k, v in res.items() if k != "neighbours"} == plain
    nn = res["neighbours"]
    assert len(nn) == 3 and all(set(n) == {"lat", "lng", "distance", "row"} for n in nn)
    want = index_of(ref, 3).search(m.last_state["embedding"], k=3, exact=True)
    tl = np.asarray(env["bank"].train_lnglat, np.float32)
    assert [n["row"] for n in nn] == want.rows[0].tolist() and [n["distance"] for n in nn] == want.distance[0].tolist()
    assert all(n["lng"] == float(tl[n["row"], 0]) and n["lat"] == float(tl[n["row"], 1]) for n in nn)
    with pytest.raises(ValueError, match="refiner"):
        serve.predict_panorama([None] * 4, m, None, preprocess=lambda views: px, neighbours=3)
