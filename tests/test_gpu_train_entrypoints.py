"""pigeon_amd.train on the GPU (run with -m gpu on an MI355X): HeadTrainer learns a separable set, keeps the model's caches honest,
resumes from its state dict; train_model saves on improvement, stops on patience and writes a file that `load_state` and
`evaluate(base_model=None)` read; the single-image (yfcc) and the one-hot routes train too."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
C = 17


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    from pigeon_amd import _lib, synthetic
    from pigeon_amd.train import synthetic_dataset
    _lib.require_gpu()
    ds, cen = synthetic_dataset(128, C, seed=7, panorama=True)
    geo = str(tmp_path_factory.mktemp("train") / "geocells.csv")
    synthetic.write_geocell_csv(geo, cen)
    cols = ds["train"].columns
    return dict(ds=ds, geo=geo, emb=cols["embedding"][:64].to(DEV), labels=cols["labels"][:64].to(DEV), clf=cols["labels_clf"][:64].to(DEV))


def model_of(world, **kw):
    from pigeon_amd.super_guessr import SuperGuessr
    kw.setdefault("panorama", True)
    torch.manual_seed(1234)                              # nn.Linear's initialisation: the same head every time
    return SuperGuessr(None, geocell_path=world["geo"], **kw).to(DEV)


def test_trainer_learns_a_separable_set_and_the_caches_follow(world, tmp_path):
    from pigeon_amd.train import HeadTrainer
    model = model_of(world, should_smooth_labels=True)
    trainer = HeadTrainer(model, lr=1e-2)
    before = model.wstats().clone()
    v0 = model.cell_layer.weight._version, model.cell_layer.bias._version
    losses = [trainer.step(world["emb"], world["labels"], world["clf"]) for _ in range(40)]
    assert all(l.dim() == 0 and l.is_cuda and l.dtype == torch.float64 for l in losses)
    losses = torch.stack(losses).cpu().numpy()
    assert np.isfinite(losses).all() and losses[-1] < 0.5 * losses[0], losses
    assert model.cell_layer.weight._version >= v0[0] + 40 and model.cell_layer.bias._version >= v0[1] + 40
    model.eval()
    out = model(embedding=world["emb"], labels=world["labels"], labels_clf=world["clf"])
    assert torch.equal(out.preds_geocell, world["clf"]), "a training row of a separable set is misclassified after 40 steps"
    # wstats() is keyed on the weight's version: after a step it is what a fresh model loaded from the saved weights computes
    path = str(tmp_path / "head.model")
    torch.save(model.state_dict(), path)
    fresh = model_of(world, should_smooth_labels=True)
    fresh.load_state(path)
    after = model.wstats()
    assert torch.equal(after, fresh.wstats()) and not torch.equal(after, before)
    # resuming: a trainer restored from state_dict() continues bit for bit
    sd = trainer.state_dict()
    twin = HeadTrainer(fresh, lr=1.0)
    twin.load_state_dict(sd)
    assert twin.t == 40 and twin.lr == 1e-2
    a, b = trainer.step(world["emb"], world["labels"], world["clf"]), twin.step(world["emb"], world["labels"], world["clf"])
    assert torch.equal(a, b) and torch.equal(model.cell_layer.weight.data, fresh.cell_layer.weight.data)
    assert torch.equal(trainer.v_W, twin.v_W) and torch.equal(model.cell_layer.bias.data, fresh.cell_layer.bias.data)


def test_train_model_saves_on_improvement_and_stops_on_patience(world, tmp_path):
    from pigeon_amd.config import TrainArgs
    from pigeon_amd.evaluate import evaluate
    from pigeon_amd.train import train_model
    path = str(tmp_path / "best.model")
    model = model_of(world, should_smooth_labels=True)
    args = TrainArgs(num_train_epochs=6, learning_rate=1e-2, per_device_train_batch_size=16, per_device_eval_batch_size=32, seed=3)
    out = train_model(model, world["ds"], True, False, args, None, patience=1, save_path=path)
    log = out.train_log
    assert out is model and log[0]["saved"] and not log[-1]["saved"] and 2 <= len(log) < 6, log       # the last epoch did not improve: patience
    assert all(np.isfinite(r["train_loss"]) for r in log) and log[-1]["train_loss"] < log[0]["train_loss"]
    best = min(r["eval_loss"] for r in log)
    assert best <= -0.9, log                                                   # a separable set: the validation rows are found
    fresh = model_of(world, should_smooth_labels=True)
    fresh.load_state(path)                                                     # the file is the best epoch's state dict
    assert set(torch.load(path, map_location="cpu")) == {"lla_geocells", "cell_layer.weight", "cell_layer.bias"}
    res = evaluate(path, world["ds"]["val"], yfcc=False, landmarks=False, base_model=None, refine=False, geocell_path=world["geo"])
    assert abs(res["Geocell_accuracy"] + best) < 1e-12, (res["Geocell_accuracy"], best)
    # the same seed gives the same run
    again = train_model(model_of(world, should_smooth_labels=True), world["ds"], True, False, args, None, patience=1, save_path=str(tmp_path / "b2.model"))
    assert [r["train_loss"] for r in again.train_log] == [r["train_loss"] for r in log]


def test_single_image_route(world):
    """yfcc: (B,1024) embeddings, P = 1"""
    from pigeon_amd.train import HeadTrainer
    model = model_of(world, panorama=False, yfcc=True, should_smooth_labels=True)
    trainer = HeadTrainer(model, lr=1e-2)
    emb = world["emb"][:, 0].contiguous()
    losses = torch.stack([trainer.step(emb, world["labels"], world["clf"]) for _ in range(30)]).cpu().numpy()
    assert losses[-1] < 0.5 * losses[0], losses
    model.eval()
    assert torch.equal(model(embedding=emb, labels_clf=world["clf"]).preds_geocell, world["clf"])


def test_one_hot_route(world):
    """should_smooth_labels=False: the targets come from labels_clf; the first loss is torch's cross entropy of the same logits"""
    from pigeon_amd.train import HeadTrainer
    model = model_of(world, should_smooth_labels=False)
    model.eval()
    ref = float(model(embedding=world["emb"], labels=world["labels"], labels_clf=world["clf"]).loss_clf)
    trainer = HeadTrainer(model, lr=1e-2)
    losses = torch.stack([trainer.step(world["emb"], world["labels"], world["clf"]) for _ in range(30)]).cpu().numpy()
    assert abs(losses[0] / ref - 1) < 1e-5, (losses[0], ref)
    assert losses[-1] < 0.5 * losses[0], losses
    with pytest.raises(ValueError, match="labels_clf"):
        trainer.step(world["emb"], world["labels"], None)


def test_bindings_refuse_wrong_tensors_by_name(world):
    """device tensors of the wrong dtype, shape or layout never reach the library"""
    from pigeon_amd import hip_ops
    from pigeon_amd._lib import PigeonHipError
    z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device=DEV)      # noqa: E731
    emb, W, bias, cen, clf = z(2, 4, 1024), z(C, 1024), z(C), z(C, 2, dt=torch.float64), z(2, dt=torch.int64)
    for kw, word in ((dict(emb=z(2, 4, 1024, dt=torch.float64)), "dtype"), (dict(emb=z(2, 3, 1024)), "3 panels"), (dict(emb=z(2, 4, 512)), "emb must have shape"),
                     (dict(W=z(C, 1000)), "W must have shape"), (dict(bias=z(C + 1)), "bias must have shape"),
                     (dict(cen=z(C, 2)), "dtype"), (dict(cen=z(C + 1, 2, dt=torch.float64)), "centroids must have shape"),
                     (dict(clf=z(2, dt=torch.int32)), "dtype"), (dict(clf=z(3, dt=torch.int64)), "labels_clf must have shape"),
                     (dict(emb=z(2, 4, 2048)[:, :, ::2]), "contiguous")):
        a = dict(emb=emb, W=W, bias=bias, cen=cen, clf=clf); a.update(kw)
        with pytest.raises(PigeonHipError, match=word):
            hip_ops.head_train_loss(a["emb"], a["W"], a["bias"], a["cen"], labels_clf=a["clf"])
    with pytest.raises(PigeonHipError, match="labels_llh must have shape"):
        hip_ops.head_train_loss(emb, W, bias, cen, labels_llh=z(2, 3, dt=torch.float64))
    with pytest.raises(PigeonHipError, match="one of labels_llh and labels_clf"):
        hip_ops.head_train_loss(emb, W, bias, cen)
    with pytest.raises(PigeonHipError, match="g must have shape"):
        hip_ops.head_train_loss(emb, W, bias, cen, labels_clf=clf, out={"g": z(2, C + 1)})
    g, xbar, st = z(2, C), z(2, 1024), [z(C, 1024), z(C), z(C, 1024), z(C, 1024), z(C), z(C)]
    for i, word in ((0, "W must have shape"), (1, "bias must have shape"), (2, "m_W must have shape"), (5, "v_b must have shape")):
        bad = list(st); bad[i] = z(C + 1, 1024) if bad[i].dim() == 2 else z(C + 1)
        with pytest.raises(PigeonHipError, match=word):
            hip_ops.head_train_update(g, xbar, *bad, 1)
    with pytest.raises(PigeonHipError, match="xbar must have shape"):
        hip_ops.head_train_update(g, z(3, 1024), *st, 1)
    with pytest.raises(PigeonHipError, match="dW_out must have shape"):
        hip_ops.head_train_update(g, xbar, *st, 1, dW_out=z(C, 1000))
    with pytest.raises(PigeonHipError, match="step"):
        hip_ops.head_train_update(g, xbar, *st, 0)
