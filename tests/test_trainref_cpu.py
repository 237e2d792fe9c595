"""tests/_trainref.py pinned, without a GPU: the restated loss against the value the real reference recorded (tests/golden/head.npz),
the restated gradient against a finite difference of the restated loss, the restated AdamW against torch.optim.AdamW, and every
planted mistake rejected at a named row, cell or column.  Also what needs no GPU of the new surface: HeadTrainer's and train_model's
refusals, the bindings' refusals and the PG_EINVAL argument checks of the three C entry points (made before any HIP call)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import _trainref as T

TAU = 65.0


def small_case(seed=3, B=3, Cn=5, P=4):
    rng = np.random.default_rng(seed)
    cen = np.array([10.0, 45.0]) + rng.normal(0, 0.6, (Cn, 2))      # neighbours within a few tau: the targets sum to more than 1
    cells = rng.integers(0, Cn - 1, B)                   # never the last cell: an off-by-one label stays inside [0, C)
    cells[1] = (cells[0] + 1) % (Cn - 1)                # neighbouring rows differ
    labels = cen[cells] + rng.normal(0, 0.3, (B, 2))
    emb = rng.normal(0.1, 0.7, (B, P, 1024)).astype(np.float32)
    W = rng.uniform(-1, 1, (Cn, 1024)).astype(np.float32) / 32
    bias = rng.uniform(-1, 1, Cn).astype(np.float32) / 32
    mom = dict(m_W=rng.normal(0, 1e-3, W.shape), v_W=rng.uniform(0, 1e-5, W.shape), m_b=rng.normal(0, 1e-3, Cn), v_b=rng.uniform(0, 1e-5, Cn))
    return dict(cen=cen, cells=cells, labels=labels, emb=emb, W=W, bias=bias, mom=mom)


# ================================================================================================================ pins
def test_restated_smoothed_loss_is_the_references(golden_dir):
    """head.npz: loss_clf_smooth came from the real reference (fp32 logits, fp64 targets).  1e-6 relative: its fp32 logits and these
    (torch's fp32 matmul here) differ by fp32 summation order"""
    from pigeon_amd import synthetic
    g = np.load(os.path.join(golden_dir, "head.npz"))
    Cn, seed, B, eseed, _ = [int(x) for x in g["meta"]]
    W, b = synthetic.make_head_weights(Cn, seed=seed)
    emb = torch.randn((B, 4, 1024), generator=torch.Generator().manual_seed(eseed)) * 0.7 + 0.1
    logits = (emb.mean(dim=1) @ W.t() + b).numpy()
    y, rel = T.targets_smooth(g["smooth_labels_in"], synthetic.make_geocells(Cn, seed=0), TAU)
    r = T.row_truth(logits, y, rel, 1.0 / B)
    assert abs(r["loss"].mean() / float(g["loss_clf_smooth"]) - 1) < 1e-6, (r["loss"].mean(), float(g["loss_clf_smooth"]))
    dropped = T.row_truth(logits, y, rel, 1.0 / B, use_S=False)
    assert abs(dropped["loss"].mean() / float(g["loss_clf_smooth"]) - 1) > 1e-3, "the factor S does not show in this fixture"


def test_restated_gradient_is_the_finite_difference_of_the_restated_loss():
    c = small_case()
    for y in (T.targets_smooth(c["labels"], c["cen"], TAU)[0], T.targets_onehot(c["cells"], 5)[0]):
        l = T.logits_of(T.xbar_of(c["emb"]), c["W"], c["bias"]).astype(np.float64)
        g = T.grad_of(l, y)
        h = T.LD(1e-6)
        for b in range(l.shape[0]):
            for k in range(l.shape[1]):
                lp, lm = l.astype(T.LD), l.astype(T.LD)
                lp[b, k] += h; lm[b, k] -= h
                fd = (T.loss_of(lp, y)[b] - T.loss_of(lm, y)[b]) / (2 * h)
                assert abs(fd - g[b, k]) <= 1e-7 * np.abs(g[b]).max(), (b, k, fd, g[b, k])
        r = T.row_truth(l.astype(np.float32), y, np.zeros(y.shape), 1.0)
        assert np.abs(r["g"] - g.astype(np.float64)).max() < 1e-15


def test_restated_adamw_is_torch_optim_adamw():
    """five steps, float64, 1e-14: the optimiser is pinned to torch, not to a formula"""
    rng = np.random.default_rng(5)
    for wd in (0.01, 0.0):
        w0 = rng.normal(0, 0.05, (5, 7))
        p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
        opt = torch.optim.AdamW([p], lr=1e-3, weight_decay=wd)
        w, m, v = w0.copy(), np.zeros_like(w0), np.zeros_like(w0)
        for t in range(1, 6):
            d = rng.normal(0, 1, w0.shape) * 10.0 ** rng.uniform(-9, 0, w0.shape)
            d[0, 0] = 0.0
            p.grad = torch.from_numpy(d.copy())
            opt.step()
            u = T.adamw_truth(w, m, v, d, t, lr=1e-3, wd=wd)
            w, m, v = u["w"], u["m"], u["v"]
            assert np.abs(w - p.detach().numpy()).max() <= 1e-14, (wd, t, np.abs(w - p.detach().numpy()).max())
            st = opt.state[p]
            assert np.abs(m - st["exp_avg"].numpy()).max() <= 1e-14 and np.abs(v - st["exp_avg_sq"].numpy()).max() <= 1e-14


def test_chain32_is_exact_on_integers_and_ordered():
    rng = np.random.default_rng(9)
    A, Bm = rng.integers(-8, 9, (5, 40)).astype(np.float32), rng.integers(-8, 9, (7, 40)).astype(np.float32)
    assert np.array_equal(T.chain32(A, Bm).astype(np.int64), A.astype(np.int64) @ Bm.astype(np.int64).T)
    big = np.array([[2.0 ** 24, 1.0, 1.0, -2.0 ** 24]], dtype=np.float32)       # ascending order: the two ones are absorbed
    assert T.chain32(big, np.ones((1, 4), dtype=np.float32))[0, 0] == 0.0
    e = rng.normal(0, 1, (3, 4, 1024)).astype(np.float32)
    assert np.array_equal(T.xbar_of(e), (((np.float32(0) + e[:, 0]) + e[:, 1]) + e[:, 2] + e[:, 3]) * np.float32(0.25))


# ================================================================================================================ planted mistakes
def _step(c, y, rel, t=2, mistake=None):
    return T.step_truth(c["emb"], c["W"], c["bias"], y=y, rel_y=rel, t=t, mistake=mistake, lr=1e-3, **c["mom"])


CHECKS = (("loss", "loss_bound", ("row",)), ("g", "g_bound", ("row", "cell")), ("W", "W_bound", ("cell", "column")),
          ("bias", "bias_bound", ("cell",)))


def _all_offenders(got, truth):
    out = []
    for k, bk, axes in CHECKS:
        out += T.offenders(k, got[k], truth[k], truth[bk], axes)
    return out


@pytest.mark.parametrize("mistake", T.MISTAKES)
def test_planted_mistake_is_rejected_at_a_named_place(mistake):
    c = small_case()
    B, Cn = 3, 5
    smooth = T.targets_smooth(c["labels"], c["cen"], TAU)
    onehot = T.targets_onehot(c["cells"], Cn)
    y, rel = onehot if mistake == "onehot_off_by_one" else smooth
    truth = _step(c, y, rel)
    assert not _all_offenders(truth, truth)
    if mistake == "no_rowmin":
        got = _step(c, *T.targets_smooth(c["labels"], c["cen"], TAU, subtract_min=False))
    elif mistake == "onehot_off_by_one":
        got = _step(c, *T.targets_onehot(c["cells"], Cn, shift=1))
    elif mistake == "neighbour_label":
        got = _step(c, *T.targets_smooth(np.roll(c["labels"], -1, axis=0), c["cen"], TAU))
    else:
        got = _step(c, y, rel, mistake=mistake)
    bad = _all_offenders(got, truth)
    assert bad, f"{mistake}: not rejected"
    where = {"S_dropped": "loss[row", "no_rowmin": "loss[row", "no_1_over_B": "g[row", "g_transposed": "W[cell",
             "bias_correction_t_minus_1": "W[cell", "coupled_decay": "W[cell", "betas_swapped": "W[cell", "bias_not_updated": "bias[cell",
             "onehot_off_by_one": "g[row", "neighbour_label": "loss[row"}[mistake]
    assert any(s.startswith(where) for s in bad), (mistake, bad[:3])
    if mistake == "bias_not_updated":
        assert all(s.startswith("bias[cell") for s in bad), bad[:3]
    if mistake == "neighbour_label":                     # rows 0 and 1 have different labels: both named
        assert any(s.startswith("loss[row 0]") for s in bad) and any(s.startswith("loss[row 1]") for s in bad)
    if mistake == "bias_correction_t_minus_1":           # t = 1: a division by 1 - beta^0 = 0
        first = T.offenders("W", _step(c, y, rel, t=1, mistake=mistake)["W"], _step(c, y, rel, t=1)["W"], _step(c, y, rel, t=1)["W_bound"],
                            ("cell", "column"))
        assert len(first) == c["W"].size


def test_bounds_are_about_fp32_rounding():
    """the derived bounds are of the order of the output format's rounding, not loose: g within 4 fp32 ulp; w, whose update term carries
    the rounding of m' / q at the size of the step, five orders below the lr-sized movement of a semantic mistake"""
    c = small_case()
    t = _step(c, *T.targets_smooth(c["labels"], c["cen"], TAU))
    assert (t["g_bound"] <= 4 * T.ulp32(t["g"]) + 2 * T.TINY32).all()
    assert (t["W_bound"] <= 8 * T.ulp32(t["W"]) + 1e-5 * 1e-3).all()


# ================================================================================================================ refusals, no GPU
def test_head_trainer_refusals(tmp_path):
    from pigeon_amd import synthetic
    from pigeon_amd.super_guessr import SuperGuessr
    from pigeon_amd.train import HeadTrainer, finetune_on_embeddings, train_model
    from pigeon_amd.config import TrainArgs
    for kw, word in ((dict(base_model=object()), "base model"), (dict(base_model=None, multi_task=True), "multi_task"),
                     (dict(base_model=None, multi_task=False, hierarchical=True), "hierarchical")):
        with pytest.raises(NotImplementedError, match=word):
            HeadTrainer(types.SimpleNamespace(**kw))
    geo = str(tmp_path / "geocells.csv")
    synthetic.write_geocell_csv(geo, synthetic.make_geocells(7, seed=1))
    model = SuperGuessr(None, panorama=True, should_smooth_labels=True, geocell_path=geo)
    with pytest.raises(RuntimeError, match="GPU only"):
        HeadTrainer(model)                               # weights on the CPU: no fallback
    with pytest.raises(NotImplementedError, match="on_embeddings=False"):
        train_model(model, {}, False, False, TrainArgs())
    with pytest.raises(NotImplementedError, match="gradient_accumulation_steps"):
        train_model(model, {}, True, False, TrainArgs(gradient_accumulation_steps=2))
    with pytest.raises(NotImplementedError, match="multi_task"):
        finetune_on_embeddings({}, True, False, False)
    a = TrainArgs()
    assert (a.learning_rate, a.per_device_train_batch_size, a.per_device_eval_batch_size, a.num_train_epochs, a.seed) == (2e-5, 256, 256, 1000, 330)


def test_bindings_refuse_by_name():
    from pigeon_amd import hip_ops
    from pigeon_amd._lib import PigeonHipError
    z = torch.zeros
    with pytest.raises(PigeonHipError, match="device tensor"):
        hip_ops.head_train_loss(z(2, 4, 1024), z(3, 1024), z(3), z(3, 2, dtype=torch.float64), labels_clf=z(2, dtype=torch.int64))
    with pytest.raises(PigeonHipError, match="device tensor"):
        hip_ops.head_train_update(z(2, 3), z(2, 1024), z(3, 1024), z(3), z(3, 1024), z(3, 1024), z(3), z(3), 1)


def test_entry_points_refuse_bad_arguments_before_any_hip_call(hip_lib):
    """PG_EINVAL with a message naming the argument; nothing here touches a device"""
    L = hip_lib
    one = C.c_void_p(16)                                 # a non-null pointer that is never dereferenced: every call below is refused

    def loss(B=2, P=4, Cn=3, tau=65.0, scale=0.5, emb=one, W=one, bias=one, cen=one, llh=one, clf=None, xbar=one, g=one, rows=one):
        return L.pg_head_train_loss(emb, B, P, W, bias, cen, Cn, llh, clf, tau, scale, xbar, g, rows, None, None)

    def update(B=2, Cn=3, step=1, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.01, g=one, xbar=one, W=one, bias=one, mW=one, vW=one, mb=one,
               vb=one):
        return L.pg_head_train_update(g, xbar, B, Cn, W, bias, mW, vW, mb, vb, step, lr, b1, b2, eps, wd, None, None, None)

    def refused(rc, word):
        assert rc == -1, rc
        assert word in L.pg_last_error().decode(), (word, L.pg_last_error())

    refused(loss(B=-1), "B = -1")
    refused(loss(Cn=0), "C must be at least 1")
    for P in (0, 2, 3, 5):
        refused(loss(P=P), "P must be 1 or 4")
    for tau in (0.0, -1.0, float("inf"), float("nan")):
        refused(loss(tau=tau), "tau")
    refused(loss(scale=float("nan")), "grad_scale")
    for name in ("emb", "W", "bias", "xbar", "g"):
        refused(loss(**{name: None}), f"null argument {name}")
    refused(loss(rows=None), "null argument loss_rows")
    refused(loss(cen=None), "null argument centroids")
    refused(loss(llh=None, clf=None), "labels_llh and labels_clf")
    assert loss(B=0, emb=None, W=None, g=None) == 0      # an empty batch is a no-op
    refused(update(B=-1), "B = -1")
    refused(update(Cn=0), "C must be at least 1")
    refused(update(step=0), "step")
    for lr in (0.0, -1e-3, float("inf"), float("nan")):
        refused(update(lr=lr), "lr")
    for eps in (0.0, -1e-8, float("nan")):
        refused(update(eps=eps), "eps")
    refused(update(b1=1.0), "beta1")
    refused(update(b2=-0.1), "beta2")
    refused(update(wd=-1.0), "weight_decay")
    for name, arg in (("g", "g"), ("xbar", "xbar"), ("W", "W"), ("bias", "bias"), ("mW", "m_W"), ("vW", "v_W"), ("mb", "m_b"), ("vb", "v_b")):
        refused(update(**{name: None}), f"null argument {arg}")
    assert update(B=0, g=None, W=None) == 0
    out = (C.c_int32 * 4)()
    refused(L.pg_head_train_plan(0, out), "C must be at least 1")
    refused(L.pg_head_train_plan(5, None), "null argument out")
    assert L.pg_head_train_plan(5, out) == 0 and list(out) == [0, 40, out[2], 256]
    top = out[2]
    assert L.pg_head_train_plan(top, out) == 0 and out[0] == 0 and out[1] == 8 * top
    assert L.pg_head_train_plan(top + 1, out) == 0 and out[0] == 1 and out[1] == 0
