"""pg_head_train_loss / pg_head_train_update on the GPU (run with -m gpu on an MI355X) against tests/_trainref.py: the logits and the
panel mean are pg_head_forward's bits, exact inputs give exact outputs (torch.equal), the row kernel is held element by element to
the derived bounds, rows and cells keep their bits wherever they stand, AdamW is held elementwise, and six steps are held to the
reference's own fp32-against-fp64 deviation (tests/golden/head_train.npz, written by tests/make_head_train_golden.py)."""
import os

import numpy as np
import pytest
import torch

import _georef as G
import _trainref as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
CELLS = (1, 2, 63, 64, 65, 257, 2076)
BATCHES = (1, 3, 17, 65, 257)
TAU = 65.0


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops
    _lib.require_gpu()
    return dict(lib=_lib, ops=hip_ops, top=hip_ops.head_train_plan(1)["lds_cells"])


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def centroids_of(Cn, seed):
    rng = np.random.default_rng([seed, Cn])
    return np.stack([rng.uniform(-180, 180, Cn), rng.uniform(-89, 89, Cn)], axis=1)


def head_of(Cn, seed, gain=8.0):
    rng = np.random.default_rng([seed, Cn, 1])
    return (rng.uniform(-1, 1, (Cn, 1024)) * gain / 32).astype(np.float32), rng.uniform(-1, 1, Cn).astype(np.float32)


def emb_of(B, P, seed):
    return (np.random.default_rng([seed, B, P]).normal(0.1, 0.7, (B, P, 1024))).astype(np.float32)


def guarded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * G.GUARD,), G.SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[G.GUARD:G.GUARD + n].view(shape)


def guards_intact(buf, n):
    return bool((buf[:G.GUARD] == G.SENTINEL).all()) and bool((buf[G.GUARD + n:] == G.SENTINEL).all())


def loss_call(env, emb, W, bias, cen, llh=None, clf=None, tau=TAU, scale=1.0):
    """numpy in -> dict of device tensors (xbar, g, loss_rows, logits); outputs sit between guards, inputs must not change"""
    B, Cn = emb.shape[0], W.shape[0]
    ins = [dev(emb), dev(W), dev(bias), dev(cen)] + [dev(x) for x in (llh, clf) if x is not None]
    keep = [t.clone() for t in ins]
    bufs = {"xbar": guarded((B, 1024), torch.float32), "g": guarded((B, Cn), torch.float32), "loss_rows": guarded((B,), torch.float64),
            "logits": guarded((B, Cn), torch.float32)}
    out = env["ops"].head_train_loss(ins[0], ins[1], ins[2], ins[3], labels_llh=ins[4] if llh is not None else None,
                                     labels_clf=ins[4] if llh is None else None, tau=tau, grad_scale=scale,
                                     out={k: v[1] for k, v in bufs.items()})
    torch.cuda.synchronize()
    for k, (buf, view) in bufs.items():
        assert guards_intact(buf, view.numel()), f"{k}: wrote outside its output"
    for t, k in zip(ins, keep):
        assert torch.equal(t.view(torch.uint8), k.view(torch.uint8)), "an input changed"
    return out


def bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8))


def update_call(env, g, xbar, W, bias, mW, vW, mb, vb, t, want_grads=True, **hyper):
    """numpy in (copied) -> dict of device tensors W, bias, m_W, v_W, m_b, v_b (+ dW, db), each between guards"""
    Cn = W.shape[0]
    gd, xd = dev(g), dev(xbar)
    keep = gd.clone(), xd.clone()
    state = {}
    for k, a in (("W", W), ("m_W", mW), ("v_W", vW)):
        state[k] = guarded((Cn, 1024), torch.float32); state[k][1].copy_(dev(a))
    for k, a in (("bias", bias), ("m_b", mb), ("v_b", vb)):
        state[k] = guarded((Cn,), torch.float32); state[k][1].copy_(dev(a))
    if want_grads:
        state["dW"], state["db"] = guarded((Cn, 1024), torch.float32), guarded((Cn,), torch.float32)
    v = {k: s[1] for k, s in state.items()}
    env["ops"].head_train_update(gd, xd, v["W"], v["bias"], v["m_W"], v["v_W"], v["m_b"], v["v_b"], t, dW_out=v.get("dW"), db_out=v.get("db"),
                                 **hyper)
    torch.cuda.synchronize()
    for k, (buf, view) in state.items():
        assert guards_intact(buf, view.numel()), f"{k}: wrote outside its tensor"
    assert bits_equal(gd, keep[0]) and bits_equal(xd, keep[1]), "an input changed"
    return v


def zeros_state(Cn):
    return [np.zeros((Cn, 1024), np.float32), np.zeros(Cn, np.float32)] + [np.zeros((Cn, 1024), np.float32)] * 2 + [np.zeros(Cn, np.float32)] * 2


# ================================================================================================================ inference's bits
def _same_as_inference(env, B, Cn, P):
    emb, (W, bias), cen = emb_of(B, P, 1), head_of(Cn, 2), centroids_of(Cn, 3)
    clf = np.random.default_rng([4, B, Cn]).integers(0, Cn, B)
    out = loss_call(env, emb if P > 1 else emb[:, 0], W, bias, cen, clf=clf)
    e = dev(emb)
    inf = env["ops"].head_forward(e if P > 1 else e[:, 0].contiguous(), dev(W), dev(bias), dev(cen), 1)
    assert torch.equal(out["logits"], inf["logits"]), f"B = {B}, C = {Cn}, P = {P}: not pg_head_forward's logits"
    acc = torch.zeros((B, 1024), device=DEV)
    for p in range(P):
        acc = acc + e[:, p]
    assert torch.equal(out["xbar"], acc * (1.0 / P)), f"B = {B}, C = {Cn}, P = {P}: xbar"
    assert torch.equal(out["xbar"].cpu(), torch.from_numpy(T.xbar_of(emb)))


def test_logits_and_xbar_are_the_bits_inference_computes(env):
    for Cn in CELLS:
        for B in BATCHES:
            _same_as_inference(env, B, Cn, 4 if (B + Cn) % 2 else 1)
    _same_as_inference(env, 65, 257, 4); _same_as_inference(env, 65, 257, 1)


def test_logits_large_tile_kernel_is_the_bits_inference_computes(env):
    """ceil(B / 128) ceil(C / 128) >= 512 takes the 128 x 128 tiles: B = 257 (three row tiles, the last one row) needs 171 cell tiles"""
    _same_as_inference(env, 257, 171 * 128 - 5, 1)


# ================================================================================================================ exact inputs
def test_integer_embeddings_and_power_of_two_weights_give_integer_logits(env):
    for Cn, B, P in ((1, 3, 4), (2, 17, 1), (63, 65, 4), (65, 257, 4), (257, 65, 1), (2076, 17, 4)):
        rng = np.random.default_rng([11, Cn, B])
        emb = rng.integers(-4, 5, (B, P, 1024)).astype(np.float32)
        W = (rng.choice([-1.0, 1.0], (Cn, 1024)) * 2.0 ** rng.integers(-2, 3, (Cn, 1024)) * (rng.random((Cn, 1024)) < 0.9)).astype(np.float32)
        bias = rng.integers(-50, 51, Cn).astype(np.float32)
        out = loss_call(env, emb if P > 1 else emb[:, 0], W, bias, centroids_of(Cn, 3), clf=rng.integers(0, Cn, B))
        want = (emb.astype(np.float64).sum(axis=1) / P) @ W.astype(np.float64).T + bias          # multiples of 1/16 below 2^18: exact
        assert torch.equal(out["logits"].cpu().double(), torch.from_numpy(want)), f"C = {Cn}, B = {B}"


def _integer_gradients(env, B, Cn):
    rng = np.random.default_rng([12, Cn, B])
    g, xbar = rng.integers(-8, 9, (B, Cn)).astype(np.float32), rng.integers(-8, 9, (B, 1024)).astype(np.float32)
    v = update_call(env, g, xbar, *zeros_state(Cn), 1)
    assert torch.equal(v["dW"].cpu().long(), torch.from_numpy(g.astype(np.int64).T @ xbar.astype(np.int64))), f"dW, C = {Cn}, B = {B}"
    assert torch.equal(v["db"].cpu().long(), torch.from_numpy(g.astype(np.int64).sum(axis=0))), f"db, C = {Cn}, B = {B}"


def test_integer_g_and_xbar_give_the_integer_gradient(env):
    for Cn in CELLS:
        for B in BATCHES:
            _integer_gradients(env, B, Cn)


def test_integer_gradient_large_tile_kernel(env):
    """ceil(C / 128) * 8 >= 512 takes the 128 x 128 tiles; C = 8200 ends in a tile of 8 cells, B = 33 in a staging step of one row"""
    _integer_gradients(env, 33, 8200)


def test_one_hot_rows_of_g_copy_single_rows_of_xbar(env):
    """row b of g is 1 at cell perm[b] and 0 elsewhere: dW[perm[b]] is xbar[b] bit for bit, every other row of dW is zero"""
    for Cn, B in ((63, 17), (64, 64), (65, 65), (257, 65), (257, 257), (2076, 257), (8200, 65)):
        rng = np.random.default_rng([13, Cn, B])
        perm = rng.permutation(Cn)[:B]
        g = np.zeros((B, Cn), np.float32); g[np.arange(B), perm] = 1.0
        xbar = rng.normal(0, 1, (B, 1024)).astype(np.float32)
        v = update_call(env, g, xbar, *zeros_state(Cn), 1)
        want = np.zeros((Cn, 1024), np.float32); want[perm] = xbar
        got = v["dW"].cpu().numpy()
        wrong = np.argwhere(got != want)
        assert not len(wrong), f"C = {Cn}, B = {B}: first wrong (cell, column) {wrong[0]}; cell belongs to batch row {np.where(perm == wrong[0][0])[0]}"
        assert torch.equal(v["db"].cpu(), torch.from_numpy(g.sum(axis=0)))


def test_a_single_cell_has_no_gradient(env):
    for P in (1, 4):
        emb, (W, bias), cen = emb_of(5, P, 21), head_of(1, 22), centroids_of(1, 23)
        lab = np.stack([np.linspace(-170, 170, 5), np.linspace(-80, 80, 5)], axis=1)
        for kw in (dict(llh=lab), dict(clf=np.zeros(5, np.int64))):
            out = loss_call(env, emb if P > 1 else emb[:, 0], W, bias, cen, scale=0.2, **kw)
            assert torch.equal(out["g"], torch.zeros_like(out["g"]))
            assert torch.equal(out["loss_rows"], torch.zeros_like(out["loss_rows"]))


# ================================================================================================================ rows against _trainref
def held(env, capsys, emb, W, bias, cen, llh=None, clf=None, scale=0.25, tau=TAU, what=""):
    out = loss_call(env, emb, W, bias, cen, llh=llh, clf=clf, scale=scale, tau=tau)
    y, rel = T.targets_smooth(llh, cen, tau) if llh is not None else T.targets_onehot(clf, W.shape[0])
    t = T.row_truth(out["logits"].cpu().numpy(), y, rel, scale)
    g, loss = out["g"].cpu().numpy(), out["loss_rows"].cpu().numpy()
    rg, rl = np.abs(g - t["g"]) / t["g_bound"], np.abs(loss - t["loss"]) / t["loss_bound"]
    with capsys.disabled():
        print(f"\nhead_train rows {what}: worst |got - truth| / bound: g {rg.max():.3g}, loss {rl.max():.3g}")
    bad = T.offenders("g", g, t["g"], t["g_bound"], ("row", "cell")) + T.offenders("loss", loss, t["loss"], t["loss_bound"], ("row",))
    assert not bad, bad[:5]
    return out


def test_rows_against_the_restatement(env, capsys):
    for Cn in CELLS:
        B, P = 5, 4 if Cn % 2 else 1
        emb, (W, bias), cen = emb_of(B, P, 31), head_of(Cn, 32), centroids_of(Cn, 33)
        emb = emb if P > 1 else emb[:, 0]
        rng = np.random.default_rng([34, Cn])
        cells = rng.integers(0, Cn, B)
        llh = cen[cells] + rng.normal(0, 0.4, (B, 2))
        llh[0] = cen[cells[0]]                                               # a label on a centroid
        held(env, capsys, emb, W, bias, cen, llh=llh, what=f"smoothed, C = {Cn}")
        held(env, capsys, emb, W, bias, cen, clf=cells, what=f"one-hot, C = {Cn}")


def test_rows_across_the_antimeridian_at_a_pole_and_equidistant(env, capsys):
    Cn, B = 257, 4
    emb, (W, bias) = emb_of(B, 4, 41), head_of(Cn, 42)
    rng = np.random.default_rng(43)
    cen = np.stack([np.where(rng.random(Cn) < 0.5, 180 - rng.uniform(0, 1, Cn), -180 + rng.uniform(0, 1, Cn)), rng.uniform(-1, 1, Cn)], axis=1)
    llh = np.array([[179.9999, 0.2], [-179.9999, -0.3], [180.0, 0.0], [-180.0, 0.5]])
    held(env, capsys, emb, W, bias, cen, llh=llh, what="antimeridian")
    cen = np.stack([rng.uniform(-180, 180, Cn), 90 - rng.uniform(0, 2, Cn)], axis=1)
    cen[7] = [33.0, 90.0]
    llh = np.array([[0.0, 90.0], [123.0, 90.0], [-77.0, 89.5], [10.0, -90.0]])
    held(env, capsys, emb, W, bias, cen, llh=llh, what="poles")
    cen = np.stack([np.linspace(-180, 179, Cn), np.full(Cn, 60.0)], axis=1)  # one parallel: every cell as far from the pole as any other
    poles = np.array([[0.0, 90.0], [50.0, 90.0], [0.0, -90.0], [-120.0, -90.0]])
    assert abs(float(T.targets_smooth(poles, cen, TAU)[0].sum()) - 4 * Cn) < 1e-6          # every target is 1: S = C
    held(env, capsys, emb, W, bias, cen, llh=poles, what="equidistant")


def test_bad_labels_do_not_train(env):
    Cn, B = 65, 6
    emb, (W, bias), cen = emb_of(B, 4, 51), head_of(Cn, 52), centroids_of(Cn, 53)
    llh = cen[[1, 2, 3, 4, 5, 6]] + 0.1
    bad_llh = llh.copy()
    bad_llh[1, 0], bad_llh[3, 1], bad_llh[5] = np.nan, np.inf, [-np.inf, np.nan]
    good, out = loss_call(env, emb, W, bias, cen, llh=llh), loss_call(env, emb, W, bias, cen, llh=bad_llh)
    clf = np.array([0, Cn, 3, -1, 64, 2 ** 40], dtype=np.int64)
    ok_clf = np.array([0, 1, 3, 1, 64, 1], dtype=np.int64)
    good_c, out_c = loss_call(env, emb, W, bias, cen, clf=ok_clf), loss_call(env, emb, W, bias, cen, clf=clf)
    for o, ref in ((out, good), (out_c, good_c)):
        for b in (1, 3, 5):
            assert bool(torch.isnan(o["loss_rows"][b])) and bool((o["g"][b] == 0).all()), f"row {b} trained"
        for b in (0, 2, 4):                                                   # the other rows: the same bits as without the bad ones
            assert bits_equal(o["g"][b], ref["g"][b]) and bits_equal(o["loss_rows"][b], ref["loss_rows"][b]), f"row {b} was touched"
        assert bits_equal(o["logits"], ref["logits"])


def test_lds_and_scratch_forms_give_the_same_bits(env):
    """the largest LDS-form C against one cell more whose logit is -1e30 and whose target is 0 (one-hot: another cell; smoothed with
    tau = 1 km: the south pole, 10^4 km from every label): its thread adds +0 to S and Z and -0 to T, every other addition is the same"""
    top = env["top"]
    assert env["ops"].head_train_plan(top)["form"] == 0 and env["ops"].head_train_plan(top + 1)["form"] == 1
    B = 3
    rng = np.random.default_rng(61)
    cen = np.stack([rng.uniform(-180, 180, top + 1), rng.uniform(10, 80, top + 1)], axis=1)
    cen[top] = [0.0, -90.0]
    W, bias = head_of(top + 1, 62)
    W[top], bias[top] = 0.0, -1e30
    emb = emb_of(B, 4, 63)
    cells = np.array([0, top - 1, 255])
    llh = cen[cells] + 0.01
    for kw in (dict(clf=cells), dict(llh=llh, tau=1.0)):
        a = loss_call(env, emb, W[:top], bias[:top], cen[:top], **kw)
        b = loss_call(env, emb, W, bias, cen, **kw)
        assert bits_equal(a["loss_rows"], b["loss_rows"]), "loss_rows differ between the LDS and the scratch form"
        assert torch.equal(a["g"].view(torch.int32), b["g"][:, :top].contiguous().view(torch.int32)), "g differs between the two forms"
        assert bool((b["g"][:, top] == 0).all()) and bool(torch.isfinite(a["loss_rows"]).all())


# ================================================================================================================ determinism
def test_a_row_keeps_its_bits_at_every_position(env):
    for Cn in (65, 2076):
        cen, (W, bias) = centroids_of(Cn, 71), head_of(Cn, 72)
        emb = emb_of(17, 4, 73)
        llh = cen[np.arange(17) % Cn] + 0.2
        clf = (np.arange(17) * 7) % Cn
        for kw in ("llh", "clf"):
            lab = llh if kw == "llh" else clf
            alone = loss_call(env, emb[:1], W, bias, cen, scale=1 / 17, **{kw: lab[:1]})
            for pos in range(17):
                e, l = emb.copy(), lab.copy()
                e[[0, pos]], l[[0, pos]] = e[[pos, 0]], l[[pos, 0]]
                batch = loss_call(env, e, W, bias, cen, scale=1 / 17, **{kw: l})
                assert bits_equal(batch["g"][pos], alone["g"][0]) and bits_equal(batch["loss_rows"][pos], alone["loss_rows"][0]), (Cn, kw, pos)


def test_a_cell_keeps_its_bits_in_any_head(env):
    """cell 3 of C = 65, of C = 257 and of C = 8200 (the large-tile kernel), given the same g column, weights and moments"""
    B = 17
    rng = np.random.default_rng(81)
    xbar = rng.normal(0, 1, (B, 1024)).astype(np.float32)
    col = rng.normal(0, 1e-2, B).astype(np.float32)
    row = [rng.normal(0, 0.03, 1024).astype(np.float32), rng.normal(0, 1e-3, 1024).astype(np.float32), rng.uniform(0, 1e-5, 1024).astype(np.float32)]
    sc = [np.float32(0.01), np.float32(1e-3), np.float32(1e-6)]
    got = []
    for Cn in (65, 257, 8200):
        r = np.random.default_rng([82, Cn])
        g = r.normal(0, 1e-2, (B, Cn)).astype(np.float32); g[:, 3] = col
        W, mW, vW = (r.normal(0, 0.03, (Cn, 1024)).astype(np.float32), r.normal(0, 1e-3, (Cn, 1024)).astype(np.float32),
                     r.uniform(0, 1e-5, (Cn, 1024)).astype(np.float32))
        bias, mb, vb = r.normal(0, 0.03, Cn).astype(np.float32), r.normal(0, 1e-3, Cn).astype(np.float32), r.uniform(0, 1e-5, Cn).astype(np.float32)
        W[3], mW[3], vW[3] = row
        bias[3], mb[3], vb[3] = sc
        v = update_call(env, g, xbar, W, bias, mW, vW, mb, vb, 7, lr=1e-3)
        got.append([v[k][3].clone() for k in ("W", "m_W", "v_W", "bias", "m_b", "v_b", "dW", "db")])
    for other in got[1:]:
        for a, b in zip(got[0], other):
            assert bits_equal(a, b)


# ================================================================================================================ AdamW, elementwise
@pytest.mark.parametrize("t", (1, 2, 1000))
@pytest.mark.parametrize("wd", (0.0, 0.01))
def test_adamw_elementwise(env, capsys, t, wd):
    """B = 1 with power-of-two g: the gradient d[c,j] = g[c] x[j] is exact, so (w, m, v, d) are planted.  d = 0, |d| around eps = 1e-8,
    v = 0, m = 0 and m against d (cancellation) are all in the grid."""
    Cn = 65
    rng = np.random.default_rng([91, t])
    x = rng.normal(0, 1, 1024).astype(np.float32)
    x[:8] = [0.0, 1e-8, -1e-8, 3e-9, 2e-8, -5e-9, 1.0, -1.0]
    a = (2.0 ** rng.integers(-30, 3, Cn)).astype(np.float32) * rng.choice([-1.0, 1.0], Cn).astype(np.float32)
    a[:3] = [1.0, 0.0, -1.0]
    W = rng.normal(0, 0.03, (Cn, 1024)).astype(np.float32)
    mW = (rng.normal(0, 1, (Cn, 1024)) * 10.0 ** rng.uniform(-9, -1, (Cn, 1024))).astype(np.float32)
    vW = (10.0 ** rng.uniform(-18, -2, (Cn, 1024))).astype(np.float32)
    mW[:, 100:200], vW[:, 150:250] = 0.0, 0.0
    mW[:, 300:400] = -(a[:, None] * x[None, 300:400]) / 9                    # b1 m = -(1 - b1) d: the two terms of m' cancel
    bias, mb, vb = W[:, 0].copy(), mW[:, 1].copy(), vW[:, 2].copy()
    hyper = dict(lr=2e-5 if t != 2 else 1e-3, weight_decay=wd)
    v = update_call(env, a[None, :], x[None, :], W, bias, mW, vW, mb, vb, t, **hyper)
    d = a.astype(np.float64)[:, None] * x.astype(np.float64)[None, :]
    assert np.array_equal(v["dW"].cpu().numpy().astype(np.float64), d) and np.array_equal(v["db"].cpu().numpy(), a)
    worst = {}
    for names, args in ((("W", "m_W", "v_W"), (W, mW, vW, d)), (("bias", "m_b", "v_b"), (bias, mb, vb, a.astype(np.float64)))):
        u = T.adamw_truth(*args, t, lr=hyper["lr"], wd=wd)
        w, m, vv = (v[k].cpu().numpy().astype(np.float64) for k in names)
        axes = ("cell", "column") if names[0] == "W" else ("cell",)
        bad = T.offenders(names[0], w, u["w"], u["bound_w"], axes)
        bad += T.offenders(names[1], m, u["m"], 2 * T.ulp32(u["m_scale"]), axes)
        bad += T.offenders(names[2], vv, u["v"], 2 * T.ulp32(u["v"]), axes)
        assert not bad, bad[:5]
        worst[names[0]] = (np.abs(w - u["w"]) / u["bound_w"]).max(), (np.abs(m - u["m"]) / T.ulp32(u["m_scale"])).max(), \
            (np.abs(vv - u["v"]) / T.ulp32(u["v"])).max()
    with capsys.disabled():
        print(f"\nadamw t = {t}, wd = {wd}: worst (w / bound, m / ulp, v / ulp): {worst}")


# ================================================================================================================ trajectory
def _trajectory(golden_dir, tmp_path):
    from pigeon_amd import synthetic
    from pigeon_amd.super_guessr import SuperGuessr
    from pigeon_amd.train import HeadTrainer
    z = np.load(os.path.join(golden_dir, "head_train.npz"))
    geo = str(tmp_path / "geocells.csv")
    synthetic.write_geocell_csv(geo, z["centroids"])
    model = SuperGuessr(None, panorama=True, should_smooth_labels=True, geocell_path=geo)
    with torch.no_grad():
        model.cell_layer.weight.copy_(torch.from_numpy(z["W0"])); model.cell_layer.bias.copy_(torch.from_numpy(z["b0"]))
        model.lla_geocells.data.copy_(torch.from_numpy(z["centroids"]))
    model.to(DEV)
    trainer = HeadTrainer(model, lr=float(z["lr"]), tau=float(z["tau"]))
    emb, labels, clf = dev(z["emb"]), dev(z["labels"]), dev(z["labels_clf"])
    losses = [trainer.step(emb, labels, clf) for _ in range(len(z["losses64"]))]
    return z, torch.stack(losses).cpu().numpy(), model.cell_layer.weight.data.clone(), model.cell_layer.bias.data.clone()


def test_six_steps_stay_within_the_references_own_fp32_deviation(env, golden_dir, tmp_path, capsys):
    """The yardstick is the reference: its fp32 run deviates from its own fp64 run by dev_W, dev_b, dev_loss; this trajectory may deviate
    from the fp64 run by 4 x as much (both are maxima of rounding noise of the same order over the same 6.7e4 elements; a semantic
    mistake moves weights by order lr, 100 x dev_W)."""
    z, losses, W, b = _trajectory(golden_dir, tmp_path)
    W64 = z["W32"].astype(np.float64) + z["W64_minus_W32"].astype(np.float64)
    dev_W, dev_b = np.abs(z["W32"] - W64).max(), np.abs(z["b32"] - z["b64"]).max()
    dev_l = np.abs(z["losses32"] - z["losses64"]).max()
    got_W, got_b = np.abs(W.cpu().numpy() - W64).max(), np.abs(b.cpu().numpy() - z["b64"]).max()
    got_l = np.abs(losses - z["losses64"])
    with capsys.disabled():
        print(f"\nhead_train trajectory: max|W - W64| = {got_W:.3e} = {got_W / dev_W:.3f} x the fp32 reference's {dev_W:.3e}; "
              f"max|b - b64| = {got_b:.3e} = {got_b / dev_b:.3f} x {dev_b:.3e}; worst loss deviation {got_l.max():.3e} = "
              f"{got_l.max() / dev_l:.3f} x {dev_l:.3e}")
    assert got_W <= 4 * dev_W and got_b <= 4 * dev_b
    assert (got_l <= 4 * dev_l).all(), got_l


def test_two_runs_of_the_trajectory_give_equal_bits(env, golden_dir, tmp_path):
    _, l1, W1, b1 = _trajectory(golden_dir, tmp_path)
    _, l2, W2, b2 = _trajectory(golden_dir, tmp_path)
    assert bits_equal(W1, W2) and bits_equal(b1, b2) and np.array_equal(l1.view(np.int64), l2.view(np.int64))
