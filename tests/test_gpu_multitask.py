"""pg_aux_heads_forward (csrc/aux_heads.hip) and SuperGuessr(multi_task=True) on the GPU (run with -m gpu on an MI355X):

  1 exact inputs     every partial sum an integer multiple of 2^-3 below 2^24: the outputs ARE the float64 ones, and pg_head_forward's
                     logits on the same weights
  2 Gaussian inputs  within the textbook rounding bound of float64 per element; a row's bits do not depend on the batch
  3 cls              torch.argmax of the kernel's own outputs; ties, NaN rows, a missing / single-class classifier
  4 tol, code        tests/_auxref.py (float64, every alternative), with and without a systematic part; row_tol in/out; a step of
                     0.9 x / 1.1 x the tolerance keeps / flips the argmax the code names
  5 refused shapes   by name, before any launch
  6 the reference    tests/golden/multitask.npz (the REAL reference's SuperGuessr(multi_task=True), tools/make_multitask_golden.py)
  7 from the pixels  2-layer tower: immediate == deferred, a row only the aux tolerance flags is re-encoded, multi_task=False next to it
  8 evaluate_model   the collected multi-task outputs and metrics; heading=True == heading=False
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _auxref  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
N3 = (6, 28, 12)


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops, synthetic
    _lib.require_gpu()
    return dict(lib=_lib, ops=hip_ops, syn=synthetic)


def _split(A):
    """The four output layouts of the tests: A -> (n_reg, n_climate, n_month)."""
    return {46: (6, 28, 12), 34: (6, 28, 0), 1: (0, 1, 0), 64: (4, 40, 20)}[A]


def _run(ops, emb, W, b, n, drift=None, row_tol=None):
    return ops.aux_heads_forward(emb.to(DEV), W.to(DEV), b.to(DEV), *n, drift=None if drift is None else drift.to(DEV), row_tol=row_tol)


def _gauss(seed, B, P, A):
    g = torch.Generator().manual_seed(seed)
    emb = torch.randn((B, P, 1024), generator=g) if P > 1 else torch.randn((B, 1024), generator=g)
    W = (torch.rand((A, 1024), generator=g) * 2 - 1) / 32
    b = (torch.rand((A,), generator=g) * 2 - 1) / 32
    return emb, W, b


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("A", [46, 34, 1, 64])
@pytest.mark.parametrize("P", [1, 4])
def test_exact_inputs_give_the_float64_outputs(env, P, A):
    ops, syn = env["ops"], env["syn"]
    g = torch.Generator().manual_seed(100 * P + A)
    W = torch.randint(-8, 9, (A, 1024), generator=g).float() / 8
    b = torch.randint(-5, 6, (A,), generator=g).float()
    cent = torch.from_numpy(syn.make_geocells(A, seed=1))
    for B in (1, 3, 64, 129):
        # |x| <= 32, multiples of 4 when four panels are averaged: the panel sum, the mean and every partial sum are exact in fp32
        emb = torch.randint(-8, 9, (B, P, 1024), generator=g).float() * (4 if P == 4 else 1)
        if P == 1:
            emb = torch.randint(-32, 33, (B, 1024), generator=g).float()
        o = _run(ops, emb, W, b, _split(A))
        want = _auxref.preds(emb.numpy(), W.numpy(), b.numpy())
        assert np.abs(want).max() < 2 ** 24 / 8
        assert torch.equal(o["preds"].cpu(), torch.from_numpy(want).float()) and o["preds"].dtype == torch.float32, (B, P, A)
        assert torch.equal(o["preds"].cpu().double(), torch.from_numpy(want)), (B, P, A)
        h = ops.head_forward(emb.to(DEV), W.to(DEV), b.to(DEV), cent.to(DEV), 1)
        assert torch.equal(h["logits"], o["preds"]), (B, P, A)


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("P", [1, 4])
def test_gaussian_inputs_within_the_rounding_bound_and_batch_invariant(env, P):
    ops = env["ops"]
    emb, W, b = _gauss(7 + P, 129, P, 46)
    o = _run(ops, emb, W, b, N3)
    got = o["preds"].cpu().double().numpy()
    want = _auxref.preds(emb.numpy(), W.numpy(), b.numpy())
    bd = _auxref.bound(emb.numpy(), W.numpy(), b.numpy())
    err = np.abs(got - want)
    print(f"\nP={P}: largest |preds - fp64| / bound = {float((err / bd).max()):.4f}")
    assert (err <= bd).all()
    for i in (0, 64, 128):                                        # first, middle, last of the batch == the row alone
        alone = _run(ops, emb[i:i + 1].contiguous(), W, b, N3)
        for k in ("preds", "cls", "tol", "code"):
            assert torch.equal(alone[k][0], o[k][i]), (i, k)


# ------------------------------------------------------------------------------------------------ 3
def test_cls_is_torch_argmax_with_ties_nan_and_missing_classifiers(env):
    ops = env["ops"]
    emb, W, b = _gauss(21, 70, 4, 46)
    o = _run(ops, emb, W, b, N3)
    p = o["preds"]
    assert torch.equal(o["cls"][:, 0], torch.argmax(p[:, 6:34], dim=-1)) and torch.equal(o["cls"][:, 1], torch.argmax(p[:, 34:], dim=-1))
    assert o["cls"].dtype == torch.int64 and o["code"].dtype == torch.int32 and tuple(o["cls"].shape) == (70, 2)
    # planted ties (exact inputs): climate classes 3, 11 and 20 share the top, month classes 5 and 7 -> the lowest index; the twin rows
    # are different weight rows (columns 0 / 1 swapped, the embedding agrees on them), so the tie is a decision with margin 0
    g = torch.Generator().manual_seed(22)
    We = torch.randint(-8, 9, (46, 1024), generator=g).float() / 8
    be = torch.randint(-3, 4, (46,), generator=g).float()
    ee = torch.randint(-8, 9, (9, 4, 1024), generator=g).float() * 4
    ee[:, :, 0] = ee[:, :, 1] = 8.0
    for base, twins in ((6, (3, 11, 20)), (34, (5, 7))):
        We[base + twins[0], 0], We[base + twins[0], 1] = 0.5, -0.25
        for t in twins[1:]:
            We[base + t] = We[base + twins[0]]
            We[base + t, 0], We[base + t, 1] = -0.25, 0.5
        for t in twins:
            be[base + t] = 1e6
    ot = _run(ops, ee, We, be, N3)
    assert (ot["cls"][:, 0] == 3).all() and (ot["cls"][:, 1] == 5).all()
    assert torch.equal(ot["cls"][:, 0], torch.argmax(ot["preds"][:, 6:34], dim=-1))
    assert (ot["tol"] == 0).all() and (ot["code"] == 1 + 11).all()                # margin 0: tolerance 0, the first twin visited sets it
    # a NaN embedding row: torch's answer (the first NaN), tolerance 0; the other rows untouched
    en = emb.clone()
    en[5, 2, 100] = float("nan")
    on = _run(ops, en, W, b, N3)
    assert torch.isnan(on["preds"][5]).all()
    assert torch.equal(on["cls"][5, 0], torch.argmax(on["preds"][5, 6:34])) and torch.equal(on["cls"][5, 1], torch.argmax(on["preds"][5, 34:]))
    assert on["cls"][5].tolist() == [0, 0] and float(on["tol"][5]) == 0.0 and int(on["code"][5]) == 2
    keep = torch.arange(70) != 5
    for k in ("preds", "cls", "tol", "code"):
        assert torch.equal(on[k].cpu()[keep], o[k].cpu()[keep]), k
    # no month classifier (yfcc): -1, and no month codes
    oy = _run(ops, emb, W[:34].contiguous(), b[:34].contiguous(), (6, 28, 0))
    assert (oy["cls"][:, 1] == -1).all() and (oy["code"] >= 1).all() and (oy["code"] < 101).all()
    assert torch.equal(oy["preds"], p[:, :34].contiguous()) and torch.equal(oy["cls"][:, 0], o["cls"][:, 0])
    # one climate class and nothing else to decide
    o1 = _run(ops, emb, W[:7].contiguous(), b[:7].contiguous(), (6, 1, 0))
    assert torch.isinf(o1["tol"]).all() and (o1["tol"] > 0).all() and (o1["code"] == 0).all() and (o1["cls"][:, 0] == 0).all()
    # regression only
    o0 = _run(ops, emb, W[:6].contiguous(), b[:6].contiguous(), (6, 0, 0))
    assert (o0["cls"] == -1).all() and torch.isinf(o0["tol"]).all() and (o0["code"] == 0).all() and torch.equal(o0["preds"], p[:, :6].contiguous())


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("with_drift", [False, True])
@pytest.mark.parametrize("P", [1, 4])
def test_tolerance_and_code_against_the_restatement(env, P, with_drift):
    ops = env["ops"]
    emb, W, b = _gauss(31 + P, 90, P, 46)
    W = W * 8
    g = torch.Generator().manual_seed(5)
    beta = (2e-4 * torch.randn((1024,), generator=g) / 32).float() if with_drift else None
    o = _run(ops, emb, W, b, N3, drift=beta)
    # the decisions are taken on the kernel's own fp32 outputs (as pg_head_certainty's are on pg_head_forward's logits)
    r = _auxref.forward(emb.numpy(), W.numpy(), b.numpy(), *N3, beta=None if beta is None else beta.numpy(),
                        preds_from=o["preds"].cpu().numpy())
    tol, code = o["tol"].cpu().double().numpy(), o["code"].cpu().numpy()
    assert np.array_equal(o["cls"].cpu().numpy(), r["cls"])
    worst = float(np.max(np.abs(tol - r["tol"]) / (2e-3 * np.abs(r["tol"]) + 1e-6)))
    print(f"\nP={P} drift={with_drift}: largest |tol - fp64| / (2e-3 |t| + 1e-6) = {worst:.4f}")
    assert (np.abs(tol - r["tol"]) <= 2e-3 * np.abs(r["tol"]) + 1e-6).all()
    assert np.array_equal(code, r["code"])
    assert (code >= 101).any() and ((code >= 1) & (code < 101)).any()             # both classifiers set it somewhere
    # row_tol in/out: the minimum with a planted vector, untouched where that is smaller
    planted = o["tol"].clone()
    planted[::2] *= 0.5
    planted[1::2] *= 2.0
    before = planted.clone()
    o2 = _run(ops, emb, W, b, N3, drift=beta, row_tol=planted)
    assert torch.equal(o2["tol"], o["tol"])
    assert torch.equal(planted, torch.minimum(before, o["tol"]))
    assert int((planted == before).sum()) >= 40 and int((planted == o["tol"]).sum()) >= 40    # untouched where smaller, lowered elsewhere


def test_tolerance_means_what_it_says(env):
    """Move the embedding against the gradient of the tightest decision: 0.9 x the tolerance keeps the argmax the code names,
    1.1 x flips it (pattern of test_head_tolerance_means_what_it_says)."""
    ops = env["ops"]
    emb, W, b = _gauss(41, 24, 1, 46)
    W = W * 8
    o = _run(ops, emb, W, b, N3)
    moved = 0
    for i in range(24):
        code = int(o["code"][i])
        which, c = (0, code - 1) if code < 101 else (1, code - 101)
        off = 6 if which == 0 else 34
        c0 = int(o["cls"][i, which])
        gvec = (W[off + c0] - W[off + c]).double()
        step = float(o["tol"][i]) / 32.0 * float(emb[i].double().norm()) * gvec / gvec.norm()
        for f, same in ((0.9, True), (1.1, False)):
            e2 = emb.clone()
            e2[i] = (emb[i].double() - f * step).float()
            assert (int(_run(ops, e2, W, b, N3)["cls"][i, which]) == c0) == same, (i, f)
        moved += 1
    assert moved == 24


# ------------------------------------------------------------------------------------------------ 5
def test_refused_shapes_by_name_and_the_empty_batch(env):
    ops, lib = env["ops"], env["lib"]
    import ctypes as C
    emb, W, b = _gauss(51, 4, 4, 46)
    e, Wd, bd = emb.to(DEV), W.to(DEV), b.to(DEV)
    W65, b65 = torch.zeros((65, 1024), device=DEV), torch.zeros((65,), device=DEV)
    with pytest.raises(lib.PigeonHipError, match="at most 64"):
        ops.aux_heads_forward(e, W65, b65, 6, 40, 19)
    with pytest.raises(lib.PigeonHipError, match="negative"):
        ops.aux_heads_forward(e, Wd, bd, -1, 35, 12)
    with pytest.raises(lib.PigeonHipError, match="no outputs"):
        ops.aux_heads_forward(e, Wd[:0].contiguous(), bd[:0].contiguous(), 0, 0, 0)
    with pytest.raises(lib.PigeonHipError, match="device tensor"):
        ops.aux_heads_forward(emb, Wd, bd, *N3)
    with pytest.raises(lib.PigeonHipError, match="dtype"):
        ops.aux_heads_forward(e.double(), Wd, bd, *N3)
    with pytest.raises(lib.PigeonHipError, match="dtype"):
        ops.aux_heads_forward(e, Wd.half(), bd, *N3)
    with pytest.raises(lib.PigeonHipError, match="shape"):
        ops.aux_heads_forward(e, Wd, bd, 6, 28, 11)                               # the counts do not add up to W's rows
    with pytest.raises(lib.PigeonHipError, match="shape"):
        ops.aux_heads_forward(e, Wd, bd, *N3, row_tol=torch.zeros(3, device=DEV))
    # straight at the C ABI: P = 0, B < 0, null pointers -- refused before any launch
    fn = lib.load().pg_aux_heads_forward
    p = lambda t: C.c_void_p(t.data_ptr())                                        # noqa: E731
    out = [torch.empty((4, 46), device=DEV), torch.empty((4, 2), dtype=torch.int64, device=DEV), torch.empty(4, device=DEV),
           torch.empty(4, dtype=torch.int32, device=DEV)]
    z = C.c_void_p(0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert fn(p(e), 4, 0, p(Wd), p(bd), 6, 28, 12, z, p(out[0]), p(out[1]), p(out[2]), p(out[3]), z, s) != 0
    assert b"P=0" in lib.load().pg_last_error()
    assert fn(p(e), -1, 4, p(Wd), p(bd), 6, 28, 12, z, p(out[0]), p(out[1]), p(out[2]), p(out[3]), z, s) != 0
    assert b"B = -1" in lib.load().pg_last_error()
    assert fn(p(e), 4, 4, z, p(bd), 6, 28, 12, z, p(out[0]), p(out[1]), p(out[2]), p(out[3]), z, s) != 0
    assert b"null pointer" in lib.load().pg_last_error()
    assert fn(p(e), 4, 4, p(Wd), p(bd), 6, 47, 12, z, p(out[0]), p(out[1]), p(out[2]), p(out[3]), z, s) != 0
    assert b"at most 64" in lib.load().pg_last_error()
    # B = 0: a no-op, NULL buffers allowed
    assert fn(z, 0, 4, z, z, 6, 28, 12, z, z, z, z, z, z, s) == 0
    o = ops.aux_heads_forward(e[:0].contiguous(), Wd, bd, *N3)
    assert tuple(o["preds"].shape) == (0, 46) and tuple(o["cls"].shape) == (0, 2) and o["tol"].numel() == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 6
SETS = {"a": dict(panorama=True, yfcc=False, P=4), "b": dict(panorama=False, yfcc=True, P=1)}


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "multitask.npz"))


def _fixture_embeddings(fx, tag):
    """The rows of the seeded stream the generator kept (numpy's frozen legacy generator; tools/make_multitask_golden.py `stream`)."""
    P = SETS[tag]["P"]
    rows = np.random.RandomState(int(fx[f"{tag}_stream_seed"])).standard_normal((int(fx[f"{tag}_stream_rows"]), P, 1024)).astype(np.float32)
    emb = torch.from_numpy(rows[fx[f"{tag}_stream_index"]] if P > 1 else rows[fx[f"{tag}_stream_index"], 0]).contiguous()
    assert abs(float(emb.double().sum()) - float(fx[f"{tag}_emb_checksum"])) <= 1e-6          # (a float64 sum: its order is the library's)
    return emb


def _fixture_model(fx, tag, tmp_path, **kw):
    from pigeon_amd import synthetic
    from pigeon_amd.super_guessr import SuperGuessr
    gp = os.path.join(str(tmp_path), f"geocells_{tag}.csv")
    synthetic.write_geocell_csv(gp, fx["geocells"])
    m = SuperGuessr(None, panorama=SETS[tag]["panorama"], yfcc=SETS[tag]["yfcc"], multi_task=True, geocell_path=gp, **kw)
    m.load_state_dict({str(k): torch.from_numpy(fx[f"{tag}_w_{k}"]) for k in fx[f"{tag}_state_keys"]})
    return m.to(DEV).eval()


def _labels(fx, tag):
    lab = {k: torch.from_numpy(fx[f"{tag}_{k}"]) for k in ("labels", "labels_clf", "labels_multi_task", "labels_climate")}
    lab["labels_month"] = torch.from_numpy(fx[f"{tag}_labels_month"]) if f"{tag}_labels_month" in fx.files else None
    return lab


def _sum_slack(n_terms):
    return (n_terms + 64) * 2.0 ** -24                           # relative, for an fp32 reduction of n_terms positive terms


@pytest.mark.parametrize("exact_top1", [True, False])
@pytest.mark.parametrize("tag", ["a", "b"])
def test_the_references_numbers(env, fx, tmp_path, tag, exact_top1):
    emb = _fixture_embeddings(fx, tag)
    lab = _labels(fx, tag)
    m = _fixture_model(fx, tag, tmp_path, exact_top1=exact_top1)
    out = m(embedding=emb, **lab)
    B = emb.shape[0]
    e = emb.numpy()
    names = ("multi_task_head", "climate_layer") + (() if tag == "b" else ("month_layer",))
    Wa = np.concatenate([fx[f"{tag}_w_{n}.weight"] for n in names])
    ba = np.concatenate([fx[f"{tag}_w_{n}.bias"] for n in names])
    bd = _auxref.bound(e, Wa, ba)
    got = {"preds_mt": out.preds_mt, "preds_climate": out.preds_climate, "preds_month": out.preds_month}
    cols = {"preds_mt": slice(0, 6), "preds_climate": slice(6, 34), "preds_month": slice(34, 46)}
    for k in ("preds_mt", "preds_climate") + (() if tag == "b" else ("preds_month",)):
        ref = fx[f"{tag}_out_{k}"].astype(np.float64)
        mine = got[k].cpu().double().numpy()
        assert got[k].is_contiguous() and mine.shape == ref.shape
        ratio = float((np.abs(mine - ref) / bd[:, cols[k]]).max())
        print(f"\nset {tag} {k}: largest |ours - reference| / bound = {ratio:.4f}")
        assert (np.abs(mine - ref) <= 2 * bd[:, cols[k]]).all(), k
    if tag == "b":
        assert out.preds_month is None and out.loss_month == 0
    # the discrete outputs: EVERY row
    assert np.array_equal(out.preds_climate.argmax(-1).cpu().numpy(), fx[f"{tag}_out_preds_climate"].argmax(-1))
    st = m.last_state
    assert np.array_equal(st["aux_cls"][:, 0].cpu().numpy(), fx[f"{tag}_out_preds_climate"].argmax(-1))
    if tag == "a":
        assert np.array_equal(out.preds_month.argmax(-1).cpu().numpy(), fx["a_out_preds_month"].argmax(-1))
        assert np.array_equal(st["aux_cls"][:, 1].cpu().numpy(), fx["a_out_preds_month"].argmax(-1))
    else:
        assert (st["aux_cls"][:, 1] == -1).all()
    # the geocell outputs
    assert np.array_equal(out.preds_geocell.cpu().numpy(), fx[f"{tag}_out_preds_geocell"])
    assert np.array_equal(out.preds_LLH.cpu().numpy(), fx[f"{tag}_out_preds_LLH"])
    assert np.array_equal(out.top5_geocells.indices[:, 0].cpu().numpy(), fx[f"{tag}_out_top5_indices"][:, 0])
    assert np.allclose(out.top5_geocells.values.cpu().numpy(), fx[f"{tag}_out_top5_values"], rtol=1e-4, atol=1e-7)
    Wc, bc = fx[f"{tag}_w_cell_layer.weight"], fx[f"{tag}_w_cell_layer.bias"]
    bdc = _auxref.bound(e, Wc, bc)
    srt = np.sort(_auxref.preds(e, Wc, bc), axis=-1)[:, ::-1]
    clear = ((srt[:, :5] - srt[:, 1:6]) >= 4 * bdc.max(axis=-1, keepdims=True)).all(axis=-1)     # the order of the top 6 is beyond rounding
    assert clear.mean() >= 0.75
    assert np.array_equal(out.top5_geocells.indices.cpu().numpy()[clear], fx[f"{tag}_out_top5_indices"][clear])
    assert torch.equal(out.embedding.cpu(), emb)
    # caller-supplied embeddings: nothing is re-encoded; the tolerances are reported either way
    assert tuple(st["aux_tol"].shape) == (B,) and bool((st["aux_tol"] > 0).all()) and bool((st["aux_code"] >= 1).all())
    assert bool((st["tol"] <= st["aux_tol"]).all()) and not bool(st["exact"].any())
    # the losses, within what the outputs' bound allows (+ the fp32 reduction of positive terms)
    y = fx[f"{tag}_labels_multi_task"].astype(np.float64)
    p = fx[f"{tag}_out_preds_mt"].astype(np.float64)
    d = bd[:, :6]
    ref_reg = float(fx[f"{tag}_out_loss_reg"])
    allow = 8 * float(np.mean(2 * np.abs(p - y) * d + d * d)) + _sum_slack(6 * B) * abs(ref_reg)
    print(f"set {tag}: loss_reg ours {float(out.loss_reg):.7f} reference {ref_reg:.7f} allowed {allow:.3g}")
    assert abs(float(out.loss_reg) - ref_reg) <= allow
    ref_cl = float(fx[f"{tag}_out_loss_climate"])
    allow_cl = 2 * (2 * float(bd[:, 6:34].max())) + _sum_slack(28 * B) * abs(ref_cl)
    print(f"set {tag}: loss_climate ours {float(out.loss_climate):.7f} reference {ref_cl:.7f} allowed {allow_cl:.3g}")
    assert abs(float(out.loss_climate) - ref_cl) <= allow_cl
    allow_mo, ref_mo = 0.0, 0.0
    if tag == "a":
        ref_mo = float(fx["a_out_loss_month"])
        allow_mo = 1 * (2 * float(bd[:, 34:].max())) + _sum_slack(12 * B) * abs(ref_mo)
        print(f"set a: loss_month ours {float(out.loss_month):.7f} reference {ref_mo:.7f} allowed {allow_mo:.3g}")
        assert abs(float(out.loss_month) - ref_mo) <= allow_mo
    ref_clf = float(fx[f"{tag}_out_loss_clf"])
    allow_clf = 2 * float(bdc.max()) + _sum_slack(64 * B) * abs(ref_clf)
    assert abs(float(out.loss_clf) - ref_clf) <= allow_clf
    ref_loss = float(fx[f"{tag}_out_loss"])
    assert abs(float(out.loss) - ref_loss) <= allow + allow_cl + allow_mo + allow_clf + 8 * 2.0 ** -24 * abs(ref_loss)
    assert float(out.loss) == float(out.loss_clf + out.loss_reg + out.loss_climate + out.loss_month)
    # labels that are not given: a loss of 0, the outputs all the same
    bare = m(embedding=emb, labels_clf=lab["labels_clf"])
    assert bare.loss_reg == 0 and bare.loss_climate == 0 and bare.loss_month == 0 and torch.equal(bare.preds_mt, out.preds_mt)
    assert float(bare.loss) == float(bare.loss_clf)
    # serving: four elements, preds_mt third
    ms = _fixture_model(fx, tag, tmp_path, exact_top1=exact_top1, serving=True)
    tup = ms(embedding=emb)
    assert len(tup) == 4 == int(fx[f"{tag}_serving_len"])
    assert torch.equal(tup[2], out.preds_mt) and torch.equal(tup[3].cpu(), emb) and torch.equal(tup[0], out.preds_LLH)
    assert np.array_equal(tup[0].cpu().numpy(), fx[f"{tag}_serving_0"])
    assert (np.abs(tup[2].cpu().double().numpy() - fx[f"{tag}_serving_2"]) <= 2 * bd[:, :6]).all()
    assert np.array_equal(tup[1].indices[:, 0].cpu().numpy(), fx[f"{tag}_serving_1_indices"][:, 0])


# ------------------------------------------------------------------------------------------------ 7
def _pixel_models(env, tmp_path, C=60, **kw):
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    from pigeon_amd.super_guessr import SuperGuessr
    syn = env["syn"]
    gp = os.path.join(str(tmp_path), "g.csv")
    syn.write_geocell_csv(gp, syn.make_geocells(C, seed=0))
    vit = HipCLIPVisionModel(syn.make_vit_weights(seed=11, layers=2, affine_jitter=True), layers=2).to(DEV)
    W, b = syn.make_head_weights(C, seed=1)
    aux = syn.make_aux_head_weights(seed=3)

    def make(multi_task, exact_top1=True):
        m = SuperGuessr(vit, panorama=True, freeze_base=True, num_candidates=5, geocell_path=gp, exact_top1=exact_top1,
                        margin_autocalibrate=False, margin_rel_tol=1e-3, multi_task=multi_task, **kw)
        with torch.no_grad():
            m.cell_layer.weight.copy_(W * 64); m.cell_layer.bias.copy_(b)
            if multi_task:
                for k, v in aux.items():
                    layer, what = k.split(".")
                    getattr(getattr(m, layer), what).copy_(v * (64 if what == "weight" else 1))
        return m.to(DEV).eval()
    return make, vit


def _engine_run(m, steps, **kw):
    from pigeon_amd.deferred import DeferredExact
    eng = DeferredExact(m, None, **kw)
    got = {}
    for i, px in enumerate(steps):
        for r in eng.submit(px, meta=i):
            got[r["meta"]] = r
    for r in eng.flush():
        got[r["meta"]] = r
    assert eng.check_nothing_dropped() == 0
    return got, eng


def test_from_the_pixels_aux_rows_reach_the_exact_tier(env, tmp_path):
    from pigeon_amd.evaluate import certain_forward
    syn = env["syn"]
    make, vit = _pixel_models(env, tmp_path)
    m, m0 = make(True), make(False)
    steps = [syn.make_pixels(4 * 6, seed=70 + i, panorama=True).to(DEV) for i in range(4)]
    AUX = ("aux_preds", "aux_cls", "aux_tol", "aux_code")
    # threshold 0: nothing is flagged -- the tolerances are data.  multi_task=False next to it: every shared output bit for bit, and
    # not one aux_* key; the multi-task row tolerance is the minimum of the geocell one and the aux one
    m.certainty.kappa = m0.certainty.kappa = 0.0
    geo, aux = [], []
    for px in steps:
        _, info = certain_forward(m, None, pixel_values=px)
        _, info0 = certain_forward(m0, None, pixel_values=px)
        st, st0 = m.last_state, m0.last_state
        assert not any(k.startswith("aux_") for k in st0) and all(k in st for k in AUX)
        for k in ("embedding", "logits", "topk_values", "topk_indices", "preds_geocell", "preds_LLH", "margin", "sens"):
            assert torch.equal(st[k], st0[k]), k
        assert torch.equal(st["tol"], torch.minimum(st0["tol"], st["aux_tol"]))
        assert torch.equal(info["aux_tol"], st["aux_tol"]) and torch.equal(info["aux_code"], st["aux_code"]) and "aux_tol" not in info0
        assert not bool(st["exact"].any())
        geo.append(st0["tol"]); aux.append(st["aux_tol"])
    geo, aux = torch.cat(geo), torch.cat(aux)
    # a threshold just above the smallest aux tolerance among the rows whose geocell tolerance is clearly larger: that row is flagged
    # by the auxiliary heads ALONE (and few others are flagged at all)
    cand = (geo > 1.05 * aux) & (aux > 0)
    assert bool(cand.any()), "no row whose aux tolerance is below its geocell tolerance"
    star = int(torch.argmin(torch.where(cand, aux, torch.full_like(aux, float("inf")))))
    thr = float(aux[star]) * 1.02
    m.certainty.kappa = m0.certainty.kappa = thr / m.certainty.rel_tol
    thr = m.certainty.threshold(False)                                            # as the engine computes it
    only_aux = (aux <= thr) & (geo > thr)
    assert bool(only_aux[star])
    # settle-every-step: a fresh engine per step, so that its exact pass takes the step's flagged rows from the head of an empty queue
    now = {i: _engine_run(m, [steps[i]], immediate=True)[0][0] for i in range(4)}
    later, eng = _engine_run(m, steps, min_flush=3, max_lag=3)
    now0 = {i: _engine_run(m0, [steps[i]], immediate=True)[0][0] for i in range(4)}
    n_exact = 0
    for i in range(4):
        a, b = now[i]["state"], later[i]["state"]
        ex = b["exact"]
        assert torch.equal(a["exact"], ex)
        for k in AUX:
            assert torch.equal(a[k][~ex], b[k][~ex]), (i, k)                     # rows the fast path settles: bit for bit
            assert k not in later[i]                                              # never gathered
        assert torch.equal(a["aux_cls"], b["aux_cls"]) and torch.equal(a["aux_code"] >= 1, b["aux_code"] >= 1)
        flagged = (geo[6 * i:6 * i + 6] <= thr) | (aux[6 * i:6 * i + 6] <= thr)
        assert torch.equal(ex, flagged), i                                        # exactly the rows either tolerance flags
        assert bool((b["aux_code"][ex] >= 1).all())
        # the rows only the aux tolerance flags: the model without the heads leaves them on the fast path
        oa = only_aux[6 * i:6 * i + 6]
        assert not bool(now0[i]["state"]["exact"][oa].any()) and bool(ex[oa].all())
        if bool(ex.any()):
            # re-encoded rows carry the exact pass's own values (the same rows through exact_rows: the same pass size, the same bits)
            sx = m.exact_rows([steps[i].reshape(6, -1)[ex].contiguous()])
            for k in AUX:
                assert torch.equal(a[k][ex], sx[k]), (i, k)
            assert torch.equal(a["embedding"][ex], sx["embedding"])
        n_exact += int(ex.sum())
    assert 1 <= n_exact < 24 and int(only_aux.sum()) >= 1
    assert sum(f["slots_run"] for f in eng.flush_log) == n_exact
    # exact_top1=False: nothing is re-encoded, the tolerance is still reported
    mf = make(True, exact_top1=False)
    mf.certainty.kappa = m.certainty.kappa
    _, info = certain_forward(mf, None, pixel_values=steps[0])
    assert info["reencoded"].numel() == 0 and torch.equal(info["aux_tol"], aux[:6]) and not bool(info["certain"][only_aux[:6]].any())


# ------------------------------------------------------------------------------------------------ 8
def test_evaluate_model_collects_the_multi_task_outputs(env, fx, tmp_path):
    from pigeon_amd.evaluate import compute_geoguessr_metrics, evaluate_model
    n = 24
    emb = _fixture_embeddings(fx, "a")[:n]
    lab = {k: v[:n] for k, v in _labels(fx, "a").items()}
    m = _fixture_model(fx, "a", tmp_path)
    mh = _fixture_model(fx, "a", tmp_path, heading=True)
    cols = {k: v.numpy() for k, v in lab.items()}

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return n

        def __getitem__(self, i):
            if isinstance(i, str):
                return cols[i]
            return dict(embedding=emb[i], **{k: v[i] for k, v in lab.items()})

    res = evaluate_model(m, DS(), compute_geoguessr_metrics, None, None, batch_size=7)
    for k, shape in (("preds_mt", (n, 6)), ("preds_climate", (n, 28)), ("preds_month", (n, 12)), ("preds", (n, 2)), ("preds_geocells", (n,))):
        assert res[k].shape == shape, k
    for k in ("loss_reg", "loss_climate", "loss_month", "loss_clf", "Climate_accuracy", "Month_accuracy", "Geocell_accuracy"):
        assert k in res and np.isfinite(res[k]), k
    assert not any(k.startswith("Mean_") and k != "Mean_km_error" for k in res)    # no scaler file here: the six errors are left out
    # the per-batch chain
    chain = [m(embedding=emb[s:s + 7], **{k: v[s:s + 7] for k, v in lab.items()}) for s in range(0, n, 7)]
    for k in ("preds_mt", "preds_climate", "preds_month"):
        assert np.array_equal(res[k], torch.cat([getattr(o, k) for o in chain]).cpu().numpy()), k
    cl = torch.cat([o.preds_climate.argmax(-1) for o in chain]).cpu().numpy()
    mo = torch.cat([o.preds_month.argmax(-1) for o in chain]).cpu().numpy()
    assert res["Climate_accuracy"] == float(np.mean(cl == cols["labels_climate"].argmax(-1)))
    assert res["Month_accuracy"] == float(np.mean(mo == cols["labels_month"]))
    assert res["loss_reg"] > 0 and res["loss_climate"] > 0 and res["loss_month"] > 0
    # heading=True (panorama, not hierarchical): the reference ignores it there, and so does this model -- bit for bit
    hd = torch.randn((n, 4, 2))
    for s in range(0, n, 7):
        o = mh(embedding=emb[s:s + 7], heading=hd[s:s + 7], **{k: v[s:s + 7] for k, v in lab.items()})
        w = chain[s // 7]
        for k in ("loss", "loss_clf", "loss_reg", "loss_climate", "loss_month", "preds_LLH", "preds_geocell", "preds_mt", "preds_climate",
                  "preds_month", "embedding"):
            assert torch.equal(getattr(o, k), getattr(w, k)), k
        assert torch.equal(o.top5_geocells.values, w.top5_geocells.values) and torch.equal(o.top5_geocells.indices, w.top5_geocells.indices)
    # a dataset without the multi-task labels: the keys the function had before
    class Plain(DS):
        def __getitem__(self, i):
            if isinstance(i, str):
                return cols[i]
            return dict(embedding=emb[i], labels=lab["labels"][i], labels_clf=lab["labels_clf"][i])

    res0 = evaluate_model(m, Plain(), compute_geoguessr_metrics, None, None, batch_size=7)
    assert "preds_mt" not in res0 and "Climate_accuracy" not in res0 and np.array_equal(res0["preds_geocells"], res["preds_geocells"])
