"""THE CONTRACT ON THE EMBEDDING ROUTE (run with -m gpu on an MI355X): a sample reported `certain` has the reference's top-1 also when
the CALLER supplies the embeddings -- `run.py evaluate` on the files `run.py embed` wrote, `SuperGuessr.forward(embedding=...)`,
`certain_forward`, `evaluate_model` on a dataset of embeddings.  tests/test_gpu_top1.py pins the claim from pixels; here the
embeddings are the 16-bit encoder's (after its de-bias, as the embed path returns them), and nothing on this route can re-encode.

A 2-layer tower, n = 32 panoramas.  Measured once per module: `fast` = what `CLIPEmbedding` returns, `exact` = `embed_precise` on the
same pixels; panel means in float64, eps_i = fast_i - exact_i.  tests/_routeref.py plants a head on `exact` whose top-1 margins are
f_i times what eps_i moves them by along a seeded RANDOM direction (f cycling through 0.25 ... 65536): from `fast` the top-1 flips
exactly where f_i < 1.  Reference: the float64 argmax of exact @ W.T + bias -- nothing of the code under test enters it.

  test_fast_embeddings_are_not_judged_at_the_exact_floor     no row reported certain has another top-1 than the reference, on four routes
  test_rows_far_from_the_boundary_stay_certain               ... and the fix may not call everything uncertain
  test_declared_exact_embeddings_keep_the_floor              a caller who declares exact embeddings keeps 3.6 x 5e-6
  test_calibration_file_sets_the_tolerance_for_embeddings    1.1 x the file's image_residual_rms, and the contract holds under it
  test_embed_then_evaluate_through_files                     compute_embeddings(save=True) -> .npy -> evaluate(base_model=None)
  test_growing_batches_reach_the_calibration_once            auto-calibration while request batches grow (1, 1, 2, 4, 8 panoramas)

Measured on the 2-layer tower (pixel seed 7): |eps| / |e| of the panel means 4.8e-5 RMS (per image 9.2e-5
after the de-bias, 2.4e-4 before).
"""
import os

import numpy as np
import pytest
import torch

import _routeref as rr

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 32
PIXEL_SEED = 7          # max_i |o_i . eps_i| * 32 / |eps|_rms = 2.23 with HEAD_SEED 0 (the calibration test wants it below 3)
HEAD_SEED = 0
KAPPA = 3.6
FLOOR = KAPPA * 5e-6            # the exact tier's threshold
CAP = 10 * KAPPA * 1e-3         # ten times the uncalibrated threshold: rows above it are far from every boundary


class _Rows(torch.utils.data.Dataset):
    """A dataset of precomputed embeddings in the form `evaluate_model` reads: items are forward() keyword dicts, columns by name."""

    def __init__(self, emb, cells):
        self.emb, self.cells = emb.detach().cpu().float().contiguous(), np.asarray(cells, dtype=np.int64)

    def __len__(self):
        return self.emb.shape[0]

    def __getitem__(self, i):
        if isinstance(i, str):
            return {"labels": np.zeros((len(self), 2)), "labels_clf": self.cells}[i]
        return {"embedding": self.emb[i], "labels": torch.zeros(2, dtype=torch.float64), "labels_clf": torch.tensor(int(self.cells[i]))}


@pytest.fixture(scope="module")
def route(tmp_path_factory):
    from pigeon_amd import _lib, synthetic
    from pigeon_amd.clip_embedder import CLIPEmbedding, HipCLIPVisionModel
    _lib.require_gpu()
    tmp = str(tmp_path_factory.mktemp("route"))
    sd = synthetic.make_vit_weights(seed=11, layers=2, affine_jitter=True)
    vit = HipCLIPVisionModel(sd, layers=2).to(DEV)
    vit.enable_precise(True)
    px = synthetic.make_pixels(4 * N, seed=PIXEL_SEED, panorama=True)                  # (N, 12, 336, 336)
    images = px.reshape(4 * N, 3, 336, 336).to(DEV)
    embedder = CLIPEmbedding("unused", device=DEV, panorama=True, clip_model=vit)      # the embed path: guard + de-bias on its first batch
    fast_img = embedder(images)
    exact_img = vit.embed_precise(images)
    assert embedder.bias is not None and not embedder.force_exact, embedder.guard_stats
    fast, exact = rr.panel_means(fast_img.cpu().numpy(), N), rr.panel_means(exact_img.cpu().numpy(), N)
    eps = fast - exact
    head = rr.plant_head(exact, eps, seed=HEAD_SEED)
    bad = rr.check_preconditions(exact, fast, head)
    assert not bad, "the planted head does not have the properties the tests rely on:\n" + "\n".join(bad)
    C = head["W"].shape[0]
    assert C == 2 * N + 32
    geocells = os.path.join(tmp, "geocells.csv")
    synthetic.write_geocell_csv(geocells, synthetic.make_geocells(C, seed=0))
    ckpt = os.path.join(tmp, "head.model")
    torch.save({"cell_layer.weight": torch.from_numpy(head["W"]), "cell_layer.bias": torch.from_numpy(head["bias"])}, ckpt)
    cal = embedder.save_calibration(os.path.join(tmp, "embed_cal.npz"))
    rel = np.linalg.norm(eps, axis=1) / np.linalg.norm(exact, axis=1)
    print(f"\n[route] 2-layer tower, {N} panoramas (pixel seed {PIXEL_SEED}): |eps| / |e| of the panel means RMS {np.sqrt((rel ** 2).mean()):.3e}, "
          f"max {rel.max():.3e}; per image after the de-bias {embedder.guard_stats.get('residual_rms'):.3e}, before {embedder.guard_stats['image_rel_err']:.3e}; "
          f"A {head['A'].max():.4g} (capped on {int((head['A'] < head['A'].max()).sum())} rows), L {head['L']:g}, largest logit "
          f"{np.abs(rr.logits64(exact, head)).max():.4g}; max |o.eps| 32 / |eps|_rms = {rr.random_direction_score(head, eps):.3f}")
    return dict(tmp=tmp, vit=vit, sd=sd, px=px, images=images, embedder=embedder, fast_emb=fast_img.reshape(N, 4, 1024).contiguous(),
                exact_emb=exact_img.reshape(N, 4, 1024).contiguous(), fast=fast, exact=exact, eps=eps, head=head,
                ref=rr.reference_top1(exact, head), geocells=geocells, ckpt=ckpt, calibration=cal)


def _model(route, base=None, **kw):
    """SuperGuessr on the planted head; every tolerance at the constructor's default unless `kw` says otherwise."""
    from pigeon_amd.super_guessr import SuperGuessr
    m = SuperGuessr(base, panorama=True, freeze_base=True, geocell_path=route["geocells"], **kw)
    with torch.no_grad():
        m.cell_layer.weight.copy_(torch.from_numpy(route["head"]["W"]))
        m.cell_layer.bias.copy_(torch.from_numpy(route["head"]["bias"]))
    return m.to(DEV).eval()


def _tol_of(model, emb):
    """pg_head_certainty's value for every row, as this model computes it (k + extra candidates listed; rows do not depend on the batch)."""
    return model.encode_head(embedding=emb)["tol"].cpu().numpy()


def _four_routes(route, emb, **kw):
    """`emb` (N, 4, 1024) as `embedding=` through the four entry points -> [(name, certain, top-1, tolerance, threshold in force)]."""
    from pigeon_amd.evaluate import certain_forward, evaluate, evaluate_model
    out = []
    m = _model(route, **kw)
    o = m(embedding=emb)
    out.append(("SuperGuessr.forward", m.last_certain.cpu().numpy(), o.preds_geocell.cpu().numpy(), m.last_tol.cpu().numpy(),
                m.certainty.kappa * m.embedding_rel_tol))
    m = _model(route, **kw)
    o, info = certain_forward(m, None, embedding=emb)
    out.append(("certain_forward", info["certain"].cpu().numpy(), o.preds_geocell.cpu().numpy(), info["head_tol"].cpu().numpy(),
                m.certainty.kappa * m.embedding_rel_tol))
    m = _model(route, **kw)
    res = evaluate_model(m, _Rows(emb, route["ref"]), batch_size=12)                   # 12 + 12 + 8 rows: a ragged last batch
    out.append(("evaluate_model", res["geocell_certain"], res["preds_geocells"], _tol_of(m, emb), m.certainty.kappa * m.embedding_rel_tol))
    out.append(_evaluate_route(route, emb, **kw))
    return out


def _evaluate_route(route, emb, **kw):
    from pigeon_amd.evaluate import evaluate
    res = evaluate(route["ckpt"], _Rows(emb, route["ref"]), yfcc=False, landmarks=False, base_model=None, refine=False,
                   geocell_path=route["geocells"], **kw)
    twin = _model(route, num_candidates=50, **kw)                                      # evaluate() builds its model with 50 candidates
    assert res["uncertain_after_exact"] == int((~res["geocell_certain"]).sum())
    return ("evaluate(base_model=None)", res["geocell_certain"], res["preds_geocells"], _tol_of(twin, emb), twin.certainty.kappa * twin.embedding_rel_tol)


def _report(route, name, certain, top1, tol, thr):
    f, ref = route["head"]["f"], route["ref"]
    rows = [f"  row {i:2d}  f {f[i]:<7g} tol {tol[i]:.3e}  thr {thr:.3e}  {'certain' if certain[i] else 'uncertain'}  top-1 {int(top1[i])} "
            f"{'=' if top1[i] == ref[i] else '!='} reference {int(ref[i])}" for i in range(len(ref))]
    print(f"[{name}]\n" + "\n".join(rows))


def _certain_but_wrong(route, results):
    """Every row a route reports certain with another top-1 than the reference's, with its f_i, tolerance and threshold."""
    f, ref = route["head"]["f"], route["ref"]
    bad = []
    for name, certain, top1, tol, thr in results:
        _report(route, name, certain, top1, tol, thr)
        assert certain.shape == (N,) and top1.shape == (N,)
        bad += [f"{name}: row {i} (f {f[i]:g}) certain at tolerance {tol[i]:.3e} > threshold {thr:.3e}, top-1 {int(top1[i])}, reference {int(ref[i])}"
                for i in np.nonzero(certain & (top1 != ref))[0]]
    return bad


def test_fast_embeddings_are_not_judged_at_the_exact_floor(route):
    """The embed path's embeddings through every entry point that takes `embedding=`, all tolerances at the constructor defaults: no
    row reported certain may have another top-1 than the float64 reference on the exact embeddings.

    Before the default changed (caller-supplied embeddings judged at the exact tier's floor, 3.6 x 5e-6 = 1.8e-5): on all four
    routes the rows 0 and 24 (f = 0.25; tolerance 2.03e-5, 3.32e-5) and 1 and 9 (f = 0.5; 3.32e-5, 3.07e-5) were reported certain
    with the wrong cell -- the top-1 from `fast`; the other four flipped rows (8, 16, 17, 25: 1.4e-6 to 1.5e-5) were below the floor."""
    bad = _certain_but_wrong(route, _four_routes(route, route["fast_emb"]))
    assert not bad, "\n".join(bad)


def test_rows_far_from_the_boundary_stay_certain(route):
    """The other side: a row whose tolerance (pg_head_certainty) exceeds 10 x 3.6 x 1e-3 is certain on every route -- judging the
    16-bit path's embeddings at its own tolerance does not mean calling everything uncertain.  The four rows with f = 65536 meet the
    condition (0.125 to 1.65; asserted, so it is not vacuous); of the four with f = 1024 two do (rows 6 and 30: 0.037, 0.108) and two
    do not (rows 14 and 22: 0.0026, 0.022 -- at |eps| / |e| = 4.8e-5 a row needs |o . eps| above 0.73 of the typical |eps| / 32)."""
    f = route["head"]["f"]
    bad = []
    for name, certain, top1, tol, thr in _four_routes(route, route["fast_emb"]):
        far = tol > CAP
        print(f"[{name}] rows above {CAP:g}: {[(int(i), float(f[i])) for i in np.nonzero(far)[0]]}; certain rows: {np.nonzero(certain)[0].tolist()}")
        assert far[f >= 65536].all(), (name, tol[f >= 65536].tolist())
        bad += [f"{name}: row {i} (f {f[i]:g}) has tolerance {tol[i]:.3e} > {CAP:g} but is not certain (threshold {thr:.3e})"
                for i in np.nonzero(far & ~certain)[0]]
    assert not bad, "\n".join(bad)


def test_declared_exact_embeddings_keep_the_floor(route):
    """A caller who hands in the exact encoder's embeddings says so (`embedding_rel_tol=margin_rel_tol_exact`) and is judged at the
    exact tier's floor: every row above 3.6 x 5e-6 is certain, and every certain row has the reference's top-1."""
    f = route["head"]["f"]
    results = _four_routes(route, route["exact_emb"], embedding_rel_tol=5e-6)
    bad = _certain_but_wrong(route, results)
    for name, certain, top1, tol, thr in results:
        assert thr == pytest.approx(FLOOR), (name, thr)
        bad += [f"{name}: row {i} (f {f[i]:g}) has tolerance {tol[i]:.3e} > the floor {FLOOR:.3e} but is not certain"
                for i in np.nonzero((tol > FLOOR) & ~certain)[0]]
        assert (tol > FLOOR).sum() >= N // 2, (name, tol.tolist())                     # the floor is not passed by nobody
    assert not bad, "\n".join(bad)


def test_calibration_file_sets_the_tolerance_for_embeddings(route):
    """With the calibration file the embed path wrote, `embedding_rel_tol` is 1.1 x the file's image_residual_rms (the per-image
    error of the embeddings after the de-bias), and the contract holds under it.  That tolerance is a statement about a RANDOM
    direction; the precondition says the planted ones are typical draws (a row flips at f < 1 and is certain only if its direction
    caught (1 - f) |o . eps| 32 / |e| > 3.6 x 1.1 x 9.3e-5, i.e. about 7 of the panel means' |eps|_rms)."""
    from pigeon_amd.certainty import Certainty
    score = rr.random_direction_score(route["head"], route["eps"])
    assert score < 3.0, score                                                          # input precondition: measured 2.23 (pixel seed 7, head seed 0)
    sd, header = Certainty.load(route["calibration"])
    resid = float(sd["stats"]["image_residual_rms"])
    m = _model(route)
    assert m.embedding_rel_tol == pytest.approx(1e-3)
    m.load_calibration(route["calibration"])
    assert m.embedding_rel_tol == 1.1 * resid and 5e-5 < resid < 2e-4 and header["panels"] == 1
    results = _four_routes(route, route["fast_emb"], calibration=route["calibration"])
    for name, certain, top1, tol, thr in results:
        assert thr == pytest.approx(KAPPA * 1.1 * resid), (name, thr)
    bad = _certain_but_wrong(route, results)
    assert not bad, "\n".join(bad)


def test_embed_then_evaluate_through_files(route, tmp_path):
    """The chain the finding names: `compute_embeddings(..., save=True)` writes the embed path's embeddings, `evaluate` reads the
    .npy back with base_model=None.  No row it reports certain has another top-1 than the reference.

    Before the default changed: rows 0, 1, 9 and 24, as in test_fast_embeddings_are_not_judged_at_the_exact_floor."""
    from pigeon_amd.clip_embedder import CLIPEmbedding
    from pigeon_amd.distributed import Communicator
    from pigeon_amd.embed import compute_embeddings
    embedder = CLIPEmbedding("unused", device=DEV, panorama=True, clip_model=route["vit"])
    out_dir = str(tmp_path / "landmark_embeddings")
    compute_embeddings("val", embedder, [(route["images"], torch.arange(4 * N))], Communicator(), out_dir=out_dir, save=True)
    saved, idx = np.load(os.path.join(out_dir, "val.npy")), np.load(os.path.join(out_dir, "val_indices.npy"))
    assert saved.shape == (1, 4 * N, 1024) and saved.dtype == np.float32 and idx.reshape(-1).tolist() == list(range(4 * N))
    emb = torch.from_numpy(saved.reshape(N, 4, 1024))
    assert torch.equal(emb, route["fast_emb"].cpu())                                  # the files hold what the fixture measured
    bad = _certain_but_wrong(route, [_evaluate_route(route, emb)])
    assert not bad, "\n".join(bad)


def test_growing_batches_reach_the_calibration_once(route):
    """A server whose request batches grow while the auto-calibration is still collecting: 1, 1, 2, 4 panoramas through
    `certain_forward`, each batch larger than the engine's ring.  What is waiting for `_calibrate` holds every submitted panorama
    ONCE, row by row, after every step; the 8-panorama batch that completes the 16 hands exactly those 16 over.  (Encoding a batch
    again after the ring was re-allocated appended its pixels twice: the even/odd held-out split of `Certainty.calibrate` then
    validated the bias on copies of the samples it was fitted on.)"""
    from pigeon_amd.evaluate import certain_forward
    m = _model(route, base=route["vit"], margin_autocalibrate=True, exact_top1=True)
    handed = []
    inner = m._calibrate

    def recording(px, *a, **kw):
        handed.append(px.detach().clone())
        return inner(px, *a, **kw)
    m._calibrate = recording
    px = route["px"].to(DEV)
    submitted, at = [], 0
    for b in (1, 1, 2, 4):
        batch = px[at:at + b]
        at += b
        certain_forward(m, None, pixel_values=batch)
        submitted.append(batch.reshape(4 * b, 3, 336, 336))
        want = torch.cat(submitted)
        got = torch.cat([t.to(want.dtype) for t in m._cal_buffer]) if m._cal_buffer else want[:0]
        assert got.shape[0] == want.shape[0] == 4 * at, f"after batches up to {b}: {got.shape[0] // 4} panoramas wait for the calibration, {at} were submitted"
        assert torch.equal(got, want)
        assert not handed and not m.certainty.calibrated
    certain_forward(m, None, pixel_values=px[at:at + 8])
    submitted.append(px[at:at + 8].reshape(32, 3, 336, 336))
    want = torch.cat(submitted)
    assert len(handed) == 1 and handed[0].shape[0] == 4 * 16 and torch.equal(handed[0].to(want.dtype), want)
    assert torch.unique(handed[0].reshape(64, -1)[:, :64], dim=0).shape[0] == 64       # no image twice
    assert m.certainty.calibrated and m._cal_buffer == [] and m.certainty.stats["samples"] == 16
