"""pg_token_attribution (csrc/attribution.hip), hip_ops.token_attribution and SuperGuessr.attribute on the GPU (run with -m gpu on an
MI355X).  Every comparison is with tests/_attrref.py (float64) or with the model's own outputs; synthetic hidden states or a 2-layer tower.

  op level, synthetic hidden
  1 exact inputs   small integers: every dot product is exact in any order, out == fp32(d) / fp32(577 P) bit for bit
  2 one-hot rows   every output is one known entry of g: rows mixed at image boundaries, columns permuted, the class and the last token
  3 Gaussian       within (1024 u sum |h g|) / (577 P) + u |truth| of float64, per element
  4 invariance     a panorama's bits at B = 1 and as row 2 of B = 3; a direction's at K = 1 and at position 5 of K = 8
  5 bad indices    exactly the stated columns are NaN, everything else as without them, 4 KB guards around `out` intact
  6 refusals       by name; n_images = 0 is a no-op
  model level, 2-layer tower with a small planted head
  7 identity       maps summed in float64 + offset == Attribution.logits within the fp32 summation bound; logits == encode_head's
  8 token -> patch the hidden row that moves most when one 14 x 14 patch changes is token 1 + 24 y + x of that view
  9 read-only      attribute leaves last_state, the calibration buffer and certainty.calibrated alone; forward after == forward before
 10 P = 1, bytes   panorama=False; pixel_bytes gives the maps of the corresponding pixel_values
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _attrref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
T, H = R.TOKENS, R.HIDDEN


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops, synthetic
    _lib.require_gpu()
    return dict(lib=_lib, ops=hip_ops, syn=synthetic)


def _run(ops, hidden, W, cells, against=None, P=1, **kw):
    a = None if against is None else torch.as_tensor(against, dtype=torch.int64).to(DEV)
    out = ops.token_attribution(hidden.to(DEV), W.to(DEV), torch.as_tensor(cells, dtype=torch.int64).to(DEV), a, panels=P, **kw)
    assert out.dtype == torch.float32 and tuple(out.shape) == (hidden.shape[0] // P, P, T, np.asarray(cells).shape[1])
    return out.cpu()


def _ints(seed, n, C):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-7, 8, (n, T, H), generator=g).float(), torch.randint(-3, 4, (C, H), generator=g).float()


def _gauss(seed, n, C):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((n, T, H), generator=g), (torch.rand((C, H), generator=g) * 2 - 1) / 32


# ------------------------------------------------------------------------------------------------ 1
EXACT_CASES = {
    "B1_P1_K1_no_against": (1, 1, 5, [[3]], None),
    "B2_P4_K3_against_per_row": (2, 4, 7, [[0, 6, 2], [5, 1, 3]], [4, -1]),
    "B3_P1_K16_C1": (3, 1, 1, [[0] * 16] * 3, [-1, 0, -1]),
    "B3_P1_K16_C7": (3, 1, 7, [[(3 * b + k) % 7 for k in range(16)] for b in range(3)], [6, -1, 2]),
    "duplicate_cells": (2, 1, 7, [[4, 4, 1, 4], [2, 5, 5, 2]], [0, 3]),
    "cell_equals_against": (2, 4, 7, [[1, 3], [6, 0]], [3, 6]),
}


@pytest.mark.parametrize("case", sorted(EXACT_CASES))
def test_exact_inputs_give_the_exact_quotient(env, case):
    B, P, C, cells, against = EXACT_CASES[case]
    hidden, W = _ints(len(case) + 17 * B + P, B * P, C)
    got = _run(env["ops"], hidden, W, cells, against, P)
    want = R.maps_exact_f32(hidden.numpy(), W.numpy(), cells, against, P)
    R.compare_maps(got.numpy(), want)                                 # names (row, view, token, k)
    assert torch.equal(got, torch.from_numpy(want))
    if case == "cell_equals_against":                                 # g = W[c] - W[c]: exact zeros, not merely small
        assert not got[0, :, :, 1].any() and not got[1, :, :, 0].any() and got[0, :, :, 0].any()
    if case == "duplicate_cells":
        assert torch.equal(got[0, :, :, 0], got[0, :, :, 1]) and torch.equal(got[0, :, :, 0], got[0, :, :, 3])


# ------------------------------------------------------------------------------------------------ 2
def test_one_hot_rows_pick_one_entry_of_g(env):
    B, P, C, K = 2, 4, 6, 3
    rows = B * P * T
    r = torch.arange(rows)
    col, val = (7 * r) % H, ((r % 5) + 1).float()
    hidden = torch.zeros((rows, H))
    hidden[r, col] = val
    _, W = _gauss(3, 1, C)
    cells, against = [[2, 0, 5], [1, 4, 3]], [3, -1]
    got = _run(env["ops"], hidden.reshape(B * P, T, H), W, cells, against, P)
    g = R.directions(W.numpy(), cells, against).astype(np.float64)                        # (B,K,1024)
    b_of = (r // (P * T)).numpy()
    prod = (val.numpy().astype(np.float64)[:, None] * g[b_of, :, col.numpy()]).astype(np.float32)   # fma(h, g, 0): one rounding
    want = (prod / np.float32(T * P)).astype(np.float32).reshape(B, P, T, K)
    R.compare_maps(got.numpy(), want)
    assert torch.equal(got, torch.from_numpy(want))


# ------------------------------------------------------------------------------------------------ 3
@pytest.mark.parametrize("B,P,K", [(2, 4, 4), (3, 1, 16)])
def test_gaussian_inputs_within_the_rounding_bound(env, B, P, K):
    C = 23
    hidden, W = _gauss(10 * B + P, B * P, C)
    g = torch.Generator().manual_seed(B)
    cells = torch.randint(0, C, (B, K), generator=g).tolist()
    against = [int(v) for v in torch.randint(0, C, (B,), generator=g)]
    against[0] = -1
    got = _run(env["ops"], hidden, W, cells, against, P).double().numpy()
    want = R.maps(hidden.numpy(), W.numpy(), cells, against, P)
    bd = R.bound(hidden.numpy(), W.numpy(), cells, against, P)
    ratio = np.abs(got - want) / np.where(bd > 0, bd, 1.0)
    print(f"\n(B,P,K)=({B},{P},{K}): largest |out - fp64| / bound = {float(ratio.max()):.4f}")
    R.compare_maps(got, want, bd)


# ------------------------------------------------------------------------------------------------ 4
def test_bits_do_not_depend_on_batch_k_or_position(env):
    ops = env["ops"]
    C, P = 11, 4
    hidden, W = _gauss(77, 3 * P, C)
    cells8 = [[1, 9, 4, 0, 7, 3, 10, 2], [5, 5, 8, 1, 0, 6, 2, 9], [3, 0, 10, 7, 6, 8, 1, 4]]
    against = [6, -1, 2]
    full = _run(ops, hidden, W, cells8, against, P)
    alone = _run(ops, hidden[2 * P:].contiguous(), W, cells8[2:], against[2:], P)         # the same panorama at B = 1
    assert torch.equal(alone[0], full[2])
    one = _run(ops, hidden, W, [[row[5]] for row in cells8], against, P)                  # position 5 of K = 8 at K = 1
    assert torch.equal(one[..., 0], full[..., 5])
    moved = _run(ops, hidden, W, [row[5:] + row[:5] for row in cells8], against, P)      # ... and at position 0 of K = 8
    assert torch.equal(moved[..., 0], full[..., 5]) and torch.equal(moved[..., 3:], full[..., :5])


# ------------------------------------------------------------------------------------------------ 5
def test_bad_indices_give_nan_columns_and_touch_nothing_else(env):
    ops = env["ops"]
    B, P, K, C = 3, 2, 4, 9
    hidden, W = _gauss(5, B * P, C)
    cells = [[1, 2, 3, 4], [8, 0, 5, 2], [7, 7, 6, 1]]
    against = [0, -1, 3]
    clean = _run(ops, hidden, W, cells, against, P)
    assert not torch.isnan(clean).any()
    bad_cells = [[1, -2, 3, 4], [C, 0, 5, 2], [7, 7, 6, 2 ** 40]]
    n_out, guard = B * P * T * K, 1024                                # 4 KB of floats in front of and behind `out`
    for bad_against in (against, [0, C, 3], [-2, -1, 3], [0, -1, -2 ** 40]):
        buf = torch.full((guard + n_out + guard,), 12345.0, dtype=torch.float32, device=DEV)
        out = buf[guard:guard + n_out].view(B, P, T, K)
        got = _run(ops, hidden, W, bad_cells, bad_against, P, out=out)
        want_nan = ~torch.from_numpy(R.valid(bad_cells, bad_against, C))                  # (B,K)
        isnan = torch.isnan(got)
        assert torch.equal(isnan, want_nan[:, None, None, :].expand_as(isnan)), bad_against
        assert torch.equal(torch.isnan(out.cpu()), isnan)
        same_against = torch.tensor([a == b for a, b in zip(against, bad_against)])
        keep = (~want_nan & same_against[:, None])[:, None, None, :].expand_as(isnan)     # columns whose direction is the clean run's
        assert keep.any() and torch.equal(got[keep], clean[keep]), bad_against
        R.compare_maps(got.numpy(), R.maps(hidden.numpy(), W.numpy(), bad_cells, bad_against, P),
                       R.bound(hidden.numpy(), W.numpy(), bad_cells, bad_against, P))
        torch.cuda.synchronize()
        assert (buf[:guard] == 12345.0).all() and (buf[guard + n_out:] == 12345.0).all(), "guard pattern overwritten"


# ------------------------------------------------------------------------------------------------ 6
def test_refusals_name_the_argument_and_empty_batch_is_a_noop(env):
    ops, lib = env["ops"], env["lib"]
    Err = lib.PigeonHipError
    hidden = torch.zeros((4, T, H), device=DEV)
    W = torch.zeros((3, H), device=DEV)
    cells = torch.zeros((4, 2), dtype=torch.int64, device=DEV)
    with pytest.raises(Err, match="cells.*K"):
        ops.token_attribution(hidden, W, cells[:, :0].contiguous())                      # K = 0
    with pytest.raises(Err, match="cells.*K"):
        ops.token_attribution(hidden, W, torch.zeros((4, 17), dtype=torch.int64, device=DEV))
    with pytest.raises(Err, match="panels"):
        ops.token_attribution(hidden, W, cells[:1], panels=3)                            # 4 images, 3 views
    with pytest.raises(Err, match="panels"):
        ops.token_attribution(hidden, W, cells, panels=0)
    with pytest.raises(Err, match="hidden.*device"):
        ops.token_attribution(hidden.cpu(), W, cells)
    with pytest.raises(Err, match="W.*device"):
        ops.token_attribution(hidden, W.cpu(), cells)
    with pytest.raises(Err, match="cells.*device"):
        ops.token_attribution(hidden, W, cells.cpu())
    with pytest.raises(Err, match="against.*device"):
        ops.token_attribution(hidden, W, cells, torch.zeros(4, dtype=torch.int64))
    with pytest.raises(Err, match="hidden.*float32"):
        ops.token_attribution(hidden.half(), W, cells)
    with pytest.raises(Err, match="W.*float32"):
        ops.token_attribution(hidden, W.double(), cells)
    with pytest.raises(Err, match="cells.*int64"):
        ops.token_attribution(hidden, W, cells.int())
    with pytest.raises(Err, match="against.*int64"):
        ops.token_attribution(hidden, W, cells, torch.zeros(4, dtype=torch.int32, device=DEV))
    with pytest.raises(Err, match="hidden"):
        ops.token_attribution(hidden[:, :576].contiguous(), W, cells)
    with pytest.raises(Err, match="cells"):
        ops.token_attribution(hidden, W, cells[:3])                                      # B = 4 rows expected
    with pytest.raises(Err, match="against"):
        ops.token_attribution(hidden, W, cells, torch.zeros(3, dtype=torch.int64, device=DEV))
    # the C entry point itself: PG_EINVAL and a message naming the argument, before anything is launched
    l = lib.load()
    out = torch.full((4 * T * 2,), 7.0, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda n, P, C, K, h=hidden, w=W, c=cells, o=out: l.pg_token_attribution(p(h) if h is not None else None, n, P,
                                                                                   p(w) if w is not None else None, C,
                                                                                   p(c) if c is not None else None, None, K,
                                                                                   p(o) if o is not None else None, None)
    for args, word in (((4, 1, 3, 0), "K = 0"), ((4, 1, 3, 17), "K = 17"), ((4, 3, 3, 2), "multiple of P"), ((4, 0, 3, 2), "P = 0"),
                       ((-1, 1, 3, 2), "n_images"), ((4, 1, 0, 2), "C = 0")):
        assert call(*args) == -1 and word in l.pg_last_error().decode(), (args, l.pg_last_error())
    for kw in (dict(h=None), dict(w=None), dict(c=None), dict(o=None)):
        assert call(4, 1, 3, 2, **kw) == -1 and "null" in l.pg_last_error().decode()
    assert call(0, 4, 3, 2, h=None, w=None, c=None, o=None) == 0                         # n_images = 0: a no-op, buffers may be NULL
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    empty = ops.token_attribution(hidden[:0], W, cells[:0], panels=4)
    assert tuple(empty.shape) == (0, 4, T, 2)


# ------------------------------------------------------------------------------------------------ model level
CELLS = 37


@pytest.fixture(scope="module")
def tower(env):
    """A 2-layer tower and three SuperGuessr heads over it (one packed encoder): panorama without auto-calibration, panorama with
    the defaults, single image."""
    import contextlib
    import io
    import tempfile
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    from pigeon_amd.super_guessr import SuperGuessr
    syn = env["syn"]
    sd = syn.make_vit_weights(seed=11, layers=2, affine_jitter=True)
    W, b = syn.make_head_weights(CELLS, seed=3)
    geo = os.path.join(tempfile.mkdtemp(prefix="pigeon_attr_"), "geocells.csv")
    syn.write_geocell_csv(geo, syn.make_geocells(CELLS, seed=0))
    base = HipCLIPVisionModel(sd, layers=2).to(DEV)
    base.enable_precise(True)

    def head(**kw):
        with contextlib.redirect_stdout(io.StringIO()):
            m = SuperGuessr(base, freeze_base=True, num_candidates=5, geocell_path=geo, **kw)
        with torch.no_grad():
            m.cell_layer.weight.copy_(W * 8); m.cell_layer.bias.copy_(b)
        return m.to(DEV).eval()

    px = syn.make_pixels(8, seed=77, panorama=True).to(DEV)                               # (2,12,336,336)
    return dict(base=base, pano=head(panorama=True, margin_autocalibrate=False), auto=head(panorama=True), single=head(panorama=False),
                px=px)


def _identity(model, att, hid, beta, norms):
    """maps summed in float64 + offset against Attribution.logits, and the bound 2 (1024 + 577 + P + 8) u S."""
    B, P, _, K = att.maps.shape
    W, hb = model.cell_layer.weight.data, model.cell_layer.bias.data
    c, a = att.cells, att.against
    none = (a == -1)
    g = W[c] - torch.where(none[:, None], torch.zeros((), device=W.device), W[a.clamp(min=0)])[:, None, :]          # (B,K,1024) fp32
    S = torch.einsum("brj,bkj->bk", hid.reshape(B, P * T, H).double().abs(), g.double().abs()) / (T * P)
    S = S + hb[c].double().abs() + torch.where(none, torch.zeros((), dtype=torch.float64, device=W.device), hb[a.clamp(min=0)].double().abs())[:, None]
    if beta is not None:
        S = S + norms.reshape(B, P).double().mean(dim=1)[:, None] * (g.double() * beta.double()).sum(-1).abs()
    total = att.maps.double().sum(dim=(1, 2)) + att.offset.double()
    tol = 2 * (H + T + P + 8) * R.U * S
    return total.cpu().numpy(), att.logits.double().cpu().numpy(), tol.cpu().numpy()


@pytest.mark.parametrize("tier", ["fast", "exact"])
@pytest.mark.parametrize("with_bias", [False, True])
def test_maps_and_offset_add_up_to_the_models_logits(tower, tier, with_bias):
    model, px = tower["pano"], tower["px"]
    enc = tower["base"]._encoder(torch.device(DEV, torch.cuda.current_device()))
    flat = px.reshape(8, 3, 336, 336)
    beta = None
    if with_bias:
        beta = (torch.randn(H, generator=torch.Generator().manual_seed(4)) * 2e-3).to(DEV)
    model.certainty.bias = beta
    try:
        att = model.attribute(pixel_values=px, k=2, tier=tier)
        assert tuple(att.maps.shape) == (2, 4, T, 2) and tuple(att.offset.shape) == (2, 2) and tuple(att.against.shape) == (2,)
        assert att.cells.dtype == torch.int64 and att.against.dtype == torch.int64 and att.logits.dtype == torch.float32
        if tier == "fast":
            st = model.encode_head(pixel_values=px)
            emb, hid = enc.forward(flat, return_hidden=True)
        else:
            st = model.exact_rows([px.reshape(2, -1)])
            emb, hid = enc.forward_precise(flat, return_hidden=True)
            model.certainty.force_exact = True                        # ... and encode_head itself, sent to the exact tier
            try:
                assert torch.equal(model.encode_head(pixel_values=px)["logits"], st["logits"])
            finally:
                model.certainty.force_exact = False
        lg = st["logits"]
        top2 = torch.topk(lg, 2, dim=-1).indices
        assert torch.equal(att.cells, top2) and torch.equal(att.against, top2[:, 1])     # cells=None: the top-k; against: the runner-up
        assert torch.equal(att.logits, lg.gather(1, att.cells) - lg.gather(1, att.against[:, None]))
        assert not att.maps[..., 1].any() and not att.logits[:, 1].any()                 # the runner-up against itself: exact zeros
        uses_beta = beta if tier == "fast" else None                  # the exact tier has no systematic part to take out
        total, logits, tol = _identity(model, att, hid, uses_beta, emb.norm(dim=1))
        print(f"\ntier={tier} bias={with_bias}: sum + offset = {total[:, 0]}, logits = {logits[:, 0]}, "
              f"largest |difference| / bound = {float((np.abs(total - logits) / np.where(tol > 0, tol, 1.0)).max()):.4f}")
        R.compare_offset(total, logits, tol)
        # the offset is the restatement's: the bias difference and, on the de-biased fast pass, -(1/P) sum_p |e_p| (g . beta)
        Wc, bc = model.cell_layer.weight.data.cpu().numpy(), model.cell_layer.bias.data.cpu().numpy()
        cn, an = att.cells.cpu().numpy(), att.against.cpu().numpy()
        norms = emb.double().norm(dim=1).reshape(2, 4).cpu().numpy()
        want_off = R.offset(Wc, bc, cn, an, norms if uses_beta is not None else None, None if uses_beta is None else uses_beta.cpu().numpy())
        bare_off = R.offset(Wc, bc, cn, an)
        R.compare_offset(att.offset.cpu().numpy(), want_off, 8 * R.U * (np.abs(bare_off) + np.abs(want_off - bare_off)) + 1e-30)
        if uses_beta is not None:
            assert (np.abs(want_off - bare_off)[:, 0] > 1e3 * R.U * np.abs(bare_off)[:, 0]).all()      # (the term is not lost in the rounding)
        # the runner-up asked about is compared with the top-1; None and a tensor are taken as given
        swap = model.attribute(pixel_values=px, cells=top2[:, 1:2], tier=tier)
        assert torch.equal(swap.against, top2[:, 0]) and torch.equal(swap.logits[:, 0], -att.logits[:, 0])
        alone = model.attribute(pixel_values=px, cells=top2[:, :1], against=None, tier=tier)
        assert (alone.against == -1).all() and torch.equal(alone.logits[:, 0], lg.gather(1, top2[:, :1])[:, 0])
        given = model.attribute(pixel_values=px, cells=top2, against=torch.tensor([CELLS, -1]), tier=tier)
        assert torch.isnan(given.maps[0]).all() and torch.isnan(given.logits[0]).all() and torch.isnan(given.offset[0]).all()
        assert torch.equal(given.maps[1], alone_maps(model, px, top2, tier)[1])
    finally:
        model.certainty.bias = None


def alone_maps(model, px, cells, tier):
    return model.attribute(pixel_values=px, cells=cells, against=None, tier=tier).maps


def test_changing_one_patch_moves_its_own_token_most(tower):
    base, px = tower["base"], tower["px"]
    flat = px.reshape(8, 3, 336, 336)[:4]
    g = torch.Generator().manual_seed(9)
    batch = [flat]
    places = [(1, 3, 5), (3, 23, 23)]                                 # (view, y, x): one of them the last row and column
    for v, y, x in places:
        q = flat.clone()
        q[v, :, 14 * y:14 * y + 14, 14 * x:14 * x + 14] = torch.randn((3, 14, 14), generator=g).to(DEV) * 2
        batch.append(q)
    hid = base.hidden(pixel_values=torch.cat(batch)).reshape(3, 4 * T, H)
    for i, (v, y, x) in enumerate(places):
        moved = (hid[1 + i] - hid[0]).double().norm(dim=1)
        assert int(moved.argmax()) == v * T + 1 + 24 * y + x, (v, y, x, int(moved.argmax()))


def _outputs(o):
    return [o.preds_LLH, o.preds_geocell, o.top5_geocells.values, o.top5_geocells.indices, o.embedding]


def test_attribute_leaves_the_object_alone(tower):
    model, px = tower["auto"], tower["px"]
    assert model.margin_autocalibrate and model.exact_top1 and not model.certainty.calibrated
    before = _outputs(model(pixel_values=px))
    state, held = model.last_state, [t.clone() for t in model._cal_buffer]
    last = (model.last_tol, model.last_margin, model.last_certain)
    engines = dict(model._engines)
    assert len(held) == 1                                             # two panoramas are waiting for the auto-calibration
    att = model.attribute(pixel_values=px, k=3)
    assert tuple(att.maps.shape) == (2, 4, T, 3)
    assert model.last_state is state and all(a is b for a, b in zip(last, (model.last_tol, model.last_margin, model.last_certain)))
    assert len(model._cal_buffer) == 1 and torch.equal(model._cal_buffer[0], held[0]) and not model.certainty.calibrated
    assert model.certainty.bias is None and dict(model._engines) == engines
    after = _outputs(model(pixel_values=px))
    assert all(torch.equal(a, b) for a, b in zip(before, after))


def test_single_image_model_and_pixel_bytes(tower, env):
    single, pano = tower["single"], tower["pano"]
    g = torch.Generator().manual_seed(21)
    by = torch.randint(0, 256, (2, 12, 336, 336), generator=g, dtype=torch.uint8).to(DEV)
    values = env["ops"].bytes_to_pixels(by.view(8, 3, 336, 336))     # the table's fp32 value of every byte
    for tier in ("fast", "exact"):
        a = pano.attribute(pixel_bytes=by, k=2, tier=tier)
        b = pano.attribute(pixel_values=values.reshape(2, 12, 336, 336), k=2, tier=tier)
        assert all(torch.equal(x, y) for x, y in zip(a, b)), tier
    one_b = single.attribute(pixel_bytes=by.view(8, 3, 336, 336)[:3].contiguous(), k=2)
    one_v = single.attribute(pixel_values=values[:3], k=2)
    assert tuple(one_v.maps.shape) == (3, 1, T, 2) and all(torch.equal(x, y) for x, y in zip(one_b, one_v))
    st = single.encode_head(pixel_values=values[:3])
    assert torch.equal(one_v.logits, st["logits"].gather(1, one_v.cells) - st["logits"].gather(1, one_v.against[:, None]))
    emb, hid = tower["base"]._encoder(torch.device(DEV, torch.cuda.current_device())).forward(values[:3], return_hidden=True)
    total, logits, tol = _identity(single, one_v, hid, None, None)
    R.compare_offset(total, logits, tol)
    with pytest.raises(ValueError):
        single.attribute(pixel_values=values[:3], tier="double")
    with pytest.raises(ValueError):
        single.attribute(pixel_values=values[:3], k=17)
    with pytest.raises(ValueError):
        single.attribute()
