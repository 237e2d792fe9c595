"""8-bit pixels end to end on the GPU (run with -m gpu on an MI355X): the resize kernels' byte output, the im2col kernels that look the
bytes up, both encoder tiers, the model route with its queue of byte rows, evaluation from raw images, and the refusals of the C ABI.

One contract runs through all of it: for a byte image b and p = table[b] as fp32 pixels, whatever is computed from b is what is
computed from p, BIT FOR BIT -- the lookup yields the fp32 value the fp32 path reads, and everything behind it is the same code.  So
every comparison here is `torch.equal` / `array_equal`; no tolerance appears except the project's own exact-tier floor (5e-6) in the
negative control, which is a lower bound on a difference."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 336
IMG = 3 * S * S                                   # 338 688 bytes: one image of 8-bit pixels
GEOMS = [(1, 1), (14, 20), (336, 336), (337, 500), (640, 400), (3000, 8)]      # (height, width); the last is a 375:1 strip
SENTINEL, GUARD = 0xA5, 4096
F32, F16, U8 = 0, 2, 4


@pytest.fixture(scope="module")
def env():
    from oracle import clip_preprocess_oracle as orc
    from pigeon_amd import _lib, hip_ops, synthetic
    _lib.require_gpu()
    rng = np.random.default_rng(99)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in GEOMS]
    plain = orc.precompute_coeffs                                   # (the strip's 126 000-row table: made once)
    orc.precompute_coeffs = functools.lru_cache(maxsize=None)(plain)
    try:
        ref = [np.ascontiguousarray(orc.clip_preprocess_u8(a).transpose(2, 0, 1)) for a in images]    # planar (3,336,336) uint8
    finally:
        orc.precompute_coeffs = plain
    table = hip_ops.norm_lut().to(DEV)
    assert np.array_equal(table.cpu().numpy().view(np.uint32), orc.normalise_lut().view(np.uint32))
    return dict(ops=hip_ops, lib=_lib, L=_lib.load(), syn=synthetic, orc=orc, images=images, ref=ref, table=table)


@pytest.fixture(scope="module")
def tower(env):
    """The 2-layer tower of the issue, with the exact tier's weight copy; graph replay on (the default)."""
    enc = env["ops"].VitEncoder(env["syn"].make_vit_weights(seed=0, layers=2), precise=True)
    yield enc
    enc.close()


def _lookup(env, b):
    """table[c][bytes] for (..., 3, 336, 336) uint8 on the device: the fp32 pixels of those bytes."""
    return env["ops"].bytes_to_pixels(b)


def _byte_images(n, seed):
    """(n,3,336,336) uint8: every plane holds all 256 byte values (its first 256 pixels, rotated by plane and image), the rest seeded noise."""
    g = torch.Generator().manual_seed(seed)
    b = torch.randint(0, 256, (n, 3, S, S), generator=g, dtype=torch.uint8)
    flat = b.view(n, 3, -1)
    for i in range(n):
        for c in range(3):
            flat[i, c, :256] = torch.roll(torch.arange(256, dtype=torch.int64), 37 * c + 11 * i).to(torch.uint8)
    return b.to(DEV)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------- 1. resize to bytes
def _guarded(n):
    return torch.full((n * IMG + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)


def _check_bytes(env, out, which, n):
    """The first len(which) of the n images in `out` against the oracle's bytes of GEOMS[which[j]]; the guard behind all n."""
    torch.cuda.synchronize()
    got = out[:n * IMG].view(n, 3, S, S)
    for j, i in enumerate(which):
        assert np.array_equal(got[j].cpu().numpy(), env["ref"][i]), f"image {GEOMS[i]}"
    assert bool((out[n * IMG:] == SENTINEL).all()), "bytes behind the output were written"
    return got


@pytest.mark.parametrize("i", range(len(GEOMS)), ids=[f"{h}x{w}" for h, w in GEOMS])
def test_prep_forward_writes_the_resized_bytes(env, i):
    """pg_prep_forward(out_dtype = U8): the oracle's resized, cropped bytes in planar order; table[c][bytes] is the same call's fp32
    output; nothing is written behind the n images."""
    ops, L = env["ops"], env["L"]
    h, w = GEOMS[i]
    prep = ops.Preprocessor(h, w)
    n = 2
    src = torch.from_numpy(np.stack([env["images"][i], env["images"][i][::-1, ::-1].copy()])).to(DEV)
    need = C.c_size_t()
    assert L.pg_prep_workspace_bytes(prep._h, n, C.byref(need)) == 0
    ws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    out = _guarded(n)
    rc = L.pg_prep_forward(prep._h, C.c_void_p(src.data_ptr()), n, C.c_void_p(out.data_ptr()), U8, C.c_void_p(ws.data_ptr()), ws.numel(), _stream())
    assert rc == 0, L.pg_last_error()
    got = _check_bytes(env, out, [i], n)                               # (image 1 is the flipped one: checked through the table below)
    assert torch.equal(_lookup(env, got), prep.forward(src, torch.float32))
    assert torch.equal(prep.forward(src, torch.uint8), got)            # the binding: same bytes
    prep.close()


def test_prep_ragged_forward_writes_the_resized_bytes(env):
    ops, L = env["ops"], env["L"]
    from pigeon_amd.packing import pack_images
    prep = ops.RaggedPreprocessor(0)
    order = [5, 0, 3, 1, 4, 2]                                         # the strip first: its rows lead the shared temp image
    plan = prep.plan([GEOMS[i] for i in order])
    packed = pack_images([env["images"][i] for i in order]).data.clone()
    packed.numpy()[:plan.header_bytes] = plan.header()
    packed = packed.to(DEV)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=DEV)
    n = len(order)
    out = _guarded(n)
    rc = L.pg_prep_ragged_forward(prep._h, C.c_void_p(packed.data_ptr()), plan.packed_bytes, plan.items, n, C.c_void_p(out.data_ptr()), U8,
                                  C.c_void_p(ws.data_ptr()), ws.numel(), _stream())
    assert rc == 0, L.pg_last_error()
    got = _check_bytes(env, out, order, n)
    assert torch.equal(_lookup(env, got), prep.forward(packed, plan, torch.float32, header_written=True))
    assert torch.equal(prep.forward(packed, plan, torch.uint8, header_written=True), got)
    prep.close()


# ---------------------------------------------------------------------------------------------------- 2. im2col
@pytest.mark.parametrize("n", [1, 3])
def test_im2col_from_bytes_equals_im2col_from_the_table(env, n):
    ops = env["ops"]
    b = _byte_images(n, seed=n)
    for c in range(3):
        assert torch.unique(b[n - 1, c]).numel() == 256                # the input really holds every byte in every plane
    p = _lookup(env, b)
    assert p.dtype == torch.float32 and p.shape == b.shape
    for dt in (torch.float16, torch.bfloat16):
        got, want = ops.im2col(b, dt), ops.im2col(p, dt)
        assert got.shape == (n * 576, 640) and torch.equal(got.view(torch.int16), want.view(torch.int16)), dt
        assert not got[:, 588:].view(torch.int16).any()                # the zero columns 588 - 639
    filled = lambda: torch.full((n * 576, 3 * 640), 7.0, dtype=torch.float16, device=DEV)      # noqa: E731
    got3, want3 = ops.x3_im2col(b, out=filled()), ops.x3_im2col(p, out=filled())
    assert torch.equal(got3.view(torch.int16), want3.view(torch.int16))
    for seg in range(3):
        assert not got3[:, 640 * seg + 588:640 * (seg + 1)].view(torch.int16).any()
        assert got3[:, 640 * seg:640 * seg + 588].view(torch.int16).any()


# ---------------------------------------------------------------------------------------------------- 3. encoder
@pytest.mark.parametrize("n", [1, 5])
def test_both_tiers_from_bytes_equal_the_tiers_from_the_table(env, tower, n):
    b = _byte_images(n, seed=10 + n)
    p = _lookup(env, b)
    r0, c0 = tower.graph(True)
    # fast tier, graph on: the first forward of a (workspace, n) runs eagerly, the second captures, the third replays
    runs = [tower.forward(b, return_hidden=True) for _ in range(3)]
    r1, c1 = tower.graph()
    assert c1 - c0 >= 1 and r1 - r0 >= 1, (r0, c0, r1, c1)
    want_e, want_h = tower.forward(p, return_hidden=True)
    for e, h in runs:
        assert torch.equal(e, want_e) and torch.equal(h, want_h)
    assert bool(torch.isfinite(want_e).all()) and float(want_e.abs().max()) > 0
    tower.graph(False)
    e, h = tower.forward(b, return_hidden=True)                        # and with the graph off
    tower.graph(True)
    assert torch.equal(e, want_e) and torch.equal(h, want_h)
    # exact tier
    xe, xh = tower.forward_precise(b, return_hidden=True)
    we, wh = tower.forward_precise(p, return_hidden=True)
    assert torch.equal(xe, we) and torch.equal(xh, wh)
    assert not torch.equal(xe, want_e)                                 # (the two tiers are different arithmetic)


# ---------------------------------------------------------------------------------------------------- 4. negative control
def test_fp16_pixels_cost_the_exact_tier_its_floor_and_bytes_do_not(env, tower):
    """Why this exists: the exact encoder on fp16-rounded pixels is off its result on the fp32 pixels by more than the exact tier's
    own floor (margin_rel_tol_exact = 5e-6) on every image; from bytes the difference is exactly 0."""
    from pigeon_amd.certainty import Certainty
    floor = Certainty().rel_tol_exact
    assert floor == 5e-6
    g = torch.Generator().manual_seed(0)
    b = torch.randint(0, 256, (3, 3, S, S), generator=g, dtype=torch.uint8).to(DEV)        # three images of uniform random bytes
    p = _lookup(env, b)
    exact = tower.forward_precise(p).double()
    from_half = tower.forward_precise(p.half()).double()
    from_bytes = tower.forward_precise(b).double()
    rel = ((from_half - exact).norm(dim=1) / exact.norm(dim=1)).cpu()
    print("exact tier, fp16 pixels vs fp32 pixels, relative:", rel.tolist())
    assert bool((rel > floor).all()), rel
    assert float((from_bytes - exact).abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------- 5. model route
def _model(env, tmp_path, C_=64):
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    from pigeon_amd.proto_refiner import ProtoRefiner
    from pigeon_amd.super_guessr import SuperGuessr
    syn = env["syn"]
    gp = os.path.join(str(tmp_path), "g.csv")
    syn.write_geocell_csv(gp, syn.make_geocells(C_, seed=0))
    vit = HipCLIPVisionModel(syn.make_vit_weights(seed=0, layers=2), layers=2).to(DEV)
    W, bias = syn.make_head_weights(C_, seed=1)
    m = SuperGuessr(vit, panorama=True, freeze_base=True, num_candidates=5, geocell_path=gp, exact_top1=True, margin_kappa=3.6,
                    margin_autocalibrate=False, margin_rel_tol=1e-3)
    with torch.no_grad():
        m.cell_layer.weight.copy_(W * 64); m.cell_layer.bias.copy_(bias)
    m = m.to(DEV).eval()
    ref = ProtoRefiner(topk=5, max_refinement=1000, temperature=1.6, bank=syn.make_bank(C_, 9, seed=5, empty_frac=0.1, max_members=6),
                       device=DEV).eval()
    return m, ref


def _same(a, b, path="out"):
    if torch.is_tensor(a):
        assert torch.is_tensor(b) and a.dtype == b.dtype and a.shape == b.shape, path
        assert torch.equal(a, b) or torch.equal(torch.nan_to_num(a.double(), nan=-7.0), torch.nan_to_num(b.double(), nan=-7.0)), path
    elif isinstance(a, dict):
        assert set(a) == set(b), path
        for k in a:
            _same(a[k], b[k], f"{path}[{k}]")
    elif isinstance(a, (tuple, list)):
        assert type(a) is type(b) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{path}[{i}]")
    else:
        assert a == b, (path, a, b)


def test_certain_forward_from_bytes_equals_certain_forward_from_the_table(env, tmp_path):
    from pigeon_amd.evaluate import certain_forward
    m, ref = _model(env, tmp_path)
    B = 3
    g = torch.Generator().manual_seed(5)
    b = torch.randint(0, 256, (B, 12, S, S), generator=g, dtype=torch.uint8)
    p = _lookup(env, b.to(DEV).view(B * 4, 3, S, S)).view(B, 12, S, S)
    labels = dict(labels=torch.tensor([[1.0, 2.0], [30.0, -40.0], [-100.0, 60.0]], dtype=torch.float64), labels_clf=torch.tensor([3, 1, 60]))
    for kappa, all_exact in ((m.certainty.kappa, False), (1e30, True)):
        m.certainty.kappa = kappa                                       # (the threshold is kappa x rel_tol: 1e30 sends every row to the exact tier)
        out_b, info_b = certain_forward(m, ref, pixel_bytes=b if not all_exact else b.to(DEV), **labels)      # host bytes once, device bytes once
        q = m.engine(ref).q_pixels
        assert q.dtype == torch.uint8 and q.numel() * q.element_size() == m.engine(ref).cap * 1354752 and m.engine(ref).cap >= B
        out_p, info_p = certain_forward(m, ref, pixel_values=p, **labels)
        assert m.engine(ref).q_pixels.dtype == torch.float32            # the same engine moved its queue to the other pixel format
        _same(tuple(out_b), tuple(out_p))
        _same(info_b, info_p, "info")
        assert info_b["reencoded"].numel() == (B if all_exact else info_p["reencoded"].numel())
        if all_exact:
            assert info_b["reencoded"].tolist() == list(range(B))
        assert out_b.preds_geocell.shape == (B,) and out_b.embedding.shape == (B, 4, 1024) and out_b.loss_clf is not None
    # `forward` and `encode_head` take the keyword too; a uint8 tensor under the OLD name is still numbers, not table indices
    m.certainty.kappa = 3.6
    _same(tuple(m(pixel_bytes=b, **labels)), tuple(m(pixel_values=p, **labels)))
    _same(m.encode_head(pixel_bytes=b.to(DEV))["logits"], m.encode_head(p)["logits"])
    _same(m.encode_head(b)["logits"], m.encode_head(b.float())["logits"])
    assert not torch.equal(m.encode_head(b)["logits"], m.encode_head(pixel_bytes=b)["logits"])


# ---------------------------------------------------------------------------------------------------- 6. evaluate from images
def test_evaluate_model_from_images_equals_evaluate_model_from_host_pixel_values(env, tmp_path):
    from pigeon_amd.evaluate import ImageEvalDataset, evaluate_model
    orc = env["orc"]
    m, ref = _model(env, tmp_path)
    rng = np.random.default_rng(3)
    sizes = [(S, S), (340, 400), (400, 350), (350, 500), (337, 336)]
    raw, host = [], []
    for i in range(6):
        lab = {"labels": torch.tensor([10.0 * i, -5.0 * i], dtype=torch.float64), "labels_clf": torch.tensor(i)}
        item = dict(lab)
        for v, key in enumerate(("image", "image_2", "image_3", "image_4")):
            h, w = sizes[(i + v) % len(sizes)]
            item[key] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        raw.append(item)
        px = np.concatenate([orc.clip_preprocess(item[k]) for k in ("image", "image_2", "image_3", "image_4")], axis=0)
        assert px.shape == (12, S, S) and px.dtype == np.float32
        host.append(dict(lab, pixel_values=torch.from_numpy(px)))
    got = evaluate_model(m, ImageEvalDataset(raw), refiner=ref, batch_size=4)
    want = evaluate_model(m, host, refiner=ref, batch_size=4)
    for k in ("preds", "preds_geocells", "top5_geocells", "geocell_certain"):
        assert got[k].shape[0] == 6 and np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["top5_probs"], want["top5_probs"]) and got["loss_clf"] == want["loss_clf"]


# ---------------------------------------------------------------------------------------------------- 7. refusals through the ABI
def test_abi_refuses_bytes_as_output_and_unknown_pixel_codes(env, tower):
    L = env["L"]
    err = lambda: (L.pg_last_error() or b"").decode()                  # noqa: E731
    b = _byte_images(1, seed=3)
    out = torch.full((576, 640), 7.0, dtype=torch.float16, device=DEV)
    args = lambda pix, o: (C.c_void_p(b.data_ptr()), pix, C.c_void_p(out.data_ptr()), o, 1, _stream())     # noqa: E731
    assert L.pg_op_im2col(*args(U8, U8)) == -1 and "PG_DTYPE_U8" in err() and "output" in err()
    assert L.pg_op_im2col(*args(F32, U8)) == -1 and "PG_DTYPE_U8" in err()
    assert L.pg_op_im2col(*args(99, F16)) == -1 and "pixel dtype 99" in err()
    assert L.pg_op_x3_im2col(C.c_void_p(b.data_ptr()), 99, C.c_void_p(out.data_ptr()), 0, _stream()) == 0      # (no images: nothing to refuse)
    big = torch.full((576, 3 * 640), 7.0, dtype=torch.float16, device=DEV)
    assert L.pg_op_x3_im2col(C.c_void_p(b.data_ptr()), 99, C.c_void_p(big.data_ptr()), 1, _stream()) == -1 and "pixel dtype 99" in err()
    emb = torch.full((1, 1024), 7.0, device=DEV)
    ws = tower._workspace(1)
    off = (-ws.data_ptr()) % 256
    for fn, extra in ((L.pg_vit_forward_hidden, (None,)), (L.pg_vit_forward_precise, (None,))):
        rc = fn(tower._h, C.c_void_p(b.data_ptr()), 99, 1, C.c_void_p(emb.data_ptr()), *extra, C.c_void_p(ws.data_ptr() + off), ws.numel() - off, _stream())
        assert rc == -1 and "bad pixel dtype" in err()
    rc = L.pg_vit_forward(tower._h, C.c_void_p(b.data_ptr() + 1), U8, 1, C.c_void_p(emb.data_ptr()), C.c_void_p(ws.data_ptr() + off), ws.numel() - off, _stream())
    assert rc == -1 and "aligned" in err()                             # bytes are read as 4-byte words: an odd address is refused
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((big == 7.0).all()) and bool((emb == 7.0).all())      # nothing was launched
    # and the resize refuses an unknown output code as before
    prep = env["ops"].Preprocessor(336, 336)
    src = torch.zeros((1, S, S, 3), dtype=torch.uint8, device=DEV)
    need = C.c_size_t()
    L.pg_prep_workspace_bytes(prep._h, 1, C.byref(need))
    pws = torch.empty(need.value, dtype=torch.uint8, device=DEV)
    guard = _guarded(1)
    rc = L.pg_prep_forward(prep._h, C.c_void_p(src.data_ptr()), 1, C.c_void_p(guard.data_ptr()), 1, C.c_void_p(pws.data_ptr()), pws.numel(), _stream())
    assert rc == -1 and "out dtype" in err()
    prep.close()


# ---------------------------------------------------------------------------------------------------- CLIPEmbedding(pixel_bytes=True)
def test_clip_embedding_preprocesses_to_bytes_and_encodes_both_tiers_from_them(env, monkeypatch):
    from pigeon_amd import clip_embedder as ce
    vit = ce.HipCLIPVisionModel(env["syn"].make_vit_weights(seed=0, layers=2), layers=2)
    images = [env["images"][i] for i in (3, 4, 2)]                     # three sizes: the ragged path
    want_bytes = torch.from_numpy(np.stack([env["ref"][i] for i in (3, 4, 2)])).to(DEV)
    seen = []
    real = ce.gpu_preprocess
    monkeypatch.setattr(ce, "gpu_preprocess", lambda im, dev, dt=torch.float32: seen.append(dt) or real(im, dev, dt))
    emb = ce.CLIPEmbedding("none", device=DEV, clip_model=vit, contract_guard="off", pixel_bytes=True)
    p = _lookup(env, want_bytes)
    fast = emb(images)
    assert seen == [torch.uint8] and torch.equal(fast, vit.embed(pixel_values=p)) and torch.equal(fast, vit.embed(pixel_bytes=want_bytes))
    emb.certainty.force_exact = True
    assert torch.equal(emb(images), vit.embed_precise(pixel_values=p))
    # the guard's measurement runs from the same bytes
    guarded = ce.CLIPEmbedding("none", device=DEV, clip_model=vit, contract_guard="exact", pixel_bytes=True)
    guarded(images)
    assert guarded.guard_stats is not None and guarded.guard_stats["images"] == 3 and seen[-1] == torch.uint8
    # the default stays what it was: fp16 pixels with fp16 operands
    monkeypatch.delenv("PIGEON_PIXEL_BYTES", raising=False)
    plain = ce.CLIPEmbedding("none", device=DEV, clip_model=vit, contract_guard="off")
    assert plain.pixel_bytes is False
    plain(images)
    assert seen[-1] == plain._pixel_dtype() != torch.uint8
    monkeypatch.setenv("PIGEON_PIXEL_BYTES", "1")
    assert ce.CLIPEmbedding("none", device=DEV, clip_model=vit, contract_guard="off").pixel_bytes is True
