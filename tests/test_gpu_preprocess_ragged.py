"""GPU side of the ragged-batch CLIP preprocessing (pg_prep_ragged_forward, pigeon_amd/csrc/preprocess.hip): device-made
coefficient tables and outputs against the numpy oracle (itself pinned to Pillow in tests/test_preprocess_cpu.py), equality with the
per-size path, buffer discipline, refusals before launch, and the paths above it (gpu_preprocess, embed_images).  Integer work:
every comparison is for equal bits."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 336
SIZES = [(1, 1), (1, 336), (336, 336), (337, 336), (336, 500), (200, 300), (50, 51), (2, 900), (900, 2), (640, 640), (640, 640),
         (1000, 350), (340, 1200)]
TALL = [(1200, 1200), (1100, 1200)]
SENTINEL = 0xA5


def _blocky(rng, h, w):
    return np.kron(rng.integers(0, 256, (h // 16 + 1, w // 16 + 1, 3), dtype=np.uint8), np.ones((16, 16, 1), dtype=np.uint8))[:h, :w]


@pytest.fixture(scope="module")
def env():
    """The batch of the issue twice -- white noise (every rounding / clipping path) and one blocky image per geometry (overshoot at
    edges) -- with the oracle's pixel_values, computed once."""
    from pigeon_amd import _lib, hip_ops
    from pigeon_amd.packing import pack_images
    from oracle import clip_preprocess_oracle as orc
    _lib.require_gpu()
    rng = np.random.default_rng(2024)
    noise = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in SIZES]
    blocky = [_blocky(rng, h, w) for h, w in SIZES]
    plain = orc.precompute_coeffs                                   # the 450:1 geometries' 151 200-row tables: made once, not four times
    orc.precompute_coeffs = functools.lru_cache(maxsize=None)(plain)
    try:
        ref = {"noise": [orc.clip_preprocess(a) for a in noise], "blocky": [orc.clip_preprocess(a) for a in blocky]}
    finally:
        orc.precompute_coeffs = plain
    prep = hip_ops.RaggedPreprocessor(0)
    plan = prep.plan(SIZES)
    packed = {"noise": pack_images(noise), "blocky": pack_images(blocky)}
    return dict(ops=hip_ops, lib=_lib, orc=orc, prep=prep, plan=plan, images={"noise": noise, "blocky": blocky}, ref=ref, packed=packed)


def _table(ws, off, rows, cols):
    return ws[off:off + rows * cols * 4].view(np.int32).reshape(rows, cols)


def test_device_tables_equal_the_oracle(env):
    """The bounds and 22-bit weights the first kernel writes, read back from the workspace at the plan's offsets: Pillow's
    precompute_coeffs + normalize_coeffs_8bpc rows [o0, o0 + 336), bit for bit -- identity axes, the 6.7x upscale of 50x51, the
    450:1 crops and 340x1200 included."""
    orc, prep = env["orc"], env["prep"]
    seen = set()
    # (the second batch: the longest filters sides of at most 1 200 pixels can have, 15 and 17 taps; only its tables are looked at)
    for sizes, data in ((SIZES, env["packed"]["noise"].data), (TALL, torch.zeros(prep.plan(TALL).packed_bytes, dtype=torch.uint8))):
        plan = prep.plan(sizes)
        prep.forward(data.to(DEV), plan, torch.float32)
        torch.cuda.synchronize()
        ws = prep._ws.cpu().numpy()
        _check_tables(orc, plan, sizes, ws, seen)
    assert {"identity", 5, 7, 9, 15, 17} <= seen, seen              # no pass, up-scaling, 1.003x .. 3.57x down-scaling


def _check_tables(orc, plan, sizes, ws, seen):
    for i, (h, w) in enumerate(sizes):
        it = plan.items[i]
        for in_size, out_size, o0, ksize, boff, koff in ((w, it.new_w, it.left, it.ksize_h, it.bounds_h_off, it.kk_h_off),
                                                         (h, it.new_h, it.top, it.ksize_v, it.bounds_v_off, it.kk_v_off)):
            bounds, kk = _table(ws, boff, S, 2), _table(ws, koff, S, ksize)
            if in_size == out_size:
                assert ksize == 1
                assert np.array_equal(bounds, np.stack([np.arange(o0, o0 + S), np.ones(S, dtype=np.int64)], axis=1)), (i, in_size)
                assert np.array_equal(kk, np.full((S, 1), 1 << 22)), (i, in_size)
                seen.add("identity")
                continue
            k, b, w_ref = orc.precompute_coeffs(in_size, out_size)
            assert ksize == k
            assert np.array_equal(bounds, b[o0:o0 + S]), (i, in_size, out_size)
            for o in range(S):
                cnt = int(b[o0 + o, 1])
                assert np.array_equal(kk[o, :cnt], w_ref[o0 + o, :cnt]), (i, in_size, out_size, o)
                assert not kk[o, cnt:].any()
            seen.add(ksize)


@pytest.mark.parametrize("kind", ["noise", "blocky"])
def test_outputs_equal_the_oracle(env, kind):
    prep, plan = env["prep"], env["plan"]
    on_dev = env["packed"][kind].data.to(DEV)
    got = prep.forward(on_dev, plan, torch.float32).cpu()
    got16 = prep.forward(on_dev, plan, torch.float16).cpu()
    assert got.shape == (len(SIZES), 3, S, S) and got16.dtype == torch.float16
    for i, ref in enumerate(env["ref"][kind]):
        assert np.array_equal(got[i].numpy(), ref), f"image {i} {SIZES[i]}: {np.abs(got[i].numpy() - ref).max()}"
        assert torch.equal(got16[i], torch.from_numpy(ref).to(torch.float16)), f"image {i} {SIZES[i]} fp16"


def test_equal_to_the_per_size_path_and_position_invariant(env):
    from pigeon_amd.packing import pack_images
    ops, prep = env["ops"], env["prep"]
    imgs = env["images"]["blocky"][:6] + env["images"]["noise"][6:]
    n = len(imgs)
    for dt in (torch.float32, torch.float16):
        batch = prep.forward(pack_images(imgs).data.to(DEV), prep.plan(SIZES), dt)
        rev = prep.forward(pack_images(imgs[::-1]).data.to(DEV), prep.plan(SIZES[::-1]), dt)
        for i, (h, w) in enumerate(SIZES):
            alone = ops.Preprocessor(h, w)(torch.from_numpy(imgs[i][None]).to(DEV), dt)[0]
            assert torch.equal(batch[i], alone), (i, dt)
            assert torch.equal(rev[n - 1 - i], alone), (i, dt)
            one = prep.forward(pack_images([imgs[i]]).data.to(DEV), prep.plan([SIZES[i]]), dt)
            assert one.shape[0] == 1 and torch.equal(one[0], alone), (i, dt)


def _raw_forward(env, items, n, packed, packed_bytes, out, out_dtype, ws, ws_bytes):
    lib = env["lib"].load()
    rc = lib.pg_prep_ragged_forward(env["prep"]._h, C.c_void_p(packed.data_ptr() if packed is not None else 0), packed_bytes, items, n,
                                    C.c_void_p(out.data_ptr() if out is not None else 0), out_dtype,
                                    C.c_void_p(ws.data_ptr() if ws is not None else 0), ws_bytes,
                                    C.c_void_p(torch.cuda.current_stream().cuda_stream))
    return rc, (lib.pg_last_error() or b"").decode()


def _with_header(env, kind="noise"):
    plan = env["plan"]
    host = env["packed"][kind].data.clone()
    host.numpy()[:plan.header_bytes] = plan.header()
    return host.to(DEV)


def test_nothing_written_outside_the_buffers(env):
    plan, n = env["plan"], len(SIZES)
    img = 3 * S * S * 4
    packed = _with_header(env)
    before = packed.clone()
    out = torch.full(((n + 1) * img,), SENTINEL, dtype=torch.uint8, device=DEV)           # one image slot behind the n outputs
    ws = torch.full((plan.workspace_bytes + 4096,), SENTINEL, dtype=torch.uint8, device=DEV)
    rc, msg = _raw_forward(env, plan.items, n, packed, plan.packed_bytes, out, env["lib"].PG_DTYPE_F32, ws, plan.workspace_bytes)
    assert rc == 0, msg
    torch.cuda.synchronize()
    assert bool((out[n * img:] == SENTINEL).all()) and bool((ws[plan.workspace_bytes:] == SENTINEL).all())
    assert torch.equal(packed, before)
    got = out[:n * img].view(torch.float32).reshape(n, 3, S, S).cpu().numpy()
    for i, ref in enumerate(env["ref"]["noise"]):
        assert np.array_equal(got[i], ref), i


def test_refused_before_launch(env):
    lib, plan, n = env["lib"], env["plan"], len(SIZES)
    packed = _with_header(env)
    out = torch.full((n, 3, S, S), -7.0, dtype=torch.float32, device=DEV)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=DEV)

    def items_with(i=None, **fields):
        items = (lib.PrepItem * n)()
        C.memmove(items, plan.items, C.sizeof(items))
        for k, v in fields.items():
            setattr(items[i], k, v)
        return items

    F32 = lib.PG_DTYPE_F32
    cases = [
        ("past packed", items_with(5, src_off=plan.packed_bytes - 16), plan.packed_bytes, F32, plan.workspace_bytes, -1, ("image 5", "packed")),
        ("short packed", items_with(), plan.packed_bytes - 16, F32, plan.workspace_bytes, -1, ("image 12", "packed")),
        ("misaligned", items_with(3, src_off=plan.items[3].src_off + 4), plan.packed_bytes, F32, plan.workspace_bytes, -1, ("image 3", "multiple of 16")),
        ("overlap", items_with(4, src_off=plan.items[3].src_off), plan.packed_bytes, F32, plan.workspace_bytes, -1, ("image 4", "overlaps")),
        ("table past ws", items_with(7, kk_v_off=(plan.workspace_bytes + 15) // 16 * 16), plan.packed_bytes, F32, plan.workspace_bytes, -1, ("image 7", "workspace")),
        ("table misaligned", items_with(7, kk_h_off=plan.items[7].kk_h_off + 4), plan.packed_bytes, F32, plan.workspace_bytes, -1, ("image 7", "multiple of 16")),
        ("geometry", items_with(2, nrows=plan.items[2].nrows + 1), plan.packed_bytes, F32, plan.workspace_bytes, -1, ("image 2", "geometry")),
        ("size", items_with(6, in_w=0), plan.packed_bytes, F32, plan.workspace_bytes, -1, ("image 6", "out of range")),
        ("prefix", items_with(9, tmp_row=plan.items[9].tmp_row - 1), plan.packed_bytes, F32, plan.workspace_bytes, -1, ("image 9", "temp row")),
        ("ws one byte short", items_with(), plan.packed_bytes, F32, plan.workspace_bytes - 1, -2, ("image 12", "workspace")),
        ("dtype", items_with(), plan.packed_bytes, lib.PG_DTYPE_BF16, plan.workspace_bytes, -1, ("dtype",)),
    ]
    for name, items, pbytes, dt, wbytes, want_rc, words in cases:
        rc, msg = _raw_forward(env, items, n, packed, pbytes, out, dt, ws, wbytes)
        assert rc == want_rc, (name, rc, msg)
        assert all(w in msg for w in words), (name, msg)
    rc, msg = _raw_forward(env, plan.items, -1, packed, plan.packed_bytes, out, F32, ws, plan.workspace_bytes)
    assert rc == -1 and "negative" in msg
    rc, msg = _raw_forward(env, plan.items, n, None, plan.packed_bytes, out, F32, ws, plan.workspace_bytes)
    assert rc == -1 and "null" in msg
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())                                # nothing was launched
    rc, msg = _raw_forward(env, None, 0, None, 0, None, F32, None, 0)
    assert rc == 0, msg
    # the binding's own refusals, before a pointer crosses the ABI
    prep, ops = env["prep"], env["ops"]
    for bad in (packed.cpu(), packed[:-16], packed.view(torch.int8), torch.zeros((2, plan.packed_bytes), dtype=torch.uint8, device=DEV)[:, ::2]):
        with pytest.raises(lib.PigeonHipError):
            prep.forward(bad, plan, torch.float32)
    with pytest.raises(lib.PigeonHipError, match="float32 or float16"):
        prep.forward(packed, plan, torch.bfloat16)
    assert prep.forward(torch.empty(0, dtype=torch.uint8, device=DEV), ops.ragged_plan([]), torch.float16).shape == (0, 3, S, S)


def test_gpu_preprocess_mixed_list_takes_the_ragged_path(env, monkeypatch):
    Image = pytest.importorskip("PIL.Image")
    from pigeon_amd import clip_embedder as ce, preprocess as pp
    ops = env["ops"]
    rng = np.random.default_rng(8)
    sizes = [(300, 400), (400, 300), (336, 336), (350, 500), (123, 457), (600, 338)]
    rgb = [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in sizes]
    ims = [rgb[0], rgb[1].convert("L"), rgb[2].convert("RGBA"), rgb[3].convert("P"), rgb[4], np.asarray(rgb[5])]
    as_pil = ims[:5] + [rgb[5]]
    want = ce.clip_preprocess(as_pil)
    ce.gpu_preprocess([rgb[0]])                                     # (the per-size cache is alive before the handles are forbidden)
    cached = list(pp._PREPROCESSORS)
    real = ops.Preprocessor

    def forbidden(*a, **k):
        raise AssertionError("a per-size handle was created")

    monkeypatch.setattr(ops, "Preprocessor", forbidden)
    got = ce.gpu_preprocess(ims)
    assert got.dtype == torch.float32 and torch.equal(got.cpu(), want)
    assert torch.equal(ce.gpu_preprocess(ims, out_dtype=torch.float16).cpu(), want.to(torch.float16))
    assert torch.equal(ce.gpu_preprocess(ims[:3]).cpu(), want[:3])  # a smaller batch through the same staging buffer
    packed = ce.pack_images(ims)
    assert torch.equal(ce.gpu_preprocess(packed).cpu(), want)
    assert not packed.data[:len(ims) * 80].any()                    # a pageable PackedImages is left as it came
    pinned = packed.pin_memory()
    assert packed.copy_event is None and torch.equal(ce.gpu_preprocess(pinned).cpu(), want)
    pinned.copy_event.synchronize()                                 # a pinned buffer is copied from in place: the event says when it is free
    assert pinned.data[:len(ims) * 80].any()
    assert ce.gpu_preprocess(ce.pack_images([])).shape == (0, 3, S, S)
    assert list(pp._PREPROCESSORS) == cached
    with pytest.raises(ValueError, match="uint8 RGB"):
        ce.gpu_preprocess([np.asarray(rgb[0]), np.zeros((5, 5, 3), dtype=np.float32)])
    # a list of one shape stays on pg_prep_forward
    made = []

    class Spy(real):
        def __init__(self, h, w, device=0):
            made.append((h, w))
            super().__init__(h, w, device=device)

    monkeypatch.setattr(ops, "Preprocessor", Spy)
    same = [Image.fromarray(rng.integers(0, 256, (211, 377, 3), dtype=np.uint8)) for _ in range(3)]
    assert torch.equal(ce.gpu_preprocess(same).cpu(), ce.clip_preprocess(same))
    assert made == [(211, 377)]


def test_gpu_preprocess_mixed_list_in_chunks_and_from_threads(env, monkeypatch):
    """A mixed list above the byte budget of one ragged call goes in consecutive chunks (same bits, same order), and callers from
    several threads, who share the pinned staging buffer, each get their own images' pixels."""
    import threading
    from pigeon_amd import clip_embedder as ce, preprocess as pp
    rng = np.random.default_rng(9)
    sizes = [(300, 400), (400, 300), (336, 336), (350, 500), (123, 457), (600, 338), (200, 210)]
    arrs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    want = ce.gpu_preprocess(arrs).cpu()
    assert torch.equal(want, ce.clip_preprocess([__import__("PIL.Image").Image.fromarray(a) for a in arrs]))
    calls = []
    real = pp._ragged_forward
    monkeypatch.setattr(pp, "_ragged_forward", lambda host, plan, *a, **k: (calls.append(plan.n), real(host, plan, *a, **k))[1])
    monkeypatch.setattr(pp, "RAGGED_MAX_BYTES", 800_000)            # 360 + 360 kB fit, + 339 do not; 339 + 525 do not; 525 + 169; 608 + 126
    assert torch.equal(ce.gpu_preprocess(arrs).cpu(), want)
    assert calls == [2, 1, 2, 2]
    monkeypatch.undo()
    got = {}

    def work(t):
        for r in range(4):
            got[(t, r)] = ce.gpu_preprocess(arrs[t:] + arrs[:t], out_dtype=torch.float16).cpu()

    threads = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    for (t, r), px in got.items():
        assert torch.equal(px, torch.cat([want[t:], want[:t]]).to(torch.float16)), (t, r)


def test_one_staging_buffer_serves_every_list_path(env):
    """The lists of ONE shape share one pinned staging buffer per device, whatever their count and shape; the lists of several shapes
    have the device's other one (with the pageable PackedImages).  Five calls with nothing synchronised in between: a shorter view of
    the one-shape buffer while the copy before may be queued, another output type, and a request that makes that buffer grow while the
    copy before may be queued.  Every call gives the host path's pixels bit for bit, and no further staging object exists."""
    import gc
    Image = pytest.importorskip("PIL.Image")
    from pigeon_amd import clip_embedder as ce, jpeg, preprocess as pp
    from pigeon_amd.packing import PinnedStaging
    rng = np.random.default_rng(10)
    a, b, c = ([rng.integers(0, 256, s + (3,), dtype=np.uint8) for _ in range(k)] for s, k in (((60, 80), 3), ((80, 60), 2), ((97, 41), 1)))
    calls = [(a, torch.float32), (a + b + c, torch.float32), (b, torch.float32), (a, torch.uint8), (c * 40, torch.float32)]
    dev, need = torch.cuda.current_device(), 40 * 97 * 41 * 3
    pp._UNIFORM_STAGING.pop(dev, None)                              # (whatever earlier tests grew it to: the last call here must grow it)
    got = [ce.gpu_preprocess(ims, out_dtype=dt) for ims, dt in calls[:4]]
    before = pp._UNIFORM_STAGING[dev].buf.numel()
    assert 3 * 60 * 80 * 3 <= before < need                         # the 2 x (80, 60) list took a shorter view of the same buffer
    got.append(ce.gpu_preprocess(*calls[4][:1], out_dtype=calls[4][1]))
    torch.cuda.synchronize()
    for k, ((ims, dt), px) in enumerate(zip(calls, got)):
        want = ce.clip_preprocess([Image.fromarray(im) for im in ims])
        assert px.dtype == dt and torch.equal(px.cpu() if dt != torch.uint8 else env["ops"].bytes_to_pixels(px.cpu()), want), k
    # exactly one buffer per device for the one-shape lists and one for the ragged path, keyed by the device alone ...
    for table in (pp._UNIFORM_STAGING, pp._STAGING):
        assert [i for i in table if type(i) is not int] == [] and type(table[dev]) is PinnedStaging and table[dev].buf.is_pinned()
    assert pp._UNIFORM_STAGING[dev] is not pp._STAGING[dev]
    assert pp._UNIFORM_STAGING[dev].buf.numel() >= need > before    # ... the first one grown by the 40-image list
    assert pp._STAGING[dev].buf.numel() >= env["ops"].ragged_plan([im.shape[:2] for im in a + b + c]).packed_bytes
    # ... and every staging object alive is one of those (or the JPEG decoder's): none kept anywhere else, per count or per shape
    known = {id(s) for table in (pp._UNIFORM_STAGING, pp._STAGING, jpeg._STAGING) for s in table.values()}
    gc.collect()
    assert {id(o) for o in gc.get_objects() if type(o) is PinnedStaging} == known


def test_embed_images_raw_equals_the_host_path(env, tmp_path):
    """`embed_images(raw_images=True)` -- workers decode and pack, the GPU resizes -- writes the embeddings and indices of the host
    path (workers run Pillow's resize, fp32 pixels cross the bus), also when the byte budget cuts every step into two chunks."""
    Image = pytest.importorskip("PIL.Image")
    from pigeon_amd import synthetic
    from pigeon_amd.clip_embedder import CLIPEmbedding, HipCLIPVisionModel, PackedImages
    from pigeon_amd.embed import embed_images
    sd = synthetic.make_vit_weights(seed=11, layers=2, affine_jitter=True)
    emb = CLIPEmbedding("synthetic", device="cuda", clip_model=HipCLIPVisionModel(sd, layers=2), contract_guard="off")
    rng = np.random.default_rng(12)
    sizes = [(400, 400 + 7 * i) for i in range(10)] + [(700, 800), (800, 700)]
    modes = ["RGB", "L", "RGB", "RGBA", "RGB", "P", "RGB", "RGB", "RGB", "RGB", "RGB", "RGB"]
    items = [{"image": Image.fromarray(rng.integers(0, 256, s + (3,), dtype=np.uint8)).convert(m), "index": i}
             for i, (s, m) in enumerate(zip(sizes, modes))]
    chunks_seen = []
    emb.register_forward_pre_hook(lambda mod, args: chunks_seen.append(len(args[0])) if isinstance(args[0], PackedImages) else None)

    def run(name, **kw):
        out = str(tmp_path / name)
        embed_images(emb, {"train": items}, batch_size=5, num_workers=2, out_dir=out, **kw)
        return np.load(os.path.join(out, "train.npy")), np.load(os.path.join(out, "train_indices.npy"))

    e_host, i_host = run("host")
    assert chunks_seen == [] and e_host.shape == (3, 5, 1024)
    e_raw, i_raw = run("raw", raw_images=True)
    assert chunks_seen == [5, 5, 2]
    assert np.array_equal(i_raw, i_host) and np.array_equal(e_raw, e_host)
    del chunks_seen[:]
    e_cut, i_cut = run("cut", raw_images=True, max_packed_bytes=1_800_000)     # 3 of the 400-row images fit, 4 do not; the 700 x 800 travel alone
    assert chunks_seen == [3, 2, 3, 2, 1, 1]
    assert np.array_equal(i_cut, i_host) and np.array_equal(e_cut, e_host)
