"""Host side of the ragged-batch CLIP preprocessing: pg_prep_ragged_plan against the oracle's arithmetic, its refusals, the packing
(pigeon_amd/packing.py) against the plan, and the chunking of collate_packed.  No GPU: the plan makes no HIP call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import clip_preprocess_oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(1, 1), (1, 336), (336, 336), (337, 336), (336, 500), (200, 300), (50, 51), (2, 900), (900, 2), (640, 640), (640, 640),
         (1000, 350), (340, 1200)]
S = 336


@pytest.fixture(scope="module")
def ops(hip_lib):
    from pigeon_amd import hip_ops
    return hip_ops


def _axis(in_size, out_size, o0):
    """(ksize, bounds rows [o0, o0 + 336)) of one axis as the oracle has them; the identity axis is one tap at the pixel itself."""
    if in_size == out_size:
        return 1, np.stack([np.arange(o0, o0 + S), np.ones(S, dtype=np.int64)], axis=1)
    ksize, bounds, _ = orc.precompute_coeffs(in_size, out_size)
    return ksize, bounds[o0:o0 + S]


def test_plan_matches_oracle(ops):
    from pigeon_amd import _lib
    plan = ops.ragged_plan(SIZES)
    n = len(SIZES)
    assert plan.n == n and plan.header_bytes == n * _lib.PREP_ITEM_BYTES == n * 80
    src_end, tab_end, rows = plan.header_bytes, 0, 0
    for i, (h, w) in enumerate(SIZES):
        it = plan.items[i]
        nh, nw = orc.resize_output_size(h, w)
        assert (it.in_h, it.in_w, it.new_h, it.new_w) == (h, w, nh, nw), i
        assert (it.top, it.left) == ((nh - S) // 2, (nw - S) // 2), i
        kh, _ = _axis(w, nw, it.left)
        kv, bv = _axis(h, nh, it.top)
        assert (it.ksize_h, it.ksize_v) == (kh, kv), i
        assert it.row0 == int(bv[0, 0]) and it.nrows == int(bv[-1, 0] + bv[-1, 1] - bv[0, 0]), i
        assert it.row0 == int(bv[:, 0].min()) and it.row0 + it.nrows == int((bv[:, 0] + bv[:, 1]).max()), i   # the span of all 336 rows
        # the image: 16-byte aligned, behind the header and the image before it, back to back
        assert it.src_off % 16 == 0 and src_end <= it.src_off < src_end + 16, i
        src_end = it.src_off + h * w * 3
        assert it.tmp_row == rows, i
        rows += it.nrows
        # the four tables: ascending, disjoint
        for off, size in ((it.bounds_h_off, S * 2 * 4), (it.kk_h_off, S * kh * 4), (it.bounds_v_off, S * 2 * 4), (it.kk_v_off, S * kv * 4)):
            assert off % 16 == 0 and off >= tab_end, i
            tab_end = off + size
        assert tuple(it.reserved) == (0, 0, 0)
    assert src_end <= plan.packed_bytes < src_end + 16 and plan.packed_bytes % 16 == 0
    tmp_off = (tab_end + 255) // 256 * 256
    assert tab_end <= plan.workspace_bytes and plan.workspace_bytes == tmp_off + rows * S * 3
    assert bytes(plan.header()) == bytes(plan.items)


def test_plan_refusals_name_the_cause(hip_lib):
    from pigeon_amd import _lib
    lib = hip_lib
    pb, wb = C.c_size_t(7), C.c_size_t(7)
    items = (_lib.PrepItem * 2)()

    def call(n, sizes, it=items, p=C.byref(pb), w=C.byref(wb)):
        hw = (C.c_int32 * max(1, len(sizes)))(*sizes) if sizes is not None else None
        rc = lib.pg_prep_ragged_plan(n, hw, it, p, w)
        return rc, (lib.pg_last_error() or b"").decode()

    rc, msg = call(-1, [5, 5])
    assert rc == -1 and "negative" in msg
    rc, msg = call(2, [400, 400, 0, 10])
    assert rc == -1 and "image 1" in msg and "0x10" in msg and "out of range" in msg
    rc, msg = call(2, [400, 16385, 10, 10])
    assert rc == -1 and "image 0" in msg and "16385" in msg and "out of range" in msg
    rc, msg = call(65536, [1, 1])
    assert rc == -1 and "65535" in msg
    rc, msg = call(1, None)
    assert rc == -1 and "null" in msg and "sizes" in msg
    rc, msg = call(1, [5, 5], it=None)
    assert rc == -1 and "null" in msg and "descriptor" in msg
    rc, msg = call(1, [5, 5], p=None)
    assert rc == -1 and "null" in msg
    rc, msg = call(1, [5, 5], w=None)
    assert rc == -1 and "null" in msg
    # an empty batch: zero bytes, no pointer needed
    pb.value = wb.value = 7
    rc, _ = call(0, None, it=None)
    assert rc == 0 and pb.value == 0 and wb.value == 0
    with pytest.raises(_lib.PigeonHipError, match="out of range"):
        from pigeon_amd import hip_ops
        hip_ops.ragged_plan([(10, 0)])


def test_plan_refuses_totals_beyond_32_bit_offsets(ops):
    """A 16384-pixel axis has 197-tap tables (~265 KB): 9000 such images outgrow the descriptor's 32-bit table offsets; 8000 fit."""
    from pigeon_amd import _lib
    assert ops.ragged_plan([(16384, 16384)] * 8000).items[7999].ksize_h == 197
    with pytest.raises(_lib.PigeonHipError, match="image 80[0-9][0-9].*32-bit"):
        ops.ragged_plan([(16384, 16384)] * 9000)


def _images(rng):
    from PIL import Image
    ims = [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in SIZES]
    rgb = Image.fromarray(rng.integers(0, 256, (30, 41, 3), dtype=np.uint8))
    modes = [rgb.convert("L"), rgb.convert("RGBA"), rgb.convert("P"), Image.fromarray(rng.integers(0, 256, (35, 35), dtype=np.uint8))]
    return ims, modes


def test_pack_images_agrees_with_the_plan(ops):
    from pigeon_amd.packing import pack_images, packed_layout
    ims, modes = _images(np.random.default_rng(3))
    arrays = [np.asarray(im) for im in ims[:4]]
    for batch in (ims, modes, ims[:3] + modes + arrays, arrays):
        packed = pack_images(batch)
        plan = ops.ragged_plan(packed.size_list())
        assert packed.data.dtype == torch.uint8 and packed.data.dim() == 1 and packed.data.numel() == plan.packed_bytes
        assert packed.sizes.dtype == torch.int32 and tuple(packed.sizes.shape) == (len(batch), 2)
        offs, total = packed_layout(packed.size_list())
        assert total == plan.packed_bytes and offs == [it.src_off for it in plan.items]
        buf = packed.data.numpy()
        assert not buf[:plan.header_bytes].any()                                   # the descriptors' place is left blank
        covered = np.zeros(total, dtype=bool)
        covered[:plan.header_bytes] = True
        for i, im in enumerate(batch):
            ref = np.asarray(im.convert("RGB")) if hasattr(im, "convert") else im   # what the list path converts to
            it = plan.items[i]
            assert (it.in_h, it.in_w) == ref.shape[:2]
            assert np.array_equal(buf[it.src_off:it.src_off + ref.size].reshape(ref.shape), ref), i
            assert np.array_equal(packed.image(i), ref)
            covered[it.src_off:it.src_off + ref.size] = True
        assert not buf[~covered].any()                                             # padding is zero
    assert len(pack_images([])) == 0 and pack_images([]).data.numel() == 0
    for bad in (np.zeros((4, 4), dtype=np.uint8), np.zeros((4, 4, 3), dtype=np.float32), np.zeros((4, 4, 4), dtype=np.uint8)):
        with pytest.raises(ValueError, match="uint8 RGB"):
            pack_images([bad])


def test_packing_needs_no_hip():
    """Packing is DataLoader-worker work: it runs with no GPU visible, without the HIP library loaded and without the modules that
    bind it imported."""
    code = (
        "import sys, numpy as np\n"
        "from PIL import Image\n"
        "from pigeon_amd.packing import pack_images\n"
        "from pigeon_amd.embed import RawImageDataset, collate_packed\n"
        "rng = np.random.default_rng(0)\n"
        "ims = [Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)) for h, w in [(5, 7), (9, 3), (336, 20)]]\n"
        "p = pack_images(ims + [ims[0].convert('L')])\n"
        "ds = RawImageDataset([{'image': im, 'index': i} for i, im in enumerate(ims)])\n"
        "chunks, idx = collate_packed([ds[i] for i in range(3)])\n"
        "assert len(p) == 4 and len(chunks) == 1 and idx.tolist() == [0, 1, 2]\n"
        "for m in ('pigeon_amd._lib', 'pigeon_amd.hip_ops', 'pigeon_amd.clip_embedder'):\n"
        "    assert m not in sys.modules, m + ' was imported'\n"
        "print('packed', p.data.numel())\n")
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert "packed" in r.stdout


def test_collate_packed_chunks():
    from pigeon_amd.embed import RawImageDataset, collate_packed
    from pigeon_amd.packing import packed_layout
    rng = np.random.default_rng(4)
    shapes = [(10, 10), (10, 10), (10, 10), (12, 9), (10, 10), (10, 10), (8, 8)]            # 300 / 324 / 192 bytes of pixels
    ds = RawImageDataset([{"image": rng.integers(0, 256, s + (3,), dtype=np.uint8), "index": 100 + i} for i, s in enumerate(shapes)])
    batch = [ds[i] for i in range(7)]
    chunks, idx = collate_packed(batch)
    assert len(chunks) == 1 and len(chunks[0]) == 7 and idx.dtype == torch.int64 and idx.tolist() == list(range(100, 107))
    # three images of 300 bytes + three descriptors = 1152 bytes at the most; a fourth does not fit into 1200
    chunks, idx = collate_packed(batch, max_packed_bytes=1200)
    assert [len(c) for c in chunks] == [3, 3, 1] and idx.tolist() == list(range(100, 107))
    k = 0
    for c in chunks:
        assert c.data.numel() == packed_layout(c.size_list())[1] <= 1200
        for j in range(len(c)):
            assert np.array_equal(c.image(j), batch[k][0])                                 # order kept across the chunks
            k += 1
    # one image above the budget travels alone, whatever stands around it
    big = (rng.integers(0, 256, (40, 40, 3), dtype=np.uint8), 7)
    chunks, idx = collate_packed([batch[0], batch[1], big, batch[2]], max_packed_bytes=1200)
    assert [len(c) for c in chunks] == [2, 1, 1] and chunks[1].size_list() == [(40, 40)] and chunks[1].data.numel() > 1200
    assert idx.tolist() == [100, 101, 7, 102]
    assert collate_packed([])[0] == []


def test_chunk_by_bytes_agrees_with_the_layout():
    """The one-pass chunking keeps every run within the budget as `packed_layout` counts it, cuts as late as it can, and caps the count."""
    from pigeon_amd.packing import chunk_by_bytes, packed_layout
    rng = np.random.default_rng(5)
    sizes = [(int(h), int(w)) for h, w in rng.integers(1, 40, (200, 2))]
    for budget in (500, 3000, 20000, 10 ** 9):
        runs = chunk_by_bytes(sizes, budget)
        assert runs[0][0] == 0 and runs[-1][1] == len(sizes) and all(a[1] == b[0] for a, b in zip(runs, runs[1:]))
        for lo, hi in runs:
            assert hi - lo == 1 or packed_layout(sizes[lo:hi])[1] <= budget
            assert hi == len(sizes) or packed_layout(sizes[lo:hi + 1])[1] > budget
    assert chunk_by_bytes(sizes, 10 ** 9, max_count=64) == [(0, 64), (64, 128), (128, 192), (192, 200)]
    assert chunk_by_bytes([], 100) == []
