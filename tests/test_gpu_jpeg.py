"""GPU side of the JPEG decoder (pg_jpeg_forward, pigeon_amd/csrc/jpeg.hip): every fixture of tests/golden/jpeg_fixtures.npz as one
ragged batch against the Pillow pixels committed with it, hand-made coefficients against the numpy restatement (tests/_jpegref.py,
itself pinned to Pillow in tests/test_jpegref_cpu.py), buffer discipline, and the paths above it.  Integer work: every comparison is
for equal bits.  No test here needs Pillow except the one that mixes in files Pillow has to decode."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _jpegref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0xA5
GUARD = 4096


def _load(golden_dir):
    z = np.load(os.path.join(golden_dir, "jpeg_fixtures.npz"))
    off, shapes = z["file_off"], z["shapes"]
    po = np.cumsum([0] + [int(h) * int(w) * 3 for h, w in shapes])
    files = [z["files"][off[i]:off[i + 1]].tobytes() for i in range(len(shapes))]
    pixels = [z["pixels"][po[i]:po[i + 1]].reshape(int(shapes[i][0]), int(shapes[i][1]), 3) for i in range(len(shapes))]
    return [str(n) for n in z["names"]], files, pixels, [str(r) for r in z["refused"]]


@pytest.fixture(scope="module")
def fx(golden_dir):
    from pigeon_amd import _lib, hip_ops, jpeg
    _lib.require_gpu()
    names, files, pixels, refused = _load(golden_dir)
    ok = [i for i, r in enumerate(refused) if not r]
    return dict(ops=hip_ops, jpeg=jpeg, names=names, files=files, pixels=pixels, refused=refused, ok=ok)


def _forward_guarded(ops, plan, coef_host):
    """pg_jpeg_forward into a packed buffer pre-filled with a pattern and followed by a guard region; returns the whole allocation."""
    whole = torch.full((plan.prep.packed_bytes + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    ops.jpeg_forward(coef_host.to(DEV), plan, whole[:plan.prep.packed_bytes])
    torch.cuda.synchronize()
    return whole.cpu().numpy()


def _check_batch(fx, order):
    ops = fx["ops"]
    files = [fx["files"][i] for i in order]
    plan = ops.jpeg_plan([ops.jpeg_probe(f) for f in files])
    coef = torch.zeros(plan.coef_bytes, dtype=torch.uint8)
    ops.jpeg_entropy_decode(files, plan, coef)
    got = _forward_guarded(ops, plan, coef)
    touched = np.zeros(got.size, dtype=bool)
    touched[:plan.prep.header_bytes] = True
    out = {}
    for k, i in enumerate(order):
        want = fx["pixels"][i]
        off = int(plan.items[k].rgb_off)
        img = got[off:off + want.size].reshape(want.shape)
        assert np.array_equal(img, want), f"{fx['names'][i]}: {R.first_mismatch(img, want)}"
        touched[off:off + want.size] = True
        out[i] = img
    assert bytes(got[:plan.prep.header_bytes]) == bytes(plan.prep.header()), "the resize's descriptors are not in the buffer's head"
    assert (got[~touched] == SENTINEL).all(), "bytes between the images or behind the buffer were written"
    return out


def test_all_fixtures_as_one_ragged_batch_equal_pillow(fx):
    """Every supported fixture in ONE call: each image equals Pillow's pixels; the bytes between images and the guard region behind the
    buffer keep their pattern; the same images in reversed order give the same bytes per image."""
    fwd = _check_batch(fx, fx["ok"])
    rev = _check_batch(fx, fx["ok"][::-1])
    for i in fx["ok"]:
        assert np.array_equal(fwd[i], rev[i]), fx["names"][i]


SAMPLINGS = {"444": (1, 1), "422": (2, 1), "420": (2, 2)}


def _handmade_plan(ops, lib, shapes):
    infos = []
    for h, w, ncomp, hs, vs in shapes:
        info = lib.JpegInfo()
        info.reason, info.height, info.width, info.ncomp, info.hs, info.vs = 0, h, w, ncomp, hs, vs
        infos.append(info)
    return ops.jpeg_plan(infos)


def _run_handmade(ops, plan, coefs, qts, qsels):
    """coefs[i][c]: (blocks, 64) int16 -> packed output (host) with guard."""
    coef = torch.zeros(plan.coef_bytes, dtype=torch.uint8)
    view = coef.numpy()
    for i in range(plan.n):
        it = plan.items[i]
        for c in range(it.ncomp):
            view[it.coef_off[c]:it.coef_off[c] + coefs[i][c].size * 2] = coefs[i][c].reshape(-1).view(np.uint8)
            it.qsel[c] = qsels[i][c]
        C.memmove(C.addressof(it.qt), qts[i].astype(np.uint16).tobytes(), 512)
    return _forward_guarded(ops, plan, coef)


@pytest.mark.parametrize("mode", list(SAMPLINGS))
def test_handmade_coefficients_equal_the_restatement(fx, mode):
    """No entropy decoder: on a 16 x 16 image, one non-zero coefficient at each of the 64 positions in turn (in a different block and
    component each time) and DC-only blocks with a distinct value per block and component, all in one batch; three different
    quantisation tables, one per component.  Per pixel against the restatement: a transposed block, a block at the wrong grid position
    or a component read with another component's table shows up at a named pixel."""
    from pigeon_amd import _lib
    ops = fx["ops"]
    hs, vs = SAMPLINGS[mode]
    grid = R.block_grid(16, 16, 3, hs, vs)
    rng = np.random.default_rng(7)
    qt = np.zeros((4, 64), dtype=np.uint16)
    qt[1], qt[2], qt[3] = rng.integers(1, 12, 64), rng.integers(1, 12, 64), rng.integers(1, 12, 64)
    qsel = [3, 1, 2]
    coefs = []
    for k in range(64):                                             # one coefficient, moving through the blocks of every component
        per = []
        for c, (bw, bh) in enumerate(grid):
            a = np.zeros((bw * bh, 64), dtype=np.int16)
            a[:, 0] = 8 * (np.arange(bw * bh) - 1)                  # (a DC so that the AC term is not clipped away)
            a[(k + c) % (bw * bh), k] = (40 + k) * (-1 if (k + c) % 2 else 1)
            per.append(a)
        coefs.append(per)
    dc = []
    for c, (bw, bh) in enumerate(grid):                             # DC only, distinct per block and component
        a = np.zeros((bw * bh, 64), dtype=np.int16)
        a[:, 0] = 10 * np.arange(bw * bh) - 20 + 7 * c
        dc.append(a)
    coefs.append(dc)
    n = len(coefs)
    plan = _handmade_plan(ops, _lib, [(16, 16, 3, hs, vs)] * n)
    got = _run_handmade(ops, plan, coefs, [qt] * n, [qsel] * n)
    for i in range(n):
        want = R.pixels_from_coefficients(coefs[i], qt, qsel, 16, 16, 3, hs, vs)
        off = int(plan.items[i].rgb_off)
        img = got[off:off + want.size].reshape(want.shape)
        assert np.array_equal(img, want), f"{mode}, image {i}: {R.first_mismatch(img, want)}"


def test_extreme_coefficients_complete_and_stay_inside_the_buffer(fx):
    """Random int16 coefficients at the extremes with 16-bit quantisation tables: far outside the range in which the integer DCT is exact,
    so NO parity with any other decoder is claimed here -- only that the call completes, the pixels are the ones the restatement's
    32-bit wrap-around arithmetic gives, and nothing outside the images is written."""
    from pigeon_amd import _lib
    ops = fx["ops"]
    rng = np.random.default_rng(11)
    shapes = [(37, 53, 3, 2, 2), (9, 17, 3, 2, 1), (33, 1, 3, 1, 1), (7, 9, 1, 1, 1)]
    plan = _handmade_plan(ops, _lib, shapes)
    pool = np.array([-32768, -32767, -1, 0, 1, 32767], dtype=np.int16)
    coefs, qts, qsels = [], [], []
    for h, w, ncomp, hs, vs in shapes:
        coefs.append([np.where(rng.random((bw * bh, 64)) < 0.5, rng.choice(pool, (bw * bh, 64)),
                               rng.integers(-32768, 32768, (bw * bh, 64))).astype(np.int16) for bw, bh in R.block_grid(h, w, ncomp, hs, vs)])
        qts.append(rng.choice(np.array([1, 255, 256, 65535], dtype=np.uint16), (4, 64)))
        qsels.append([0, 1, 3][:ncomp])
    got = _run_handmade(ops, plan, coefs, qts, qsels)
    touched = np.zeros(got.size, dtype=bool)
    touched[:plan.prep.header_bytes] = True
    for i, (h, w, ncomp, hs, vs) in enumerate(shapes):
        off = int(plan.items[i].rgb_off)
        touched[off:off + h * w * 3] = True
        want = R.pixels_from_coefficients(coefs[i], qts[i], qsels[i], h, w, ncomp, hs, vs)
        assert np.array_equal(got[off:off + want.size].reshape(want.shape), want), i
    assert (got[~touched] == SENTINEL).all()


def test_forward_refuses_inconsistent_descriptors_before_launch(fx):
    from pigeon_amd import _lib
    ops = fx["ops"]
    plan = _handmade_plan(ops, _lib, [(16, 16, 3, 2, 2), (9, 17, 1, 1, 1)])
    coef = torch.zeros(plan.coef_bytes, dtype=torch.uint8, device=DEV)
    packed = torch.full((plan.prep.packed_bytes,), SENTINEL, dtype=torch.uint8, device=DEV)

    def refused(match):
        with pytest.raises(_lib.PigeonHipError, match=match):
            ops.jpeg_forward(coef, plan, packed)
        torch.cuda.synchronize()
        assert (packed == SENTINEL).all(), "something was written although the call was refused"

    for field, index, value, match in (("bw", 0, 3, "image 0.*block grid"), ("rgb_off", None, 8, "image 1"),
                                       ("coef_off", 0, plan.coef_bytes, "image 1.*coefficients"), ("hs", None, 3, "image 1.*sampling"),
                                       ("plane_off", 0, 0, "image 1.*overlaps")):
        it = plan.items[1] if "image 1" in match else plan.items[0]
        old = getattr(it, field) if index is None else getattr(it, field)[index]
        if index is None:
            setattr(it, field, value)
        else:
            getattr(it, field)[index] = value
        refused(match)
        if index is None:
            setattr(it, field, old)
        else:
            getattr(it, field)[index] = old
    ops.jpeg_forward(coef, plan, packed)                             # and the untouched plan is accepted


@pytest.fixture(scope="module")
def subset(fx):
    """A handful of fixtures of every mode (the largest size, all three colour samplings and grey, a restart and an optimised file)."""
    want = ["37x53_420_noise_q75", "37x53_422_smooth_q75", "37x53_444_noise_q100", "37x53_grey_noise_q1", "17x33_420_smooth_rst1",
            "9x17_422_smooth_opt", "1x1_420_noise_q75", "2x7_420_smooth_q75"]
    return [fx["names"].index(n) for n in want]


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float16, torch.float32])
def test_decode_then_resize_equals_resize_of_pillow_pixels(fx, subset, dtype):
    from pigeon_amd.clip_embedder import EncodedImages, gpu_preprocess, pack_images
    got = gpu_preprocess(EncodedImages([fx["files"][i] for i in subset]), DEV, dtype)
    want = gpu_preprocess(pack_images([fx["pixels"][i] for i in subset]), DEV, dtype)
    assert got.shape == (len(subset), 3, 336, 336) and torch.equal(got, want)


def test_mixed_batch_with_host_fallbacks(fx, subset):
    """Supported files mixed with a progressive, a CMYK and a PNG file: all equal Pillow, three fallbacks with their reasons."""
    pytest.importorskip("PIL")
    extra = [i for i, r in enumerate(fx["refused"]) if r]
    order = [subset[0], extra[0], subset[1], extra[1], extra[2], subset[2]]
    dec = fx["jpeg"].decode_images(fx["jpeg"].EncodedImages([fx["files"][i] for i in order]), DEV)
    for k, i in enumerate(order):
        assert np.array_equal(dec.image(k).cpu().numpy(), fx["pixels"][i]), fx["names"][i]
    assert dec.fallbacks == [(1, "progressive"), (3, "components"), (4, "not_jpeg")]
    assert "3 image(s)" in fx["jpeg"].fallback_summary() or sum(fx["jpeg"].FALLBACKS.values()) >= 3


def test_two_decodes_in_a_row_share_the_coefficient_staging_buffer(fx, subset):
    """A larger batch, then a smaller one, nothing synchronised in between: the second call's coefficients go into the pinned buffer
    the first call's copy may still be reading.  Both give Pillow's pixels."""
    jpeg = fx["jpeg"]
    first, second = subset, subset[5:1:-1]
    decs = [jpeg.decode_images([fx["files"][i] for i in order], DEV) for order in (first, second)]
    torch.cuda.synchronize()
    for order, dec in zip((first, second), decs):
        assert len(dec) == len(order)
        for k, i in enumerate(order):
            assert np.array_equal(dec.image(k).cpu().numpy(), fx["pixels"][i]), fx["names"][i]
    staging = jpeg._STAGING[torch.cuda.current_device()]
    assert type(staging).__name__ == "PinnedStaging" and staging.buf.is_pinned() and staging.event is not None


def test_entropy_error_names_the_image_and_launches_nothing(fx, subset, monkeypatch):
    bad = bytearray(fx["files"][subset[0]])
    h = R.parse(bytes(bad))
    del bad[h["scan"] + 40:]                                         # the scan ends inside an MCU, no EOI
    files = [fx["files"][subset[1]], fx["files"][subset[2]], bytes(bad), fx["files"][subset[3]]]
    launched = []
    monkeypatch.setattr(fx["ops"], "jpeg_forward", lambda *a, **k: launched.append(1))
    with pytest.raises(ValueError, match="image 2") as e:
        fx["jpeg"].decode_images(files, DEV)
    assert e.value.index == 2 and not launched


def test_clip_embedding_on_bytes_equals_decoded_images(fx, subset):
    """CLIPEmbedding on a 2-layer tower: files as bytes and the same images decoded give the same embeddings, bit for bit."""
    from pigeon_amd import clip_embedder as ce, synthetic
    vit = ce.HipCLIPVisionModel(synthetic.make_vit_weights(seed=0, layers=2), layers=2)
    for kw in (dict(), dict(pixel_bytes=True)):
        model = ce.CLIPEmbedding("none", device=DEV, clip_model=vit, contract_guard="off", **kw)
        a = model(ce.EncodedImages([fx["files"][i] for i in subset]))
        b = model(ce.pack_images([fx["pixels"][i] for i in subset]))
        assert a.shape == (len(subset), 1024) and torch.equal(a, b)
