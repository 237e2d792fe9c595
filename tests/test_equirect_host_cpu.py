"""Host side of the equirectangular views, without a GPU: pg_equirect_plan against pg_prep_ragged_plan, every refusal of the plan and
of pg_equirect_forward by its message (the forward checks everything before its first HIP call, so no device is needed to be
refused), n = 0, and the Python side's rotation matrix and default view size."""
import ctypes as C
import math

import numpy as np
import pytest

import _equirectref as E

IDENT = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


@pytest.fixture(scope="module")
def ops(hip_lib):
    from pigeon_amd import _lib, hip_ops
    return _lib, hip_ops


def _views(sizes_src_s):
    """[(H, W, src index, S)] -> plan input with a plain view."""
    return [(h, w, k, s, IDENT, 1.0 / s) for h, w, k, s in sizes_src_s]


def test_plan_equals_the_ragged_resize_plan(ops):
    _lib, hip_ops = ops
    srcs = [(32, 64), (17, 33), (1, 1)]
    src_plan = hip_ops.ragged_plan(srcs)                                      # the panoramas lie where a packed buffer has them
    offs = [int(it.src_off) for it in src_plan.items]
    views = _views([(32, 64, 0, 24), (32, 64, 0, 1), (17, 33, 1, 21), (17, 33, 1, 41), (1, 1, 2, 2), (32, 64, 0, 336), (17, 33, 1, 7), (1, 1, 2, 5)])
    plan = hip_ops.equirect_plan(views, offs)
    want = hip_ops.ragged_plan([(v[3], v[3]) for v in views])
    assert plan.n == 8 and plan.prep.packed_bytes == want.packed_bytes and plan.prep.workspace_bytes == want.workspace_bytes
    assert bytes(plan.prep.header()) == bytes(want.header())
    for it, pi, v in zip(plan.items, plan.prep.items, views):
        assert int(it.dst_off) == int(pi.src_off) and int(it.dst_off) % 16 == 0
        assert int(it.src_off) == offs[v[2]]                                   # several views name one panorama
        assert (it.src_h, it.src_w, it.size) == (v[0], v[1], v[3])
        assert list(it.rot) == list(IDENT) and it.inv_f == v[5]
        assert it.reserved0 == 0 and list(it.reserved) == [0, 0, 0, 0]
    assert plan.src_bytes == max(o + h * w * 3 for o, (h, w) in zip(offs, srcs))
    assert C.sizeof(_lib.EqItem) == _lib.EQ_ITEM_BYTES == 128


def test_n_zero(ops):
    _lib, hip_ops = ops
    plan = hip_ops.equirect_plan([], [])
    assert plan.n == 0 and plan.prep.packed_bytes == 0 and plan.prep.workspace_bytes == 0
    lib = _lib.load()
    packed, ws = C.c_size_t(7), C.c_size_t(7)
    assert lib.pg_equirect_plan(0, None, 0, None, None, None, C.byref(packed), C.byref(ws)) == 0 and packed.value == 0 and ws.value == 0
    assert lib.pg_equirect_forward(None, 0, None, None, 0, None, 0, None) == 0          # a no-op: no pointer is looked at


@pytest.mark.parametrize("view,offs,message", [
    ((0, 64, 0, 24, IDENT, 0.1), [0], r"view 1: source size 0x64 out of range \(1\.\.16384\)"),
    ((32, 16385, 0, 24, IDENT, 0.1), [0], r"view 1: source size 32x16385 out of range"),
    ((32, 64, 0, 0, IDENT, 0.1), [0], r"view 1: view size 0 out of range \(1\.\.4096\)"),
    ((32, 64, 0, 4097, IDENT, 0.1), [0], r"view 1: view size 4097 out of range"),
    ((32, 64, 0, 24, IDENT[:4] + (float("nan"),) + IDENT[5:], 0.1), [0], r"view 1: rot\[4\] is not finite"),
    ((32, 64, 0, 24, (float("inf"),) + IDENT[1:], 0.1), [0], r"view 1: rot\[0\] is not finite"),
    ((32, 64, 0, 24, IDENT, 0.0), [0], r"view 1: inv_f = 0 is not finite and positive"),
    ((32, 64, 0, 24, IDENT, -0.5), [0], r"view 1: inv_f = -0\.5 is not finite and positive"),
    ((32, 64, 0, 24, IDENT, float("inf")), [0], r"view 1: inv_f = inf is not finite and positive"),
    ((32, 64, 0, 24, IDENT, float("nan")), [0], r"view 1: inv_f = -?nan is not finite and positive"),
    ((32, 64, 1, 24, IDENT, 0.1), [0], r"view 1: source index 1 outside the 1 sources"),
    ((32, 64, -1, 24, IDENT, 0.1), [0], r"view 1: source index -1 outside the 1 sources"),
    ((32, 64, 1, 24, IDENT, 0.1), [0, 8], r"view 1: source offset 8 is not a multiple of 16"),
])
def test_plan_refusals_name_the_view(ops, view, offs, message):
    _lib, hip_ops = ops
    good = (32, 64, 0, 24, IDENT, 0.1)
    with pytest.raises(_lib.PigeonHipError, match="equirect_plan: " + message):
        hip_ops.equirect_plan([good, view], offs)


def test_plan_refuses_bad_counts_and_null_pointers(ops):
    _lib, _ = ops
    lib = _lib.load()
    sz = C.c_size_t()
    err = lambda: lib.pg_last_error().decode()
    assert lib.pg_equirect_plan(-1, None, 0, None, None, None, C.byref(sz), C.byref(sz)) == -1 and "n = -1 is negative" in err()
    assert lib.pg_equirect_plan(0, None, 0, None, None, None, None, None) == -1 and "null size pointer" in err()
    assert lib.pg_equirect_plan(1, None, 0, None, None, None, C.byref(sz), C.byref(sz)) == -1 and "null argument" in err()
    n = 65536
    views, items, prep = (_lib.EqView * n)(), (_lib.EqItem * n)(), (_lib.PrepItem * n)()
    offs = (C.c_uint64 * 1)(0)
    assert lib.pg_equirect_plan(n, views, 1, offs, items, prep, C.byref(sz), C.byref(sz)) == -1 and "at most 65535 views per call" in err()


# ---- pg_equirect_forward: refused before its first HIP call ---------------------------------------------------------------------
SRC, PACKED = 0x10000000, 0x20000000                # never dereferenced: every call below is refused by the host-side checks


def _good(hip_ops):
    offs = [int(it.src_off) for it in hip_ops.ragged_plan([(32, 64), (17, 33)]).items]
    src_bytes = hip_ops.ragged_plan([(32, 64), (17, 33)]).packed_bytes
    plan = hip_ops.equirect_plan(_views([(32, 64, 0, 24), (17, 33, 1, 21), (32, 64, 0, 5)]), offs)
    return plan, src_bytes


def _forward(_lib, plan, src_bytes, src=SRC, packed=PACKED, packed_bytes=None, n=None):
    rc = _lib.load().pg_equirect_forward(C.c_void_p(src), src_bytes, plan.items, plan.prep.items, plan.n if n is None else n,
                                         C.c_void_p(packed), plan.prep.packed_bytes if packed_bytes is None else packed_bytes, None)
    return rc, _lib.load().pg_last_error().decode()


FORWARD_REFUSALS = [
    ("src_h", lambda p: setattr(p.items[1], "src_h", 16385), r"view 1: source size 16385x33 out of range"),
    ("src_w", lambda p: setattr(p.items[1], "src_w", 0), r"view 1: source size 17x0 out of range"),
    ("size_big", lambda p: setattr(p.items[1], "size", 4097), r"view 1: view size 4097 out of range"),
    ("size_zero", lambda p: setattr(p.items[1], "size", 0), r"view 1: view size 0 out of range"),
    ("rot_nan", lambda p: p.items[1].rot.__setitem__(7, float("nan")), r"view 1: rot\[7\] is not finite"),
    ("inv_f_neg", lambda p: setattr(p.items[1], "inv_f", -1.0), r"view 1: inv_f = -1 is not finite and positive"),
    ("inv_f_inf", lambda p: setattr(p.items[1], "inv_f", float("inf")), r"view 1: inv_f = inf is not finite and positive"),
    ("reserved", lambda p: p.items[1].reserved.__setitem__(2, 1), r"view 1: a reserved field is not zero"),
    ("reserved0", lambda p: setattr(p.items[1], "reserved0", 1), r"view 1: a reserved field is not zero"),
    ("size_differs", lambda p: setattr(p.items[1], "size", 20), r"view 1: size or offset differs from the resize's descriptor"),
    ("dst_differs", lambda p: setattr(p.items[1], "dst_off", p.items[1].dst_off + 16), r"view 1: size or offset differs from the resize's descriptor"),
    ("src_align", lambda p: setattr(p.items[1], "src_off", p.items[1].src_off + 8), r"view 1: source offset \d+ is not a multiple of 16"),
    ("src_range", lambda p: setattr(p.items[1], "src_off", p.items[1].src_off + 16), r"view 1: source range \[\d+, \+1683\) ends past the source buffer's \d+ bytes"),
    ("src_range_far", lambda p: setattr(p.items[1], "src_off", 1 << 40), r"view 1: source range .* ends past the source buffer"),
]


@pytest.mark.parametrize("name,damage,message", FORWARD_REFUSALS, ids=[r[0] for r in FORWARD_REFUSALS])
def test_forward_refusals_name_the_view(ops, name, damage, message):
    import re
    _lib, hip_ops = ops
    plan, src_bytes = _good(hip_ops)
    damage(plan)
    rc, msg = _forward(_lib, plan, src_bytes)
    assert rc == -1 and re.search("equirect_forward: " + message, msg), msg


def test_forward_refuses_destination_layouts(ops):
    """Offsets the resize's descriptors agree with, yet misaligned, overlapping, descending or past the buffer."""
    import re
    _lib, hip_ops = ops

    def both(plan, i, off):
        plan.items[i].dst_off = off
        plan.prep.items[i].src_off = off

    plan, src_bytes = _good(hip_ops)
    both(plan, 1, int(plan.items[1].dst_off) + 4)
    rc, msg = _forward(_lib, plan, src_bytes)
    assert rc == -1 and re.search(r"view 1: destination offset \d+ is not a multiple of 16", msg), msg

    plan, src_bytes = _good(hip_ops)
    both(plan, 1, int(plan.items[0].dst_off) + 16)                            # inside view 0
    rc, msg = _forward(_lib, plan, src_bytes)
    assert rc == -1 and re.search(r"view 1: destination offset \d+ overlaps what lies before it \(ends at \d+\)", msg), msg

    plan, src_bytes = _good(hip_ops)
    both(plan, 0, 0)                                                          # inside the descriptors' region
    rc, msg = _forward(_lib, plan, src_bytes)
    assert rc == -1 and re.search(r"view 0: destination offset 0 overlaps what lies before it \(ends at 240\)", msg), msg

    plan, src_bytes = _good(hip_ops)
    a, b = int(plan.items[1].dst_off), int(plan.items[2].dst_off)
    both(plan, 1, b); both(plan, 2, a)                                        # descending (in a buffer with room for view 1 there)
    rc, msg = _forward(_lib, plan, src_bytes, packed_bytes=plan.prep.packed_bytes + 4096)
    assert rc == -1 and re.search(r"view 2: destination offset \d+ overlaps what lies before it", msg), msg

    plan, src_bytes = _good(hip_ops)
    rc, msg = _forward(_lib, plan, src_bytes, packed_bytes=plan.prep.packed_bytes - 16)
    assert rc == -1 and re.search(r"view 2: destination range \[\d+, \+75\) ends past the packed buffer's \d+ bytes", msg), msg


def test_forward_refuses_buffers(ops):
    _lib, hip_ops = ops
    plan, src_bytes = _good(hip_ops)
    rc, msg = _forward(_lib, plan, src_bytes, src=SRC + 8)
    assert rc == -1 and "must be 16-byte aligned" in msg
    rc, msg = _forward(_lib, plan, src_bytes, packed=PACKED + 4)
    assert rc == -1 and "must be 16-byte aligned" in msg
    for packed in (SRC, SRC + src_bytes - 16, SRC - plan.prep.packed_bytes + 16):
        rc, msg = _forward(_lib, plan, src_bytes, packed=packed)
        assert rc == -1 and "the source buffer and the packed buffer overlap" in msg, (hex(packed), msg)
    rc, msg = _forward(_lib, plan, src_bytes, n=-2)
    assert rc == -1 and "n = -2 is negative" in msg
    rc, msg = _forward(_lib, plan, src_bytes, src=0)
    assert rc == -1 and "null argument" in msg
    rc, msg = _forward(_lib, plan, src_bytes, n=65536)
    assert rc == -1 and "at most 65535 views per call" in msg


def test_wrappers_validate_their_arguments(ops):
    import torch
    _lib, hip_ops = ops
    plan, src_bytes = _good(hip_ops)
    with pytest.raises(_lib.PigeonHipError, match="expected a device tensor"):
        hip_ops.equirect_forward(torch.zeros(src_bytes, dtype=torch.uint8), plan)
    with pytest.raises(_lib.PigeonHipError, match="9 entries"):
        hip_ops.equirect_plan([(32, 64, 0, 24, (1.0, 0.0), 0.1)], [0])
    with pytest.raises(_lib.PigeonHipError, match="negative"):
        hip_ops.equirect_plan([(32, 64, 0, 24, IDENT, 0.1)], [-16])


# ---- the Python side's angles -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("yaw,pitch", [(0, 0), (90, 0), (180, 0), (270, 0), (37.5, -20), (0, 90), (-45, 30), (123.4, -90)])
def test_view_rotation_is_the_contract_matrix(yaw, pitch):
    from pigeon_amd import panorama
    R = panorama.view_rotation(yaw, pitch)
    C_, Sn, c, s = math.cos(math.radians(yaw)), math.sin(math.radians(yaw)), math.cos(math.radians(pitch)), math.sin(math.radians(pitch))
    want = np.array([[C_, Sn * s, Sn * c], [0.0, c, -s], [-Sn, C_ * s, C_ * c]])
    assert R.dtype == np.float64 and R.shape == (3, 3)
    assert np.abs(R - want).max() <= 4e-16                                    # (libm against numpy: an ulp of a value below 1)
    assert np.array_equal(R, E.view_rotation(yaw, pitch))                     # the restatement's: the same bits
    # Ry(yaw) . Rx(pitch) composed from the two steps of the contract: y2 = y c - z s, z2 = y s + z c; x3 = x C + z2 Sn, z3 = -x Sn + z2 C
    for vec in np.eye(3):
        x, y, z = vec
        y2, z2 = y * c - z * s, y * s + z * c
        assert np.allclose(R @ vec, [x * C_ + z2 * Sn, y2, -x * Sn + z2 * C_], atol=1e-15)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15)


def test_view_directions():
    """Yaw positive to the right, pitch positive upwards, y down: the centre ray of (yaw 90) lands a quarter of the width to the right
    of the centre column, the centre ray of (pitch 30) above the centre row."""
    from pigeon_amd import panorama
    fwd = np.array([0.0, 0.0, 1.0])
    wx, wy, wz = panorama.view_rotation(90, 0) @ fwd
    assert math.isclose(math.atan2(wx, wz), math.pi / 2)
    wx, wy, wz = panorama.view_rotation(0, 30) @ fwd
    assert math.isclose(math.atan2(-wy, math.hypot(wx, wz)), math.radians(30))


def test_default_view_size_and_focal():
    from pigeon_amd import panorama
    assert panorama.default_view_size(4096) == 1304 == round(4096 / math.pi)
    assert panorama.default_view_size(2048) == 652
    assert panorama.default_view_size(64) == 336 and panorama.default_view_size(1) == 336          # clamped below
    assert panorama.default_view_size(1055) == 336 and panorama.default_view_size(1058) == 337
    assert panorama.default_view_size(16384) == 4096 and panorama.default_view_size(12868) == 4096  # clamped above
    assert panorama.default_view_size(12866) == 4095
    assert panorama.inv_focal(90.0, 336) == E.inv_focal(90.0, 336) == float(np.tan(np.deg2rad(90.0) / 2) / 168.0)
    for bad in (0.0, 180.0, -10.0):
        with pytest.raises(ValueError, match="fov"):
            panorama.inv_focal(bad, 336)
    views = panorama.view_list([(32, 64), (17, 33)], centre_heading=[10.0, 90.0], size=24)
    assert len(views) == 8 and [v[2] for v in views] == [0, 0, 0, 0, 1, 1, 1, 1]
    assert np.array_equal(views[0][4], panorama.view_rotation(-10.0, 0.0)) and np.array_equal(views[5][4], panorama.view_rotation(0.0, 0.0))


def test_kernel_has_no_scratch_and_reads_its_descriptor_uniformly(hip_lib):
    """The view is blockIdx.y: the ISA of the built library shows no scratch and no readfirstlane loop around the descriptor
    (tools/asm_audit.py, as tests/test_asm_audit.py)."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import asm_audit
    res = {k: v for k, v in asm_audit.audit(os.path.join(root, "pigeon_amd", "libpigeon_hip.so")).items() if "equirect" in k}
    assert len(res) == 1, list(res)
    for name, v in res.items():
        assert v["scratch"] == 0 and v["waterfall"] == 0 and 0 < v["vgpr"] <= 128, (name, v)


def test_serve_parses_a_panorama_request_without_a_gpu():
    import base64
    import io
    from PIL import Image
    from pigeon_amd import serve
    buf = io.BytesIO()
    Image.fromarray(E.random_source(8, 16, 3)).save(buf, "PNG")
    uri = "data:image/png;base64," + base64.b64encode(buf.getvalue()).decode()
    req = serve.panorama_from_request({"panorama": uri})
    assert isinstance(req, serve.EquirectRequest) and req.centre_heading == 0.0 and req.image.size == (16, 8)
    req = serve.panorama_from_request({"panorama": uri, "panorama_heading": 123}, encoded=True)
    assert req.centre_heading == 123.0 and req.image == buf.getvalue()
    for key in serve.IMAGE_KEYS:
        with pytest.raises(serve.BadRequest, match="cannot be combined"):
            serve.panorama_from_request({"panorama": uri, key: uri})
    for bad in ("north", None, True, float("nan"), float("inf")):
        with pytest.raises(serve.BadRequest, match="panorama_heading"):
            serve.panorama_from_request({"panorama": uri, "panorama_heading": bad})
    with pytest.raises(serve.BadRequest, match="non-empty data URI"):
        serve.panorama_from_request({"panorama": ""})
    with pytest.raises(serve.BadRequest, match="injected"):                     # the views exist on the device only
        serve.predict_panorama(req, model=None, preprocess=lambda views: None)
    assert len(serve.panorama_from_request({"image": uri})) == 4                # the four-view request is as it was


def test_run_py_refuses_equirect_without_raw_images(monkeypatch):
    import importlib
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import run
    importlib.reload(run)
    for argv in (["evaluate", "none", "--synthetic", "2", "--equirect"], ["embed", "random", "--synthetic", "2", "--raw-images", "--equirect"]):
        with pytest.raises(SystemExit, match="--equirect is a mode of evaluate --raw-images"):
            run._dispatch(run.argp.parse_args(argv), comm=None)
