"""GPU side of the equirectangular views (pg_equirect_forward, pigeon_amd/csrc/equirect.hip) against the numpy restatement
(tests/_equirectref.py, itself checked in tests/test_equirectref_cpu.py) under its comparator: tight pixels equal, loose ones within
one step of a / b, pole pixels left out.  Sources are seeded random bytes and an image whose channels encode column and row.  Every
run is made into buffers filled with a pattern and surrounded by guard regions, which must keep it."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _equirectref as E  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0xA5
GUARD = 4096
_SOURCES = {}


def _source(kind, H, W):
    """One array per (kind, size) for the whole module: computed once, never written."""
    key = (kind, H, W)
    if key not in _SOURCES:
        a = E.random_source(H, W, 1000 + H * 7 + W) if kind == "random" else E.location_source(H, W)
        a.setflags(write=False)
        _SOURCES[key] = a
    return _SOURCES[key]


@pytest.fixture(scope="module")
def ops():
    from pigeon_amd import _lib, hip_ops
    _lib.require_gpu()
    return hip_ops


def _layout(ops, sources):
    from pigeon_amd.packing import packed_layout
    return packed_layout([s.shape[:2] for s in sources])


def _run(ops, sources, views, damage=None):
    """`views`: [(source index, S, rot, inv_f)].  The sources lie as a packed buffer has them, between two guard regions; the views go
    into a pattern-filled buffer with a guard region behind it.  Returns (plan, the packed allocation as numpy); asserts that the
    source allocation is unchanged, the head holds the resize's descriptors and nothing but the views was written."""
    offs, total = _layout(ops, sources)
    src_host = np.full(GUARD + total + GUARD, SENTINEL, dtype=np.uint8)
    for s, o in zip(sources, offs):
        src_host[GUARD + o:GUARD + o + s.size] = s.reshape(-1)
    src_all = torch.from_numpy(src_host).to(DEV)
    plan = ops.equirect_plan([(sources[k].shape[0], sources[k].shape[1], k, S, rot, f) for k, S, rot, f in views], offs)
    whole = torch.full((plan.prep.packed_bytes + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    if damage is not None:
        damage(plan)
    ops.equirect_forward(src_all[GUARD:GUARD + total], plan, whole[:plan.prep.packed_bytes])
    torch.cuda.synchronize()
    got = whole.cpu().numpy()
    assert np.array_equal(src_all.cpu().numpy(), src_host), "the source buffer or its guard regions were written"
    touched = np.zeros(got.size, dtype=bool)
    touched[:plan.prep.header_bytes] = True
    for it in plan.items:
        touched[int(it.dst_off):int(it.dst_off) + it.size * it.size * 3] = True
    assert bytes(got[:plan.prep.header_bytes]) == bytes(plan.prep.header()), "the resize's descriptors are not in the buffer's head"
    assert (got[~touched] == SENTINEL).all(), "bytes between the views or behind the buffer were written"
    return plan, got


def _view(plan, got, i):
    S, off = plan.items[i].size, int(plan.items[i].dst_off)
    return got[off:off + S * S * 3].reshape(S, S, 3)


@pytest.mark.parametrize("kind", ["random", "location"])
@pytest.mark.parametrize("case", E.CASES, ids=[c[0] for c in E.CASES])
def test_every_case_alone_against_the_restatement(ops, case, kind):
    H, W, S, rot, inv_f = E.case_params(case)
    src = _source(kind, H, W)
    plan, got = _run(ops, [src], [(0, S, rot, inv_f)])
    E.compare(_view(plan, got, 0), src, S, rot, inv_f, view=0)


# eight views of mixed sizes out of three panoramas, in an order that is not by source: (case name, source kind)
BATCH = [("32x64_s24_seam", "random"), ("1x1_s1", "random"), ("64x128_s41_up", "location"), ("17x33_s21", "random"),
         ("32x64_s24_y90", "random"), ("1x2_s2", "random"), ("64x128_s41_down", "location"), ("32x64_s24_y270_fov120", "random")]


def test_a_view_alone_equals_the_view_inside_a_ragged_batch(ops):
    cases = {c[0]: c for c in E.CASES}
    sources, index, views = [], {}, []
    for name, kind in BATCH:
        H, W, S, rot, inv_f = E.case_params(cases[name])
        key = (kind, H, W)
        if key not in index:
            index[key] = len(sources)
            sources.append(_source(kind, H, W))
        views.append((index[key], S, rot, inv_f))
    assert len(views) == 8 and len({v[1] for v in views}) >= 5
    plan, got = _run(ops, sources, views)
    for i, (k, S, rot, inv_f) in enumerate(views):
        inside = _view(plan, got, i)
        E.compare(inside, sources[k], S, rot, inv_f, view=i)
        alone_plan, alone = _run(ops, [sources[k]], [(0, S, rot, inv_f)])
        assert torch.equal(torch.from_numpy(_view(alone_plan, alone, 0).copy()), torch.from_numpy(inside.copy())), f"view {i} ({BATCH[i][0]})"


def test_four_views_of_one_panorama_share_its_bytes(ops):
    """One panorama, four headings (what the product renders): every view against the restatement, in one launch."""
    src = _source("random", 32, 64)
    views = [(0, 24, E.view_rotation(h, 0.0), E.inv_focal(90.0, 24)) for h in (0.0, 90.0, 180.0, 270.0)]
    plan, got = _run(ops, [src], views)
    assert len({int(it.src_off) for it in plan.items}) == 1
    for i, (_, S, rot, f) in enumerate(views):
        E.compare(_view(plan, got, i), src, S, rot, f, view=i)


def test_views_through_the_resize_equal_the_same_views_as_ordinary_images(ops):
    from pigeon_amd import panorama
    from pigeon_amd.preprocess import gpu_preprocess
    src = _source("random", 64, 128)
    dec = panorama.equirect_views(np.array(src), size=41, device=DEV)
    assert len(dec) == 4 and dec.plan.sizes == [(41, 41)] * 4
    views = [dec.image(i).cpu().numpy().copy() for i in range(4)]
    for i, h in enumerate(panorama.HEADINGS):
        E.compare(views[i], src, 41, E.view_rotation(h, 0.0), E.inv_focal(90.0, 41), view=i)
    for dt in (torch.float32, torch.uint8):
        a = gpu_preprocess(dec, DEV, dt)
        b = gpu_preprocess(views, DEV, dt)
        assert a.shape == (4, 3, 336, 336) and torch.equal(a, b)
    # the default size: round(W / pi) clamped to 336
    dec = panorama.equirect_views([np.array(src)], device=DEV)
    assert dec.plan.sizes == [(336, 336)] * 4
    E.compare(dec.image(2).cpu().numpy(), src, 336, E.view_rotation(180.0, 0.0), E.inv_focal(90.0, 336), view=2)


def test_python_front_end_chunks_and_takes_every_input_kind(ops):
    """Arrays, a PackedImages and PIL images give the same views; the chunked generator gives the same bytes as one run."""
    from PIL import Image
    from pigeon_amd import panorama
    from pigeon_amd.packing import pack_images
    a, b = np.array(_source("random", 32, 64)), np.array(_source("location", 17, 33))
    whole = panorama.equirect_views([a, b], size=24, centre_heading=[0.0, 30.0], device=DEV)
    want = [whole.image(i).cpu().numpy().copy() for i in range(8)]
    E.compare(want[5], b, 24, E.view_rotation(90.0 - 30.0, 0.0), E.inv_focal(90.0, 24), view=5)
    for other in (pack_images([a, b]), [Image.fromarray(a), Image.fromarray(b)]):
        dec = panorama.equirect_views(other, size=24, centre_heading=[0.0, 30.0], device=DEV)
        assert all(np.array_equal(dec.image(i).cpu().numpy(), want[i]) for i in range(8))
    chunks = list(panorama.equirect_view_chunks([a, b], size=24, centre_heading=[0.0, 30.0], device=DEV, max_bytes=3 * (24 * 24 * 3 + 80)))
    assert len(chunks) >= 3 and sum(len(c) for c in chunks) == 8
    flat = [c.image(i).cpu().numpy() for c in chunks for i in range(len(c))]
    assert all(np.array_equal(x, y) for x, y in zip(flat, want))
    pix = panorama.panorama_pixels([a, b], device=DEV, out_dtype=torch.uint8, size=24, centre_heading=[0.0, 30.0])
    assert pix.shape == (8, 3, 336, 336) and pix.view(2, 12, 336, 336).shape == (2, 12, 336, 336)


REFUSALS = {
    "view_size": (lambda p: setattr(p.items[1], "size", 4097), "view 1: view size 4097 out of range"),
    "source_size": (lambda p: setattr(p.items[1], "src_w", 16385), "view 1: source size"),
    "rot": (lambda p: p.items[1].rot.__setitem__(0, float("nan")), r"view 1: rot\[0\] is not finite"),
    "inv_f": (lambda p: setattr(p.items[1], "inv_f", 0.0), "view 1: inv_f = 0 is not finite and positive"),
    "reserved": (lambda p: p.items[1].reserved.__setitem__(0, 9), "view 1: a reserved field is not zero"),
    "source_alignment": (lambda p: setattr(p.items[1], "src_off", p.items[1].src_off + 4), "view 1: source offset .* multiple of 16"),
    "source_range": (lambda p: setattr(p.items[1], "src_h", 33), "view 1: source range .* ends past the source buffer"),
    "destination_differs": (lambda p: setattr(p.items[1], "dst_off", p.items[1].dst_off + 16), "view 1: size or offset differs"),
    "destination_overlap": (lambda p: [setattr(p.items[1], "dst_off", p.items[0].dst_off), setattr(p.prep.items[1], "src_off", p.items[0].dst_off)],
                            "view 1: destination offset .* overlaps"),
    "destination_range": (lambda p: [setattr(p.items[1], "dst_off", 1 << 30), setattr(p.prep.items[1], "src_off", 1 << 30)],
                          "view 1: destination range .* ends past the packed buffer"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_a_refusal_leaves_the_output_untouched(ops, name):
    from pigeon_amd import _lib
    damage, message = REFUSALS[name]
    src = _source("random", 32, 64)
    rot, f = E.view_rotation(0.0, 0.0), E.inv_focal(90.0, 24)
    offs, total = _layout(ops, [src])
    src_dev = torch.full((total,), SENTINEL, dtype=torch.uint8, device=DEV)
    plan = ops.equirect_plan([(32, 64, 0, 24, rot, f)] * 2, offs)
    whole = torch.full((plan.prep.packed_bytes + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    damage(plan)
    with pytest.raises(_lib.PigeonHipError, match="equirect_forward: " + message):
        ops.equirect_forward(src_dev, plan, whole[:plan.prep.packed_bytes])
    torch.cuda.synchronize()
    assert (whole.cpu().numpy() == SENTINEL).all(), "a refused call wrote to the packed buffer"


def test_overlapping_buffers_are_refused_and_n_zero_is_a_no_op(ops):
    from pigeon_amd import _lib
    src = _source("random", 32, 64)
    offs, total = _layout(ops, [src])
    plan = ops.equirect_plan([(32, 64, 0, 24, E.view_rotation(0.0, 0.0), E.inv_focal(90.0, 24))], offs)
    both = torch.full((total + plan.prep.packed_bytes,), SENTINEL, dtype=torch.uint8, device=DEV)
    with pytest.raises(_lib.PigeonHipError, match="the source buffer and the packed buffer overlap"):
        ops.equirect_forward(both[:total], plan, both[total - 16:total - 16 + plan.prep.packed_bytes])
    torch.cuda.synchronize()
    assert (both.cpu().numpy() == SENTINEL).all()
    empty = ops.equirect_plan([], [])
    out = ops.equirect_forward(both[:total], empty, torch.empty(0, dtype=torch.uint8, device=DEV))
    assert out.numel() == 0 and (both.cpu().numpy() == SENTINEL).all()
