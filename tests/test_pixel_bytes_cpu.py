"""8-bit pixels, host side (no GPU): the one normalisation table against the numpy statement of it, the ctypes table, the refusals
that must name `pixel_bytes` before anything crosses the ABI (host tensors, a model that never reaches a device), and the
image-column evaluation dataset with its collate function."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 336


def test_norm_lut_equals_the_numpy_statement_bit_for_bit(hip_lib):
    from oracle.clip_preprocess_oracle import normalise_lut
    out = (C.c_float * 768)()
    assert hip_lib.pg_prep_norm_lut(out) == 0
    got = np.frombuffer(out, dtype=np.float32).reshape(3, 256)
    want = normalise_lut()
    assert want.dtype == np.float32 and want.shape == (3, 256)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))            # all 768 entries, as bits
    assert hip_lib.pg_prep_norm_lut(None) == -1 and b"null" in hip_lib.pg_last_error()
    from pigeon_amd import hip_ops
    assert np.array_equal(hip_ops.norm_lut().numpy().view(np.uint32), want.view(np.uint32))


def test_ctypes_table_and_header_cover_the_new_symbol(hip_lib):
    from pigeon_amd import _lib
    header = open(os.path.join(ROOT, "include", "pigeon_hip.h")).read()
    assert re.search(r"\bint\s+pg_prep_norm_lut\s*\(\s*float\s+out\[768\]\s*\)\s*;", header)
    assert re.search(r"#define\s+PG_DTYPE_U8\s+4\b", header) and _lib.PG_DTYPE_U8 == 4
    assert re.search(r"#define\s+PG_ABI_VERSION\s+7\b", header) and hip_lib.pg_abi_version() == 7
    res, args = _lib.SIGNATURES["pg_prep_norm_lut"]
    assert res is C.c_int and len(args) == 1
    assert hip_lib.pg_prep_norm_lut.argtypes == args


def _bad_inputs():
    ok = torch.zeros((2, 12, S, S), dtype=torch.uint8)
    return {
        "another shape": torch.zeros((2, 4, S, S), dtype=torch.uint8),
        "three dims": torch.zeros((12, S, S), dtype=torch.uint8),
        "HWC": torch.zeros((2, S, S, 3), dtype=torch.uint8),
        "another size": torch.zeros((2, 3, 224, 224), dtype=torch.uint8),
        "not contiguous": torch.zeros((2, 12, S, 2 * S), dtype=torch.uint8)[..., ::2],
        "floats": ok.float(),
    }


@pytest.fixture(scope="module")
def stub(tmp_path_factory):
    """A tower without weights and a panorama model around it, both on the host: any call that got as far as the encoder would fail
    for want of a device, so a ValueError that names the argument was raised before."""
    from pigeon_amd import synthetic as syn
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    from pigeon_amd.super_guessr import SuperGuessr
    gp = os.path.join(str(tmp_path_factory.mktemp("pb")), "g.csv")
    syn.write_geocell_csv(gp, syn.make_geocells(16, seed=0))
    vit = HipCLIPVisionModel(state_dict={})
    model = SuperGuessr(vit, panorama=True, freeze_base=True, num_candidates=5, geocell_path=gp, exact_top1=True, margin_autocalibrate=False)
    return vit, model.eval()


def test_check_pixel_bytes_accepts_the_two_shapes():
    from pigeon_amd.clip_embedder import check_pixel_bytes
    for views in (3, 12):
        t = torch.zeros((2, views, S, S), dtype=torch.uint8)
        assert check_pixel_bytes(t) is t
    assert check_pixel_bytes(torch.zeros((0, 12, S, S), dtype=torch.uint8)).shape[0] == 0


@pytest.mark.parametrize("what", sorted(_bad_inputs()))
def test_refusals_name_the_argument(stub, what):
    from pigeon_amd.deferred import DeferredExact
    from pigeon_amd.evaluate import certain_forward
    vit, model = stub
    bad = _bad_inputs()[what]
    calls = [lambda: vit.embed(pixel_bytes=bad), lambda: vit.embed_precise(pixel_bytes=bad), lambda: vit.hidden(pixel_bytes=bad),
             lambda: model(pixel_bytes=bad), lambda: model.encode_head(pixel_bytes=bad), lambda: certain_forward(model, None, pixel_bytes=bad),
             lambda: DeferredExact(model, None).submit(pixel_bytes=bad)]
    for call in calls:
        with pytest.raises(ValueError, match="pixel_bytes"):
            call()
    if what == "HWC":
        with pytest.raises(ValueError, match="HWC"):
            vit.embed(pixel_bytes=bad)
    if what == "not contiguous":
        with pytest.raises(ValueError, match="contiguous"):
            vit.embed(pixel_bytes=bad)


def test_pixel_bytes_stands_alone_and_fits_the_model(stub):
    from pigeon_amd.deferred import DeferredExact
    from pigeon_amd.evaluate import PanoramaPipeline, certain_forward
    vit, model = stub
    good = torch.zeros((2, 12, S, S), dtype=torch.uint8)
    px, emb = torch.zeros((2, 12, S, S)), torch.zeros((2, 4, 1024))
    for call in (lambda: vit.embed(pixel_values=px, pixel_bytes=good), lambda: vit.embed_precise(pixel_values=px, pixel_bytes=good),
                 lambda: vit.hidden(pixel_values=px, pixel_bytes=good), lambda: model(pixel_values=px, pixel_bytes=good),
                 lambda: model(embedding=emb, pixel_bytes=good), lambda: model.encode_head(px, None, pixel_bytes=good),
                 lambda: model.encode_head(None, emb, pixel_bytes=good), lambda: certain_forward(model, None, pixel_values=px, pixel_bytes=good),
                 lambda: certain_forward(model, None, embedding=emb, pixel_bytes=good),
                 lambda: DeferredExact(model, None).submit(px, pixel_bytes=good), lambda: DeferredExact(model, None).submit(None, emb, pixel_bytes=good)):
        with pytest.raises(ValueError, match="pixel_bytes cannot be given together with"):
            call()
    # a panorama model takes four views per sample
    with pytest.raises(ValueError, match=r"pixel_bytes must be \(B,12,336,336\)"):
        model(pixel_bytes=torch.zeros((2, 3, S, S), dtype=torch.uint8))
    # the data-parallel step hands the keyword on
    pipe = PanoramaPipeline.__new__(PanoramaPipeline)
    pipe.model, pipe.refiner, pipe.engine, pipe.last_info = model, None, DeferredExact(model, None), None
    with pytest.raises(ValueError, match="pixel_bytes"):
        pipe.step(pixel_bytes=torch.zeros((2, S, S, 12), dtype=torch.uint8))


def _samples(n=6):
    rng = np.random.default_rng(7)
    sizes = [(S, S), (340, 400), (400, 350), (350, 500), (337, 336)]
    out = []
    for i in range(n):
        item = {"labels": torch.tensor([10.0 + i, -3.0 * i], dtype=torch.float64), "labels_clf": torch.tensor(i % 5)}
        for v, key in enumerate(("image", "image_2", "image_3", "image_4")):
            h, w = sizes[(i + v) % len(sizes)]
            item[key] = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        out.append(item)
    return out


def test_image_eval_dataset_packs_views_and_passes_labels_through():
    from pigeon_amd.evaluate import ImageEvalDataset
    from pigeon_amd.packing import PackedImages
    samples = _samples(6)
    ds = ImageEvalDataset(samples)
    assert len(ds) == 6
    one = ds[2]
    assert set(one) == {"labels", "labels_clf", "images"} and isinstance(one["images"], PackedImages) and len(one["images"]) == 4
    batch = ImageEvalDataset.collate([ds[i] for i in range(6)])
    packed = batch["images"]
    assert isinstance(packed, PackedImages) and len(packed) == 24 and batch["views"] == 4
    k = 0
    for s in samples:
        for key in ("image", "image_2", "image_3", "image_4"):
            assert tuple(packed.sizes[k].tolist()) == s[key].shape[:2]
            assert np.array_equal(packed.image(k), s[key]), (k, key)
            k += 1
    assert torch.equal(batch["labels"], torch.stack([s["labels"] for s in samples])) and batch["labels"].dtype == torch.float64
    assert torch.equal(batch["labels_clf"], torch.stack([s["labels_clf"] for s in samples]))
    # the packed buffer is the one the ragged plan expects for these sizes
    from pigeon_amd import hip_ops
    plan = hip_ops.ragged_plan(packed.size_list())
    assert packed.data.numel() == plan.packed_bytes and not packed.data[:plan.header_bytes].any()
    # through a DataLoader, in two batches, PIL images and single-view items as well
    from torch.utils.data import DataLoader
    got = list(DataLoader(ds, 4, shuffle=False, collate_fn=ImageEvalDataset.collate))
    assert [len(b["images"]) for b in got] == [16, 8] and np.array_equal(got[1]["images"].image(0), samples[4]["image"])
    Image = pytest.importorskip("PIL.Image")
    single = ImageEvalDataset([{"image": Image.fromarray(s["image"]), "labels_clf": s["labels_clf"]} for s in samples[:3]])
    b = ImageEvalDataset.collate([single[i] for i in range(3)])
    assert b["views"] == 1 and len(b["images"]) == 3 and np.array_equal(b["images"].image(1), samples[1]["image"])


def test_image_eval_dataset_column_access_and_mixed_view_counts():
    from pigeon_amd.evaluate import ImageEvalDataset

    class Columns(list):
        def __getitem__(self, i):
            if isinstance(i, str):
                return np.stack([np.asarray(s[i]) for s in self])
            return list.__getitem__(self, i)

    samples = _samples(3)
    ds = ImageEvalDataset(Columns(samples))
    assert np.array_equal(ds["labels"], np.stack([s["labels"].numpy() for s in samples]))
    assert np.array_equal(ds["labels_clf"], np.stack([s["labels_clf"].numpy() for s in samples]))
    mixed = [ds[0], ImageEvalDataset([{"image": samples[1]["image"], "labels_clf": samples[1]["labels_clf"], "labels": samples[1]["labels"]}])[0]]
    with pytest.raises(ValueError, match="views"):
        ImageEvalDataset.collate(mixed)
    with pytest.raises(KeyError, match="image"):
        ImageEvalDataset([{"labels": 1}])[0]
