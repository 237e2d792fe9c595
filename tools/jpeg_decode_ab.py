"""JPEG decode A/B: the host stage (pg_jpeg_entropy_decode) against Pillow's full decode, and -- with --gpu -- the two kernels, the whole
`gpu_preprocess(EncodedImages)` route, a serving request and `embed_images` on files, against their Pillow routes.

  python tools/jpeg_decode_ab.py                      # CPU part: no GPU needed
  python tools/jpeg_decode_ab.py --gpu [--embed 2048] [--layers 24]

Prints one JSON object.  The test file is a 640 x 640 quality-90 4:2:0 photo-like image (smooth shapes plus texture, about 170 KB)."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def photo_like(h, w, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([127 + 100 * np.sin(x / 37.0 + seed) * np.cos(y / 53.0), 127 + 90 * np.sin((x + y) / 71.0), 127 + 110 * np.cos(y / 29.0 - x / 97.0)], -1)
    tex = rng.normal(0, 1, (h // 2 + 1, w // 2 + 1, 3)).repeat(2, 0).repeat(2, 1)[:h, :w] * 14 + rng.normal(0, 9, (h, w, 3))
    return np.clip(base + tex, 0, 255).astype(np.uint8)


def jpeg_file(arr, quality=90, subsampling=2):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, "JPEG", quality=quality, subsampling=subsampling)
    return buf.getvalue()


def pillow_decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def mean_ms(fn, reps):
    fn()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t) / reps * 1e3


def cpu_part(files, reps):
    from pigeon_amd import hip_ops
    one = files[0]
    plan1 = hip_ops.jpeg_plan([hip_ops.jpeg_probe(one)])
    coef1 = torch.empty(plan1.coef_bytes, dtype=torch.uint8)
    out = {"file_bytes": len(one), "pillow_full_decode_ms": mean_ms(lambda: pillow_decode(one), reps),
           "host_stage_probe_plan_decode_ms": mean_ms(lambda: hip_ops.jpeg_entropy_decode(
               [one], hip_ops.jpeg_plan([hip_ops.jpeg_probe(one)]), coef1, threads=1), reps),
           "host_stage_decode_only_ms": mean_ms(lambda: hip_ops.jpeg_entropy_decode([one], plan1, coef1, threads=1), reps)}
    plan = hip_ops.jpeg_plan([hip_ops.jpeg_probe(f) for f in files])
    coef = torch.empty(plan.coef_bytes, dtype=torch.uint8)
    for th in (1, min(16, len(os.sched_getaffinity(0)))):
        ms = mean_ms(lambda: hip_ops.jpeg_entropy_decode(files, plan, coef, threads=th), 3)
        out[f"host_stage_{len(files)}_images_{th}_threads_ms"] = ms
        out[f"host_stage_{th}_threads_images_per_s"] = len(files) / ms * 1e3
    out["cpus_available"] = len(os.sched_getaffinity(0))
    return out, plan, coef


def event_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def gpu_part(files, plan, coef, args):
    from pigeon_amd import hip_ops, jpeg
    from pigeon_amd.clip_embedder import EncodedImages, gpu_preprocess, pack_images
    dev = "cuda"
    n = len(files)
    coef_dev = coef.to(dev)
    packed = torch.empty(plan.prep.packed_bytes, dtype=torch.uint8, device=dev)
    ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=dev)
    out = {"images": n}
    out["jpeg_forward_two_kernels_ms"] = event_ms(lambda: hip_ops.jpeg_forward(coef_dev, plan, packed, ws), 10)
    blocks = sum(it.bw[c] * it.bh[c] for it in plan.items for c in range(it.ncomp))
    rgb = sum(it.height * it.width * 3 for it in plan.items)
    out["bytes_moved_MB"] = {"coefficients_read": blocks * 128 / 1e6, "planes_written": blocks * 64 / 1e6, "planes_read_at_least": blocks * 64 / 1e6,
                             "rgb_written": rgb / 1e6}
    out["effective_GB_per_s"] = (blocks * 256 + rgb) / 1e9 / (out["jpeg_forward_two_kernels_ms"] / 1e3)
    prep = hip_ops.RaggedPreprocessor(0)
    out["ragged_resize_u8_ms"] = event_ms(lambda: prep.forward(packed, plan.prep, torch.uint8, header_written=True), 10)
    want = [pillow_decode(f) for f in files[:8]]
    dec = jpeg.DecodedImages(packed, plan.prep, [])
    out["first_8_equal_pillow"] = all(np.array_equal(dec.image(i).cpu().numpy(), want[i]) for i in range(8))
    # whole routes, wall time with the host work in it
    enc = EncodedImages(files)

    def route_files():
        gpu_preprocess(enc, dev, torch.uint8)
        torch.cuda.synchronize()

    def route_pillow():
        gpu_preprocess(pack_images([pillow_decode(f) for f in files]), dev, torch.uint8)
        torch.cuda.synchronize()

    out["route_files_to_pixel_bytes_ms"] = mean_ms(route_files, 3)
    out["route_pillow_pack_to_pixel_bytes_ms"] = mean_ms(route_pillow, 2)
    # one serving request, four 640 x 640 payloads
    from pigeon_amd import serve, synthetic
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    from pigeon_amd.super_guessr import SuperGuessr
    import tempfile
    gp = os.path.join(tempfile.mkdtemp(prefix="jpeg_ab_"), "g.csv")
    synthetic.write_geocell_csv(gp, synthetic.make_geocells(1000, seed=0))
    model = SuperGuessr(HipCLIPVisionModel(seed=0, layers=args.layers), panorama=True, serving=True, freeze_base=True, geocell_path=gp).to(dev).eval()
    import base64
    uris = ["data:image/jpeg;base64," + base64.b64encode(f).decode() for f in files[:4]]
    body = dict(zip(serve.IMAGE_KEYS, uris))

    def request(encoded):
        res = serve.predict_panorama(serve.panorama_from_request(body, encoded), model)
        torch.cuda.synchronize()
        return res

    a, b = request(False), request(True)
    out["serving_same_answer"] = a == b
    out["serving_request_pillow_ms"] = mean_ms(lambda: request(False), 20)
    out["serving_request_encoded_ms"] = mean_ms(lambda: request(True), 20)
    if args.embed:
        from pigeon_amd.clip_embedder import CLIPEmbedding
        from pigeon_amd.embed import embed_images
        sizes = [(640, 640), (480, 640), (600, 800), (512, 384)]
        distinct = [jpeg_file(photo_like(*sizes[k % 4], seed=100 + k), subsampling=(2, 2, 1, 0)[k % 4]) for k in range(32)]

        class Files:
            def __init__(self, decoded):
                self.decoded = decoded

            def __len__(self):
                return args.embed

            def __getitem__(self, i):
                from PIL import Image
                f = distinct[i % len(distinct)]
                return {"image": Image.open(io.BytesIO(f)) if self.decoded else {"bytes": f, "path": None}, "index": i}

        emb = CLIPEmbedding("random", device=dev, clip_model=HipCLIPVisionModel(seed=0, layers=args.layers), contract_guard="off")
        for tag, kw, ds in (("raw_images", {}, Files(True)), ("raw_images_encoded", {"encoded": True}, Files(False))):
            t = time.perf_counter()
            embed_images(emb, {"train": ds}, batch_size=512, num_workers=8, out_dir=tempfile.mkdtemp(prefix="jpeg_ab_"), raw_images=True, **kw)
            out[f"embed_images_{tag}_images_per_s"] = args.embed / (time.perf_counter() - t)
        out["embed_images"] = {"images": args.embed, "workers": 8, "batch": 512, "layers": args.layers, "mean_file_bytes": int(np.mean([len(f) for f in distinct]))}
        out["fallbacks"] = jpeg.fallback_summary()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--gpu", action="store_true")
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--embed", type=int, default=0, help="also time embed_images on this many files, decoded by the workers / on the GPU")
    ap.add_argument("--layers", type=int, default=24)
    args = ap.parse_args()
    distinct = [jpeg_file(photo_like(640, 640, seed=s)) for s in range(8)]
    files = [distinct[i % len(distinct)] for i in range(args.images)]
    res, plan, coef = cpu_part(files, args.reps)
    if args.gpu:
        res["gpu"] = gpu_part(files, plan, coef, args)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
