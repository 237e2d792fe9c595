"""A/B of the ragged-batch CLIP preprocessing (pg_prep_ragged_forward) against the per-size path (pg_prep_forward, one handle, copy
and launch pair per distinct size), from host arrays to pixels on the device, and of `embed_images(raw_images=True)` against the
host preprocessing path.  Arms alternate after a warm-up; every time is a host clock around work that ends in a device synchronise.

   python tools/prep_ragged_ab.py                      # (a) mixed list, (b) uniform list, (c) embed_images end to end
   python tools/prep_ragged_ab.py --only a --reps 3    # what a `rocprofv3 --kernel-trace --stats` run of (a) executes
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pigeon_amd import clip_embedder as ce, hip_ops  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--only", default="abc")
ap.add_argument("--n", type=int, default=512)
ap.add_argument("--sizes", type=int, default=128)
ap.add_argument("--reps", type=int, default=8)
ap.add_argument("--embed-n", type=int, default=4096)
ap.add_argument("--layers", type=int, default=24)
ap.add_argument("--workers", type=int, default=8)
a = ap.parse_args()
DEV = torch.device("cuda", 0)


def mixed_sizes(k, seed=7):
    """k distinct seeded (h, w): short side 240..500, long side <= 640, either orientation."""
    rng, out = np.random.default_rng(seed), []
    while len(out) < k:
        short = int(rng.integers(240, 501))
        long = int(rng.integers(short, 641))
        s = (short, long) if rng.integers(2) else (long, short)
        if s not in out:
            out.append(s)
    return out


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3, out


def ab(name, arms, reps, warm=2):
    """arms: {label: fn}; alternating after `warm` rounds.  Prints every sample, the medians and the ratio first / second."""
    ms = {k: [] for k in arms}
    for r in range(warm + reps):
        for k, fn in arms.items():
            t, _ = timed(fn)
            if r >= warm:
                ms[k].append(t)
    for k, v in ms.items():
        print(f"{name} {k}: median {statistics.median(v):.2f} ms, min {min(v):.2f}, max {max(v):.2f}  samples " + " ".join(f"{x:.1f}" for x in v))
    k0, k1 = list(arms)
    print(f"{name} {k0} / {k1} (medians): {statistics.median(ms[k0]) / statistics.median(ms[k1]):.2f}x", flush=True)


def grouped(ims):
    """The retired arm of the list path, restated: one gpu_preprocess call (pg_prep_forward) per distinct size, scattered into place."""
    by_size = {}
    for i, im in enumerate(ims):
        by_size.setdefault(im.shape, []).append(i)
    out = torch.empty((len(ims), 3, 336, 336), dtype=torch.float16, device=DEV)
    for idx in by_size.values():
        out[torch.as_tensor(idx, device=DEV)] = ce.gpu_preprocess([ims[i] for i in idx], DEV, torch.float16)
    return out


if "a" in a.only:
    sizes = mixed_sizes(a.sizes)
    rng = np.random.default_rng(1)
    arrs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in sizes]
    ims = [arrs[i % a.sizes] for i in range(a.n)]
    plan = hip_ops.ragged_plan([x.shape[:2] for x in ims])
    src = sum(x.size for x in ims)
    tmp = sum(it.nrows for it in plan.items) * 336 * 3
    outb = a.n * 3 * 336 * 336 * 2
    tab = (plan.workspace_bytes - tmp)
    print(f"(a) {a.n} images, {a.sizes} distinct sizes, fp16 out: source {src / 1e6:.1f} MB ({src / a.n / 1e3:.0f} kB/image), packed "
          f"{plan.packed_bytes / 1e6:.1f} MB, temp rows {tmp / 1e6:.1f} MB, tables {tab / 1e6:.1f} MB, output {outb / 1e6:.1f} MB")
    print(f"    kernel bytes: tables write {tab / 1e6:.1f} MB; horizontal read {src / 1e6:.1f} + write {tmp / 1e6:.1f} MB; vertical read "
          f"{tmp / 1e6:.1f} (+ taps re-read from cache) + write {outb / 1e6:.1f} MB")
    same = torch.equal(grouped(ims), ce.gpu_preprocess(ims, DEV, torch.float16))
    print(f"    ragged output equals the grouped path's bits: {same}")
    assert same
    ab("(a) mixed", {"grouped": lambda: grouped(ims), "ragged": lambda: ce.gpu_preprocess(ims, DEV, torch.float16)}, a.reps)

if "b" in a.only:
    rng = np.random.default_rng(2)
    base = [rng.integers(0, 256, (640, 640, 3), dtype=np.uint8) for _ in range(16)]
    ims = [base[i % 16] for i in range(a.n)]
    same = torch.equal(ce.gpu_preprocess(ims, DEV, torch.float16), ce.gpu_preprocess(ce.pack_images(ims), DEV, torch.float16))
    print(f"(b) {a.n} images of 640x640, fp16 out; packed path equals the per-size path's bits: {same}")
    assert same
    ab("(b) uniform", {"per-size": lambda: ce.gpu_preprocess(ims, DEV, torch.float16),
                       "packed": lambda: ce.gpu_preprocess(ce.pack_images(ims), DEV, torch.float16)}, a.reps)

if "c" in a.only:
    from PIL import Image
    from pigeon_amd.embed import embed_images
    sizes = mixed_sizes(a.sizes, seed=9)
    rng = np.random.default_rng(3)
    pil = [Image.fromarray(rng.integers(0, 256, s + (3,), dtype=np.uint8)) for s in sizes]
    emb = ce.CLIPEmbedding("random", device="cuda", clip_model=ce.HipCLIPVisionModel(seed=0, layers=a.layers), contract_guard="off")
    moved = []
    emb.register_forward_pre_hook(lambda m, args: moved.append(args[0].data.numel() if isinstance(args[0], ce.PackedImages)
                                                               else args[0].numel() * args[0].element_size()))

    def run(n, raw):
        items = [{"image": pil[i % a.sizes], "index": i} for i in range(n)]
        del moved[:]
        with tempfile.TemporaryDirectory() as d:
            t, _ = timed(lambda: embed_images(emb, {"train": items}, batch_size=512, num_workers=a.workers, out_dir=d, raw_images=raw))
        return t, sum(moved) / n

    for raw in (False, True):
        run(512, raw)                                                  # warm-up: encoder build, staging, code objects
    print(f"(c) embed_images, {a.embed_n} mixed-size images ({a.sizes} sizes), {a.layers}-layer random tower, {a.workers} workers, batch 512")
    for rep in range(2):
        for raw in (False, True):
            t, per = run(a.embed_n, raw)
            print(f"(c) rep {rep} {'raw_images=True' if raw else 'host path      '}: {t / 1e3:.2f} s, {a.embed_n / t * 1e3:.0f} images/s, "
                  f"host-to-device {per / 1e6:.3f} MB/image", flush=True)
