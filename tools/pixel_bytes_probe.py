"""Measurements around the 8-bit pixel path (PG_DTYPE_U8); none of them is a pass/fail threshold.

    python tools/pixel_bytes_probe.py im2col [--images 512] [--rounds 20]
        the encoder's im2col profile class (pg_vit_profile_*: device events around the im2col launch of pg_vit_forward) on a 2-layer
        tower at `--images` images, for fp32, fp16 and byte pixels: milliseconds per forward, median and range over the rounds after
        two warm-up forwards, the three formats taking turns.  The exact tier's im2col (pg_op_x3_im2col) is timed with device
        events around the launch, the same way.
    python tools/pixel_bytes_probe.py cpu
        the CPU measurement behind the feature, in float64 (needs no GPU): how far fp16-rounded pixels move the embedding of
        oracle.pigeon_oracle.vit_last_hidden_state(...).mean(1), 2 and 6 layers, three images of uniform random bytes.
"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def im2col(args):
    from pigeon_amd import hip_ops as ops, synthetic as syn
    n = args.images
    enc = ops.VitEncoder(syn.make_vit_weights(seed=0, layers=2), max_chunk=n)
    g = torch.Generator().manual_seed(0)
    b = torch.randint(0, 256, (n, 3, 336, 336), generator=g, dtype=torch.uint8).to("cuda")
    p32 = ops.bytes_to_pixels(b)
    inputs = {"fp32": p32, "fp16": p32.half(), "bytes": b}
    enc.profile_enable(True, classes=["im2col"])
    fast = {k: [] for k in inputs}
    x3 = {k: [] for k in inputs}
    out3 = torch.empty((min(n, 128) * 576, 3 * 640), dtype=torch.float16, device="cuda")
    for r in range(args.rounds + 2):
        for k, px in inputs.items():
            enc.profile_reset()
            enc.forward(px)
            torch.cuda.synchronize()
            launches, ms = enc.profile_read()["im2col"]
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            ops.x3_im2col(px[:min(n, 128)], out=out3)
            e.record()
            e.synchronize()
            if r >= 2:
                fast[k].append(ms / max(launches, 1))
                x3[k].append(a.elapsed_time(e))
    mb = {"fp32": 4, "fp16": 2, "bytes": 1}
    print(f"im2col profile class, {n} images, 2-layer tower, {args.rounds} rounds; patch matrix written: {n * 576 * 640 * 2 / 1e6:.0f} MB")
    for k in inputs:
        v = fast[k]
        print(f"  {k:>5} pixels ({n * 3 * 336 * 336 * mb[k] / 1e6:7.1f} MB read): median {statistics.median(v) * 1e3:8.1f} us  "
              f"(min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f})")
    print(f"pg_op_x3_im2col, {min(n, 128)} images (one internal pass of the exact tier), device events around the launch")
    for k in inputs:
        v = x3[k]
        print(f"  {k:>5} pixels: median {statistics.median(v) * 1e3:8.1f} us  (min {min(v) * 1e3:.1f}, max {max(v) * 1e3:.1f})")
    enc.close()


def cpu(args):
    import numpy as np
    from oracle import pigeon_oracle
    from oracle.clip_preprocess_oracle import normalise_lut
    from pigeon_amd import synthetic as syn
    lut = torch.from_numpy(normalise_lut())
    rng = np.random.default_rng(0)
    b = torch.from_numpy(rng.integers(0, 256, (3, 3, 336, 336), dtype=np.uint8)).long()
    px = torch.stack([lut[c][b[:, c]] for c in range(3)], dim=1)
    for layers in (2, 6):
        sd = syn.make_vit_weights(seed=0, layers=layers)
        emb = lambda p: pigeon_oracle.vit_last_hidden_state(sd, p, dtype=torch.float64).mean(1)      # noqa: E731
        ref, half = emb(px), emb(px.half().float())
        rel = (half - ref).norm(dim=1) / ref.norm(dim=1)
        print(f"{layers} layers: fp16-rounded pixels move the fp64 embedding by {[f'{v:.2e}' for v in rel.tolist()]} relative")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["im2col", "cpu"])
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=20)
    a = ap.parse_args()
    {"im2col": im2col, "cpu": cpu}[a.what](a)
