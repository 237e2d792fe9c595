"""Time pg_token_attribution against pg_op_token_mean on the same hidden buffer (run on an MI355X):

    python tools/attribution_time.py [--images 512] [--panels 4] [--cells 1000] [--reps 20]

Both kernels stream the (images, 577, 1024) fp32 hidden states once; the attribution adds K directions read from LDS, one wave
reduction per direction and row, and K floats written per row.  Device-event timing, the two kernels alternated inside every
repetition, the median of `reps` repetitions after a warm-up; bytes are counted from the shapes (hidden + out; the 2 K rows of W a
block reads are L2 hits and not counted).  The hidden buffer of 512 images is 1.2 GB, far beyond the 256 MiB Infinity Cache.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pigeon_amd import _lib, hip_ops  # noqa: E402


def _time(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--panels", type=int, default=4)
    ap.add_argument("--cells", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--ks", default="1,2,8,16")
    args = ap.parse_args(argv)
    _lib.require_gpu()
    dev, n, P = "cuda", args.images, args.panels
    g = torch.Generator(device=dev).manual_seed(0)
    hidden = torch.randn((n, 577, 1024), generator=g, device=dev)
    W = (torch.rand((args.cells, 1024), generator=g, device=dev) * 2 - 1) / 32
    against = torch.randint(0, args.cells, (n // P,), generator=g, device=dev)
    hid_bytes = hidden.numel() * 4
    rows = []
    for K in (int(k) for k in args.ks.split(",")):
        cells = torch.randint(0, args.cells, (n // P, K), generator=g, device=dev)
        out = torch.empty((n // P, P, 577, K), device=dev)
        mean = lambda: hip_ops.token_mean(hidden)
        attr = lambda: hip_ops.token_attribution(hidden, W, cells, against, panels=P, out=out)
        for _ in range(3):
            mean(); attr()
        torch.cuda.synchronize()
        tm, ta = [], []
        for _ in range(args.reps):                                    # alternated: both see the same neighbours on the machine
            tm.append(_time(mean, 4))
            ta.append(_time(attr, 4))
        m, a = statistics.median(tm), statistics.median(ta)
        row = {"images": n, "panels": P, "K": K, "token_mean_ms": round(m, 4), "attribution_ms": round(a, 4), "ratio": round(a / m, 3),
               "token_mean_TBps": round((hid_bytes + n * 4096) / m / 1e9, 3), "attribution_TBps": round((hid_bytes + out.numel() * 4) / a / 1e9, 3),
               "attribution_ms_min_max": [round(min(ta), 4), round(max(ta), 4)], "token_mean_ms_min_max": [round(min(tm), 4), round(max(tm), 4)]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


if __name__ == "__main__":
    main()
