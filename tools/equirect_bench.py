"""Time of the equirectangular view kernel (pg_equirect_forward) at the size a user of 360-degree imagery runs, next to the ragged
resize (pg_prep_ragged_forward) on the views it wrote, in the same run.

   python tools/equirect_bench.py                      # 128 panoramas of 4096 x 2048 -> 512 views at the default size (1304)

Device events around one call each, the two alternated, median of `--reps` samples after a warm-up.  The panoramas are seeded random
bytes made on the device (nothing is copied from the host inside the timed window; the two descriptor copies of a call are).  Bytes:
what the algorithm needs -- every source byte once and every view byte once for the gnomonic kernel; every view byte once and the
8-bit pixels out for the resize.  Prints one JSON line.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pigeon_amd import _lib, hip_ops, panorama  # noqa: E402
from pigeon_amd.packing import packed_layout  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--panoramas", type=int, default=128)
ap.add_argument("--height", type=int, default=2048)
ap.add_argument("--width", type=int, default=4096)
ap.add_argument("--size", type=int, default=None, help="view size (default: panorama.default_view_size(width))")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()

_lib.require_gpu()
DEV = torch.device("cuda", 0)
torch.cuda.set_device(DEV)
sizes = [(a.height, a.width)] * a.panoramas
offs, total = packed_layout(sizes)
views = panorama.view_list(sizes, size=a.size)
plan = hip_ops.equirect_plan(views, offs)
S = views[0][3]
src = torch.empty(total, dtype=torch.uint8, device=DEV)
g = torch.Generator(device=DEV).manual_seed(0)
for o in offs:                                                       # panorama by panorama: no second buffer of the whole size
    src[o:o + a.height * a.width * 3].random_(0, 256, generator=g)
packed = torch.empty(plan.prep.packed_bytes, dtype=torch.uint8, device=DEV)
resize = hip_ops.RaggedPreprocessor(DEV.index)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


arms = {"equirect_ms": lambda: hip_ops.equirect_forward(src, plan, packed),
        "ragged_resize_ms": lambda: resize.forward(packed, plan.prep, torch.uint8, header_written=True)}
ms = {k: [] for k in arms}
for r in range(a.warmup + a.reps):
    for k, fn in arms.items():
        t = timed(fn)
        if r >= a.warmup:
            ms[k].append(t)
n_views = plan.n
view_bytes = n_views * S * S * 3
res = {"panoramas": a.panoramas, "source": [a.height, a.width], "views": n_views, "view_size": S, "reps": a.reps}
for k, v in ms.items():
    res[k] = round(statistics.median(v), 4)
    res[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
res["equirect_bytes"] = a.panoramas * a.height * a.width * 3 + view_bytes
res["equirect_GBps"] = round(res["equirect_bytes"] / (res["equirect_ms"] * 1e-3) / 1e9, 1)
res["equirect_Gpixel_per_s"] = round(n_views * S * S / (res["equirect_ms"] * 1e-3) / 1e9, 2)
res["ragged_resize_bytes"] = view_bytes + n_views * 3 * 336 * 336
res["ratio_equirect_over_resize"] = round(res["equirect_ms"] / res["ragged_resize_ms"], 3)
print(json.dumps(res))
