"""Why the one-shape list path of gpu_preprocess keeps a pinned staging buffer of its own: 512 images of 640 x 640 (629 MB) through
that path, alone and alternating with a pageable PackedImages of the same images (arm (b) of tools/prep_ragged_ab.py), with the
library's arrangement (`own`: pigeon_amd.preprocess._UNIFORM_STAGING) and with the ragged path's buffer in its place (`shared`), phase
by phase on the host clock.  One process; every sample ends in a device synchronise.

   python tools/prep_staging_probe.py            # both arrangements, alternation and phases
   python tools/prep_staging_probe.py --alone    # the one-shape path alone, through clip_embedder.gpu_preprocess only (any commit)
"""
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pigeon_amd import clip_embedder as ce  # noqa: E402

DEV = torch.device("cuda", 0)
rng = np.random.default_rng(2)
base = [rng.integers(0, 256, (640, 640, 3), dtype=np.uint8) for _ in range(16)]
ims = [base[i % 16] for i in range(512)]


def timed(fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def per_size():
    ce.gpu_preprocess(ims, DEV, torch.float16)


def packed():
    ce.gpu_preprocess(ce.pack_images(ims), DEV, torch.float16)


def report(name, v):
    print(f"{name}: median {statistics.median(v):.2f} ms, min {min(v):.2f}, max {max(v):.2f}  samples " + " ".join(f"{x:.1f}" for x in v), flush=True)


report("one-shape list alone", [timed(per_size) for _ in range(10)][2:])
if "--alone" in sys.argv:
    sys.exit(0)

from pigeon_amd import preprocess as pp  # noqa: E402
from pigeon_amd.packing import as_rgb_array, check_rgb_u8  # noqa: E402

packed()
own, ragged = pp._UNIFORM_STAGING[0], pp._STAGING[0]


def phases():
    """The one-shape list path by hand (pigeon_amd/preprocess.py gpu_preprocess), with a clock between its steps."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    arrs = [as_rgb_array(im) for im in ims]
    for a in arrs:
        check_rgb_u8(a)
    t1 = time.perf_counter()
    staging = pp._staging(DEV, uniform=True)
    t = staging.take(len(arrs) * arrs[0].size).view((len(arrs),) + arrs[0].shape)
    view = t.numpy()
    t2 = time.perf_counter()
    for j, a in enumerate(arrs):
        view[j] = a
    t3 = time.perf_counter()
    with torch.cuda.device(DEV):
        on_dev = t.to(DEV, non_blocking=True).contiguous()
        staging.copied()
        staging.event.synchronize()
        t4 = time.perf_counter()
        pp._preprocessor(640, 640, 0)(on_dev, torch.float16)
    torch.cuda.synchronize()
    t5 = time.perf_counter()
    return [(b - a) * 1e3 for a, b in ((t0, t1), (t1, t2), (t2, t3), (t3, t4), (t4, t5), (t0, t5))]


for name, staging in (("own", own), ("shared", ragged), ("own", own), ("shared", ragged)):
    pp._UNIFORM_STAGING[0] = staging
    a, b = [], []
    for r in range(10):
        ta, tb = timed(per_size), timed(packed)
        if r >= 2:
            a.append(ta), b.append(tb)
    report(f"{name:6s} buffer, alternating: one-shape list", a)
    report(f"{name:6s} buffer, alternating: packed        ", b)
    for label, between in (("alone       ", None), ("after packed", packed)):
        rows = []
        for r in range(10):
            if between is not None:
                between()
            p = phases()
            if r >= 2:
                rows.append(p)
        m = [statistics.median(c) for c in zip(*rows)]
        print(f"{name:6s} buffer, phases {label}: convert+check {m[0]:.2f}  take {m[1]:.3f}  host fill {m[2]:.2f}  copy {m[3]:.2f}  kernels {m[4]:.2f}  "
              f"total {m[5]:.2f} ms", flush=True)
pp._UNIFORM_STAGING[0] = own
