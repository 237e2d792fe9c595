"""Time the point-in-region lookup: pigeon_amd.regions.find_regions / contains (GPU classification + host rational fallback) next to
the host rational classifier alone (pigeon_amd.regions.exact_state, first covering region in index order) on the same inputs, in one
process on the same machine.

    python tools/regions_bench.py [--points 100000] [--host-points 300] [--repeats 5]

Workloads: a geocell-like bank (a 50 x 40 grid of 2 000 one-degree cells, 5 vertices each: one wave per point) and a country-like bank
(12 x 8 stars of 4 096 edges each, 393 312 vertices: one workgroup per point), uniform points over each bank's extent plus 1 % on cell
edges (ambiguous on the device, settled exactly).  Every GPU figure is the median of `--repeats` timed runs after one untimed warm-up of
the same call; wall clock with a device synchronisation on both sides, so uploads, downloads and the host fallback are included.  The
host leg runs `--host-points` of the same points and is reported per point.  Results of the two legs are compared on those points.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def star(n, cx, cy, r0, r1):
    ang = 0.1 + 2 * np.pi * np.arange(n) / n
    ring = np.stack([cx + np.where(np.arange(n) % 2 == 0, r1, r0) * np.cos(ang), cy + np.where(np.arange(n) % 2 == 0, r1, r0) * np.sin(ang)], axis=1)
    return np.concatenate([ring, ring[:1]])


def box(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1], [x0, y0]], dtype=np.float64)


def timed(fn, repeats):
    import torch
    fn()                                                           # warm-up, untimed
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t)
    return out, statistics.median(ts), min(ts), max(ts)


def host_first_cover(rg, bank, p):
    for g in np.nonzero((bank.region_bbox[:, 0] <= p[0]) & (p[0] <= bank.region_bbox[:, 2]) & (bank.region_bbox[:, 1] <= p[1]) & (p[1] <= bank.region_bbox[:, 3]))[0]:
        if rg.exact_state(bank, p, int(g)) != rg.OUTSIDE:
            return int(g)
    return -1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100000)
    ap.add_argument("--host-points", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    from pigeon_amd import hip_ops, regions as rg
    print(f"device: {torch.cuda.get_device_name(0)}; points {args.points}, host leg {args.host_points}, repeats {args.repeats}")
    rng = np.random.default_rng(0)
    banks = {
        "geocells (2000 cells x 4 edges)": (rg.RegionBank([[box(-25.0 + ix, -20.0 + iy, -24.0 + ix, -19.0 + iy)] for iy in range(40) for ix in range(50)]), (-25.5, 25.5, -20.5, 20.5)),
        "countries (96 stars x 4096 edges)": (rg.RegionBank([[star(4096, -165.0 + 30 * ix, -70.0 + 20 * iy, 5.0, 9.0)] for iy in range(8) for ix in range(12)]), (-180, 180, -80, 80)),
    }
    for name, (bank, (x0, x1, y0, y1)) in banks.items():
        pts = np.stack([rng.uniform(x0, x1, args.points), rng.uniform(y0, y1, args.points)], axis=1)
        pts[::100, 0] = np.round(pts[::100, 0])                    # 1 %: on a cell edge of the grid bank
        plan = hip_ops.region_plan(bank.handle)
        (idx, info), med, lo, hi = timed(lambda: rg.find_regions(bank, pts), args.repeats)
        print(f"{name}: plan {plan}")
        print(f"  find_regions, {args.points} points: median {med * 1e3:.1f} ms (min {lo * 1e3:.1f}, max {hi * 1e3:.1f}) = {med / args.points * 1e6:.2f} us/point; "
              f"{info['ambiguous']} ambiguous settled on the host, {info['nearest']} to the nearest region")
        d_pts = torch.from_numpy(pts).to("cuda")
        _, med, lo, hi = timed(lambda: hip_ops.region_locate(bank.handle, d_pts), args.repeats)
        print(f"  pg_region_locate alone (points resident): median {med * 1e3:.2f} ms (min {lo * 1e3:.2f}, max {hi * 1e3:.2f})")
        _, med, lo, hi = timed(lambda: hip_ops.region_nearest(bank.handle, d_pts[:2000]), args.repeats)
        print(f"  pg_region_nearest alone, 2000 points: median {med * 1e3:.2f} ms (min {lo * 1e3:.2f}, max {hi * 1e3:.2f})")
        sub = pts[:args.host_points]
        t = time.perf_counter()
        host = np.array([host_first_cover(rg, bank, p) for p in sub])
        dt = time.perf_counter() - t
        covered = host >= 0
        same = bool(np.array_equal(idx[:args.host_points][covered], host[covered]))
        print(f"  host rational classifier (exact_state, boxes first), {args.host_points} points: {dt * 1e3:.1f} ms = {dt / args.host_points * 1e6:.1f} us/point; "
              f"covered points agree with the GPU leg: {same}")


if __name__ == "__main__":
    main()
