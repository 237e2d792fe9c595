"""Time the prototype clustering: pigeon_amd.prototypes.cluster_cells (GPU graphs + host xi extraction) against sklearn's
OPTICS.fit_predict on the same distance matrices, in one process on the same machine.

    python tools/optics_bench.py [--min-samples 20] [--xi 0.1] [--repeats 5] [--no-sklearn]

Workload: 2048 cells of 64 points plus cells of 1000, 2049 and 8192 points, clumped seeded coordinates.  Every GPU figure is the median
of `--repeats` timed runs after one untimed warm-up run of the same call (first-call costs: library load, LDS attribute, allocator
pools); wall clock with a device synchronisation on both sides, so host work (grouping, uploads, xi) is included where the line
says so.  The sklearn leg runs the 1000- and the 2049-point cell and 64 of the small cells (the rest is extrapolated, and said so); the
8192-point cell is left out of it, it would not finish in a benchmark's time.  Labels of the two legs are compared cell by cell.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def workload(seed=0):
    rng = np.random.default_rng(seed)
    sizes = [64] * 2048 + [1000, 2049, 8192]
    pts, cell = [], []
    for c, n in enumerate(sizes):
        centre = np.array([rng.uniform(-150, 150), rng.uniform(-60, 60)])
        k = max(2, n // 200)
        which = rng.integers(0, k, n)
        centres = centre + rng.normal(0, 0.5, (k, 2))
        pts.append(centres[which] + rng.normal(0, 0.02, (n, 2)) * (1 + which[:, None]))
        cell += [c] * n
    return np.concatenate(pts), np.array(cell, dtype=np.int64), sizes


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--min-samples", type=int, default=20)
    ap.add_argument("--xi", type=float, default=0.1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-sklearn", action="store_true")
    a = ap.parse_args()
    import torch
    from pigeon_amd import hip_ops, prototypes
    lnglat, cell, sizes = workload()
    args = (a.min_samples, a.xi)
    print(f"workload: {len(sizes)} cells, {len(cell)} points (2048 x 64, 1000, 2049, 8192); min_samples {a.min_samples}, xi {a.xi}; "
          f"{torch.cuda.get_device_name(0)}; median [min .. max] of {a.repeats} runs after one warm-up")

    labels, med, lo, hi = timed(lambda: prototypes.cluster_cells(lnglat, cell, args), a.repeats)
    print(f"cluster_cells, all cells (host grouping + GPU distances and graphs + host xi): {med * 1e3:9.1f} ms [{lo * 1e3:.1f} .. {hi * 1e3:.1f}]")
    _, med_g, lo_g, hi_g = timed(lambda: prototypes.optics_graph_cells(lnglat, cell, a.min_samples), a.repeats)
    print(f"optics_graph_cells, all cells (the same without the xi extraction):            {med_g * 1e3:9.1f} ms [{lo_g * 1e3:.1f} .. {hi_g * 1e3:.1f}]")
    for name, pick in (("2048 cells of 64", cell < 2048), ("the 1000-point cell", cell == 2048), ("the 2049-point cell", cell == 2049),
                       ("the 8192-point cell", cell == 2050)):
        pts = torch.from_numpy(lnglat[pick]).to("cuda")
        sz = np.bincount(cell[pick] - cell[pick].min())
        off = torch.from_numpy(np.concatenate([[0], np.cumsum(sz)]).astype(np.int64))
        (dist, mo), t_d, _, _ = timed(lambda: hip_ops.haversine_blocks(pts, off), a.repeats)
        _, t_g, lo_k, hi_k = timed(lambda: hip_ops.optics_graph(dist, off, mo, a.min_samples), a.repeats)
        print(f"  device only, {name:20s}: pg_haversine_blocks {t_d * 1e3:8.2f} ms, pg_optics_graph {t_g * 1e3:8.2f} ms [{lo_k * 1e3:.2f} .. {hi_k * 1e3:.2f}]")
        del dist

    if a.no_sklearn:
        return
    from sklearn.cluster import OPTICS
    total, agree, cells_run = 0.0, 0, 0
    small_t = 0.0
    for c in list(range(64)) + [2048, 2049]:
        pick = cell == c
        pts = torch.from_numpy(lnglat[pick]).to("cuda")
        n = int(pick.sum())
        off = torch.tensor([0, n], dtype=torch.int64)
        D = hip_ops.haversine_blocks(pts, off)[0].cpu().numpy().reshape(n, n)
        t = time.perf_counter()
        lab = OPTICS(min_samples=a.min_samples, xi=a.xi, metric="precomputed").fit_predict(D)
        dt = time.perf_counter() - t
        if c < 2048:
            small_t += dt
        else:
            print(f"sklearn OPTICS.fit_predict, the {n}-point cell: {dt * 1e3:9.1f} ms")
        total += dt
        cells_run += 1
        agree += int(np.array_equal(lab, labels[pick]))
    print(f"sklearn OPTICS.fit_predict, 64 cells of 64 points: {small_t * 1e3:9.1f} ms (x 32 = {small_t * 32 * 1e3:.0f} ms extrapolated to the 2048)")
    print(f"labels equal to cluster_cells' in {agree} of the {cells_run} cells sklearn ran")


if __name__ == "__main__":
    main()
