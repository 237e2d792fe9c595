"""Times the paired bootstrap of the evaluate stat list on the GPU next to numpy on the same box's CPUs.
`python tools/bootstrap_bench.py [--out FILE] [-N 100000] [-R 10000]`.

The workload: N = 10^5 items, R = 10^4 replicates, the columns `pigeon_amd.bootstrap.metric_columns` builds for a run with --guess
and --neighbours: 20 columns whose means are taken (the km error, the rounded score and the ten Under_*_km indicators of the model's
guess, two geocell hits, and km, score and one indicator for each of the two other guesses) and 3 whose medians are taken (the three
km columns), plus the six paired differences, which cost nothing more.
GPU: event timing after warm-up, median of --reps: pg_bootstrap_means, the stable sort and rank scatter, pg_bootstrap_quantiles, and
`bootstrap()` end to end under a host clock that ends in a synchronise (it includes the copies and the percentile summary).
numpy: (a) tests/_bootref.py, the bit-exact restatement (Philox in numpy, the kernel's summation order, numpy.quantile), and (b) the
plain way a user would write it -- Generator.integers, fancy indexing, mean and median -- each on --np-reps replicates split over
--procs worker processes (16), wall clock, scaled to R.  Before timing, two replicates of the GPU result are held to (a) bit for bit.
Draws per second = R N / time; gathers per second = R N columns / time."""
import argparse
import os
import statistics
import sys
import time
from concurrent.futures import ProcessPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KMS = (1, 5, 10, 25, 50, 100, 200, 750, 1000, 2500)


def make_columns(N, seed=0):
    rng = np.random.default_rng(seed)
    cols = {}
    km = rng.gamma(0.6, 900.0, N)
    for tag, d in (("", km), ("_best", km * rng.uniform(0.7, 1.2, N)), ("_nn", rng.gamma(0.6, 1500.0, N))):
        cols["km" + tag] = d
        cols["score" + tag] = np.round(5000 * np.exp(-d / 1492.7))
    for k in KMS:
        cols[f"under_{k}_km"] = (km < k).astype(np.float64)
    cols["geocell_hit"] = (rng.random(N) < 0.4).astype(np.float64)
    cols["geocell_top5_hit"] = (rng.random(N) < 0.7).astype(np.float64)
    cols["best_taken"] = (rng.random(N) < 0.3).astype(np.float64)
    cols["nn_beats_model"] = (cols["km_nn"] < km).astype(np.float64)
    stats = {c: ("mean", c) for c in cols}
    for tag in ("", "_best", "_nn"):
        stats["median km" + tag] = ("median", "km" + tag)
        if tag:
            stats[f"mean km{tag} - km"] = ("mean_diff", "km" + tag, "km")
            stats[f"median km{tag} - km"] = ("median_diff", "km" + tag, "km")
            stats[f"mean score{tag} - score"] = ("mean_diff", "score" + tag, "score")
    return cols, stats


def _np_restated(args):
    import _bootref as B
    xm, xq, seed, rs = args
    t = time.perf_counter()
    B.means(xm, 0, seed, replicates=rs)
    B.quantiles(xq, 0, seed, (0.5,), replicates=rs)
    return time.perf_counter() - t


def _np_plain(args):
    xm, xq, seed, rs = args
    t = time.perf_counter()
    N = xm.shape[1]
    for r in rs:
        idx = np.random.default_rng([seed, r]).integers(0, N, N)
        xm[:, idx].mean(axis=1)
        np.median(xq[:, idx], axis=1)
    return time.perf_counter() - t


def numpy_seconds(fn, xm, xq, seed, reps, procs):
    """Wall clock of `reps` replicates over `procs` processes (after one replicate each to warm the workers up)."""
    with ProcessPoolExecutor(procs) as ex:
        list(ex.map(fn, [(xm, xq, seed, [0])] * procs))
        parts = [list(range(p, reps, procs)) for p in range(procs)]
        t = time.perf_counter()
        list(ex.map(fn, [(xm, xq, seed, rs) for rs in parts]))
        return time.perf_counter() - t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("-N", type=int, default=100000)
    ap.add_argument("-R", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--np-reps", type=int, default=160)
    ap.add_argument("--procs", type=int, default=16)
    args = ap.parse_args()
    import torch
    import _bootref as B
    from pigeon_amd import _lib, bootstrap as boot, hip_ops
    _lib.require_gpu()
    N, R, seed = args.N, args.R, 1
    cols, stats = make_columns(N)
    mean_names = [c for c in cols]
    q_names = ["km", "km_best", "km_nn"]
    xm = np.stack([cols[c] for c in mean_names])
    xq = np.stack([cols[c] for c in q_names])
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    say(f"bootstrap_bench: {torch.cuda.get_device_name(0)}, N = {N}, R = {R}, {len(mean_names)} mean columns, {len(q_names)} median columns, "
        f"plan {hip_ops.bootstrap_plan(N, R, len(q_names), 1)}")
    dm, dq = torch.from_numpy(xm).cuda(), torch.from_numpy(xq).cuda()

    def ranks():
        srt, order = torch.sort(dq, dim=1, stable=True)
        rank = torch.empty(order.shape, dtype=torch.int32, device="cuda")
        rank.scatter_(1, order, torch.arange(N, dtype=torch.int32, device="cuda").expand_as(order))
        return rank, srt.contiguous()

    rank, srt = ranks()
    gm = hip_ops.bootstrap_means(dm, R, seed)
    gq = hip_ops.bootstrap_quantiles(rank, srt, R, (0.5,), seed)
    pick = [0, R - 1]
    ok = np.array_equal(gm[pick].cpu().numpy(), B.means(xm, R, seed, replicates=pick)) and \
        np.array_equal(gq[pick].cpu().numpy(), B.quantiles(xq, R, seed, (0.5,), replicates=pick))
    say(f"replicates {pick} against the restatement, bit for bit: {'equal' if ok else 'DIFFERENT'}")

    def event_ms(fn):
        out = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            b.synchronize()
            out.append(a.elapsed_time(b))
        return statistics.median(out), min(out), max(out)

    out_m, out_q = torch.empty_like(gm), torch.empty_like(gq)
    rows = (("pg_bootstrap_means", lambda: hip_ops.bootstrap_means(dm, R, seed, out=out_m), len(mean_names)),
            ("stable sort + rank scatter", ranks, 0),
            ("pg_bootstrap_quantiles", lambda: hip_ops.bootstrap_quantiles(rank, srt, R, (0.5,), seed, out=out_q), len(q_names)))
    total = 0.0
    for name, fn, ncol in rows:
        med, lo, hi = event_ms(fn)
        total += med
        groups = -(-ncol // 4) if ncol else 0
        passes = 1 if name.endswith("means") else hip_ops.bootstrap_plan(N, R, 1, 1)["passes"]
        extra = f"  {R * N * groups * passes / med / 1e6:8.2f} G draws/s  {R * N * ncol * passes / med / 1e6:8.2f} G gathers/s" if ncol else ""
        say(f"  {name:28s} {med:10.2f} ms (min {lo:.2f}, max {hi:.2f}){extra}")
    ends = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        boot.bootstrap(cols, stats, R=R, seed=seed)
        torch.cuda.synchronize()
        ends.append(time.perf_counter() - t)
    say(f"  the three together            {total:10.2f} ms;  bootstrap() end to end, host clock: {statistics.median(ends) * 1e3:.2f} ms "
        f"({len(stats)} statistics)")
    for name, fn in (("numpy, the bit-exact restatement", _np_restated), ("numpy, Generator.integers + mean + median", _np_plain)):
        sec = numpy_seconds(fn, xm, xq, seed, args.np_reps, args.procs)
        say(f"  {name:42s} {args.np_reps} replicates on {args.procs} processes: {sec:.2f} s -> {sec * R / args.np_reps:.1f} s for R = {R} "
            f"({sec * R / args.np_reps * 1e3 / total:.0f} x the kernels)")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
