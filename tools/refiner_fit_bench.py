"""Times the refiner's grid sweep next to the way the same grid is evaluated without it.
`python tools/refiner_fit_bench.py [--out FILE] [--rows 8192] [--candidates 50]`.

The workload: a synthetic prototype bank (`synthetic.make_bank`, --cells x --protos prototypes), --rows queries with --candidates
random candidate cells each, and the default pass-1 grid of `pigeon_amd.refiner_fit` for that many candidates (every topk, 24
temperatures plus the current one, nine radii).  Event timing after a warm-up, median of --reps windows (50, 10, 10 and 1 calls a window for
the four rows, so that no window is shorter than a few milliseconds):
  (a) the sweep of the whole grid from the records of one refine_forward: pg_refine_sweep and pg_refine_sweep_totals separately
      (the values table of 12 columns is built once, outside the timed window, as the fit builds it once);
  (b) one hip_ops.refine_forward call at topk = --candidates: what leaves the records;
  (c) 64 grid points done the way they are done without the sweep -- 64 refine_forward calls, each streaming the bank again, at
      64 points spread over the grid -- scaled to the grid's G points.  (c) leaves the metrics of its 64 guesses uncomputed, which
      favours it.
The ratio reported is (c) / (a).  Before timing, the 64 points' choices are held against the sweep's, bit for bit."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--candidates", type=int, default=50)
    ap.add_argument("--cells", type=int, default=1000)
    ap.add_argument("--protos", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    from pigeon_amd import _lib, hip_ops, refiner_fit as F, synthetic
    _lib.require_gpu()
    B, k = args.rows, args.candidates
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    bank = hip_ops.DeviceBank(synthetic.make_bank(args.cells, args.protos, seed=2, exact_means=False), device="cuda")
    g = torch.Generator().manual_seed(5)
    q = torch.randn((B, 1024), generator=g).cuda()
    init = torch.stack([torch.rand(B, generator=g, dtype=torch.float64) * 360 - 180, torch.rand(B, generator=g, dtype=torch.float64) * 180 - 90], dim=1).cuda()
    cand = torch.stack([torch.randperm(args.cells, generator=g)[:k] for _ in range(B)]).cuda()
    probs = torch.sort(torch.softmax(torch.randn((B, k), generator=g), dim=1), dim=1, descending=True).values.float().contiguous().cuda()
    labels = init + 0.5
    topks, temps, max_kms = F.pass1_grid(k, (5, F.f32(1.6), 1000.0))
    nK, nT, nR = len(topks), len(temps), len(max_kms)
    G = nK * nT * nR
    say(f"refiner_fit_bench: {torch.cuda.get_device_name(0)}, {B} rows x {k} candidates, bank {bank.num_protos} prototypes / {bank.num_train} "
        f"training rows, grid {nK} x {nT} x {nR} = {G} points, plan {hip_ops.refine_sweep_plan(B, k, G, 12)}")

    def event_ms(fn, inner=1):
        """per call: `inner` calls in one event window (a window of a fraction of a millisecond measures the clock)"""
        out = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) / inner)
        return statistics.median(out), min(out), max(out)

    forward = lambda topk, T, km: hip_ops.refine_forward(bank, q, init, cand, probs, topk, T, km, return_scratch=True)
    scratch = forward(k, 1.0, float("inf"))[3]
    points = scratch[:, :, 1:3].reshape(B * k, 2).contiguous()
    km = hip_ops.haversine_pairs(labels[:, None, :].expand(B, k, 2).reshape(B * k, 2).contiguous(), points).reshape(B, k)
    values = torch.stack([km, torch.round(5000 * torch.exp(-km / 1492.7))] + [(km < r).double() for r in F.UNDER_KM], dim=2).contiguous()
    choice = hip_ops.refine_sweep_choice(scratch, probs, init, topks, temps, max_kms)
    totals = torch.empty((G, 14), dtype=torch.float64, device="cuda")

    rng = np.random.default_rng(0)
    sample = [(int(rng.integers(nK)), int(rng.integers(nT)), int(rng.integers(nR))) for _ in range(64)]
    same = all(torch.equal((choice[(i * nT + j) * nR + r] & 63).int(), forward(topks[i], temps[j], max_kms[r])[2]) for i, j, r in sample)
    say(f"64 sampled grid points against refine_forward, bit for bit: {'equal' if same else 'DIFFERENT'}")

    def the_old_way():
        for i, j, r in sample:
            hip_ops.refine_forward(bank, q, init, cand, probs, topks[i], temps[j], max_kms[r])

    for fn in (lambda: forward(k, 1.0, float("inf")), the_old_way):        # warm-up
        fn()
    sw = event_ms(lambda: hip_ops.refine_sweep_choice(scratch, probs, init, topks, temps, max_kms, out=choice), inner=50)
    to = event_ms(lambda: hip_ops.refine_sweep_totals(choice, values, out=totals), inner=10)
    one = event_ms(lambda: forward(k, 1.0, float("inf")), inner=10)
    old = event_ms(the_old_way)
    a_ms = sw[0] + to[0]
    c_ms = old[0] / 64 * G
    fmt = lambda t: f"{t[0]:10.3f} ms (min {t[1]:.3f}, max {t[2]:.3f})"
    say(f"  (a) pg_refine_sweep, {G} points        {fmt(sw)}   {G * B / sw[0] / 1e6:.2f} G selections/s, {G * B / sw[0] / 1e6:.2f} GB/s of choice bytes")
    say(f"  (a) pg_refine_sweep_totals            {fmt(to)}   {G * B * 12 / to[0] / 1e6:.2f} G gathered values/s")
    say(f"  (a) the sweep of the grid, both       {a_ms:10.3f} ms")
    say(f"  (b) one refine_forward, topk {k:<3d}      {fmt(one)}")
    say(f"  (c) 64 refine_forward calls           {fmt(old)}   mean topk {np.mean([topks[i] for i, _, _ in sample]):.1f}")
    say(f"  (c) scaled to {G} points            {c_ms:10.3f} ms")
    say(f"  (c) / (a) = {c_ms / a_ms:.1f}   ((c) / ((a) + (b)), the records included: {c_ms / (a_ms + one[0]):.1f})")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
