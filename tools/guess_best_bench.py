"""Times the guess by expected score (pg_score_table once, pg_guess_best per batch) next to the kernels it sits between and against the
only other route to the same answer.  `python tools/guess_best_bench.py [--out FILE]`.

B = 128 panoramas, C = M in {2076, 11000}: the table's build (its own line: 34 MB and 968 MB, built once per model), then per batch
pg_guess_best, and in the same run pg_head_forward and pg_guess_spread (G = 1).  Then the route that existed before this kernel:
pg_guess_spread asked about every candidate (G = M) followed by a torch argmax, at C = 2076 with M = 64 and M = 2076.  The new kernel
must be faster at both (the process exits with 1 if it is not): it does the row's exps once, not M times, and none of the bisection
passes.  Event timing after warm-up, median of --reps (30); the G = M route takes --route-reps (10).  FLOP and bytes from the shapes:
  guess_best   FLOP 2 B M C (fp64)   bytes 8 (M C + 2 B C + B M) + 4 B C    table, weights written and read, expected, logits
against 78.6 TFLOP/s (the MI355X's public fp64 matrix rate) and the achievable HBM rate given with --hbm-tbs (default 5.0 TB/s)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_F64_TF = 78.6
B = 128


def event_ms(fn, n):
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def median_ms(fn, n, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    return statistics.median(event_ms(fn, n))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--route-reps", type=int, default=10)
    ap.add_argument("--hbm-tbs", type=float, default=5.0)
    args = ap.parse_args()
    from pigeon_amd import hip_ops, synthetic
    dev = "cuda"
    lines = [f"guess_best_bench: {torch.cuda.get_device_name(0)}, B = {B}, median of {args.reps} after warm-up, ms"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    say("     C      M | form tile  wgs scratch MB | table build | guess_best  +expected | GFLOP    MB  bound ms  share | head_forward  spread G=1")
    for Cn in (2076, 11000):
        M = Cn
        g = torch.Generator().manual_seed(Cn)
        cen = torch.from_numpy(synthetic.make_geocells(Cn, seed=0)).to(dev)
        emb = (torch.randn((B, 4, 1024), generator=g) * 0.7 + 0.1).to(dev)
        W0, b0 = synthetic.make_head_weights(Cn, seed=0)
        W, bias = (W0 * 64).to(dev), b0.to(dev)
        head = hip_ops.head_forward(emb, W, bias, cen, 5)
        logits, llh = head["logits"], head["preds_LLH"]
        t_build = median_ms(lambda: hip_ops.score_table(cen, cen, kind="score"), 5 if Cn > 4000 else args.reps, warm=1)
        table = hip_ops.score_table(cen, cen, kind="score")
        best_fn = lambda: hip_ops.guess_best(logits, table)                                      # noqa: E731
        exp_fn = lambda: hip_ops.guess_best(logits, table, return_expected=True)                 # noqa: E731
        for fn in (best_fn, exp_fn) * 5:                             # warm-up, alternating as the measurement does
            fn()
        torch.cuda.synchronize()
        ours, with_exp = [], []
        for _ in range(args.reps):
            ours += event_ms(best_fn, 1); with_exp += event_ms(exp_fn, 1)
        t_best, t_exp = statistics.median(ours), statistics.median(with_exp)
        t_head = median_ms(lambda: hip_ops.head_forward(emb, W, bias, cen, 5), args.reps)
        t_spread = median_ms(lambda: hip_ops.guess_spread(logits, cen, llh, (0.5, 0.9)), args.reps)
        plan = hip_ops.guess_best_plan(B, Cn, M)
        flop = 2.0 * B * M * Cn
        by = 8.0 * (M * Cn + 2 * B * Cn + B * M) + 4.0 * B * Cn
        t_f, t_b = flop / (PEAK_F64_TF * 1e12) * 1e3, by / (args.hbm_tbs * 1e12) * 1e3
        floor = max(t_f, t_b)
        say(f"{Cn:6d} {M:6d} | {plan['form']:4d} {plan['rows_per_tile']:4d} {plan['workgroups']:4d} {plan['scratch_bytes'] / 1e6:10.1f} | "
            f"{t_build:11.3f} | {t_best:10.3f} {t_exp:10.3f} | {flop / 1e9:5.2f} {by / 1e6:5.0f}  {'MFMA' if t_f > t_b else 'bytes'} {floor:.3f} "
            f"{floor / t_best:6.1%} | {t_head:12.3f} {t_spread:11.3f}")
        del table

    say("the route before this kernel, C = 2076: pg_guess_spread with G = M, then torch.argmax")
    say("     M | spread G=M + argmax | table route: guess_best | faster by")
    Cn, slower = 2076, []
    g = torch.Generator().manual_seed(7)
    cen = torch.from_numpy(synthetic.make_geocells(Cn, seed=0)).to(dev)
    logits = (torch.randn((B, Cn), generator=g) * 3).to(dev)
    for M in (64, 2076):
        cand = cen[:M].contiguous()
        pts = cand[None].expand(B, M, 2).contiguous()
        table = hip_ops.score_table(cand, cen, kind="score")

        def old():
            return hip_ops.guess_spread(logits, cen, pts, (1.0,))[1].argmax(dim=1)

        def new():
            return hip_ops.guess_best(logits, table)[0]

        agree = float((old() == new()).double().mean())
        t_old = median_ms(old, args.route_reps, warm=2)
        t_new = median_ms(new, args.reps)
        say(f"{M:6d} | {t_old:19.3f} | {t_new:23.3f} | {t_old / t_new:8.1f}x   (the two routes pick the same candidate in {agree:.1%} of the rows)")
        if not t_new < t_old:
            slower.append(M)
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    if slower:
        print(f"guess_best_bench: the table route is NOT faster than pg_guess_spread + argmax at M = {slower}: a defect")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
