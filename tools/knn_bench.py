"""Times the exact nearest-neighbour search (pg_knn_search) over a bank of 2^20 x 1024 embeddings, k = 10, B = 1, 8 and 128, next to the
two torch compositions that answer the same question on the same GPU.  `python tools/knn_bench.py [--out FILE] [--log2n 20]`.

Per B, event timing after warm-up, median of --reps:
  fast     mode 2: the 16-bit MFMA pass, the merge and the rerank (what a certified query costs).  The pass reads the fp16 bank once
           per tile of 32 queries, so its bytes are ceil(B / 32) * N * 2048; the rate printed divides them by the WHOLE time of the
           three kernels, a lower bound on the pass's own rate, to be read against the 6.0-6.1 TB/s of an in-order HBM sweep.
  search   mode 0: the above plus the exact tier for the queries the certificate did not settle (how many: the `cert` column).
  exact    mode 1: the exact tier alone, fp32 at the vector rate (--exact-reps runs; it is the slow arm every other one is compared with).
  cdist    torch.cdist (fp32) + topk: materialises B x N.
  mm16     fp16 matmul + fp32 half norms + topk: materialises B x N, and `wrong` counts the queries whose k rows differ from the
           exact answer (as sets) -- what 16 bits alone cost.
The bank is clustered (a latent-8 manifold around a unit vector plus 2^-9 relative noise) and the queries are bank rows plus noise of
the same size, searched leave-one-out: near neighbours are closer than fp16 resolves, as street-level panoramas are."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

K = 10
HBM_SWEEP_TBS = (6.0, 6.1)


def median_ms(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def make_bank(n, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    base = torch.randn(1024, generator=g, device=dev)
    base /= base.norm()
    A = torch.randn(1024, 8, generator=g, device=dev) / 32
    x = torch.empty((n, 1024), dtype=torch.float32, device=dev)
    for s in range(0, n, 1 << 16):
        e = min(n, s + (1 << 16))
        z = torch.randn(e - s, 8, generator=g, device=dev)
        x[s:e] = base + 0.3 * z @ A.T + 2.0 ** -9 / 32 * torch.randn(e - s, 1024, generator=g, device=dev)
    return x, g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--exact-reps", type=int, default=1)
    args = ap.parse_args()
    from pigeon_amd import hip_ops
    dev = "cuda"
    n = 1 << args.log2n
    lines = [f"knn_bench: {torch.cuda.get_device_name(0)}, N = 2^{args.log2n} x 1024, k = {K}, median of {args.reps} after warm-up"]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    x, g = make_bank(n, dev)
    torch.cuda.synchronize()
    prep_ms = median_ms(lambda: hip_ops.knn_prepare(x), 3, warm=1)
    bank = hip_ops.knn_prepare(x)
    plan = hip_ops.knn_plan(n, 128, K)
    say(f"prepare (fp16 copy, half norms, statistics): {prep_ms:.2f} ms = {n * 6144 / prep_ms / 1e9:.2f} TB/s of 6 KB a row; bad values "
        f"{bank.bad_values}, xmax {bank.xmax:.3f}; plan {plan}")
    say("    B | fast ms  TB/s of the fp16 bank | search ms  cert | exact ms | cdist+topk ms | mm16+topk ms  wrong | in-order sweep "
        f"{HBM_SWEEP_TBS[0]}-{HBM_SWEEP_TBS[1]} TB/s: {n * 2048 / HBM_SWEEP_TBS[1] / 1e9:.3f} ms a pass")
    hn16 = None
    for B in (1, 8, 128):
        rows = torch.randint(0, n, (B,), generator=g, device=dev)
        q = (x[rows] * (1 + 2.0 ** -9 * torch.randn(B, 1024, generator=g, device=dev))).contiguous()
        ws = torch.empty((hip_ops.knn_workspace_bytes(n, B, K) + 256,), dtype=torch.uint8, device=dev)
        run = lambda mode: hip_ops.knn_search(bank, q, K, exclude=rows, mode=mode, workspace=ws)     # noqa: E731
        fast = median_ms(lambda: run("filter"), args.reps)
        auto = median_ms(lambda: run("auto"), args.reps)
        exact = median_ms(lambda: run("exact"), args.exact_reps, warm=1)
        idx_e, d2_e, _ = run("exact")
        idx_a, d2_a, cert = run("auto")
        same = torch.equal(idx_a, idx_e) and torch.equal(d2_a.view(torch.int32), d2_e.view(torch.int32))

        def cdist_topk():
            d = torch.cdist(q, x)
            d[torch.arange(B, device=dev), rows] = float("inf")
            return d.topk(K, dim=1, largest=False)

        if hn16 is None:
            hn16 = 0.5 * (bank.x16.float() ** 2).sum(dim=1) if n <= 1 << 18 else torch.cat(
                [0.5 * (bank.x16[s:s + (1 << 18)].float() ** 2).sum(dim=1) for s in range(0, n, 1 << 18)])
        q16 = q.half()

        def mm16_topk():
            a = hn16[None, :] - (q16 @ bank.x16.T).float()
            a[torch.arange(B, device=dev), rows] = float("inf")
            return a.topk(K, dim=1, largest=False)

        cd = median_ms(cdist_topk, max(2, args.reps // 2))
        mm = median_ms(mm16_topk, max(2, args.reps // 2))
        idx_m = mm16_topk().indices
        wrong = sum(set(idx_m[b].tolist()) != set(idx_e[b].tolist()) for b in range(B))
        idx_c = cdist_topk().indices
        wrong_c = sum(set(idx_c[b].tolist()) != set(idx_e[b].tolist()) for b in range(B))
        passes = (B + plan["queries_per_tile"] - 1) // plan["queries_per_tile"]
        say(f"{B:5d} | {fast:7.3f}  {passes * n * 2048 / fast / 1e9:5.2f} ({passes} pass{'es' if passes > 1 else ''}) | {auto:9.3f}  {int(cert.sum()):3d}/{B} "
            f"| {exact:8.1f} | {cd:13.3f} | {mm:12.3f}  {wrong:3d}/{B} | mode 0 == mode 1 bit for bit: {same}; cdist sets differ: {wrong_c}/{B}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
