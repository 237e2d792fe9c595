"""A/B of two library builds on the kernels that run the 32 x 64 slab epilogue (profiles/r07/gemm_shared_epilogue_ab.txt): the four
model GEMM shapes through gemm_tail (variant 70, 512 rows) and through gemm_mid (variant 71, 4 x 577 and 16 x 577 rows).
   PIGEON_HIP_LIB=<library> python tools/slab_epilogue_ab.py LABEL >> LOG    # one arm, a fresh process: prints `AB {json}`, median us per launch
   python tools/slab_epilogue_ab.py --table LOG                              # arms labelled parent1 new1 parent2 new2 -> the table
Run the arms alternating parent / new / parent / new in one session on one machine.  Margin: the spread of the parent's two arms; the
median of the new arms (of two arms: their mean) may exceed the parent's by no more."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WARMUP, SAMPLES, BATCH = 200, 21, 500
SHAPES = {"qkv": (3072, 1024, "qkv_ln"), "out": (1024, 1024, "resid_stat"), "fc1": (4096, 1024, "gelu_ln"), "fc2": (1024, 4096, "resid_stat")}
CASES = [(70, 512), (71, 4 * 577), (71, 16 * 577)]


def arm(label):
    import torch
    from pigeon_amd import _lib, hip_ops
    dev, dt = "cuda", torch.float16
    res = {"label": label}
    g = torch.Generator(device=dev).manual_seed(1)
    for V, M in CASES:
        for name, (N, K, kind) in SHAPES.items():
            A = torch.randn((M, K), generator=g, device=dev).to(dt)
            W = (torch.randn((N, K), generator=g, device=dev) * 0.03).to(dt)
            bias = torch.randn(N, generator=g, device=dev) * 0.1
            cs = torch.randn(N, generator=g, device=dev) * 0.1
            rs = torch.rand((M, 2), generator=g, device=dev) + 0.5
            X = torch.zeros((M + 384, N), device=dev)[:M] if kind == "resid_stat" else None   # + the slack the residual epilogue may read

            def run():
                if kind == "resid_stat":
                    return hip_ops.gemm16_resid_stat(A, W, bias, X, variant=V)
                return hip_ops.gemm16_ln(A, W, bias, cs, rs, _lib.EPI_QKV_LN if kind == "qkv_ln" else _lib.EPI_GELU_LN, qscale=0.125, qcols=1024, variant=V)

            for _ in range(WARMUP):
                run()
            torch.cuda.synchronize()
            ts = []
            for _ in range(SAMPLES):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(BATCH):
                    run()
                b.record(); torch.cuda.synchronize()
                ts.append(a.elapsed_time(b) * 1000 / BATCH)
            ts.sort()
            res[f"v{V}_{name}_M{M}"] = round(ts[len(ts) // 2], 3)
            del A, W, X
    print("AB " + json.dumps(res), flush=True)


def table(log):
    arms = [json.loads(l[3:]) for l in open(log) if l.startswith("AB ")]
    par = [a for a in arms if a["label"].startswith("parent")]
    new = [a for a in arms if a["label"].startswith("new")]
    assert len(par) == 2 and len(new) == 2, [a["label"] for a in arms]
    print(f"# median us per launch (device events, {WARMUP} warm-up launches, {SAMPLES} samples of {BATCH} launches), fp16, arms in the order parent / new / parent / new,")
    print("# each a fresh process.  spread = |parent1 - parent2|; verdict: mean(new) - mean(parent) <= spread.")
    print(f"{'case':22s} {'parent1':>9s} {'new1':>9s} {'parent2':>9s} {'new2':>9s} {'spread':>8s} {'new-parent':>11s}  verdict")
    for k in par[0]:
        if k == "label":
            continue
        p1, p2, n1, n2 = par[0][k], par[1][k], new[0][k], new[1][k]
        spread, d = abs(p1 - p2), (n1 + n2) / 2 - (p1 + p2) / 2
        print(f"{k:22s} {p1:9.3f} {n1:9.3f} {p2:9.3f} {n2:9.3f} {spread:8.3f} {d:+11.3f}  {'ok' if d <= spread else 'SLOWER'}")


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--table":
        table(sys.argv[2])
    elif len(sys.argv) == 2:
        arm(sys.argv[1])
    else:
        sys.exit(__doc__)
