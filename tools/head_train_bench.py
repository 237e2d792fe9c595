"""Times one training step of the geocell head (pg_head_train_loss + pg_head_train_update) against the same step in stock torch on the
same GPU, alternating, and says what bounds each launch.  `python tools/head_train_bench.py [--out FILE]`.

Shapes: B in {256, 1024} x C in {2076, 11000}, P = 4.  Event timing after warm-up, median of 30.  The torch step is what the
reference runs: nn.Linear on the panel mean, haversine + smoothing in torch ops as preprocessing/geo_utils.py and
preprocessing/utils.py write them, CrossEntropyLoss, backward, torch.optim.AdamW.  Bytes and FLOP are computed from the shapes:
  loss    FLOP 2 B 1024 C (the logits)        bytes 4 (B P 1024 + C 1024 + 3 B C + B 1024)   emb, W, logits written / read / g written
  update  FLOP 2 B 1024 C (the gradient)      bytes 4 (6 C 1024 + B C + B 1024)              W, m, v read and written; g, xbar
against 155 TFLOP/s (f32-input MFMA, measured peak) and the achievable HBM rate given with --hbm-tbs (default 5.0 TB/s)."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_TF = 155.0


def event_ms(fn, n):
    out = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def torch_haversine_matrix(x, y):
    """preprocessing/geo_utils.py:58-74 in torch ops: x (N,2), y (2,M) degrees -> (N,M) km"""
    x_rad, y_rad = torch.deg2rad(x), torch.deg2rad(y)
    delta = x_rad.unsqueeze(2) - y_rad
    p = torch.cos(x_rad[:, 1]).unsqueeze(1) * torch.cos(y_rad[1, :]).unsqueeze(0)
    a = torch.sin(delta[:, 1, :] / 2) ** 2 + p * torch.sin(delta[:, 0, :] / 2) ** 2
    return (2 * torch.arcsin(torch.sqrt(a)) * 6378137.0) / 1000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--hbm-tbs", type=float, default=5.0)
    args = ap.parse_args()
    from pigeon_amd import hip_ops, synthetic
    dev = "cuda"
    lines = [f"head_train_bench: {torch.cuda.get_device_name(0)}, median of {args.reps} after warm-up, P = 4, ms",
             "     B      C |   loss  update   both  fused-step |  torch-step | loss: GFLOP    MB  bound | update: GFLOP    MB  bound | ours/torch"]
    for B in (256, 1024):
        for Cn in (2076, 11000):
            g = torch.Generator().manual_seed(B + Cn)
            emb = (torch.randn((B, 4, 1024), generator=g) * 0.7 + 0.1).to(dev)
            cen = torch.from_numpy(synthetic.make_geocells(Cn, seed=0)).to(dev)
            labels = cen[torch.randint(0, Cn, (B,), generator=g).to(dev)] + 0.1
            W0, b0 = synthetic.make_head_weights(Cn, seed=0)
            W, b = W0.to(dev).clone(), b0.to(dev).clone()
            mW, vW, mb, vb = torch.zeros_like(W), torch.zeros_like(W), torch.zeros_like(b), torch.zeros_like(b)
            out = {"xbar": torch.empty((B, 1024), device=dev), "g": torch.empty((B, Cn), device=dev),
                   "loss_rows": torch.empty((B,), dtype=torch.float64, device=dev)}
            step = [0]

            def loss_fn():
                hip_ops.head_train_loss(emb, W, b, cen, labels_llh=labels, tau=65.0, grad_scale=1.0 / B, out=out)

            def update_fn():
                step[0] += 1
                hip_ops.head_train_update(out["g"], out["xbar"], W, b, mW, vW, mb, vb, step[0])

            def both_fn():
                loss_fn(); update_fn()

            lin = torch.nn.Linear(1024, Cn).to(dev)
            with torch.no_grad():
                lin.weight.copy_(W0); lin.bias.copy_(b0)
            opt = torch.optim.AdamW(lin.parameters(), lr=2e-5)
            ce = torch.nn.CrossEntropyLoss()
            cen_t = cen.t().contiguous()

            def torch_fn():
                opt.zero_grad(set_to_none=True)
                logits = lin(emb.mean(dim=1))
                d = torch_haversine_matrix(labels, cen_t)
                y = torch.exp(-(d - d.min(dim=-1, keepdim=True)[0]) / 65.0)
                y = torch.nan_to_num(y, nan=0.0, posinf=0.0, neginf=0.0)
                ce(logits, y.to(logits.dtype)).backward()
                opt.step()

            for fn in (both_fn, torch_fn, both_fn, torch_fn, both_fn, torch_fn):          # warm-up, alternating as the measurement does
                fn()
            torch.cuda.synchronize()
            ours, theirs = [], []
            for _ in range(args.reps):
                ours += event_ms(both_fn, 1); theirs += event_ms(torch_fn, 1)
            t_loss = statistics.median(event_ms(loss_fn, args.reps))
            t_upd = statistics.median(event_ms(update_fn, args.reps))
            t_both, t_torch = statistics.median(ours), statistics.median(theirs)
            flop = 2.0 * B * 1024 * Cn
            by_loss = 4.0 * (B * 4 * 1024 + Cn * 1024 + 3 * B * Cn + B * 1024)
            by_upd = 4.0 * (6 * Cn * 1024 + B * Cn + B * 1024)

            def bound(fl, by):
                t_f, t_b = fl / (PEAK_TF * 1e12), by / (args.hbm_tbs * 1e12)
                return ("MFMA" if t_f > t_b else "bytes") + f" {max(t_f, t_b) * 1e3:.3f}"

            lines.append(f"{B:6d} {Cn:6d} | {t_loss:6.3f}  {t_upd:6.3f} {t_loss + t_upd:6.3f}      {t_both:6.3f} |      {t_torch:6.3f} | "
                         f"{flop / 1e9:11.2f} {by_loss / 1e6:5.0f}  {bound(flop, by_loss):>11s} | {flop / 1e9:13.2f} {by_upd / 1e6:5.0f}  "
                         f"{bound(flop, by_upd):>11s} | {t_both / t_torch:.2f}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
