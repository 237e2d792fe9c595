"""Measurements around pg_aux_heads_forward (csrc/aux_heads.hip); none of them is a pass/fail threshold.

    python tools/aux_heads_probe.py kernel [--launches 400]
        device-event time per launch, after a warm-up, at B = 1 and B = 128 rows (P = 4, A = 46) of
          * pg_aux_heads_forward,
          * pg_head_forward on the same 46 x 1024 weight (k = 1),
          * the eight-launch composition the kernel replaces: pg_head_forward on the regression, climate and month rows (two
            launches each) + pg_head_certainty on the climate and the month rows.
    python tools/aux_heads_probe.py share [--panoramas 2048] [--layers 24]
        the benchmark's tower and head (bench.py: synthetic.make_vit_weights(seed 0), 10 000 geocells centred on the mean embedding,
        the 1M-prototype bank) with default-init auxiliary layers: the share of panoramas that ONLY the climate / month tolerance
        sends to the exact tier, next to the share the geocell head and the refiner send; and the time per 128-panorama step of
        PanoramaPipeline with multi_task=False and multi_task=True on the same batches.
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, launches, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(launches):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / launches                # microseconds per call


def kernel(args):
    from pigeon_amd import hip_ops as ops, synthetic as syn
    dev = "cuda"
    g = torch.Generator().manual_seed(0)
    sd = syn.make_aux_head_weights(seed=0)
    names = ("multi_task_head", "climate_layer", "month_layer")
    W = torch.cat([sd[f"{n}.weight"] for n in names]).to(dev).contiguous()
    b = torch.cat([sd[f"{n}.bias"] for n in names]).to(dev).contiguous()
    parts = [(W[s:e].contiguous(), b[s:e].contiguous()) for s, e in ((0, 6), (6, 34), (34, 46))]
    cent = torch.from_numpy(syn.make_geocells(46, seed=1)).to(dev)
    wst = torch.tensor([1.0, 0.0], device=dev)
    print(f"{'B':>4} {'aux_heads us':>13} {'head_forward(A=46) us':>22} {'8-launch composition us':>24}")
    for B in (1, 128):
        emb = torch.randn((B, 4, 1024), generator=g).to(dev)

        def aux():
            ops.aux_heads_forward(emb, W, b, 6, 28, 12)

        def head():
            ops.head_forward(emb, W, b, cent, 1)

        def composed():
            for i, (Wp, bp) in enumerate(parts):
                n = Wp.shape[0]
                o = ops.head_forward(emb, Wp, bp, cent[:n], n if i else 1)
                if i:
                    ops.head_certainty(o["logits"], emb, Wp, o["topk_indices"], None, wst)
        t = [_time(f, args.launches) for f in (aux, head, composed)]
        print(f"{B:>4} {t[0]:>13.2f} {t[1]:>22.2f} {t[2]:>24.2f}")
    print(f"({args.launches} calls per point after 20 warm-up calls, device events around the loop: the figures include the host's launch "
          f"path -- output allocation and the ctypes call -- wherever the GPU waits for it)")


def share(args):
    import numpy as np
    from pigeon_amd import hip_ops as ops, synthetic as syn
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    from pigeon_amd.deferred import LocalComm
    from pigeon_amd.evaluate import PanoramaPipeline
    from pigeon_amd.proto_refiner import ProtoRefiner
    from pigeon_amd.super_guessr import SuperGuessr
    dev = torch.device("cuda:0")
    cells, per = 10000, 128
    base = HipCLIPVisionModel(syn.make_vit_weights(seed=0, layers=args.layers), layers=args.layers)
    geo_csv = os.path.join(tempfile.mkdtemp(prefix="pigeon_probe_"), "geocells.csv")
    syn.write_geocell_csv(geo_csv, syn.make_geocells(cells, seed=0))
    W, b = syn.make_head_weights(cells, seed=0)
    models = {}
    for mt in (False, True):
        with contextlib.redirect_stdout(io.StringIO()):
            m = SuperGuessr(base, panorama=True, freeze_base=True, num_candidates=5, geocell_path=geo_csv, exact_top1=True,
                            margin_autocalibrate=False, multi_task=mt)
        with torch.no_grad():
            m.cell_layer.weight.copy_(W); m.cell_layer.bias.copy_(b)
            if mt:
                m.load_state_dict(syn.make_aux_head_weights(seed=0), strict=False)
        models[mt] = m.to(dev).eval()
    bank = syn.make_bank_device(cells, 100, seed=2, device=str(dev))
    refiner = ProtoRefiner(topk=5, max_refinement=1000, temperature=1.6, bank=bank, device=str(dev)).eval()
    steps = args.panoramas // per
    gen = torch.Generator(device=dev).manual_seed(1234)
    batches = [torch.randn((per, 12, 336, 336), generator=gen, device=dev) for _ in range(min(steps, 4))]
    m = models[True]
    with torch.no_grad():                                     # the benchmark's head: centred on the mean embedding, logit sigma 4
        pe = m.encode_head(batches[0])["embedding"].mean(dim=1)
        center = pe.mean(dim=0)
        sig = float(((pe - center) @ m.cell_layer.weight.data.t()).std())
        sc = float(2.0 ** np.round(np.log2(4.0 / max(sig, 1e-12))))
        for mm in models.values():
            mm.cell_layer.weight.mul_(sc)
            mm.cell_layer.bias.copy_(b.to(dev) - mm.cell_layer.weight.data @ center)
    cal = torch.randn((per, 12, 336, 336), generator=torch.Generator(device=dev).manual_seed(4321), device=dev)
    m.calibrate_certainty(cal, max_samples=per)
    del cal
    models[False].certainty = m.certainty                     # the same measured error, the same threshold
    thr = m.certainty.threshold(False)
    # ---- who flags what, on the fast pass (fresh pixels per step, as many as asked for)
    n = n_geo_ref = n_aux = n_aux_only = 0
    by_code = {}
    gen = torch.Generator(device=dev).manual_seed(1234)
    with torch.no_grad():
        for s in range(steps):
            px = torch.randn((per, 12, 336, 336), generator=gen, device=dev)
            st = m.encode_head(px)
            geo, _, _, _ = ops.head_certainty(st["logits"], st["head_in"], m.cell_layer.weight.data, st["topk_indices"], st["drift"], st["wstats"])
            _, _, rtol, _, _ = refiner.forward_certain(st["embedding"], st["preds_LLH"], st["topk_indices"], st["topk_values"],
                                                       m.cell_layer.weight.data, st["wstats"], st["drift"])
            assert torch.equal(st["tol"], torch.minimum(geo, st["aux_tol"]))
            f_gr = ~(geo > thr) | ~(rtol > thr)
            f_aux = ~(st["aux_tol"] > thr)
            n += per; n_geo_ref += int(f_gr.sum()); n_aux += int(f_aux.sum()); n_aux_only += int((f_aux & ~f_gr).sum())
            for c in st["aux_code"][f_aux & ~f_gr].tolist():
                by_code["climate" if c < 101 else "month"] = by_code.get("climate" if c < 101 else "month", 0) + 1
    print(f"{n} panoramas, threshold {thr:.3g} (kappa {m.certainty.kappa} x calibrated error {m.certainty.rel_tol:.3g}):")
    print(f"  flagged by the geocell head or the refiner : {n_geo_ref} ({100.0 * n_geo_ref / n:.2f} %)")
    print(f"  flagged by the climate / month tolerance   : {n_aux} ({100.0 * n_aux / n:.2f} %)")
    print(f"  ... and by nothing else (the added share)  : {n_aux_only} ({100.0 * n_aux_only / n:.3f} %)  {by_code}")
    # ---- what it costs: the same batches through the pipeline, without and with the auxiliary heads
    for mt in (False, True):
        pipe = PanoramaPipeline(models[mt], refiner, LocalComm())
        idx = torch.arange(per, device=dev)
        for i in range(3):
            pipe.submit(batches[i % len(batches)], idx)
        pipe.flush()
        torch.cuda.synchronize()
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        done = []
        for i in range(steps):
            done += pipe.submit(batches[i % len(batches)], idx)
        done += pipe.flush()
        e.record()
        e.synchronize()
        ex = sum(int(r["exact"].sum()) for r in done)
        print(f"  multi_task={mt!s:5}: {a.elapsed_time(e) / steps:8.2f} ms per step of {per} panoramas over {steps} steps; "
              f"{ex} rows re-encoded ({100.0 * ex / (steps * per):.2f} %), {len(pipe.engine.flush_log)} exact passes")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "share"])
    ap.add_argument("--launches", type=int, default=400)
    ap.add_argument("--panoramas", type=int, default=2048)
    ap.add_argument("--layers", type=int, default=24)
    a = ap.parse_args()
    (kernel if a.what == "kernel" else share)(a)
