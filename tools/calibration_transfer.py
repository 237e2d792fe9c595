"""Does a calibration fitted on Gaussian pixels transfer to images?  (VERDICT r06 weak #2.)

The bias vector `pg_embedding_debias` subtracts is fitted on whatever images the calibration sees; the tests and the benchmark fit it on
seeded N(0,1) pixels.  This tool fits one bias on such pixels and one on PHOTO-LIKE images -- smooth seeded uint8 fields with a
natural-image-like 1/f^alpha amplitude spectrum and correlated colour channels, sent through pg_prep_forward like a photograph (there
are no photographs in the repository) -- and reports, on HELD-OUT images of each kind, the per-image RMS relative error of the fast
encoder against the exact one: raw, after the Gaussian-fitted bias, after the photo-fitted bias.  A measurement and a record
(profiles/), not a test.

    python tools/calibration_transfer.py [--layers 24] [--images 64] [-o profiles/r07/calibration_transfer.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def photo_like(n: int, size: int = 448, seed: int = 0, alpha: float = 1.1) -> np.ndarray:
    """(n, size, size, 3) uint8: a luminance field and two weaker chroma fields with amplitude spectrum 1/f^alpha (alpha ~ 1 is the
    classic natural-image figure), a vertical illumination gradient, per-image contrast and exposure; clipped to 0..255."""
    rng = np.random.default_rng(seed)
    fy, fx = np.meshgrid(np.fft.fftfreq(size), np.fft.rfftfreq(size), indexing="ij")
    f = np.sqrt(fy * fy + fx * fx)
    f[0, 0] = 1.0
    amp = 1.0 / f ** alpha
    amp[0, 0] = 0.0

    def field():
        spec = amp * (rng.standard_normal(amp.shape) + 1j * rng.standard_normal(amp.shape))
        x = np.fft.irfft2(spec, s=(size, size))
        return x / x.std()
    out = np.empty((n, size, size, 3), dtype=np.uint8)
    ramp = np.linspace(0.5, -0.5, size)[:, None]
    for i in range(n):
        lum = field() + rng.uniform(0.0, 1.0) * ramp * 2.0
        c1, c2 = field() * 0.35, field() * 0.25
        rgb = np.stack([lum + c1, lum - 0.5 * c1 + c2, lum - c1 - c2], axis=-1)
        img = rng.uniform(90, 150) + rng.uniform(35, 70) * rgb
        out[i] = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return out


def rel_rows(a, b):
    return (a - b).norm(dim=1) / b.norm(dim=1).clamp_min(1e-30)


def rms(x):
    return float(x.pow(2).mean().sqrt())


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--images", type=int, default=64, help="images per kind: the even ones fit the bias, the odd ones are held out")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("-o", "--output", default=os.path.join("profiles", "r07", "calibration_transfer.txt"))
    args = ap.parse_args(argv)
    from pigeon_amd.certainty import Certainty
    from pigeon_amd.clip_embedder import HipCLIPVisionModel, gpu_preprocess
    tower = HipCLIPVisionModel(seed=0, layers=args.layers).to("cuda")
    tower.enable_precise(True)
    n = args.images
    sets = {
        "gaussian": torch.randn((n, 3, 336, 336), generator=torch.Generator().manual_seed(1000 + args.seed)).to("cuda"),
        "photo-like": gpu_preprocess(torch.from_numpy(photo_like(n, seed=2000 + args.seed)), "cuda", torch.float32),
    }
    fast, exact, bias = {}, {}, {}
    with torch.no_grad():
        for k, px in sets.items():
            fast[k], exact[k] = tower.embed(px), tower.embed_precise(px)
            rel = (fast[k] - exact[k]) / exact[k].norm(dim=1, keepdim=True)
            bias[k] = rel[0::2].mean(dim=0)
    lines = [f"calibration transfer: seeded random-init ViT-L/14-336, {args.layers} layers, fingerprint {tower.fingerprint()}, "
             f"{n} images per kind (even: fit, odd: held out), seed {args.seed}",
             f"pixel statistics after preprocessing: " + "; ".join(f"{k} mean {float(px.float().mean()):+.3f} std {float(px.float().std()):.3f}"
                                                                   for k, px in sets.items()),
             f"bias norms: " + ", ".join(f"{k} {float(b.norm()):.3e}" for k, b in bias.items())
             + f"; cosine between them {float(torch.dot(bias['gaussian'], bias['photo-like']) / (bias['gaussian'].norm() * bias['photo-like'].norm())):.4f}"
             + f"; |difference| {float((bias['gaussian'] - bias['photo-like']).norm()):.3e}",
             "held-out per-image RMS relative error of the fast encoder against the exact one:",
             f"  {'held-out set':<12} {'raw':>10} {'gaussian bias':>14} {'photo-like bias':>16}"]
    for k in sets:
        f, e = fast[k][1::2], exact[k][1::2]
        lines.append(f"  {k:<12} {rms(rel_rows(f, e)):>10.3e} {rms(rel_rows(Certainty.apply_bias(f, bias['gaussian']), e)):>14.3e} "
                     f"{rms(rel_rows(Certainty.apply_bias(f, bias['photo-like']), e)):>16.3e}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(args.output)), exist_ok=True)
    with open(args.output, "w") as fh:
        fh.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
