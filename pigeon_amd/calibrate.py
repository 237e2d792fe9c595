"""An explicit calibration run: measure the 16-bit encoder against the exact one on a fixed set of samples and write the calibration
file (pigeon_amd/certainty.py: bias vector, certainty tolerance, exact-encoder verdict; keyed by the weight fingerprint).

    python -m pigeon_amd.calibrate --base CKPT|random [--layers L] (--synthetic N --seed S | --images DIR) [--panels 4] -o FILE

Every rank of a later job, the embed path (`run.py embed --calibration FILE`), the query path (`run.py evaluate --calibration FILE`)
and the server (`python -m pigeon_amd.serve --calibration FILE`) then load the SAME measurement instead of each taking its own inside
its first forward: same weights + same file -> same embedding for the same image, in every process.

`--panels` is the number of images per sample the tolerance is measured on: 4 for the panorama model (the head sees the mean of four
panel embeddings), 1 for single images.  `SuperGuessr.load_calibration` refuses a file whose `panels` is not its own; `CLIPEmbedding`
takes any (the bias is per image).  Calibrate on inputs like the ones the model will see ("which inputs to calibrate on").
"""
from __future__ import annotations

import argparse
import os
import sys


def _arg_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog='python -m pigeon_amd.calibrate', description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--base', required=True, help='checkpoint holding the vision tower (base_model.* / vision_model.* / flat names), or "random" '
                                                  'for the seeded random-init ViT-L/14-336')
    ap.add_argument('--layers', type=int, default=24, help='encoder layers of a "random" tower')
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--synthetic', type=int, default=0, metavar='N', help='N seeded samples of Gaussian pixels')
    src.add_argument('--images', default=None, metavar='DIR', help='directory of images (sorted by name; consecutive --panels images form a sample)')
    ap.add_argument('--seed', type=int, default=0, help='seed of the synthetic samples')
    ap.add_argument('--panels', type=int, default=4, help='images per sample (4: panoramas, 1: single images)')
    ap.add_argument('--max-samples', type=int, default=32, help='samples measured at most')
    ap.add_argument('-o', '--output', required=True, metavar='FILE')
    return ap


def load_tower(base: str, layers: int = 24):
    """The vision tower `--base` names, as run.py resolves it."""
    import torch
    from .clip_embedder import HipCLIPVisionModel
    if base == 'random':
        return HipCLIPVisionModel(seed=0, layers=layers)
    if not os.path.exists(base):
        raise FileNotFoundError(base)
    sd = torch.load(base, map_location='cpu')
    sd = {('.'.join(k.split('.')[1:]) if 'base_model' in k.split('.')[0] else k): v for k, v in sd.items()}
    return HipCLIPVisionModel(sd)


def synthetic_pixels(n_samples: int, panels: int, seed: int):
    import torch
    g = torch.Generator().manual_seed(int(seed))
    return torch.randn((n_samples * panels, 3, 336, 336), generator=g)


def directory_pixels(path: str, panels: int, max_samples: int, device='cuda'):
    import torch
    from PIL import Image
    from .clip_embedder import gpu_preprocess
    names = sorted(f for f in os.listdir(path) if f.lower().endswith(('.jpg', '.jpeg', '.png', '.bmp', '.webp')))
    names = names[:(min(len(names) // panels, max_samples)) * panels]
    if not names:
        raise ValueError(f'{path!r} holds fewer than {panels} images')
    return gpu_preprocess([Image.open(os.path.join(path, f)).convert('RGB') for f in names], device, out_dtype=torch.float32)


def calibrate_tower(tower, pixels, panels: int, max_samples: int = 32):
    """`pixels` (n * panels, 3, 336, 336) through the fast and the exact encoder -> a calibrated `Certainty` (what
    `SuperGuessr.calibrate_certainty` measures, without a head)."""
    import torch
    from .certainty import Certainty
    n = min(int(max_samples), int(pixels.shape[0]) // panels)
    if n < 8:
        raise ValueError(f'{n} samples: a calibration needs at least 8 (half of them fit the bias, the other half measure what is left)')
    px = pixels[:n * panels].to('cuda')
    with torch.no_grad():
        fast_i, exact_i = tower.embed(px), tower.embed_precise(px)
    c = Certainty()
    c.calibrate(fast_i.reshape((n, panels, -1)).mean(dim=1), exact_i.reshape((n, panels, -1)).mean(dim=1), fast_images=fast_i, exact_images=exact_i)
    return c


def main(argv=None) -> int:
    ap = _arg_parser()
    args = ap.parse_args(argv)
    if args.panels < 1:
        ap.error('--panels must be at least 1')
    import torch
    tower = load_tower(args.base, args.layers).to('cuda')
    if args.images:
        pixels = directory_pixels(args.images, args.panels, args.max_samples)
        source = f'pigeon_amd.calibrate --images {os.path.basename(os.path.normpath(args.images))}'
    else:
        pixels = synthetic_pixels(min(args.synthetic, args.max_samples), args.panels, args.seed)
        source = f'pigeon_amd.calibrate --synthetic {args.synthetic} --seed {args.seed}'
    c = calibrate_tower(tower, pixels, args.panels, args.max_samples)
    meta = tower.encoder_config()
    meta['source'] = source
    fp = tower.fingerprint()
    c.save(args.output, fp, args.panels, meta)
    torch.cuda.synchronize()
    print(f'fingerprint {fp}  ({meta["layers"]} layers, {meta["mma_dtype"]}, ln_fold {meta["ln_fold"]})')
    print(c.describe())
    print(f'Calibration written to {args.output}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
