"""Patch attribution, read: what `SuperGuessr.attribute` returns turned into grids, shares, overlays and JSON.

`SuperGuessr.attribute` writes each geocell logit (or the difference of two) as an exact sum over the tokens of the views
(pg_token_attribution, csrc/attribution.hip):  maps (B,P,577,K), with  maps.sum((1,2)) + offset == logits.  Token 0 of a view is the
class token; token 1 + 24 y + x is the 14 x 14 patch in row y, column x of the 336 x 336 crop the encoder saw.  This module only
re-arranges those numbers -- it runs on the host, on torch tensors or numpy arrays, and imports neither torch.cuda nor the HIP library
until the command line builds a model:

    python -m pigeon_amd.explain [--head H] [--geocells G] [--layers L] [--tier fast|exact] [--against runner_up|none] -o DIR \\
        view1 [view2 view3 view4]

writes DIR/view1.png .. view4.png (the crop the model saw with the map of the first cell laid over it) and DIR/attribution.json.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Sequence

import numpy as np

TOKENS, GRID, PATCH, CROP = 577, 24, 14, 336


def _np(x) -> np.ndarray:
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.asarray(x)


def _maps(maps) -> np.ndarray:
    m = _np(maps)
    if m.ndim != 4 or m.shape[2] != TOKENS:
        raise ValueError(f"maps must be (B,P,{TOKENS},K), got {m.shape}")
    return m


def patch_grid(maps):
    """maps (B,P,577,K) -> (grid (B,P,24,24,K), cls (B,P,K)): grid[b,p,y,x,k] = maps[b,p,1 + 24 y + x,k], cls = token 0."""
    m = _maps(maps)
    B, P, _, K = m.shape
    return m[:, :, 1:, :].reshape(B, P, GRID, GRID, K), m[:, :, 0, :]


def view_share(maps):
    """maps (B,P,577,K) -> (B,P,K): what each view adds to the logit (difference), class token included; summed in float64."""
    return _maps(maps).astype(np.float64).sum(axis=2)


def overlay(crop_u8, grid, alpha: float = 0.55, scale: float = None):
    """The crop the model saw with one map laid over it -> PIL RGB image of the crop's size.  crop_u8 (336,336,3) uint8 (the bytes
    `gpu_preprocess(..., out_dtype=torch.uint8)` writes, moved to HWC); grid (24,24): red where a patch speaks for the cell, blue
    where it speaks against it, opacity proportional to |value| / scale (default: the grid's largest magnitude)."""
    from PIL import Image
    crop = _np(crop_u8)
    g = _np(grid).astype(np.float64)
    if crop.ndim != 3 or crop.shape[2] != 3 or crop.dtype != np.uint8:
        raise ValueError(f"crop_u8 must be uint8 (H,W,3), got {crop.dtype} {crop.shape}")
    if g.shape != (GRID, GRID):
        raise ValueError(f"grid must be ({GRID},{GRID}), got {g.shape}")
    h, w = crop.shape[:2]
    top = float(np.nanmax(np.abs(g))) if scale is None else float(scale)
    g = np.nan_to_num(g / top if top > 0 else np.zeros_like(g))
    big = np.asarray(Image.fromarray(g.astype(np.float32), mode="F").resize((w, h), Image.BILINEAR), dtype=np.float64).clip(-1.0, 1.0)
    colour = np.where(big[..., None] >= 0, np.array([220.0, 30.0, 30.0]), np.array([30.0, 60.0, 220.0]))
    a = (alpha * np.abs(big))[..., None]
    return Image.fromarray(np.rint((1.0 - a) * crop.astype(np.float64) + a * colour).clip(0, 255).astype(np.uint8), mode="RGB")


def attribution_json(att, index: int = 0) -> Dict:
    """Sample `index` of an `Attribution` as plain JSON types: cells, against, logits, offset (K,), view_share and cls_share (P,K),
    grids (P,24,24,K), token_sum (K,) = the maps summed in float64 -- token_sum + offset reproduces logits."""
    maps = _maps(att.maps)[index:index + 1]
    grid, cls = patch_grid(maps)
    share = view_share(maps)
    return {"cells": [int(c) for c in _np(att.cells)[index]], "against": int(_np(att.against)[index]),
            "logits": [float(v) for v in _np(att.logits)[index]], "offset": [float(v) for v in _np(att.offset)[index]],
            "token_sum": [float(v) for v in share[0].sum(axis=0)],
            "view_share": [[float(v) for v in row] for row in share[0]], "cls_share": [[float(v) for v in row] for row in cls[0]],
            "grids": grid[0].astype(np.float64).tolist()}


def write_report(out_dir: str, att, crops_u8: Sequence, index: int = 0, column: int = 0) -> Dict:
    """out_dir/view{i}.png (i = 1..P: crop i with the map of cell `column` over it, one colour scale for all views) and
    out_dir/attribution.json.  crops_u8: P arrays (336,336,3) uint8.  Returns the JSON object."""
    os.makedirs(out_dir, exist_ok=True)
    obj = attribution_json(att, index)
    grids = np.asarray(obj["grids"])                                  # (P,24,24,K)
    finite = np.abs(grids[..., column][np.isfinite(grids[..., column])])
    scale = float(finite.max()) if finite.size else 0.0
    for p, crop in enumerate(crops_u8):
        overlay(crop, grids[p, :, :, column], scale=scale).save(os.path.join(out_dir, f"view{p + 1}.png"))
    with open(os.path.join(out_dir, "attribution.json"), "w") as f:
        json.dump(obj, f)
    return obj


def _arg_parser():
    import argparse
    ap = argparse.ArgumentParser(prog="python -m pigeon_amd.explain", description="Which patches of the four views speak for the "
                                 "model's cell (and against its runner-up): overlays and the numbers behind them.")
    ap.add_argument("views", nargs="+", help="1 or 4 image files (one view is used four times, as the server does)")
    ap.add_argument("-o", "--out", required=True, metavar="DIR")
    ap.add_argument("--head", default=None, help="SuperGuessr checkpoint (torch.save state dict); random init if omitted")
    ap.add_argument("--geocells", default=None)
    ap.add_argument("--layers", type=int, default=24, help="layers of the seeded random tower used when no pretrained one is found")
    ap.add_argument("--tier", choices=("fast", "exact"), default="fast")
    ap.add_argument("--against", choices=("runner_up", "none"), default="runner_up")
    ap.add_argument("-k", type=int, default=1, help="explain the top-k cells (the overlays show the first)")
    return ap


def main(argv=None) -> Dict:
    ap = _arg_parser()
    args = ap.parse_args(argv)
    if len(args.views) not in (1, 4):
        ap.error(f"1 or 4 views expected, got {len(args.views)}")
    import torch
    from PIL import Image
    from .clip_embedder import HipCLIPVisionModel, load_pretrained_clip
    from .preprocess import gpu_preprocess
    from .super_guessr import SuperGuessr
    views = [Image.open(v).convert("RGB") for v in args.views]
    views = views * 4 if len(views) == 1 else views
    try:
        base = load_pretrained_clip()
    except RuntimeError as why:
        print(f"[explain] no pretrained tower ({why}); using a seeded random-init ViT-L/14-336 with {args.layers} layers")
        base = HipCLIPVisionModel(seed=0, layers=args.layers)
    kw = {"geocell_path": args.geocells} if args.geocells else {}
    model = SuperGuessr(base, panorama=True, serving=True, freeze_base=True, **kw).to("cuda").eval()
    if args.head:
        model.load_state(args.head)
    crops = gpu_preprocess(views, "cuda", torch.uint8)                # (4,3,336,336) uint8: the bytes the encoder reads
    att = model.attribute(pixel_bytes=crops.reshape(1, 12, CROP, CROP), k=args.k,
                          against=None if args.against == "none" else "runner_up", tier=args.tier)
    obj = write_report(args.out, att, crops.permute(0, 2, 3, 1).cpu().numpy())
    print(f"[explain] cells {obj['cells']} against {obj['against']}: logits {obj['logits']} = tokens {obj['token_sum']} + offset "
          f"{obj['offset']}; written to {args.out}")
    return obj


if __name__ == "__main__":
    main()
