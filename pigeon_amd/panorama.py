"""Equirectangular panoramas -> the perspective views the model predicts from, rendered on the GPU (pg_equirect_* in
include/pigeon_hip.h) straight into the packed buffer the ragged resize reads.

A panorama from a 360-degree camera is ONE equirectangular image; `SuperGuessr(panorama=True)`, `serve` and `run.py evaluate` take four
90-degree views at compass headings 0 / 90 / 180 / 270.  This module defines which four views those are ("Equirectangular
panoramas in": one integer result per pixel) and renders them: file bytes -> JPEG kernels -> gnomonic kernel -> resize, no host
round trip.  The host computes only the rotation and the focal factor of every view, in float64.

The default view size is round(W / pi) clamped to [336, 4096]: there the view samples the source 1:1 at its centre and finer
everywhere else, so the (bilinear) gnomonic step never minifies and all downsampling is left to the Pillow-exact antialiased resize
behind it.  A smaller `size` is allowed and may alias.

`python -m pigeon_amd.panorama pano.jpg -o views/` writes view1.png .. view4.png: what the model will see."""
from __future__ import annotations

import math
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, hip_ops
from .jpeg import DecodedImages, EncodedImages, decode_chunks
from .packing import PackedImages, as_rgb_array, check_rgb_u8, chunk_by_bytes, pack_into, packed_layout

HEADINGS = (0.0, 90.0, 180.0, 270.0)
MIN_VIEW, MAX_VIEW = 336, 4096
MAX_BYTES = 256 << 20                 # packed bytes per call, of the sources and of the views (preprocess.RAGGED_MAX_BYTES)


def view_rotation(yaw: float, pitch: float) -> np.ndarray:
    """R = Ry(yaw) . Rx(pitch), camera -> panorama, (3,3) float64; degrees.  Axes x right, y DOWN, z forward; yaw positive to the right
    (clockwise seen from above), pitch positive upwards."""
    yw, pt = np.deg2rad(np.float64(yaw)), np.deg2rad(np.float64(pitch))
    C, Sn, c, s = np.cos(yw), np.sin(yw), np.cos(pt), np.sin(pt)
    return np.array([[C, Sn * s, Sn * c], [0.0, c, -s], [-Sn, C * s, C * c]], dtype=np.float64)


def inv_focal(fov: float, size: int) -> float:
    """tan(fov / 2) / (size / 2): the step of one view pixel on the plane z = 1; degrees."""
    if not (0.0 < float(fov) < 180.0):
        raise ValueError(f"fov must lie in (0, 180) degrees, got {fov}")
    return float(np.tan(np.deg2rad(np.float64(fov)) / 2) / (np.float64(size) / 2))


def default_view_size(w: int) -> int:
    """round(W / pi) clamped to [336, 4096]: 1:1 with the source at the view's centre, finer elsewhere -- never minifying."""
    return int(min(max(round(int(w) / math.pi), MIN_VIEW), MAX_VIEW))


def view_list(sizes: Sequence[Tuple[int, int]], headings=HEADINGS, pitch: float = 0.0, fov: float = 90.0, size: Optional[int] = None,
              centre_heading=0.0, first: int = 0) -> List[tuple]:
    """The views of panoramas of the given (height, width), panorama-major, as hip_ops.equirect_plan takes them.  `centre_heading`: the
    compass heading of the source's centre column, one number or one per panorama; the view's yaw is heading - centre_heading.
    `first`: index of sizes[0] in `centre_heading` where that is a sequence."""
    views = []
    for k, (h, w) in enumerate(sizes):
        s = default_view_size(w) if size is None else int(size)
        ch = float(centre_heading[first + k]) if hasattr(centre_heading, "__len__") else float(centre_heading)
        f = inv_focal(fov, s)
        for hd in headings:
            views.append((int(h), int(w), k, s, view_rotation(float(hd) - ch, pitch), f))
    return views


def _source_chunks(panoramas, dev) -> Iterator[Tuple[torch.Tensor, List[Tuple[int, int]], List[int]]]:
    """(device buffer, sizes, byte offsets) over consecutive runs of the panoramas of at most MAX_BYTES packed bytes each."""
    if isinstance(panoramas, EncodedImages):
        for dec in decode_chunks(panoramas, dev, MAX_BYTES):
            yield dec.packed, list(dec.plan.sizes), [int(it.src_off) for it in dec.plan.items]
        return
    if isinstance(panoramas, PackedImages):
        data = panoramas.data
        if not torch.is_tensor(data) or data.dtype != torch.uint8 or data.dim() != 1 or data.is_cuda or not data.is_contiguous():
            raise ValueError("equirect_views: PackedImages.data must be a contiguous 1-D uint8 host tensor")
        sizes = panoramas.size_list()
        offs, total = packed_layout(sizes)
        if data.numel() != total:
            raise ValueError(f"equirect_views: PackedImages holds {data.numel()} bytes, its {len(sizes)} sizes need {total}")
        if sizes:
            yield data.to(dev), sizes, offs
        return
    if hasattr(panoramas, "convert") or ((isinstance(panoramas, np.ndarray) or torch.is_tensor(panoramas)) and panoramas.ndim == 3):
        panoramas = [panoramas]
    arrs = [as_rgb_array(p.cpu() if torch.is_tensor(p) else p) for p in panoramas]
    for a in arrs:
        check_rgb_u8(a)
    from . import preprocess                                       # host panoramas travel through the ragged path's pinned staging buffer
    for lo, hi in chunk_by_bytes([a.shape[:2] for a in arrs], MAX_BYTES):
        sizes = [tuple(int(v) for v in a.shape[:2]) for a in arrs[lo:hi]]
        offs, total = packed_layout(sizes)
        with preprocess._PREP_LOCK, torch.cuda.device(dev):          # "fill the buffer ... copy queued" is one caller's at a time
            staging = preprocess._staging(dev)
            stage = staging.take(total)
            pack_into(arrs[lo:hi], offs, stage.numpy())
            on_dev = stage.to(dev, non_blocking=True)
            staging.copied()
        yield on_dev, sizes, offs


def equirect_view_chunks(panoramas, headings=HEADINGS, pitch: float = 0.0, fov: float = 90.0, size: Optional[int] = None,
                         centre_heading=0.0, device="cuda", max_bytes: Optional[int] = MAX_BYTES) -> Iterator[DecodedImages]:
    """Generator of DecodedImages (packed DEVICE buffer of views + its RaggedPlan) over consecutive runs of the views, panorama-major:
    the sources go to the device in runs of at most MAX_BYTES packed bytes, the views of one run of sources are rendered in runs of
    at most `max_bytes` (None: one run per run of sources)."""
    dev = hip_ops.indexed_device(device)
    _lib.require_gpu()
    headings = [float(h) for h in headings]
    if not headings:
        raise ValueError("equirect_views: no headings")
    done = 0
    for src, sizes, offs in _source_chunks(panoramas, dev):
        views = view_list(sizes, headings, pitch, fov, size, centre_heading, first=done)
        done += len(sizes)
        vs = [(v[3], v[3]) for v in views]
        for lo, hi in ([(0, len(views))] if max_bytes is None else chunk_by_bytes(vs, max_bytes)):
            plan = hip_ops.equirect_plan(views[lo:hi], offs)
            yield DecodedImages(hip_ops.equirect_forward(src, plan), plan.prep, [])


def equirect_views(panoramas, headings=HEADINGS, pitch: float = 0.0, fov: float = 90.0, size: Optional[int] = None,
                   centre_heading=0.0, device="cuda") -> DecodedImages:
    """`panoramas`: an EncodedImages (files as bytes, decoded on the GPU), a PackedImages, one raw uint8 (H,W,3) array, or a list of
    arrays / PIL images -- equirectangular, any H and W.  Returns the views of all of them, panorama-major (panorama 0's headings,
    then panorama 1's, ...), as one DecodedImages: the packed DEVICE buffer with the resize's descriptors in its head and its plan,
    which `gpu_preprocess` takes as it is.  The sources must fit one run (256 MiB of packed bytes); `equirect_view_chunks` and
    `panorama_pixels` take any number."""
    chunks = list(equirect_view_chunks(panoramas, headings, pitch, fov, size, centre_heading, device, None))
    if len(chunks) > 1:
        raise ValueError(f"equirect_views: the panoramas need {len(chunks)} runs of {MAX_BYTES} bytes; use equirect_view_chunks or panorama_pixels")
    if not chunks:
        dev = hip_ops.indexed_device(device)
        return DecodedImages(torch.empty(0, dtype=torch.uint8, device=dev), hip_ops.ragged_plan([]), [])
    return chunks[0]


def panorama_pixels(panoramas, device="cuda", out_dtype: torch.dtype = torch.float32, **view_kw) -> torch.Tensor:
    """Panoramas -> (N * len(headings), 3, 336, 336) pixel_values on the device, panorama-major: the views rendered and resized run by
    run.  `.view(N, 12, 336, 336)` of the default four is the `panorama=True` input of SuperGuessr."""
    from .preprocess import gpu_preprocess
    dev = hip_ops.indexed_device(device)
    outs = [gpu_preprocess(dec, dev, out_dtype) for dec in equirect_view_chunks(panoramas, device=dev, **view_kw)]
    if not outs:
        return torch.empty((0, 3, 336, 336), dtype=out_dtype, device=dev)
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


def main(argv=None) -> int:
    import argparse
    import os
    from PIL import Image
    ap = argparse.ArgumentParser(prog="python -m pigeon_amd.panorama", description="Render the four views the model sees of an equirectangular panorama.")
    ap.add_argument("panorama", help="image file (a baseline JPEG is decoded on the GPU)")
    ap.add_argument("-o", "--out", required=True, help="directory for view1.png .. view4.png")
    ap.add_argument("--centre-heading", type=float, default=0.0, help="compass heading of the file's centre column (default 0)")
    ap.add_argument("--size", type=int, default=None, help="view size in pixels (default round(W / pi) clamped to [336, 4096])")
    ap.add_argument("--fov", type=float, default=90.0, help="field of view in degrees (default 90)")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    with open(a.panorama, "rb") as f:
        dec = equirect_views(EncodedImages([f.read()]), fov=a.fov, size=a.size, centre_heading=a.centre_heading, device=a.device)
    os.makedirs(a.out, exist_ok=True)
    for i in range(len(dec)):
        path = os.path.join(a.out, f"view{i + 1}.png")
        Image.fromarray(dec.image(i).cpu().numpy()).save(path)
        print(path)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
