"""CLIP image preprocessing: `clip_preprocess`, the reference's CLIPProcessor restated on the host, and `gpu_preprocess`, the device
path with the same bits -- raw pixels, packed batches or files as bytes in, (N,3,336,336) pixel_values on the device out."""
from __future__ import annotations

import threading
from collections import OrderedDict
from typing import Dict

import numpy as np
import torch
from torch import Tensor

from . import hip_ops
from .config import OPENAI_CLIP_MEAN, OPENAI_CLIP_STD
from .jpeg import DecodedImages, EncodedImages, decode_chunks
from .packing import PackedImages, PinnedStaging, as_rgb_array, check_rgb_u8, chunk_by_bytes, pack_into


def _resize_output_size(h: int, w: int, size: int = 336):
    """transformers 4.23.1 (reference env.yml:60) ImageFeatureExtractionMixin.resize with an int size and
    default_to_square=False: the shorter edge becomes `size`, the longer one int(size * long / short)."""
    short, long = (w, h) if w <= h else (h, w)
    if short == size:
        return h, w
    new_short, new_long = size, int(size * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def clip_preprocess(images) -> Tensor:
    """CLIPProcessor restated for PIL inputs on the HOST (what `self.processor(images=...)` does at reference
    models/clip_embedder.py:52; this is DataLoader-worker work in the reference too): convert RGB, resize shorter edge
    to 336 (PIL BICUBIC), centre crop 336x336, float32 / 255.0, (x - mean) / std -> (N,3,336,336) fp32.
    `gpu_preprocess` below is the device path and produces bit-identical values."""
    from PIL import Image
    if not isinstance(images, (list, tuple)):
        images = [images]
    out = []
    mean = np.asarray(OPENAI_CLIP_MEAN).astype(np.float32)
    std = np.asarray(OPENAI_CLIP_STD).astype(np.float32)
    for im in images:
        im = im.convert("RGB")
        w, h = im.size
        nh, nw = _resize_output_size(h, w)
        if (nh, nw) != (h, w):
            im = im.resize((nw, nh), resample=Image.BICUBIC)
        left, top = (nw - 336) // 2, (nh - 336) // 2
        im = im.crop((left, top, left + 336, top + 336))
        a = np.asarray(im).astype(np.float32) / 255.0
        out.append(((a - mean) / std).transpose(2, 0, 1))
    return torch.from_numpy(np.ascontiguousarray(np.stack(out)))


# pg_prep handles by (in_h, in_w, device): each owns the resize coefficient tables of one input geometry.  Street-view panels come
# in a handful of sizes, photo collections (YFCC) in thousands: least-recently-used handles beyond the cap are destroyed.
_PREPROCESSORS: OrderedDict = OrderedDict()
_PREPROCESSORS_MAX = 64
# The ragged path (pg_prep_ragged_forward): one RaggedPreprocessor per device -- it owns the normalisation table and a workspace,
# nothing per geometry.  Lists of more than one shape take it: 512 images in 128 sizes measured 17.7 ms against 45.0 ms grouped by
# size (tools/prep_ragged_ab.py, profiles/r07/prep_ragged_ab.txt).
_RAGGED: Dict = {}
RAGGED_MAX_BYTES = 256 << 20                                       # packed bytes per ragged call of the list path
# Two PinnedStaging per device: one for the packed buffers of the ragged path (a list of several shapes, a pageable PackedImages), one
# for lists of ONE shape.  A buffer of its own keeps a 629 MB one-shape list 1.1 ms faster where such lists alternate with pageable
# PackedImages of that size, which torch copies into the staging buffer from all its threads (tools/prep_staging_probe.py,
# profiles/r11/image_input_refactor_ab.txt).  A buffer is filled before its copy is queued, and the handle caches are shared: one
# caller of gpu_preprocess at a time.
_STAGING: Dict = {}
_UNIFORM_STAGING: Dict = {}
_PREP_LOCK = threading.RLock()


def _preprocessor(in_h: int, in_w: int, device_index: int) -> "hip_ops.Preprocessor":
    key = (int(in_h), int(in_w), int(device_index))
    p = _PREPROCESSORS.pop(key, None)
    if p is None:
        p = hip_ops.Preprocessor(key[0], key[1], device=key[2])
    _PREPROCESSORS[key] = p                                        # most recently used last
    while len(_PREPROCESSORS) > _PREPROCESSORS_MAX:
        old_key, old = _PREPROCESSORS.popitem(last=False)
        torch.cuda.synchronize(old_key[2])                         # ITS device: its tables may still be read by a queued kernel
        old.close()
    return p


def _ragged_preprocessor(device_index: int) -> "hip_ops.RaggedPreprocessor":
    p = _RAGGED.get(int(device_index))
    if p is None:
        p = _RAGGED[int(device_index)] = hip_ops.RaggedPreprocessor(int(device_index))
    return p


def _staging(dev, uniform: bool = False) -> PinnedStaging:
    return (_UNIFORM_STAGING if uniform else _STAGING).setdefault(int(dev.index), PinnedStaging())


def _ragged_forward(host: Tensor, plan, dev, out_dtype, staging: PinnedStaging = None) -> Tensor:
    """`host`: plan.packed_bytes bytes with the pixels in place, taken from `staging` if one is given.  The descriptors go into its
    head, one copy, one forward."""
    host.numpy()[:plan.header_bytes] = plan.header()
    with torch.cuda.device(dev):
        on_dev = host.to(dev, non_blocking=True)
        if staging is not None:
            staging.copied()
        return _ragged_preprocessor(dev.index).forward(on_dev, plan, out_dtype, header_written=True)


def _gpu_preprocess_packed(packed: PackedImages, dev, out_dtype) -> Tensor:
    data = packed.data
    if not torch.is_tensor(data) or data.dtype != torch.uint8 or data.dim() != 1 or data.is_cuda or not data.is_contiguous():
        raise ValueError("gpu_preprocess: PackedImages.data must be a contiguous 1-D uint8 host tensor")
    plan = hip_ops.ragged_plan(packed.size_list())
    if data.numel() != plan.packed_bytes:
        raise ValueError(f"gpu_preprocess: PackedImages holds {data.numel()} bytes, its {plan.n} sizes need {plan.packed_bytes}")
    if plan.n == 0:
        return torch.empty((0, 3, 336, 336), dtype=out_dtype, device=dev)
    if data.is_pinned():
        out = _ragged_forward(data, plan, dev, out_dtype)          # its head was left blank for exactly this
        with torch.cuda.device(dev):
            packed.copy_event = torch.cuda.Event()                 # the caller may rewrite the pinned buffer once this has passed
            packed.copy_event.record()
        return out
    staging = _staging(dev)
    stage = staging.take(plan.packed_bytes)
    stage.copy_(data)
    return _ragged_forward(stage, plan, dev, out_dtype, staging)


def _gpu_preprocess_encoded(encoded: EncodedImages, dev, out_dtype) -> Tensor:
    """Files as bytes: decoded on the GPU into the packed buffer (pigeon_amd/jpeg.py), resized from there -- no host round trip."""
    outs = []
    for dec in decode_chunks(encoded, dev, RAGGED_MAX_BYTES):
        with torch.cuda.device(dev):
            outs.append(_ragged_preprocessor(dev.index).forward(dec.packed, dec.plan, out_dtype, header_written=True))
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


def _gpu_preprocess_mixed(arrs, dev, out_dtype) -> Tensor:
    """A list of several shapes.  One beyond the byte budget or the 65535 images of one call goes in consecutive chunks: the staging
    buffer and the workspace stay bounded."""
    staging, outs = _staging(dev), []
    for lo, hi in chunk_by_bytes([a.shape[:2] for a in arrs], RAGGED_MAX_BYTES):
        plan = hip_ops.ragged_plan([a.shape[:2] for a in arrs[lo:hi]])
        stage = staging.take(plan.packed_bytes)                    # the images go straight to their places in the pinned buffer
        pack_into(arrs[lo:hi], [int(it.src_off) for it in plan.items], stage.numpy())
        outs.append(_ragged_forward(stage, plan, dev, out_dtype, staging))
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


def gpu_preprocess(images, device="cuda", out_dtype: torch.dtype = torch.float32) -> Tensor:
    """CLIP preprocessing on the GPU: `images` is a uint8 RGB tensor / ndarray (N,H,W,3) or (H,W,3), a list of PIL images / arrays,
    a `PackedImages`, an `EncodedImages` (files as bytes: decoded on the GPU, Pillow's pixels bit for bit, then resized in place) or a
    `DecodedImages` (a packed DEVICE buffer with its plan: what `decode_images` and `panorama.equirect_views` return).
    Tensors and lists of ONE shape run pg_prep_forward (a handle per geometry); a `PackedImages` and a list of several shapes run
    pg_prep_ragged_forward: one packed staging buffer and, per chunk of at most RAGGED_MAX_BYTES (256 MiB) of packed bytes, one copy
    and three launches whatever the sizes.  A PINNED `PackedImages` is copied from in place: its head is overwritten with the
    descriptors and the buffer belongs to the call until `copy_event` (set on the object) has passed.  Returns the (N,3,336,336)
    pixel_values on `device`, bit-identical to `clip_preprocess` / the reference's CLIPProcessor.
    `out_dtype`: torch.float32, torch.float16 (the fp32 value rounded) or torch.uint8 -- the resized, cropped byte itself, planar, in
    front of the normalisation table: what the `pixel_bytes` arguments of the encoder and the model take (a quarter of the fp32 size).
    Callers from several threads are served one after the other: the pinned staging buffers and the handles are shared."""
    dev = hip_ops.indexed_device(device)
    with _PREP_LOCK:
        if isinstance(images, PackedImages):
            return _gpu_preprocess_packed(images, dev, out_dtype)
        if isinstance(images, EncodedImages):
            return _gpu_preprocess_encoded(images, dev, out_dtype)
        if isinstance(images, DecodedImages):                      # pixels on the device already: decoded files, rendered panorama views
            with torch.cuda.device(images.packed.device):
                return _ragged_preprocessor(images.packed.device.index).forward(images.packed, images.plan, out_dtype, header_written=True)
        if hasattr(images, "convert"):                             # one PIL image, as `processor(images=img)` accepts it
            images = [images]
        staging = None
        if torch.is_tensor(images) or isinstance(images, np.ndarray):
            t = torch.as_tensor(images)                            # copied from where it is, no staging
            if t.dim() == 3:
                t = t[None]
            if t.dtype != torch.uint8 or t.shape[-1] != 3:
                raise ValueError(f"gpu_preprocess expects uint8 RGB (N,H,W,3), got {t.dtype} {tuple(t.shape)}")
        else:
            # (a PIL image that is RGB already is not copied by `convert`: a serving request's four views are; round 6)
            arrs = [as_rgb_array(im) for im in images]
            for a in arrs:
                check_rgb_u8(a)
            if not arrs:
                return torch.empty((0, 3, 336, 336), dtype=out_dtype, device=dev)
            if len({a.shape for a in arrs}) > 1:
                return _gpu_preprocess_mixed(arrs, dev, out_dtype)
            # the images of one size go straight into their PINNED staging buffer (one copy instead of np.stack + the driver's own staging
            # of a pageable source), from which the transfer below is asynchronous
            staging = _staging(dev, uniform=True)
            t = staging.take(len(arrs) * arrs[0].size).view((len(arrs),) + arrs[0].shape)
            view = t.numpy()
            for j, a in enumerate(arrs):
                view[j] = a
        with torch.cuda.device(dev):
            on_dev = t.to(dev, non_blocking=True).contiguous()
            if staging is not None:
                staging.copied()
            return _preprocessor(t.shape[1], t.shape[2], dev.index)(on_dev, out_dtype)
