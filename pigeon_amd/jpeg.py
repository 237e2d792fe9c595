"""JPEG files as bytes -> RGB pixels on the GPU, in the packed buffer the ragged resize reads (pg_jpeg_* in include/pigeon_hip.h).

The host parses headers and undoes the Huffman coding (a thread per file, GIL released); the GPU does the rest and writes the pixels
Pillow would give for `Image.open(f).convert('RGB')`, bit for bit.  A file the decoder refuses (progressive, CMYK, PNG, ...) is decoded
by Pillow on the host and copied to its place in the same device buffer: the caller gets one buffer whatever the mix.  A supported
file whose scan is damaged raises ValueError naming its index."""
from __future__ import annotations

import io
import threading
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib, hip_ops
from .packing import PinnedStaging, chunk_by_bytes


class EncodedImages:
    """A list of image files as `bytes`: what DataLoader workers ship instead of decoded pixels (plain picklable data)."""

    def __init__(self, files: Sequence[bytes]):
        files = [files] if isinstance(files, (bytes, bytearray, memoryview)) else list(files)
        for i, f in enumerate(files):
            if not isinstance(f, (bytes, bytearray, memoryview)):
                raise TypeError(f"EncodedImages: item {i} is {type(f).__name__}, not bytes")
        self.files: List[bytes] = [bytes(f) for f in files]

    def __len__(self) -> int:
        return len(self.files)

    def __getitem__(self, i):
        return EncodedImages(self.files[i]) if isinstance(i, slice) else self.files[i]

    def __iter__(self):
        return iter(self.files)

    @staticmethod
    def concat(parts: Sequence["EncodedImages"]) -> "EncodedImages":
        return EncodedImages([f for p in parts for f in p.files])


def image_bytes(value) -> bytes:
    """The file of one dataset item as bytes: `bytes` itself, the dict a HF `Image(decode=False)` column yields (its `bytes`, else the
    file at its `path`), or a path.  Nothing is decoded: this is all a DataLoader worker does in the `encoded` modes."""
    import os
    if isinstance(value, (bytes, bytearray, memoryview)):
        return bytes(value)
    if isinstance(value, dict) and (value.get("bytes") is not None or value.get("path")):
        if value.get("bytes") is not None:
            return bytes(value["bytes"])
        value = value["path"]
    if isinstance(value, (str, os.PathLike)):
        with open(value, "rb") as f:
            return f.read()
    raise TypeError(f"encoded=True needs the image file's bytes (bytes, a path, or the dict of a datasets.Image(decode=False) column), "
                    f"got {type(value).__name__}")


class DecodedImages:
    """`packed`: DEVICE 1-D uint8, the packed buffer of pg_prep_ragged_forward with the descriptors in its head; `plan`: its RaggedPlan;
    `fallbacks`: [(index, reason)] of the files Pillow decoded on the host."""

    def __init__(self, packed: torch.Tensor, plan: "hip_ops.RaggedPlan", fallbacks: List[Tuple[int, str]]):
        self.packed, self.plan, self.fallbacks = packed, plan, fallbacks

    def __len__(self) -> int:
        return self.plan.n

    def image(self, i: int) -> torch.Tensor:
        """View of image i on the device, (H, W, 3) uint8."""
        h, w = self.plan.sizes[i]
        off = int(self.plan.items[i].src_off)
        return self.packed[off:off + h * w * 3].view(h, w, 3)


# Fallbacks seen by this process, by reason: the CLI prints them once per run
FALLBACKS: dict = {}
_LOCK = threading.RLock()
_STAGING: dict = {}                   # device index -> PinnedStaging of the coefficients, taken and copied from under _LOCK


def fallback_summary() -> str:
    with _LOCK:
        if not FALLBACKS:
            return ""
        total = sum(FALLBACKS.values())
        return f"{total} image(s) decoded by Pillow on the host: " + ", ".join(f"{k} x{v}" for k, v in sorted(FALLBACKS.items()))


def pillow_rgb(data: bytes) -> np.ndarray:
    from PIL import Image
    return np.array(Image.open(io.BytesIO(data)).convert("RGB"))     # (a writable copy: it goes through torch)


def probe_all(files: Sequence[bytes]):
    """(infos with the size of every image filled in, {index: pixels Pillow decoded})."""
    infos, host = [], {}
    for i, f in enumerate(files):
        info = hip_ops.jpeg_probe(f)
        if info.reason != 0:
            arr = host[i] = pillow_rgb(f)
            info.height, info.width = int(arr.shape[0]), int(arr.shape[1])
        infos.append(info)
    return infos, host


def _decode(files, infos, host, dev, threads) -> DecodedImages:
    plan = hip_ops.jpeg_plan(infos)
    fallbacks = [(i, hip_ops.jpeg_reason(infos[i].reason)) for i in sorted(host)]
    with _LOCK:
        for _, r in fallbacks:
            FALLBACKS[r] = FALLBACKS.get(r, 0) + 1
        with torch.cuda.device(dev):
            packed = torch.empty(plan.prep.packed_bytes, dtype=torch.uint8, device=dev)
            if plan.n == 0:
                return DecodedImages(packed, plan.prep, fallbacks)
            staging = _STAGING.setdefault(int(dev.index), PinnedStaging())
            stage = staging.take(plan.coef_bytes)
            hip_ops.jpeg_entropy_decode(files, plan, stage, threads)           # raises before anything is queued on the GPU
            coef_dev = stage.to(dev, non_blocking=True)
            staging.copied()
            for i, arr in host.items():
                off = int(plan.items[i].rgb_off)
                packed[off:off + arr.size].copy_(torch.from_numpy(np.ascontiguousarray(arr)).view(-1))
            hip_ops.jpeg_forward(coef_dev, plan, packed)
    return DecodedImages(packed, plan.prep, fallbacks)


def decode_chunks(encoded, device="cuda", max_bytes: Optional[int] = None, threads: Optional[int] = None):
    """Generator of DecodedImages over consecutive runs of the files whose packed buffers hold at most `max_bytes` bytes each (None: one
    run).  Indices in errors and in `fallbacks` count from the start of `encoded`."""
    files = encoded.files if isinstance(encoded, EncodedImages) else EncodedImages(encoded).files
    dev = hip_ops.indexed_device(device)
    _lib.require_gpu()
    infos, host = probe_all(files)
    sizes = [(i.height, i.width) for i in infos]
    runs = [(0, len(files))] if max_bytes is None else chunk_by_bytes(sizes, max_bytes)
    for lo, hi in runs or [(0, 0)]:
        try:
            dec = _decode(files[lo:hi], infos[lo:hi], {i - lo: a for i, a in host.items() if lo <= i < hi}, dev, threads)
        except hip_ops.JpegEntropyError as e:
            err = ValueError(f"decode_images: image {e.index + lo} is damaged: {e}")
            err.index = e.index + lo
            raise err from e
        dec.fallbacks = [(i + lo, r) for i, r in dec.fallbacks]
        yield dec


def decode_images(encoded, device="cuda", threads: Optional[int] = None) -> DecodedImages:
    """`encoded`: an EncodedImages (or a list of bytes).  Returns the packed DEVICE buffer with every image's RGB at its offset and the
    resize's descriptors in its head, plus its plan: `RaggedPreprocessor.forward(packed, plan, header_written=True)` takes it as it is.
    `threads`: workers of the host stage, default min(16, CPUs this process may use).  ValueError (with `.index`) for a damaged file."""
    return next(decode_chunks(encoded, device, None, threads))
