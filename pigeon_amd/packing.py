"""Packed batches of raw images for the ragged GPU preprocessing (pg_prep_ragged_forward): host side, numpy / PIL only.

Nothing here touches the HIP library or a GPU, so DataLoader workers can pack: `pack_images` lays a list of images of any sizes
out in ONE uint8 buffer by the rule of pg_prep_ragged_plan (include/pigeon_hip.h) and leaves the head of the buffer -- where the
descriptors travel -- blank; the process that owns the GPU plans, fills that head in and makes one host-to-device copy
(pigeon_amd.preprocess.gpu_preprocess).  `PinnedStaging` is that process's side of the copy: it reaches torch.cuda only when used."""
from __future__ import annotations

from typing import List, Sequence, Tuple

import numpy as np
import torch

ITEM_BYTES = 80        # PG_PREP_ITEM_BYTES: one descriptor per image at the head of the buffer
ALIGN = 16             # every image starts at a multiple of 16 bytes; the total is rounded up to one


def packed_layout(sizes: Sequence[Tuple[int, int]]) -> Tuple[List[int], int]:
    """(byte offset of every image, total bytes) for images of the given (height, width): the descriptors' region first, then the
    images back to back in order, each at the next multiple of 16.  The same integers as pg_prep_ragged_plan's `src_off` /
    `packed_bytes` (tests hold the two together).  No images: no bytes."""
    n = len(sizes)
    if n == 0:
        return [], 0
    off, offs = n * ITEM_BYTES, []
    for h, w in sizes:
        off = (off + ALIGN - 1) // ALIGN * ALIGN
        offs.append(off)
        off += int(h) * int(w) * 3
    return offs, (off + ALIGN - 1) // ALIGN * ALIGN


def chunk_by_bytes(sizes: Sequence[Tuple[int, int]], max_bytes: int, max_count: int = 65535) -> List[Tuple[int, int]]:
    """Cut a sequence of (height, width) into consecutive runs [start, end) whose packed buffers (`packed_layout`) hold at most
    `max_bytes` bytes and `max_count` images each; an image above the budget forms a run of its own.  One pass with a running offset:
    the descriptor region is a multiple of 16 bytes, so the images' offsets behind it do not depend on the count."""
    runs, start, pix = [], 0, 0
    for i, (h, w) in enumerate(sizes):
        nxt = (pix + ALIGN - 1) // ALIGN * ALIGN + int(h) * int(w) * 3
        k = i - start + 1
        if i > start and (k > max_count or k * ITEM_BYTES + (nxt + ALIGN - 1) // ALIGN * ALIGN > max_bytes):
            runs.append((start, i))
            start, nxt = i, int(h) * int(w) * 3
        pix = nxt
    if len(sizes) > start:
        runs.append((start, len(sizes)))
    return runs


def as_rgb_array(im) -> np.ndarray:
    """A PIL image (any mode: converted to RGB as the reference's processor does; an RGB one is not copied) or an array -> ndarray."""
    if hasattr(im, "convert"):
        return np.asarray(im if getattr(im, "mode", None) == "RGB" else im.convert("RGB"))
    return np.asarray(im)


def check_rgb_u8(a: np.ndarray) -> None:
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"gpu_preprocess expects uint8 RGB (H,W,3) images, got {a.dtype} {tuple(a.shape)}")


class PackedImages:
    """n raw RGB images of any sizes in one 1-D uint8 tensor (`data`: descriptor region + pixels, layout of `packed_layout`; host
    memory, pinned or not) and their sizes (`sizes`: (n,2) int32 tensor of (height, width))."""

    def __init__(self, data: torch.Tensor, sizes: torch.Tensor):
        self.data, self.sizes = data, sizes
        self._offs = None                                          # the images' offsets, laid out on first use
        self.copy_event = None                                     # set by gpu_preprocess on a pinned buffer it copied from in place

    def __len__(self) -> int:
        return int(self.sizes.shape[0])

    def size_list(self) -> List[Tuple[int, int]]:
        return [(int(h), int(w)) for h, w in self.sizes.tolist()]

    def image(self, i: int) -> np.ndarray:
        """View of image i, (H,W,3) uint8."""
        if self._offs is None:
            self._offs = packed_layout(self.size_list())[0]
        h, w = (int(v) for v in self.sizes[i])
        off = self._offs[i]
        return self.data.numpy()[off:off + h * w * 3].reshape(h, w, 3)

    def pin_memory(self) -> "PackedImages":                        # (what DataLoader(pin_memory=True) calls on a custom batch)
        return PackedImages(self.data.pin_memory(), self.sizes)


class PinnedStaging:
    """One pinned host buffer that grows with the largest request, and the one rule of reusing it: it is rewritten only after the last
    host-to-device copy that read it has run.  `take` hands out its first bytes, waiting for that copy if it is still pending; the
    caller fills them, queues its `non_blocking` copy and calls `copied` on the stream that did the copy.  No lock of its own: the
    caller's lock spans "fill the buffer ... copy queued"."""

    def __init__(self):
        self.buf, self.event = None, None

    def take(self, nbytes: int) -> torch.Tensor:
        """A 1-D uint8 pinned view of exactly `nbytes` bytes."""
        if self.buf is None or self.buf.numel() < nbytes:
            grown = nbytes if self.buf is None else max(nbytes, self.buf.numel() * 3 // 2)
            # (the old buffer is dropped without waiting: torch's pinned allocator keeps it alive under a copy still in flight)
            self.buf, self.event = torch.empty(grown, dtype=torch.uint8).pin_memory(), None
        elif self.event is not None:
            self.event.synchronize()
        return self.buf[:nbytes]

    def copied(self) -> None:
        """The copy out of the buffer has just been queued on the current stream of the current device."""
        self.event = torch.cuda.Event()
        self.event.record()


def pack_into(arrs: Sequence[np.ndarray], offs: Sequence[int], buf: np.ndarray) -> None:
    """Copy (H,W,3) uint8 arrays to their offsets in the 1-D uint8 `buf`."""
    for a, off in zip(arrs, offs):
        buf[off:off + a.size].reshape(a.shape)[...] = a


def pack_images(images) -> PackedImages:
    """A list of PIL images / uint8 (H,W,3) arrays -> PackedImages.  Bytes between images and the descriptor region are zero."""
    if hasattr(images, "convert") or (isinstance(images, np.ndarray) and images.ndim == 3):
        images = [images]
    arrs = [as_rgb_array(im) for im in images]
    for a in arrs:
        check_rgb_u8(a)
    sizes = [(a.shape[0], a.shape[1]) for a in arrs]
    offs, total = packed_layout(sizes)
    buf = np.zeros(total, dtype=np.uint8)
    pack_into(arrs, offs, buf)
    return PackedImages(torch.from_numpy(buf), torch.tensor(sizes, dtype=torch.int32).reshape(-1, 2))


def concat_packed(parts: Sequence[PackedImages]) -> PackedImages:
    """Several PackedImages (e.g. what DataLoader workers packed per item) -> ONE holding all their images in order: the images are
    copied to their places in a new buffer laid out for the whole list (the descriptor region grows with the count, so the parts'
    buffers cannot simply be joined)."""
    sizes = [s for p in parts for s in p.size_list()]
    offs, total = packed_layout(sizes)
    buf = np.zeros(total, dtype=np.uint8)
    pack_into([p.image(i) for p in parts for i in range(len(p))], offs, buf)
    return PackedImages(torch.from_numpy(buf), torch.tensor(sizes, dtype=torch.int32).reshape(-1, 2))
