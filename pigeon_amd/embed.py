"""Multi-GPU batch embedding, behind the reference's call surface (preprocessing/embed.py).

`compute_embeddings(name, model, data, accelerator)` and `embed_images(loaded_model, dataset)` keep the
reference's names, arguments and on-disk outputs (`data/landmark_embeddings/{name}.npy` = (steps, world*batch, 1024)
float32 array of the gathered batches, `{name}_indices.npy` = (steps, world*batch) int64; embed.py:41-43).  `accelerate.Accelerator` is replaced by
`pigeon_amd.distributed.Communicator` (same `.gather`, `.is_local_main_process`, `.wait_for_everyone`), one
process per GPU, RCCL all-gather over xGMI.
"""
from __future__ import annotations

import logging
import os
from typing import Any, Iterable, Optional

import numpy as np
import torch

from .config import EMBED_BATCH_SIZE_PER_GPU
from .distributed import Communicator, shard_batches

logging.basicConfig(level=logging.INFO)
logger = logging.getLogger('embed')


class EmbedDataset:
    """reference dataset_creation/finetune/embed_dataset.py:6-25: yields (pixel_values (3,336,336), index).
    Items whose 'image' is already a tensor are passed through; PIL images go through the restated CLIP
    preprocessing (pigeon_amd.clip_embedder.clip_preprocess)."""

    def __init__(self, dataset):
        self.dataset = dataset

    def __getitem__(self, idx):
        data = self.dataset[idx]
        image = data['image']
        if not torch.is_tensor(image):
            from .clip_embedder import clip_preprocess
            image = clip_preprocess(image)
        return image.squeeze(), data['index']

    def __len__(self):
        return len(self.dataset)


class RawImageDataset:
    """The raw flavour of EmbedDataset: yields (uint8 (H,W,3) RGB array, index).  Decoding and `convert('RGB')` run here, in the
    DataLoader worker; nothing is resized -- that happens on the GPU (pg_prep_ragged_forward), for the whole batch at once.
    encoded=True: yields (file bytes, index) instead -- the item's `image` is bytes, a path or the dict of a HF `Image(decode=False)`
    column; the worker only reads, and the decode runs on the GPU as well (pg_jpeg_forward)."""

    def __init__(self, dataset, encoded: bool = False):
        self.dataset, self.encoded = dataset, encoded

    def __getitem__(self, idx):
        from .packing import as_rgb_array, check_rgb_u8
        data = self.dataset[idx]
        if self.encoded:                                           # the file's bytes as they are: the GPU decodes (pigeon_amd/jpeg.py)
            from .jpeg import image_bytes
            return image_bytes(data['image']), data['index']
        a = as_rgb_array(data['image'])
        check_rgb_u8(a)
        return a, data['index']

    def __len__(self):
        return len(self.dataset)


MAX_PACKED_BYTES = 256 << 20


def collate_packed(batch, max_packed_bytes: int = MAX_PACKED_BYTES, encoded: bool = False):
    """collate_fn for RawImageDataset: [(array, index), ...] -> ([PackedImages, ...], index tensor).  The batch is cut, in order,
    into chunks of at most `max_packed_bytes` packed bytes each (an image above the budget travels alone), which bounds the
    staging buffer and the GPU workspace whatever the photo sizes; the chunks' images, concatenated, are the batch's."""
    from .packing import chunk_by_bytes, pack_images
    if encoded:                                                    # one EncodedImages: gpu_preprocess cuts it by the decoded sizes itself
        from .jpeg import EncodedImages
        return [EncodedImages([f for f, _ in batch])], torch.as_tensor([int(i) for _, i in batch], dtype=torch.int64)
    arrs = [a for a, _ in batch]
    chunks = [pack_images(arrs[lo:hi]) for lo, hi in chunk_by_bytes([a.shape[:2] for a in arrs], max_packed_bytes)]
    return chunks, torch.as_tensor([int(i) for _, i in batch], dtype=torch.int64)


class _ChunkedModel:
    """model([PackedImages, ...]) -> the chunks' embeddings, concatenated: one step's output for compute_embeddings."""

    def __init__(self, model):
        self.model = model

    def __call__(self, chunks):
        return torch.cat([self.model(c) for c in chunks], dim=0)


def _stack_padded(batches, fill):
    """np.stack of per-step arrays; a shorter last step is padded to the common length (fill None: indices -> int max so
    they sort last)."""
    if not batches:
        return np.zeros((0,))
    n = max(b.shape[0] for b in batches)
    out = []
    for b in batches:
        if b.shape[0] < n:
            pad_shape = (n - b.shape[0],) + b.shape[1:]
            v = np.iinfo(b.dtype).max if fill is None else fill
            b = np.concatenate([b, np.full(pad_shape, v, dtype=b.dtype)], axis=0)
        out.append(b)
    return np.stack(out)


def compute_embeddings(name: str, model: Any, data: Iterable, accelerator: Communicator,
                       out_dir: str = 'data/landmark_embeddings', save: bool = True):
    """reference preprocessing/embed.py:16-43.  `data` yields (pixels, index) batches ALREADY sharded for this
    rank (see embed_images).  Every step: output = model(pixels); all-gather index and output (rank-major, one
    collective); rank 0 keeps the numpy copies and finally np.save's them."""
    logger.warning(f'Starting {name} embedding ...')
    all_outputs, all_indices = [], []
    for pixels, index in data:
        output = model(pixels)
        index = torch.as_tensor(index).to(output.device)
        all_indic, all_output = accelerator.gather_many([index, output])       # embed.py:36-37 in one collective
        all_outputs.append(all_output.cpu().detach().numpy())
        all_indices.append(all_indic.cpu().detach().numpy())
    if accelerator.is_local_main_process and save:
        os.makedirs(out_dir, exist_ok=True)
        # plain numeric arrays (steps, world*batch, 1024) / (steps, world*batch): what the reference's np.save of a list of
        # equal-shape batches produces (:41-43) and what its reader np.load's WITHOUT allow_pickle
        # (preprocessing/dataset_preprocessing.py:294-300).  A ragged last batch (single process, drop_last=False) is
        # padded with zero rows whose index is INT64_MAX, which sort behind every real sample in that reader's argsort
        # -- the reference itself cannot save that case with numpy >= 1.24.
        np.save(f'{out_dir}/{name}.npy', _stack_padded(all_outputs, 0.0))
        np.save(f'{out_dir}/{name}_indices.npy', _stack_padded(all_indices, None))
    return all_outputs, all_indices


def embed_images(loaded_model: Any, dataset, accelerator: Optional[Communicator] = None,
                 batch_size: int = EMBED_BATCH_SIZE_PER_GPU, num_workers: int = 8,
                 out_dir: str = 'data/landmark_embeddings', raw_images: bool = False,
                 max_packed_bytes: int = MAX_PACKED_BYTES, exact: bool = False, encoded: bool = False):
    """reference preprocessing/embed.py:45-83: wrap every split in EmbedDataset, one DataLoader per split
    (bs 512 per GPU, shuffle False), shard batches over ranks, embed train/val/test with a barrier between.

    raw_images=True (one image of any size per item): the workers decode and PACK (RawImageDataset, collate_packed) and the model
    resizes on the GPU -- uint8 pixels of the source size cross the bus instead of 1.35 MB of fp32 per image, and no worker runs
    Pillow's resize.  The batches are dealt to the ranks by the same rule, applied to the sample indices before anything is
    loaded, so every rank decodes its own batches only.  What is written is the same.

    encoded=True (with raw_images): the workers only READ -- items carry the file's bytes (`RawImageDataset(encoded=True)`), about a
    tenth of the decoded pixels through the workers' pipes -- and baseline JPEGs are decoded on the GPU into the buffer the resize
    reads (pigeon_amd/jpeg.py; other files by Pillow in the main process).  What is written is the same.

    exact=True: every image goes through the exact encoder (`CLIPEmbedding.exact`: pg_vit_forward_precise, about 3x the time per
    image; no guard measurement, no collectives for one) -- the embeddings to build a prototype bank from when its certainty is to
    be judged at the exact tier's floor.  Either way rank 0 writes `embedding_meta.json` next to the `.npy` files when the model
    can say what its embeddings are (`CLIPEmbedding.embedding_meta`: encoder, embedding_rel_tol, debias, fingerprint, mma_dtype)."""
    from torch.utils.data import DataLoader
    accelerator = accelerator or Communicator()
    results = {}
    loaded_model.eval()
    if exact:
        if not hasattr(loaded_model, 'exact'):
            raise TypeError(f'embed_images(exact=True): {type(loaded_model).__name__} has no exact encoder route (`exact` attribute)')
        loaded_model.exact = True
    if encoded and not raw_images:
        raise ValueError('embed_images(encoded=True) is a mode of raw_images=True')
    for split_name in ('train', 'val', 'test'):
        if split_name not in dataset:
            continue
        if raw_images:
            from functools import partial
            n = len(dataset[split_name])
            mine = list(shard_batches([list(range(i, min(i + batch_size, n))) for i in range(0, n, batch_size)],
                                      accelerator.rank, accelerator.world_size))
            sharded = DataLoader(RawImageDataset(dataset[split_name], encoded=encoded), batch_sampler=mine, num_workers=num_workers,
                                 collate_fn=partial(collate_packed, max_packed_bytes=max_packed_bytes, encoded=encoded))
            model = _ChunkedModel(loaded_model)
        else:
            loader = DataLoader(EmbedDataset(dataset[split_name]), batch_size, shuffle=False, num_workers=num_workers)
            sharded = shard_batches(loader, accelerator.rank, accelerator.world_size)
            model = loaded_model
        results[split_name] = compute_embeddings(split_name, model, sharded, accelerator, out_dir)
        accelerator.wait_for_everyone()
    if accelerator.is_local_main_process and callable(getattr(loaded_model, 'embedding_meta', None)):
        import json
        os.makedirs(out_dir, exist_ok=True)
        with open(os.path.join(out_dir, META_NAME), 'w') as f:       # as of the END of the run: after the guard's measurement
            json.dump(loaded_model.embedding_meta(source=f'embed_images, splits {sorted(results)}'), f, indent=1, sort_keys=True)
    return results


META_NAME = 'embedding_meta.json'


def load_embedding_meta(path: str) -> dict:
    """Read a sidecar `embed_images` wrote (the file, or the directory that holds it).  ValueError when it is not one."""
    import json
    if os.path.isdir(path):
        path = os.path.join(path, META_NAME)
    with open(path) as f:
        meta = json.load(f)
    need = ('encoder', 'embedding_rel_tol', 'debias', 'fingerprint', 'mma_dtype')
    if not isinstance(meta, dict) or any(k not in meta for k in need):
        raise ValueError(f'{path!r} is not an embedding sidecar (needs {", ".join(need)})')
    return meta
