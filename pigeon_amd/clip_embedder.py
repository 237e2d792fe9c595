"""CLIP ViT-L/14-336 image embedder on the HIP kernels, behind the reference's call surface.

Mirrors reference models/clip_embedder.py (class CLIPEmbedding: same constructor arguments, `forward(image)`
accepts PIL image(s) or an (N,3,336,336) tensor and returns the (N,1024) mean-over-577-tokens embedding on
the device), with `transformers.CLIPVisionModel` replaced by `HipCLIPVisionModel`, a module whose forward
runs entirely inside libpigeon_hip.so.
"""
from __future__ import annotations

import os
import threading
from types import SimpleNamespace
from typing import Callable, Dict, Optional

import numpy as np
import torch
from torch import Tensor

from . import hip_ops, synthetic
from .certainty import SAFETY, CalibrationError, Certainty, combine_ranks, outside_contract, require_fingerprint
from .config import CLIP_MODEL, OPENAI_CLIP_MEAN, OPENAI_CLIP_STD
from .jpeg import EncodedImages, decode_chunks, decode_images  # noqa: F401  (re-exported)
from .packing import PackedImages, as_rgb_array, check_rgb_u8, chunk_by_bytes, pack_images, pack_into, packed_layout  # noqa: F401  (re-exported)
from .utils import load_state_dict


class HipCLIPVisionModel(torch.nn.Module):
    """Stand-in for transformers.CLIPVisionModel on this path.

    * holds the fp32 parameters under the SAME state-dict names as transformers (flat 5.x layout; the 4.23.1
      `vision_model.` prefix is accepted on load), so the reference's name-wise checkpoint loading
      (models/utils.py:24-45, models/super_guessr.py:222-238) keeps working;
    * `forward(pixel_values=...)` returns an object with `.last_hidden_state` (N,577,1024), taken before
      post_layernorm exactly like the HF module the reference calls (models/clip_embedder.py:63);
    * `embed(pixel_values)` returns the token mean directly (what both reference call sites compute next,
      clip_embedder.py:64-65 / super_guessr.py:397-398) without materialising the hidden states.
    The packed bf16 device copy (hip_ops.VitEncoder) is built lazily and rebuilt after any weight load.
    """

    def __init__(self, state_dict: Optional[Dict[str, Tensor]] = None, layers: int = synthetic.LAYERS,
                 seed: Optional[int] = None, max_chunk: int = 0):
        super().__init__()
        if state_dict is None:
            if seed is None:
                raise ValueError("HipCLIPVisionModel needs a state_dict or an explicit seed for random init")
            state_dict = synthetic.make_vit_weights(seed=seed, layers=layers)
        sd = {}
        for k, v in state_dict.items():
            if not torch.is_tensor(v) or not v.is_floating_point():
                continue
            k = k[len("vision_model."):] if k.startswith("vision_model.") else k
            sd[k] = v.detach().to("cpu", torch.float32).clone()
        self._sd = sd
        self.config = SimpleNamespace(hidden_size=1024, _name_or_path=CLIP_MODEL, num_hidden_layers=layers)
        self._enc: Optional[hip_ops.VitEncoder] = None
        self._enc_device = None
        self._max_chunk = max_chunk
        # exact mode (`embed_precise`): the encoder additionally packs the split-fp16 weight copy (3x the 16-bit weight memory)
        self._precise = False                             # SuperGuessr(exact_top1) / enable_precise(True) switch it on
        self._dummy = torch.nn.Parameter(torch.zeros(1), requires_grad=False)   # lets .to()/is_cuda work

    # ---- nn.Module protocol over the plain weight dict ----
    def state_dict(self, *args, prefix: str = "", **kwargs):
        return {prefix + k: v for k, v in self._sd.items()}

    def load_state_dict(self, state_dict, strict: bool = True):
        load_state_dict(self, state_dict)
        return SimpleNamespace(missing_keys=[], unexpected_keys=[])

    def parameters(self, recurse: bool = True):
        yield self._dummy

    def _weights_changed(self):
        if self._enc is not None:
            self._enc.close()
        self._enc = None

    @property
    def base_model(self):
        return self                                      # HF: model.base_model is model for CLIPVisionModel

    def _encoder(self, device: torch.device) -> hip_ops.VitEncoder:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        if self._enc is None or self._enc_device != idx:
            if self._enc is not None:
                self._enc.close()
            self._enc = hip_ops.VitEncoder(self._sd, device=idx, max_chunk=self._max_chunk, precise=self._precise)
            self._enc_device = idx
        return self._enc

    def enable_precise(self, on: bool = True):
        """Make `embed_precise` available (the packed encoder is rebuilt with the split-weight copy on next use)."""
        if bool(on) != self._precise:
            self._precise = bool(on)
            self._weights_changed()

    def _pixels(self, pixel_values: Optional[Tensor], pixel_bytes: Optional[Tensor]) -> Tensor:
        """The (N,3,336,336) device tensor the encoder reads: float `pixel_values` as before, or `pixel_bytes` -- uint8 (B,12,336,336) /
        (B,3,336,336), checked by name before anything moves -- as (B*4 or B, 3,336,336) uint8."""
        if pixel_bytes is None:
            return _to_device_pixels(pixel_values, self._dummy.device)
        exclusive_pixel_bytes(pixel_bytes, pixel_values=pixel_values)
        return pixel_bytes_to_device(pixel_bytes, self._dummy.device)

    def embed_precise(self, pixel_values: Tensor = None, out: Optional[Tensor] = None, pixel_bytes: Tensor = None) -> Tensor:
        """The exact mode of `embed`: near-fp32 arithmetic (pg_vit_forward_precise), ~3x the time per image at 40+ images, more below.
        `out` (N,1024) fp32: write there instead of a fresh tensor.  `pixel_bytes`: as `embed`."""
        px = self._pixels(pixel_values, pixel_bytes)
        self.enable_precise(True)
        return self._encoder(px.device).forward_precise(px, out=out)

    def embed(self, pixel_values: Tensor = None, pixel_bytes: Tensor = None) -> Tensor:
        """`pixel_bytes` (instead of `pixel_values`): uint8 (B,12,336,336) or (B,3,336,336), device or host -- the resized bytes in
        front of the normalisation table (`gpu_preprocess(..., out_dtype=torch.uint8)`).  The encoder looks them up itself: the same
        bits as from the fp32 pixel_values, a quarter of the bytes.  Returns one row per image (B*4 or B)."""
        px = self._pixels(pixel_values, pixel_bytes)
        return self._encoder(px.device).forward(px)

    def hidden(self, pixel_values: Tensor = None, pixel_bytes: Tensor = None) -> Tensor:
        """last_hidden_state (N,577,1024) of `pixel_values` or `pixel_bytes` (as `embed`)."""
        px = self._pixels(pixel_values, pixel_bytes)
        return self._encoder(px.device).forward(px, return_hidden=True)[1]

    def fingerprint(self) -> str:
        """32 hex digits identifying the weights the fast encoder computes with (pg_vit_fingerprint over the packed device buffers;
        builds the packed encoder if needed, on the module's device).  What a calibration file is keyed by."""
        dev = self._dummy.device if self._dummy.is_cuda else torch.device("cuda", torch.cuda.current_device())
        return "%016x%016x" % self._encoder(dev).fingerprint()

    def encoder_config(self) -> dict:
        """What, besides the weights, changes the fast path's bits (part of the fingerprint; written into a calibration file's header)."""
        fold = os.environ.get("PIGEON_LN_FOLD", "1")[:1] != "0"
        mma = self._enc.mma_dtype if self._enc is not None else ("bf16" if os.environ.get("PIGEON_MMA_DTYPE", "").lower() == "bf16" else "f16")
        layers = 0
        while f"encoder.layers.{layers}.layer_norm1.weight" in self._sd:
            layers += 1
        return {"layers": layers, "mma_dtype": mma, "ln_fold": bool(fold)}

    def forward(self, pixel_values: Tensor = None, **kwargs):
        pixel_values = _to_device_pixels(pixel_values, self._dummy.device)
        emb, hid = self._encoder(pixel_values.device).forward(pixel_values, return_hidden=True)
        return SimpleNamespace(last_hidden_state=hid, pooler_output=None, token_mean=emb)


def load_pretrained_clip(name: Optional[str] = None) -> HipCLIPVisionModel:
    """`CLIPVisionModel.from_pretrained(CLIP_MODEL)` of the reference (models/clip_embedder.py:26, evaluation/evaluate.py:36), offline:
    `name` (default: env PIGEON_CLIP_MODEL, else config.CLIP_MODEL) is resolved by transformers with `local_files_only=True` -- a
    directory written by `save_pretrained`, or the hub id if it sits in the local HuggingFace cache -- and its vision-tower state
    dict is packed into a `HipCLIPVisionModel`.  A full CLIPModel checkpoint works as well (its `vision_model.*` keys are taken).
    Raises RuntimeError with the reason when neither is there (this container has no network and no cache)."""
    name = name or os.environ.get("PIGEON_CLIP_MODEL") or CLIP_MODEL
    try:
        from transformers import CLIPVisionModel
        hf = CLIPVisionModel.from_pretrained(name, local_files_only=True)
    except Exception as e:  # noqa  (OSError: not cached; ImportError: no transformers; ValueError: bad directory)
        raise RuntimeError(f"CLIPVisionModel.from_pretrained({name!r}, local_files_only=True) failed: {type(e).__name__}: {e}") from e
    cfg = hf.config
    geom = (cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.image_size, cfg.patch_size)
    if geom != (1024, 4096, 16, 336, 14):
        raise RuntimeError(f"{name!r} is not a ViT-L/14-336 vision tower (hidden, mlp, heads, image, patch = {geom}); "
                           "the HIP encoder is built for that geometry only")
    m = HipCLIPVisionModel(hf.state_dict(), layers=cfg.num_hidden_layers)
    m.config._name_or_path = name
    return m


def _to_device_pixels(pixel_values: Tensor, device) -> Tensor:
    if not pixel_values.is_cuda:
        dev = device if (isinstance(device, torch.device) and device.type == "cuda") else torch.device("cuda")
        pixel_values = pixel_values.to(dev)
    if pixel_values.dtype not in (torch.float32, torch.float16, torch.bfloat16):
        pixel_values = pixel_values.float()
    return pixel_values.contiguous()


def check_pixel_bytes(pixel_bytes, name: str = "pixel_bytes") -> Tensor:
    """The one form 8-bit pixels are accepted in, anywhere: a CONTIGUOUS uint8 tensor (B,12,336,336) or (B,3,336,336), planar (what
    `gpu_preprocess(..., out_dtype=torch.uint8)` writes, four views side by side for a panorama).  Anything else -- HWC images, another
    shape or dtype, a strided view -- is a ValueError that names the argument, raised before the tensor goes anywhere."""
    if not torch.is_tensor(pixel_bytes) or pixel_bytes.dtype != torch.uint8:
        got = pixel_bytes.dtype if torch.is_tensor(pixel_bytes) else type(pixel_bytes).__name__
        raise ValueError(f"{name} must be a uint8 tensor (B,12,336,336) or (B,3,336,336), got {got}")
    shape = tuple(pixel_bytes.shape)
    if len(shape) != 4 or shape[1] not in (3, 12) or shape[2:] != (336, 336):
        hwc = " -- HWC images are not pixel bytes: resize them with gpu_preprocess(..., out_dtype=torch.uint8)" if shape[-1:] == (3,) else ""
        raise ValueError(f"{name} must be uint8 (B,12,336,336) or (B,3,336,336) planar, got shape {shape}{hwc}")
    if not pixel_bytes.is_contiguous():
        raise ValueError(f"{name} must be contiguous, got strides {tuple(pixel_bytes.stride())} for shape {shape}")
    return pixel_bytes


def exclusive_pixel_bytes(pixel_bytes, **others) -> None:
    """`pixel_bytes` stands alone: a ValueError naming it and the other input it was given with."""
    given = [k for k, v in others.items() if v is not None]
    if pixel_bytes is not None and given:
        raise ValueError(f"pixel_bytes cannot be given together with {' / '.join(given)}: one input per call")


def pixel_bytes_to_device(pixel_bytes: Tensor, device) -> Tensor:
    """Checked `pixel_bytes` -> (B*4 or B, 3,336,336) uint8 on the device (a host tensor is copied as bytes)."""
    check_pixel_bytes(pixel_bytes)
    if not pixel_bytes.is_cuda:
        dev = device if (isinstance(device, torch.device) and device.type == "cuda") else torch.device("cuda")
        pixel_bytes = pixel_bytes.to(dev)
    return pixel_bytes.view((-1, 3, 336, 336))


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
_PREPROCESSORS: "OrderedDict" = None
_PREPROCESSORS_MAX = 64


def _preprocessor(in_h: int, in_w: int, device_index: int) -> "hip_ops.Preprocessor":
    global _PREPROCESSORS
    from collections import OrderedDict
    if _PREPROCESSORS is None:
        _PREPROCESSORS = OrderedDict()
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


# Pinned host staging buffers of gpu_preprocess's PIL / ndarray-list path, one per (count, image shape, device): [tensor, event of the
# last host-to-device copy that read it].  A buffer is rewritten only after that copy has run (the event is long past in practice).
_STAGING: Dict = {}
_STAGING_MAX = 8


def _staging(n: int, shape, dev) -> Tensor:
    key = (int(n), tuple(int(v) for v in shape), int(dev.index))
    ent = _STAGING.get(key)
    if ent is None:
        if len(_STAGING) >= _STAGING_MAX:
            _STAGING.pop(next(iter(_STAGING)))
        ent = _STAGING[key] = [torch.empty((key[0],) + key[1], dtype=torch.uint8).pin_memory(), None]
    elif ent[1] is not None:
        ent[1].synchronize()
    return ent[0]


def _staging_done(t: Tensor) -> None:
    for ent in _STAGING.values():
        if ent[0] is t:
            ent[1] = torch.cuda.Event()
            ent[1].record()
            return


# The ragged path (pg_prep_ragged_forward): one RaggedPreprocessor per device -- it owns the normalisation table and a workspace,
# nothing per geometry -- and ONE pinned staging buffer per device, grown when a batch needs more: [tensor, event of the last copy].
_RAGGED: Dict = {}
_RAGGED_STAGING: Dict = {}
# Lists of more than one shape take the ragged path: 512 images in 128 sizes measured 17.7 ms against 45.0 ms grouped by size
# (tools/prep_ragged_ab.py, profiles/r07/prep_ragged_ab.txt); PIGEON_PREP_RAGGED=0 keeps them on the grouped path.
RAGGED_LISTS = os.environ.get("PIGEON_PREP_RAGGED", "1") not in ("", "0")
RAGGED_MAX_BYTES = 256 << 20                                       # packed bytes per ragged call of the list path
# gpu_preprocess fills shared pinned staging buffers (_STAGING, _RAGGED_STAGING) before it queues their copies: one caller at a time
_PREP_LOCK = threading.RLock()


def _ragged_preprocessor(device_index: int) -> "hip_ops.RaggedPreprocessor":
    p = _RAGGED.get(int(device_index))
    if p is None:
        p = _RAGGED[int(device_index)] = hip_ops.RaggedPreprocessor(int(device_index))
    return p


def _ragged_staging(nbytes: int, dev) -> Tensor:
    ent = _RAGGED_STAGING.get(int(dev.index))
    if ent is None or ent[0].numel() < nbytes:
        grown = nbytes if ent is None else max(nbytes, ent[0].numel() * 3 // 2)
        ent = _RAGGED_STAGING[int(dev.index)] = [torch.empty(grown, dtype=torch.uint8).pin_memory(), None]
    elif ent[1] is not None:
        ent[1].synchronize()                                       # rewritten only after the last copy out of it has run
    return ent[0][:nbytes]


def _ragged_forward(host: Tensor, plan, dev, out_dtype, staged: bool) -> Tensor:
    """`host`: plan.packed_bytes bytes with the pixels in place.  The descriptors go into its head, one copy, one forward."""
    host.numpy()[:plan.header_bytes] = plan.header()
    with torch.cuda.device(dev):
        on_dev = host.to(dev, non_blocking=True)
        if staged:
            ent = _RAGGED_STAGING[int(dev.index)]
            ent[1] = torch.cuda.Event()
            ent[1].record()
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
        out = _ragged_forward(data, plan, dev, out_dtype, staged=False)        # its head was left blank for exactly this
        with torch.cuda.device(dev):
            packed.copy_event = torch.cuda.Event()                 # the caller may rewrite the pinned buffer once this has passed
            packed.copy_event.record()
        return out
    stage = _ragged_staging(plan.packed_bytes, dev)
    stage.copy_(data)
    return _ragged_forward(stage, plan, dev, out_dtype, staged=True)


def _gpu_preprocess_encoded(encoded: EncodedImages, dev, out_dtype) -> Tensor:
    """Files as bytes: decoded on the GPU into the packed buffer (pigeon_amd/jpeg.py), resized from there -- no host round trip."""
    outs = []
    for dec in decode_chunks(encoded, dev, RAGGED_MAX_BYTES):
        with torch.cuda.device(dev):
            outs.append(_ragged_preprocessor(dev.index).forward(dec.packed, dec.plan, out_dtype, header_written=True))
    return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)


def gpu_preprocess(images, device="cuda", out_dtype: torch.dtype = torch.float32) -> Tensor:
    """See `_gpu_preprocess`.  Callers from several threads are served one after the other: the pinned staging buffers are shared."""
    with _PREP_LOCK:
        return _gpu_preprocess(images, device, out_dtype)


def _gpu_preprocess(images, device="cuda", out_dtype: torch.dtype = torch.float32) -> Tensor:
    """CLIP preprocessing on the GPU: `images` is a uint8 RGB tensor / ndarray (N,H,W,3) or (H,W,3), a list of PIL images / arrays,
    a `PackedImages`, or an `EncodedImages` (files as bytes: decoded on the GPU, Pillow's pixels bit for bit, then resized in place).  Tensors and lists of ONE shape run pg_prep_forward (a handle per geometry); a `PackedImages` and a list of
    several shapes run pg_prep_ragged_forward: one packed staging buffer and, per chunk of at most RAGGED_MAX_BYTES (256 MiB) of packed
    bytes, one copy and three launches whatever the sizes.  A PINNED `PackedImages` is copied from in place: its head is overwritten
    with the descriptors and the buffer belongs to the call until `copy_event` (set on the object) has passed.  Returns the
    (N,3,336,336) pixel_values on `device`, bit-identical to `clip_preprocess` / the reference's CLIPProcessor.
    `out_dtype`: torch.float32, torch.float16 (the fp32 value rounded) or torch.uint8 -- the resized, cropped byte itself, planar, in
    front of the normalisation table: what the `pixel_bytes` arguments of the encoder and the model take (a quarter of the fp32 size)."""
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if isinstance(images, PackedImages):
        return _gpu_preprocess_packed(images, dev, out_dtype)
    if isinstance(images, EncodedImages):
        return _gpu_preprocess_encoded(images, dev, out_dtype)
    if hasattr(images, "convert"):                                 # one PIL image, as `processor(images=img)` accepts it
        images = [images]
    if torch.is_tensor(images) or isinstance(images, np.ndarray):
        t = torch.as_tensor(images)
        if t.dim() == 3:
            t = t[None]
        groups = [(None, t)]
    else:
        # (a PIL image that is RGB already is not copied by `convert`: a serving request's four views are; round 6)
        arrs = [as_rgb_array(im) for im in images]
        by_size: Dict = {}
        for i, a in enumerate(arrs):
            by_size.setdefault(a.shape, []).append(i)
        if RAGGED_LISTS and len(by_size) > 1:
            for a in arrs:
                check_rgb_u8(a)
            # (a list beyond the byte budget or the 65535 images of one call goes in consecutive chunks: the staging buffer and the
            # workspace stay bounded, and no list the grouped path took is refused)
            outs = []
            for lo, hi in chunk_by_bytes([a.shape[:2] for a in arrs], RAGGED_MAX_BYTES):
                plan = hip_ops.ragged_plan([a.shape[:2] for a in arrs[lo:hi]])
                stage = _ragged_staging(plan.packed_bytes, dev)    # the images go straight to their places in the pinned buffer
                pack_into(arrs[lo:hi], [int(it.src_off) for it in plan.items], stage.numpy())
                outs.append(_ragged_forward(stage, plan, dev, out_dtype, staged=True))
            return outs[0] if len(outs) == 1 else torch.cat(outs, dim=0)
        groups = []
        for idx in by_size.values():
            a0 = arrs[idx[0]]
            if a0.dtype != np.uint8 or a0.ndim != 3:
                groups.append((idx, torch.from_numpy(np.stack([arrs[i] for i in idx]))))       # refused below with the usual message
                continue
            # the images of one size go straight into a PINNED staging buffer (one copy instead of np.stack + the driver's own staging
            # of a pageable source), from which the transfer below is asynchronous
            stage = _staging(len(idx), a0.shape, dev)
            view = stage.numpy()
            for j, i in enumerate(idx):
                view[j] = arrs[i]
            groups.append((idx, stage))
    n_total = sum(g[1].shape[0] for g in groups)
    out = torch.empty((n_total, 3, 336, 336), dtype=out_dtype, device=dev)
    for idx, t in groups:
        if t.dtype != torch.uint8 or t.shape[-1] != 3:
            raise ValueError(f"gpu_preprocess expects uint8 RGB (N,H,W,3), got {t.dtype} {tuple(t.shape)}")
        with torch.cuda.device(dev):
            on_dev = t.to(dev, non_blocking=True).contiguous()
            _staging_done(t)                                       # (a pinned staging buffer is reused only after this copy has run)
            px = _preprocessor(t.shape[1], t.shape[2], dev.index)(on_dev, out_dtype)
        if idx is None:
            out = px
        else:
            out[torch.as_tensor(idx, device=dev)] = px
    return out


class CLIPEmbedding(torch.nn.Module):
    def __init__(self, model_name: str, device: str = 'cuda', load_checkpoint: bool = False,
                 panorama: bool = False, state_dict: Optional[Dict[str, Tensor]] = None,
                 clip_model: Optional[HipCLIPVisionModel] = None, contract_guard: Optional[str] = None,
                 calibration: Optional[str] = None, pixel_bytes: Optional[bool] = None):
        """CLIP embedding model (not trainable) -- reference models/clip_embedder.py:11-40.

        Args follow the reference.  The reference pulls the base weights from the HuggingFace hub
        (`CLIPVisionModel.from_pretrained(CLIP_MODEL)`, :26); here the same call runs with `local_files_only=True`
        (`load_pretrained_clip`: the local HF cache, or a `save_pretrained` directory named by env PIGEON_CLIP_MODEL), and two extra
        keyword arguments can supply the weights instead: `state_dict` (transformers CLIPVisionModel names) or a ready
        `clip_model`.  With `load_checkpoint=True`, `model_name` is a torch checkpoint copied over the weights by
        name with the leading `base_model.` component stripped, exactly as :30-32 does.

        `contract_guard` (round 6; default env PIGEON_EMBED_GUARD, else 'exact'): what to do when THIS set of weights puts the 16-bit
        encoder outside the embedding contract (1e-3 relative per image against the fp32 reference).  The first forward sends up to 32
        of its images through the fast and the exact encoder (pg_vit_forward / pg_vit_forward_precise), prints the measured per-image
        error and -- above 0.85e-3 overall or 0.95e-3 on the worst image, the rule `SuperGuessr` applies -- 'exact': encodes everything
        in the exact mode from then on (~3x the time per image), 'raise': raises, 'off': no check.  The embeddings `run.py embed`
        writes are what prototype banks are built from: a tower with large attention logits must not write them out of tolerance
        silently.

        `calibration` (a path): `load_calibration(path)` at the end of construction -- bias and verdict come from the file, and the
        first forward runs neither the guard's measurement nor its collectives.  Without it nothing changes.

        `pixel_bytes` (default: env PIGEON_PIXEL_BYTES, else False): images given as PIL / uint8 HWC / `PackedImages` are preprocessed
        to 8-bit pixels (`gpu_preprocess(..., out_dtype=torch.uint8)`) and the fast tier, `force_exact` and the guard's measurement all
        encode from those bytes: both tiers start from the identical fp32 value, where the default hands the exact tier fp16-rounded
        pixels.  Float tensors given as pixel_values are encoded as before.
        """
        super().__init__()
        self.device = device
        self.processor = clip_preprocess
        if clip_model is not None:
            self.clip_model = clip_model
        elif state_dict is not None:
            self.clip_model = HipCLIPVisionModel(state_dict)
        else:
            try:                                                     # the reference's way (:25-26), from local files only
                self.clip_model = load_pretrained_clip()
            except RuntimeError as why:
                if load_checkpoint and os.path.exists(model_name):   # no base weights here, but the checkpoint carries the tower
                    ckpt = torch.load(model_name, map_location='cpu')
                    ckpt = {('.'.join(k.split('.')[1:]) if 'base_model' in k else k): v for k, v in ckpt.items()}
                    self.clip_model = HipCLIPVisionModel(ckpt)
                    load_checkpoint = False
                else:
                    raise RuntimeError(
                        "CLIPEmbedding: no weights. The reference downloads openai/clip-vit-large-patch14-336 from the hub; offline, "
                        "point PIGEON_CLIP_MODEL at a directory written by save_pretrained (or have the hub id in the local HF cache), "
                        "pass state_dict=... / clip_model=..., or a checkpoint path with load_checkpoint=True.  " + str(why)) from why
        self.panorama = panorama
        self.pixel_bytes = (os.environ.get('PIGEON_PIXEL_BYTES', '0') not in ('', '0')) if pixel_bytes is None else bool(pixel_bytes)
        self.contract_guard = (contract_guard or os.environ.get('PIGEON_EMBED_GUARD', 'exact')).lower()
        if self.contract_guard not in ('exact', 'raise', 'off'):
            raise ValueError(f"contract_guard must be 'exact', 'raise' or 'off', got {self.contract_guard!r}")
        self.guard_stats = None                  # what the first forward measured / a file said (None until then / with the guard off)
        # the measurement and its verdict (pigeon_amd/certainty.py): `bias`, `force_exact` and the calibration file are views of it
        self.certainty = Certainty()

        if load_checkpoint:
            sd = torch.load(model_name, map_location='cpu')
            load_state_dict(self.clip_model.base_model, sd, embedder=True)
            print('Loaded embedder from checkpoint:', model_name)

        if type(device) == str:
            self.clip_model = self.clip_model.to(self.device)
        else:
            self.clip_model = self.clip_model.cuda(self.device)
        self.eval()
        self.calibration_header = None           # header of the calibration file in force (None: none loaded)
        # `exact`: every image through the exact encoder (pg_vit_forward_precise) by the route `force_exact` takes, chosen by the caller
        # (`run.py embed --exact`: embeddings a prototype bank is built from) instead of by the guard -- which then measures nothing
        self.exact = False
        if calibration is not None:
            self.load_calibration(calibration)

    bias = property(lambda self: self.certainty.bias, doc="(1024,) fp32 or None: the systematic part subtracted from every fast embedding")
    force_exact = property(lambda self: self.certainty.force_exact, doc="every image is encoded in the exact mode")
    debias = property(lambda self: self.certainty.debias)

    # ---- calibration as a file (pigeon_amd/certainty.py) ----
    def save_calibration(self, path: str, source: str = '') -> str:
        """Write what the first forward's guard measured -- the bias this module subtracts (in a data-parallel job: the one vector
        all ranks share) and the verdict -- as a calibration file keyed by the encoder's weight fingerprint.  `panels` is 1: the
        tolerance in the file is a per-image one.  A `SuperGuessr` on precomputed embeddings (base_model=None) or another
        `CLIPEmbedding` loads it; a panorama `SuperGuessr` with an encoder wants a file measured on panoramas."""
        st, c = self.guard_stats, self.certainty
        if st is None:
            raise CalibrationError('CLIPEmbedding.save_calibration: nothing measured yet (the guard runs in the first forward; '
                                   "contract_guard='off' never measures)")
        # The file's tolerance is the per-image error of what THIS module returns, by its own rule and not `calibrate`'s: what is left
        # after the bias (held out) -- or, without a bias, the raw error of the whole batch (`image_rel_err`, a norm over all images,
        # where `calibrate` records the RMS of the per-image ratios).  Banks were built from files that say this; it stays.
        resid = st.get('residual_rms') if (c.bias is not None or st.get('image_rel_err') is None) else st.get('image_rel_err')
        if resid is None:
            raise CalibrationError('CLIPEmbedding.save_calibration: the guard statistics hold no per-image error')
        resid = float(resid)
        c.rel_tol = max(SAFETY * resid, 2.0 * c.rel_tol_exact)
        # ... and its statistics are the guard's (on top of a loaded file's), not the panorama-shaped ones `calibrate` reports
        c.stats = dict(st.get('file_stats') or {})
        c.stats.update({k: v for k, v in st.items() if isinstance(v, (bool, int, float, str))})
        c.stats.update(samples=int(st['images']), image_residual_rms=resid, rel_tol=c.rel_tol, kappa=c.kappa,
                       force_exact=c.force_exact, debias=c.bias is not None)
        base = self.clip_model.base_model
        meta = base.encoder_config()
        meta['source'] = source or f"CLIPEmbedding, {st['images']} images"
        return c.save(path, base.fingerprint(), 1, meta)

    def load_calibration(self, path: str) -> dict:
        """Take `bias` and `force_exact` from a calibration file and fill `guard_stats`: the first forward then measures nothing and
        joins no collective (every rank of a job loads the same file instead).  The file is loaded into a fresh `Certainty` and checked
        before anything changes: an unreadable file, an unknown format_version and a fingerprint that is not this encoder's are refused
        (CalibrationError, both fingerprints named).  Any `panels` is accepted: the bias is per image.  Returns the header."""
        sd, header = Certainty.load(path)
        c = Certainty()
        c.load_state_dict(sd)
        require_fingerprint(path, header, self.clip_model.base_model.fingerprint())
        if c.force_exact and self.contract_guard == 'raise':
            raise RuntimeError(f'CLIPEmbedding: {path!r} records the 16-bit encoder outside the 1e-3 embedding contract on these weights; '
                               "construct with contract_guard='exact' to encode in the exact mode")
        st = {'images': int(c.stats.get('samples', header['samples'])), 'image_rel_err': c.stats.get('image_rel_err'),
              'worst_image_rel_err': c.stats.get('worst_image_rel_err'), 'contract': 1e-3, 'debias': c.bias is not None,
              'outside': bool(c.force_exact), 'from_file': str(path), 'fingerprint': header['fingerprint'], 'file_stats': dict(c.stats)}
        if 'image_residual_rms' in c.stats:
            st['residual_rms'] = c.stats['image_residual_rms']
        self.certainty, self.guard_stats, self.calibration_header = c, st, header
        return header

    def embedding_meta(self, source: str = '') -> dict:
        """What the embeddings this module returns NOW are: the sidecar `run.py embed` writes next to its `.npy` files
        (`embedding_meta.json`), from which a bank built on them declares its error (`HostBank.embedding_rel_tol`,
        `run.py evaluate --bank-rel-tol`).  `embedding_rel_tol`: the exact tier's floor for the exact encoder, else the value a
        `SuperGuessr` judges caller-supplied embeddings at -- 1.1 x the per-image residual the guard measured (or a loaded
        calibration file records), 1e-3 where nothing was measured.  It is a declaration derived from the calibration's sample, not a
        measurement of the written files."""
        c, st, base = self.certainty, self.guard_stats, self.clip_model.base_model
        exact = bool(self.exact or c.force_exact)
        tol = c.rel_tol_exact
        if not exact:
            resid = None
            if st is not None:
                resid = st.get('residual_rms') if (c.bias is not None or st.get('image_rel_err') is None) else st.get('image_rel_err')
            tol = SAFETY * float(resid) if resid is not None and float(resid) > 0.0 else c.rel_tol
        meta = dict(base.encoder_config(), encoder='exact' if exact else 'fast', embedding_rel_tol=float(tol),
                    debias=bool(not exact and c.bias is not None), fingerprint=base.fingerprint(),
                    source=source or 'CLIPEmbedding')
        return meta

    def _get_embedding(self, image) -> Tensor:
        """reference models/clip_embedder.py:42-66"""
        with torch.no_grad():
            if isinstance(image, Tensor) == False or image.dtype == torch.uint8:
                # PIL image(s) / uint8 HWC arrays / a PackedImages: resize + crop + normalise on the GPU (bit-identical to the
                # reference's host-side CLIPProcessor); 16-bit pixels when the encoder's MFMA operands are fp16
                dev = self.device if type(self.device) == str else f'cuda:{self.device}'
                pixel_values = gpu_preprocess(image, dev, torch.uint8 if self.pixel_bytes else self._pixel_dtype())
            else:
                pixel_values = image
            if type(self.device) == str:
                pixel_values = pixel_values.to(self.device)
            else:
                pixel_values = pixel_values.cuda(self.device)
            base = self.clip_model.base_model
            if self.exact:                                           # no guard measurement, no collectives, no bias
                return base.embed_precise(pixel_bytes=pixel_values) if pixel_values.dtype == torch.uint8 else base.embed_precise(pixel_values)
            if self.contract_guard != 'off' and self.guard_stats is None and pixel_values.shape[0] > 0:
                self._check_contract(base, pixel_values)
            # last_hidden_state.mean(dim=1), fused in the library (token_mean kernel)
            # (uint8 here is what gpu_preprocess wrote just above with `pixel_bytes`: (N,3,336,336) planar bytes)
            as_input = (lambda px: dict(pixel_bytes=px)) if pixel_values.dtype == torch.uint8 else (lambda px: dict(pixel_values=px))
            if self.force_exact:
                return base.embed_precise(**as_input(pixel_values))
            emb = base.embed(**as_input(pixel_values))
            bias = self.certainty.bias_on(emb.device)
            if bias is not None:
                # the 16-bit encoder's measured systematic error taken out of every image's embedding (pigeon_amd/certainty.py `debias`)
                hip_ops.embedding_debias(emb, bias)
            return emb

    def _check_contract(self, base, pixel_values: Tensor, max_images: int = 32) -> dict:
        """Once per set of weights: the 16-bit encoder against the exact one on up to `max_images` images of the first batch -- the
        measurement; `_judge` is what follows from it.
        (A first batch of fewer than 8 images measures the error but fits no bias: nothing is subtracted for the lifetime of this
        object -- hand the embed path a full first batch, as `run.py embed` does, or set PIGEON_DEBIAS=0 on both entry points.)"""
        if pixel_values.dtype == torch.uint8:                        # `pixel_bytes`: both encoders from the same bytes
            px = pixel_values[:max_images].contiguous()
            return self._judge(base.embed(pixel_bytes=px), base.embed_precise(pixel_bytes=px))
        px = _to_device_pixels(pixel_values[:max_images], base._dummy.device)
        return self._judge(base.embed(px), base.embed_precise(px))

    def _judge(self, fast: Tensor, exact: Tensor, contract: float = 1e-3) -> dict:
        """(n,1024) embeddings of the same images by the two encoders -> `certainty` (bias, verdict) and `guard_stats`: one image per
        sample through `Certainty.calibrate` -- the fit on the even images, the residual on the odd ones, the verdict on the RAW error
        (the conservative reading) -- and, in a data-parallel job (`run.py embed` under torchrun), `combine_ranks` over what every
        rank measured on its own first batch, so that the files the ranks write together mix neither encoders nor vectors."""
        c = self.certainty
        # (`use_drift`: without PIGEON_DEBIAS there is nothing here that a drift vector could be handed to -- no fit at all)
        cs = c.calibrate(fast, exact, fast_images=fast, exact_images=exact, contract=contract, use_drift=c.debias)
        st = {'images': cs['samples'], 'image_rel_err': cs['image_rel_err'], 'worst_image_rel_err': cs['worst_image_rel_err'],
              'contract': contract}
        if 'held_out_residual_rms' in cs:                            # a fit was made (8 images or more); kept or not, it is reported
            st['bias_norm'], st['residual_rms'] = cs['drift_norm'], cs['held_out_residual_rms']
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            errs, vecs = [None] * dist.get_world_size(), [None] * dist.get_world_size()
            dist.all_gather_object(errs, (st['image_rel_err'], st['worst_image_rel_err']))
            dist.all_gather_object(vecs, None if c.bias is None else c.bias.cpu())
            st['image_rel_err_all_ranks'], st['worst_image_rel_err_all_ranks'], bias = combine_ranks([e + (b,) for e, b in zip(errs, vecs)])
            c.bias = None if bias is None else bias.to(fast.device)
            c.force_exact = outside_contract(st['image_rel_err_all_ranks'], st['worst_image_rel_err_all_ranks'], contract)
        st['debias'], st['outside'] = c.bias is not None, c.force_exact
        self.guard_stats = st
        print(f"pigeon_amd.CLIPEmbedding: 16-bit encoder vs exact encoder on {st['images']} images of the first batch: "
              f"{st['image_rel_err']:.2e} relative overall, worst image {st['worst_image_rel_err']:.2e} (contract {contract:g})"
              + (f"; its systematic part ({st['bias_norm']:.2e}) is subtracted from every embedding, {st['residual_rms']:.2e} left" if c.bias is not None else ""))
        if st['outside']:
            if self.contract_guard == 'raise':
                c.force_exact = False                                # ('raise' never encodes in the exact mode: the caller has been told)
                raise RuntimeError('CLIPEmbedding: the 16-bit encoder is outside the 1e-3 embedding contract on these weights '
                                   f"({st['image_rel_err']:.2e} overall, worst image {st['worst_image_rel_err']:.2e}); construct with "
                                   "contract_guard='exact' to encode in the exact mode")
            print('pigeon_amd.CLIPEmbedding: outside the embedding contract on these weights -- every image will be encoded in the '
                  'exact mode (about 3x the time per image).')
        return st

    def _pixel_dtype(self) -> torch.dtype:
        mma = os.environ.get("PIGEON_MMA_DTYPE", "f16").lower()
        return torch.float16 if mma != "bf16" else torch.float32

    def _pre_embed_hook(self) -> Callable:
        def hook(model, input, output):
            self.pre_embed_outputs = output[0]
        return hook

    def forward(self, image) -> Tensor:
        """reference models/clip_embedder.py:79-89"""
        return self._get_embedding(image)
