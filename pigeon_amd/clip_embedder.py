"""CLIP ViT-L/14-336 image embedder on the HIP kernels, behind the reference's call surface.

Mirrors reference models/clip_embedder.py (class CLIPEmbedding: same constructor arguments, `forward(image)`
accepts PIL image(s) or an (N,3,336,336) tensor and returns the (N,1024) mean-over-577-tokens embedding on
the device), with `transformers.CLIPVisionModel` replaced by `HipCLIPVisionModel`, a module whose forward
runs entirely inside libpigeon_hip.so.
"""
from __future__ import annotations

import os
from types import SimpleNamespace
from typing import Callable, Dict, Optional

import torch
from torch import Tensor

from . import hip_ops, synthetic
from .certainty import SAFETY, CalibrationError, Certainty, combine_ranks, outside_contract, require_fingerprint
from .config import CLIP_MODEL
from .jpeg import EncodedImages, decode_chunks, decode_images  # noqa: F401  (re-exported)
from .packing import PackedImages, as_rgb_array, check_rgb_u8, chunk_by_bytes, pack_images, pack_into, packed_layout  # noqa: F401  (re-exported)
from .preprocess import clip_preprocess, gpu_preprocess  # noqa: F401  (re-exported; CLIPEmbedding calls this module's `gpu_preprocess`)
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


def _on_cuda(t: Tensor, device) -> Tensor:
    """A host tensor goes to `device` if that is a cuda torch.device, else to the current one; a device tensor stays where it is."""
    if t.is_cuda:
        return t
    return t.to(device if (isinstance(device, torch.device) and device.type == "cuda") else torch.device("cuda"))


def _to_device_pixels(pixel_values: Tensor, device) -> Tensor:
    pixel_values = _on_cuda(pixel_values, device)
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
    return _on_cuda(pixel_bytes, device).view((-1, 3, 336, 336))


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
