"""SuperGuessr geocell classification model on the HIP kernels, behind the reference's call surface.

Mirrors reference models/super_guessr.py (same constructor signature, `load_geocells`, `load_state`,
`forward(pixel_values | embedding, ..., labels_clf, ...)` returning `ModelOutput` or the serving tuple).
The inference branch is accelerated and supported: the configuration evaluation/evaluate.py:42-44 constructs
(`hierarchical=False`, `heading` as the caller passes it: a no-op with `panorama=True`, :273-274) and `multi_task=True`
(:316-348: the regression, climate and month heads of a multi-task checkpoint -- pg_aux_heads_forward, one launch, with the
tolerance of the climate and month argmaxes taking part in the decision which rows go to the exact tier).  `hierarchical=True`
and the 1026-wide heading head (`heading=True` without `panorama`) raise NotImplementedError: the reference's final model uses
neither (models/README.md).  Training is out of scope: the losses are computed for logging only.
"""
from __future__ import annotations

import math
import os
from collections import namedtuple

import numpy as np
import pandas as pd
import torch
from torch import nn, Tensor
from torch.nn.parameter import Parameter

from . import hip_ops
from .certainty import SAFETY, CalibrationError, Certainty, require_fingerprint
from .geo_utils import haversine_matrix, smooth_labels
from .clip_embedder import HipCLIPVisionModel, check_pixel_bytes, exclusive_pixel_bytes
from .config import CLIP_EMBED_DIM, GEOCELL_PATH, GEOCELL_PATH_YFCC
from .utils import ModelOutput, TopK, resolve_name

# reference models/super_guessr.py:12-23
MultiTaskPredictions = namedtuple('MultiTaskPredictions', 'loss_reg preds_mt loss_climate preds_climate loss_month preds_month')
# what `SuperGuessr.attribute` returns: maps (B,P,577,K), offset (B,K), cells (B,K), against (B,), logits (B,K)
Attribution = namedtuple('Attribution', 'maps offset cells against logits')
# what `SuperGuessr.spread` returns: expected_km (B,) / (B,G), expected_score likewise, radius_km (B,nq) / (B,G,nq), the quantiles
Spread = namedtuple('Spread', 'expected_km expected_score radius_km quantiles')
# what `SuperGuessr.best_guess` returns: index (B,) int64 of the best candidate (-1: none), point (B,2) fp64 the chosen [lng, lat],
# expected (B,) fp64 the best candidate's expectation, incumbent_expected (B,) fp64 the incumbent's, taken (B,) bool
BestGuess = namedtuple('BestGuess', 'index point expected incumbent_expected taken')
GUESS_OBJECTIVES = ('score', 'km')
NUM_MULTI_TASK_VARIABLES = 6
REGRESSION_LOSS_SCALING = 8
NUM_CLIMATES = 28
CLIMATE_LOSS_SCALING = 2
NUM_MONTHS = 12
MONTHS_LOSS_SCALING = 1


# candidates the head computes beyond `num_candidates`: never exposed, they tell the certainty pass how far the next cells are
EXTRA_CANDIDATES = 4


class SuperGuessr(nn.Module):
    def __init__(self, base_model: nn.Module, panorama: bool = False, hierarchical: bool = False,
                 should_smooth_labels: bool = False, multi_task: bool = False, heading: bool = False,
                 yfcc: bool = False, serving: bool = False, freeze_base: bool = False,
                 num_candidates: int = 5, embed_dim: int = CLIP_EMBED_DIM, **kwargs):
        """Same arguments as reference models/super_guessr.py:31-34.

        base_model: None (run on precomputed embeddings), a `HipCLIPVisionModel`, or any module exposing a
        transformers-CLIPVisionModel state dict (e.g. a HuggingFace CLIPVisionModel): its weights are packed
        into the HIP encoder on first use.
        One extra keyword, `geocell_path`, overrides config.GEOCELL_PATH(_YFCC) (the reference hard-wires the
        path through its config module, :87-88).

        The geocell argmax is the reference's for every sample called certain -- a z ~ 4 statistical statement, see pigeon_amd/certainty.py
        -- and for the re-encoded ones (round 5: on by default).  The reference's `torch.argmax(geocell_probs)`
        (:454) is fp32 end to end; this path's embeddings carry the rounding of 16-bit MFMA operands (2.7e-4 relative on default-init
        weights, 7e-4 on a high-gain tower), so a sample whose margins are smaller than what that error moves could come out with a
        runner-up.  Every forward therefore measures, per sample, the TOLERANCE of its top-1 against every other cell
        (pg_head_certainty; error model and calibration: pigeon_amd/certainty.py) and -- `exact_top1`, default True, env
        PIGEON_EXACT_TOP1=0 switches it off -- re-encodes the samples that are not certain FROM THEIR PIXELS in the encoder's exact mode
        (pg_vit_forward_precise: split-fp16 GEMM operands, fp32 attention; ~2e-6 relative) and recomputes their head outputs.
        After every forward (ModelOutput keeps its 12 fields):
          .last_tol      (B,) fp32  the tolerance (see certainty.py), compared with .certainty.threshold()
          .last_certain  (B,) bool  the top-1 is the reference's (after the re-encode: judged at the exact tier's floor)
          .last_margin   (B,) fp32  logit(top-1) - logit(top-2);  .last_bound (B,) fp32 the margin change the threshold stands for
          .last_reencoded (n,) int64  the samples the exact tier re-encoded (empty when it is off)
        With a ProtoRefiner, `pigeon_amd.evaluate.certain_forward` extends the same statement to the refined cell and point.
        Caller-supplied `embedding`s are judged against `embedding_rel_tol`.  Without the keyword that is the fast path's tolerance
        in force at the time of the call (`certainty.rel_tol`: 1e-3 uncalibrated, the calibrated value afterwards) -- what embeddings
        written by the 16-bit encoder (`run.py embed`) carry; a loaded calibration file sets 1.1 x its `image_residual_rms` instead.
        A caller whose embeddings come from the exact encoder (or the fp32 reference) says so: `embedding_rel_tol=5e-6`, the value
        of `margin_rel_tol_exact`.  An explicit keyword always wins.
        Extra keywords: `debias` (default True / env PIGEON_DEBIAS: the calibrated systematic part of the 16-bit encoder's error is
        subtracted from every fast embedding -- pg_embedding_debias -- instead of only being accounted for in the certainty test),
        `exact_top1`, `margin_kappa` (z-score, default 3.6), `margin_rel_tol` (default 1e-3 = the contract's embedding
        tolerance until `calibrate_certainty` -- called explicitly, or by the first forward that sees >= 8 samples with pixels, or
        once 16 samples have come in through smaller batches -- replaces it by the measured error of THIS set of weights), `margin_rel_tol_exact` (5e-6).
        `calibration` (a path): `load_calibration(path)` at the end of construction -- the stored measurement instead of one taken
        inside the first forward(s); without it nothing changes.
        """
        super(SuperGuessr, self).__init__()
        geocell_path = kwargs.pop('geocell_path', None)
        calibration = kwargs.pop('calibration', None)
        exact_top1 = kwargs.pop('exact_top1', None)
        self.exact_top1 = (os.environ.get('PIGEON_EXACT_TOP1', '1') not in ('', '0')) if exact_top1 is None else bool(exact_top1)
        self.certainty = Certainty(kappa=float(kwargs.pop('margin_kappa', os.environ.get('PIGEON_MARGIN_KAPPA', 3.6))),
                                   rel_tol=float(kwargs.pop('margin_rel_tol', os.environ.get('PIGEON_MARGIN_REL_TOL', 1e-3))),
                                   rel_tol_exact=float(kwargs.pop('margin_rel_tol_exact', 5e-6)), debias=kwargs.pop('debias', None))
        self.margin_autocalibrate = bool(kwargs.pop('margin_autocalibrate', True))
        self.embedding_rel_tol = kwargs.pop('embedding_rel_tol', None)     # None: the fast path's tolerance at the time of the call
        self.last_margin = self.last_certain = self.last_tol = None
        self.last_state = None
        if len(kwargs) > 0:
            print(f'Not using keyword arguments: {list(kwargs.keys())}')
        if hierarchical:
            raise NotImplementedError('pigeon_amd.SuperGuessr: hierarchical=True (the self-attention combiner of the four panels, '
                                      'models/super_guessr.py:95-103,417-433) is not implemented; the reference\'s final model '
                                      'averages the panels (hierarchical=False)')
        if heading and not panorama:
            raise NotImplementedError('pigeon_amd.SuperGuessr: heading=True without panorama=True (the 1026-wide cell_layer fed with '
                                      'the compass heading, models/super_guessr.py:90-92,276-297) is not implemented; with '
                                      'panorama=True the heading is ignored, as in the reference (:273-274)')

        self.base_model = base_model
        self.panorama = panorama
        self.hidden_size = embed_dim
        self.serving = serving
        self.should_smooth_labels = should_smooth_labels
        self.multi_task = multi_task
        self.heading = heading
        self.yfcc = yfcc
        self.freeze_base = freeze_base
        self.hierarchical = hierarchical
        self.num_candidates = num_candidates

        self._set_hidden_size()
        if geocell_path is None:
            geocell_path = GEOCELL_PATH_YFCC if self.yfcc else GEOCELL_PATH
        self.lla_geocells = self.load_geocells(geocell_path)
        self.num_cells = self.lla_geocells.size(0)
        # how far every cell reaches from its centroid, km (`spread`): not persistent, the state dict keeps the reference's keys
        self.register_buffer('cell_extent_km', self.load_cell_extents(geocell_path), persistent=False)
        self.input_dim = self.hidden_size

        self.cell_layer = nn.Linear(self.input_dim, self.num_cells)
        self.softmax = nn.Softmax(dim=-1)
        if self.multi_task:                                  # :110-124, under the reference's attribute names (= state dict keys)
            print('Model is multi-task.')
            self.multi_task_head = nn.Linear(self.hidden_size, NUM_MULTI_TASK_VARIABLES)
            self.loss_fnc_mt = nn.MSELoss(reduction='mean')
            self.climate_layer = nn.Linear(self.input_dim, NUM_CLIMATES)
            self.loss_fnc_climate = nn.CrossEntropyLoss()
            if not self.yfcc:
                self.month_layer = nn.Linear(self.input_dim, NUM_MONTHS)
                self.loss_fnc_month = nn.CrossEntropyLoss()
        self._aux_pack = None                                # (key, W (A,1024), bias (A,)): see _aux_weights()
        self._freeze_params()
        self.loss_fnc = nn.CrossEntropyLoss()
        self._hip_base = None
        self._wnorm = {}                                     # exact? -> (key, device tensor): see wstats()
        self._cal_buffer = []                                # pixels of small first batches, until there are enough to calibrate on
        self._engines = {}                                   # refiner -> settle-before-return engine (see `engine`)
        self._guess_tables = {}                              # objective -> (key, candidates, table): see best_guess()
        self._temperature = 1.0                              # see `temperature`
        self.temperature_fit = None                          # the TemperatureFit behind it, when it came from a sidecar
        self._last_exact = None
        self._rel_tol0 = self.certainty.rel_tol              # the constructor's uncalibrated tolerance: what a weight load goes back to
        if self.exact_top1 and isinstance(self.base_model, HipCLIPVisionModel):
            self.base_model.enable_precise(True)             # pack the split-weight copy with the first build, not inside a request
        self._embedding_rel_tol0 = None                      # (`embedding_rel_tol` as given, None included,) before a calibration file set it: load_state gives it back
        self.calibration_header = None                       # header of the calibration file in force (None: none loaded)
        print(f'Initialized SuperGuessr classification model with {self.num_cells} geocells.')
        if calibration is not None:
            self.load_calibration(calibration)

    # legacy names of the certainty parameters (round 4)
    @property
    def margin_kappa(self) -> float:
        return self.certainty.kappa

    @margin_kappa.setter
    def margin_kappa(self, v: float):
        self.certainty.kappa = float(v)

    @property
    def margin_rel_tol(self) -> float:
        return self.certainty.rel_tol

    @margin_rel_tol.setter
    def margin_rel_tol(self, v: float):
        self.certainty.rel_tol = float(v)

    @property
    def margin_rel_tol_exact(self) -> float:
        return self.certainty.rel_tol_exact

    @property
    def embedding_rel_tol(self) -> float:
        """What caller-supplied embeddings are judged against: the explicit value (constructor keyword, assignment, or a calibration
        file loaded without a base model), else the fast path's tolerance as it is NOW."""
        return self.certainty.rel_tol if self._embedding_rel_tol is None else self._embedding_rel_tol

    @embedding_rel_tol.setter
    def embedding_rel_tol(self, v):
        self._embedding_rel_tol = None if v is None else float(v)

    @property
    def temperature(self) -> float:
        """The temperature T of the calibrated probabilities softmax(logits / T) that `spread` and `best_guess` integrate over
        (pigeon_amd/temperature.py fits it; default 1.0: the head's own softmax, and nothing new runs).  Unchanged at any
        temperature, and reference-parity: the argmax, the top-k indices, the `topk_values` the reference's outputs carry, the
        refiner's inputs and every certainty computation -- they read the head's own logits."""
        return self._temperature

    @temperature.setter
    def temperature(self, v: float):
        v = float(v)
        if not (math.isfinite(v) and v > 0):
            raise ValueError(f'SuperGuessr.temperature must be a finite positive number, got {v!r}')
        self._temperature = v
        self.temperature_fit = None

    def load_temperature(self, path_or_number) -> float:
        """Set `temperature` from a number or from the sidecar `pigeon_amd.temperature.save` wrote for THIS head (ValueError naming
        both fingerprints for another head's).  Load it after the weights."""
        from . import temperature as _temperature
        if isinstance(path_or_number, (int, float)):
            self.temperature = path_or_number
            return self._temperature
        try:
            number = float(path_or_number)
        except (TypeError, ValueError):
            number = None
        if number is not None:
            self.temperature = number
            return self._temperature
        fit = _temperature.load(path_or_number, self)
        self.temperature = fit.temperature
        self.temperature_fit = fit
        return self._temperature

    def _calibrated_logits(self, st: dict) -> Tensor:
        """The logits `spread` and `best_guess` integrate over: the state's own at temperature 1.0 (nothing runs, nothing is kept),
        else logits * float32(1 / T) -- one pg_temper_logits launch per state and temperature, cached in the state."""
        logits = st['logits']
        if self._temperature == 1.0:
            return logits
        key = (self._temperature, logits.data_ptr(), tuple(logits.shape), logits._version)
        hit = st.get('calibrated_logits')
        if hit is None or hit[0] != key:
            hit = st['calibrated_logits'] = (key, hip_ops.temper_logits(logits, 1.0 / self._temperature))
        return hit[1]

    def _set_hidden_size(self):
        if self.base_model is not None:
            self.hidden_size = self.base_model.config.hidden_size
            self.mode = 'transformer'

    def _freeze_params(self):
        if self.base_model is not None and self.freeze_base:
            for param in self.base_model.parameters():
                param.requires_grad = False

    def load_geocells(self, path: str) -> Tensor:
        """reference models/super_guessr.py:162-174: CSV columns lng,lat -> (C,2) float64 Parameter"""
        geo_df = pd.read_csv(path)
        lla_coords = torch.tensor(np.ascontiguousarray(geo_df[['lng', 'lat']].values))
        return nn.parameter.Parameter(data=lla_coords, requires_grad=False)

    def load_cell_extents(self, path: str) -> Tensor:
        """(C,) float64 km: with a `polygon` column (the one `RegionBank.from_geocell_csv` reads) the haversine distance from every
        cell's centroid to its farthest ring vertex, computed once on the host (pigeon_amd.regions.cell_extents_km); zeros without."""
        centroids = self.lla_geocells.data.cpu().numpy()
        if 'polygon' not in pd.read_csv(path, nrows=0).columns:
            return torch.zeros((centroids.shape[0],), dtype=torch.float64)
        from .regions import RegionBank, cell_extents_km
        try:
            return torch.from_numpy(cell_extents_km(RegionBank.from_geocell_csv(path), centroids))
        except ValueError as why:                        # a table whose polygons do not parse still serves every other entry point
            print(f'Cell extents: the `polygon` column of {path} could not be read ({why}); using 0 km')
            return torch.zeros((centroids.shape[0],), dtype=torch.float64)

    def load_state(self, path: str):
        """reference models/super_guessr.py:222-238: name-wise copy of a saved state dict"""
        own_state = self.state_dict()
        state_dict = torch.load(path, map_location=torch.device('cuda') if torch.cuda.is_available() else 'cpu')
        matched = 0
        for name, param in state_dict.items():
            name = resolve_name(name, own_state)         # transformers 4.23.1 `base_model.vision_model.*` -> `base_model.*`
            if name not in own_state:
                print(f'Parameter {name} not in model\'s state.')
                continue
            if isinstance(param, Parameter):
                param = param.data
            own_state[name].copy_(param)
            matched += 1
        if len(state_dict) > 0 and matched == 0:
            raise KeyError(f'load_state: none of the {len(state_dict)} parameters in {path} matched the model')
        self._hip_base = None
        if isinstance(self.base_model, HipCLIPVisionModel):
            self.base_model._weights_changed()
        # other weights: the measured error is void -- back to the constructor's tolerance (not a hard-coded one), nothing half-collected
        # (a calibration LOADED from a file goes the same way: it is keyed to the weights that have just been replaced -- load it again
        # after the weights, `evaluate()` does it in that order)
        self.certainty = Certainty(self.certainty.kappa, self._rel_tol0, self.certainty.rel_tol_exact, debias=self.certainty.debias)
        if self._embedding_rel_tol0 is not None:
            self.embedding_rel_tol, self._embedding_rel_tol0 = self._embedding_rel_tol0[0], None
        self.calibration_header = None
        self._cal_buffer = []
        self._engines = {}
        self._aux_pack = None
        if self.temperature_fit is not None:             # a sidecar's temperature is keyed to the head that has just been replaced
            self._temperature, self.temperature_fit = 1.0, None

    def state_dict(self, *args, **kwargs):
        sd = super().state_dict(*args, **kwargs)
        sd.pop('base_model._dummy', None)
        if isinstance(self.base_model, HipCLIPVisionModel):
            sd.update(self.base_model.state_dict(prefix='base_model.'))
        return sd

    # ------------------------------------------------------------------------------------------ hot path
    def _encoder(self) -> HipCLIPVisionModel:
        if isinstance(self.base_model, HipCLIPVisionModel):
            return self.base_model
        if self._hip_base is None:                       # e.g. a transformers CLIPVisionModel: pack its weights once
            self._hip_base = HipCLIPVisionModel(self.base_model.state_dict())
            if self.exact_top1:
                self._hip_base.enable_precise(True)
            self._hip_base.to(self.cell_layer.weight.device)
        return self._hip_base

    def _embed(self, px: Tensor, exact: bool = False, out: Tensor = None) -> Tensor:
        """(N,3,336,336) device pixels, float or uint8 bytes (what `encode_head` made of `pixel_bytes`), through the fast or exact encoder."""
        enc = self._encoder()
        kw = {'pixel_bytes': px} if px.dtype == torch.uint8 else {'pixel_values': px}
        return enc.embed_precise(out=out, **kw) if exact else enc.embed(**kw)

    def _check_pixel_bytes(self, pixel_bytes, pixel_values=None, embedding=None) -> None:
        """`pixel_bytes` by name, before anything else happens: alone, uint8 (B,12,336,336) [panorama] or (B,3,336,336), contiguous."""
        if pixel_bytes is None:
            return
        exclusive_pixel_bytes(pixel_bytes, pixel_values=pixel_values, embedding=embedding)
        check_pixel_bytes(pixel_bytes)
        if self.base_model is None:
            raise ValueError('pixel_bytes needs a base model: this SuperGuessr takes embeddings')
        views = 12 if self.panorama else 3
        if pixel_bytes.shape[1] != views:
            raise ValueError(f'pixel_bytes must be (B,{views},336,336) for a {"panorama" if self.panorama else "single-image"} model, '
                             f'got shape {tuple(pixel_bytes.shape)}')

    def _assert_requirements(self, pixel_values=None, embedding=None, heading=None):
        if self.base_model is not None:
            assert pixel_values is not None, 'Parameter "pixel_values" must be supplied if model has a base model.'
        else:
            assert embedding is not None, 'Parameter "embedding" must be supplied if model does not have a base model.'

    def _to_one_hot(self, tensor: Tensor) -> Tensor:
        if tensor.dim() == 0:
            one_hot = torch.zeros(self.num_cells, device=tensor.device)
            one_hot[tensor.item()] = 1
            return one_hot
        return tensor

    def wstats(self, exact: bool = False) -> Tensor:
        """(2,) fp32 on the head's device: [largest row norm of cell_layer.weight, max over cells of |W[c] . drift|] -- what bounds
        |W[a] - W[c]| and (W[a] - W[c]).drift for the cells the certainty pass does not visit one by one (pg_head_wstats).  `exact`: the
        exact tier has no systematic part (second entry 0).  Recomputed when the weight tensor (in-place edits bump its version) or the
        calibrated drift changes."""
        W = self.cell_layer.weight
        drift = None if exact else self.certainty.drift_on(W.device)
        key = (W.data_ptr(), W._version, str(W.device), None if drift is None else (drift.data_ptr(), drift._version))
        if not isinstance(self._wnorm, dict):
            self._wnorm = {}
        hit = self._wnorm.get(exact)
        if hit is None or hit[0] != key:
            Wd = W.data if W.dtype == torch.float32 else W.data.float()
            self._wnorm[exact] = (key, hip_ops.head_wstats(Wd.contiguous(), drift))
        return self._wnorm[exact][1]

    def _aux_layers(self):
        return [self.multi_task_head, self.climate_layer] + ([] if self.yfcc else [self.month_layer])

    def _aux_weights(self):
        """(W (A,1024), bias (A,)) fp32 on the head's device: the rows of multi_task_head, climate_layer and month_layer one after the
        other, as pg_aux_heads_forward takes them.  Packed once; packed again when any of the layers' tensors is replaced, edited in
        place (its version) or moved."""
        ts = [t for l in self._aux_layers() for t in (l.weight, l.bias)]
        key = tuple((t.data_ptr(), t._version, str(t.device), t.dtype) for t in ts)
        if self._aux_pack is None or self._aux_pack[0] != key:
            dev = self.cell_layer.weight.device
            W = torch.cat([l.weight.data.to(dev, torch.float32) for l in self._aux_layers()]).contiguous()
            b = torch.cat([l.bias.data.to(dev, torch.float32) for l in self._aux_layers()]).contiguous()
            self._aux_pack = (key, W, b)
        return self._aux_pack[1], self._aux_pack[2]

    def _panels(self) -> int:
        return 4 if self.panorama else 1

    def _head_rows(self, layer_input: Tensor) -> Tensor:
        if self.panorama:
            head_in = layer_input if layer_input.dim() == 3 else layer_input[:, None, :]   # mean over panels :437
        elif layer_input.dim() == 3 and layer_input.size(1) == 4:
            head_in = layer_input[:, 0].contiguous()                            # :440-441
        else:
            head_in = layer_input
        return head_in.contiguous()

    def _head_with_tol(self, head_in: Tensor, exact: bool) -> dict:
        """cell_layer + softmax + top-(k + extra) + argmax + centroid gather (:447-459), and the tolerance of the top-1."""
        W = self.cell_layer.weight.data
        kx = min(self.num_cells, self.num_candidates + EXTRA_CANDIDATES)
        o = hip_ops.head_forward(head_in, W, self.cell_layer.bias.data, self.lla_geocells.data, kx)
        drift = None if exact else self.certainty.drift_on(W.device)
        o['tol'], o['code'], o['margin'], o['sens'] = hip_ops.head_certainty(o['logits'], head_in, W, o['topk_indices'], drift,
                                                                             self.wstats(exact))
        if self.multi_task:
            # :333-338 the regression, climate and month layers on the same rows, one launch.  The climate and month argmaxes
            # (evaluation/metrics.py:187,198) are discrete outputs like the top-1 cell: their tolerance lowers the row's (`row_tol`,
            # in place), so a row that only they cannot settle goes to the exact tier too
            Wa, ba = self._aux_weights()
            a = hip_ops.aux_heads_forward(head_in, Wa, ba, NUM_MULTI_TASK_VARIABLES, NUM_CLIMATES, 0 if self.yfcc else NUM_MONTHS,
                                          drift=drift, row_tol=o['tol'])
            o['aux_preds'], o['aux_cls'], o['aux_tol'], o['aux_code'] = a['preds'], a['cls'], a['tol'], a['code']
        return o

    @torch.no_grad()
    def encode_head(self, pixel_values: Tensor = None, embedding: Tensor = None, pixel_bytes: Tensor = None) -> dict:
        """Fast pass: ViT + token mean (:395-398), head, tolerance of the top-1.  No re-encode.  Returns the step's STATE: a dict
        with `embedding` (as ModelOutput carries it), `head_in`, the head outputs over k + extra candidates (`topk_values`,
        `topk_indices`, `logits`, `preds_geocell`, `preds_LLH`), `tol`, `certain`, `exact` (rows on the exact tier: none yet) and
        `pixel_values` (the reshaped device pixels, or None).  `package` turns it into the reference's outputs; pigeon_amd.deferred.DeferredExact
        settles the rows that are not certain.  `pixel_bytes` (uint8 (B,12,336,336) / (B,3,336,336), instead of the other two): the
        8-bit pixels in front of the normalisation table; the state's `pixel_values` then holds those bytes, and the exact tier
        re-encodes from them."""
        self._check_pixel_bytes(pixel_bytes, pixel_values, embedding)
        dev = self.cell_layer.weight.device
        px = None
        if pixel_bytes is not None:
            pixel_values = pixel_bytes
        if self.panorama and pixel_values is not None:                          # :386-388
            num_samples = pixel_values.size(0)
            pixel_values = pixel_values.reshape((num_samples * 4, 3, 336, 336))
        if self.base_model is not None and pixel_values is not None:
            if pixel_values.dim() > 4:
                pixel_values = pixel_values.squeeze(1)                          # :392-393
            px = pixel_values.to(dev)
            if pixel_bytes is None and px.dtype == torch.uint8:
                px = px.float()                          # a uint8 tensor under the name pixel_values is numbers, as it always was: bytes come as pixel_bytes
            if self.exact_top1 and self.margin_autocalibrate and not self.certainty.calibrated:
                self._autocalibrate(px)
            # a tower on which the calibration measured the 16-bit path OUTSIDE the embedding contract: every sample through the exact encoder
            exact_tier = bool(self.certainty.force_exact and self.exact_top1)
            embedding = self._embed(px, exact=exact_tier)                       # :395-398 (ViT + token mean)
            bias = None if exact_tier else self.certainty.bias_on(dev)
            if bias is not None:
                # the 16-bit encoder's measured systematic error, taken out of every image's embedding (pigeon_amd/certainty.py `debias`):
                # what the head, the refiner and the caller see is the corrected embedding; the certainty kernels get no drift
                hip_ops.embedding_debias(embedding, bias)
            if self.panorama:
                embedding = embedding.reshape((num_samples, 4, embedding.shape[-1]))   # :404-405 (explicit width: B = 0 stays legal)
        else:
            embedding = embedding.to(dev, torch.float32).contiguous()
            exact_tier = False
        head_in = self._head_rows(embedding)
        # Which error the tolerances are compared with: the calibrated fast-path error (pixels through the 16-bit encoder), the exact
        # tier's floor (pixels through the exact encoder), or -- caller-supplied embeddings, which carry no error of THIS forward --
        # `embedding_rel_tol` (default: the fast path's tolerance, since `run.py embed` writes the 16-bit path's embeddings; whoever
        # feeds exact ones declares it with the keyword).  No systematic part in the last two cases.
        at_floor = exact_tier or px is None
        st = self._head_with_tol(head_in, exact=at_floor)
        st['embedding'], st['head_in'], st['pixel_values'], st['exact_tier'] = embedding, head_in, px, exact_tier
        st['thr'] = (self.certainty.kappa * self.embedding_rel_tol) if px is None else self.certainty.threshold(exact=exact_tier)
        st['drift'] = None if at_floor else self.certainty.drift_on(dev)
        st['wstats'] = self.wstats(at_floor)
        return st

    @torch.no_grad()
    def exact_rows(self, pixel_rows) -> dict:
        """The exact tier for queued rows (pigeon_amd.deferred): `pixel_rows` is a list of (n_i, P*3*336*336) pixel-row tensors (the two
        segments of a circular queue); they go through pg_vit_forward_precise, the head and the tolerance pass at the exact tier's
        floor.  Returns the head state of the n = sum n_i rows (`embedding` as ModelOutput carries it)."""
        P = self._panels()
        n = sum(int(t.shape[0]) for t in pixel_rows)
        dev = self.cell_layer.weight.device
        emb = torch.empty((n * P, CLIP_EMBED_DIM), dtype=torch.float32, device=dev)
        off = 0
        for t in pixel_rows:
            m = int(t.shape[0])
            if m:
                self._embed(t.reshape((m * P, 3, 336, 336)), exact=True, out=emb[off * P:(off + m) * P])
            off += m
        if self.panorama:
            emb = emb.reshape((n, P, CLIP_EMBED_DIM))
        o = self._head_with_tol(self._head_rows(emb), exact=True)
        o['embedding'] = emb
        return o

    @torch.no_grad()
    def attribute(self, pixel_values: Tensor = None, pixel_bytes: Tensor = None, cells=None, k: int = 1, against='runner_up',
                  tier: str = 'fast') -> Attribution:
        """WHY a cell: each geocell logit -- or the difference of two -- as an exact sum over the views' tokens.

        The embedding is the plain mean of the 577 rows of last_hidden_state (:398) and the head one Linear over the mean of the views
        (:437, :447), so for g = W[cell] - W[against]
            logit[cell] - logit[against] = (b[cell] - b[against]) + sum_p sum_t h[p,t,:] . g / (577 P)
        is an identity: the class-activation map of a mean-pooled linear head.  One encoder pass that keeps the hidden states
        (`tier='fast'`: pg_vit_forward_hidden, `tier='exact'`: pg_vit_forward_precise; a tower whose calibration sends every sample to the
        exact encoder is attributed there whatever `tier` says, as `encode_head` encodes it), the embedding treated as `encode_head`
        treats it (pg_embedding_debias on the fast tier when a calibrated bias is loaded), pg_head_forward, and pg_token_attribution
        over the hidden rows.  Returns `Attribution`:
          maps    (B,P,577,K) fp32  the summands; token 0 is the class token, token 1 + 24 y + x the patch in row y, column x of the
                                    336 x 336 crop (pigeon_amd/explain.py `patch_grid`); P = 4 views, 1 with panorama=False
          offset  (B,K) fp32        everything that is not a token: b[cell] - b[against] and, on a de-biased fast pass,
                                    -(1/P) sum_p |e_p|_2 (g . beta) for the bias vector beta the embeddings had subtracted
          cells   (B,K) int64       `cells` as given, or with cells=None this pass's top-`k` cells (k <= 16)
          against (B,) int64        -1: none (the maps explain logit[cell] itself)
          logits  (B,K) fp32        the model's own logit[cell] - logit[against] of this pass (pg_head_forward's fp32 logits)
        so that maps.sum((1,2)) + offset reproduces logits up to fp32 summation error.
        `against`: None; a (B,) tensor of cells (-1: none for that sample); or 'runner_up' (default): the pass's top-2 cell -- the
        direction W[top1] - W[top2] is the one the certainty contract reasons about -- except for a sample whose FIRST listed cell is
        that runner-up itself, which is compared against the top-1.  A column whose cell equals `against` is exact zeros.  With a single
        geocell there is no runner-up (-1).  A listed index outside [0, C) gives NaN in its column (its sample, for `against`) of maps,
        offset and logits.
        Images go through the encoder in chunks of at most 128 (the hidden states of a chunk are 0.28 GiB).  The call is read-only on
        the object: it neither starts nor feeds the auto-calibration, leaves `last_*` alone and queues nothing on the deferred engine."""
        self._check_pixel_bytes(pixel_bytes, pixel_values, None)
        if self.base_model is None:
            raise ValueError('attribute needs a base model: the attribution is over the encoder\'s tokens')
        if (pixel_values is None) == (pixel_bytes is None):
            raise ValueError('attribute: exactly one of pixel_values and pixel_bytes')
        if tier not in ('fast', 'exact'):
            raise ValueError(f"attribute: tier must be 'fast' or 'exact', got {tier!r}")
        if not self.cell_layer.weight.is_cuda:
            raise RuntimeError('pigeon_amd.SuperGuessr runs on the GPU only: call .to("cuda") first (no CPU fallback)')
        if not (against is None or torch.is_tensor(against) or against == 'runner_up'):
            raise ValueError(f"attribute: against must be 'runner_up', None or a (B,) tensor, got {against!r}")
        dev = self.cell_layer.weight.device
        P, Cn = self._panels(), self.num_cells
        px = pixel_bytes if pixel_bytes is not None else pixel_values
        px = px.reshape((-1, 3, 336, 336)).to(dev)
        if pixel_bytes is None and px.dtype == torch.uint8:
            px = px.float()                              # (pixel_values: numbers, as in `encode_head`)
        if px.shape[0] % P:
            raise ValueError(f'attribute: {px.shape[0]} images are not whole samples of {P} views')
        B = px.shape[0] // P
        if cells is not None:
            cells = torch.as_tensor(cells, dtype=torch.int64).to(dev).reshape((B, -1)).contiguous()
            k = int(cells.shape[1])
        if not 1 <= int(k) <= 16 or (cells is None and k > Cn):
            raise ValueError(f'attribute: k = {k} cells per sample (1..16, at most the {Cn} geocells)')
        if torch.is_tensor(against):
            against = against.to(dev, torch.int64).reshape((B,)).contiguous()
        exact = tier == 'exact' or bool(self.certainty.force_exact and self.exact_top1)
        base = self._encoder()
        px = base._pixels(None, px) if pixel_bytes is not None else base._pixels(px, None)
        if exact:
            base.enable_precise(True)
        enc = base._encoder(px.device)
        W = self.cell_layer.weight.data
        W = (W if W.dtype == torch.float32 else W.float()).contiguous()
        hb = self.cell_layer.bias.data.float()
        beta = None if exact else self.certainty.bias_on(dev)
        per = max(1, 128 // P)                           # samples per chunk: at most 128 images
        parts = []
        for s0 in range(0, B, per):
            n = min(per, B - s0)
            chunk = px[s0 * P:(s0 + n) * P].contiguous()
            emb, hid = (enc.forward_precise if exact else enc.forward)(chunk, return_hidden=True)
            norms = None
            if beta is not None:
                norms = emb.double().norm(dim=1).reshape((n, P))       # |e_p|_2 of the embeddings as the encoder wrote them
                hip_ops.embedding_debias(emb, beta)
            head_in = self._head_rows(emb.reshape((n, 4, emb.shape[-1])) if self.panorama else emb)
            o = hip_ops.head_forward(head_in, W, hb, self.lla_geocells.data, min(Cn, max(2, k)))
            top = o['topk_indices']
            c = top[:, :k].contiguous() if cells is None else cells[s0:s0 + n]
            if torch.is_tensor(against):
                a = against[s0:s0 + n]
            elif against is None or Cn < 2:
                a = torch.full((n,), -1, dtype=torch.int64, device=dev)
            else:                                        # 'runner_up'
                a = torch.where(c[:, 0] == top[:, 1], top[:, 0], top[:, 1]).contiguous()
            maps = hip_ops.token_attribution(hid, W, c, a, panels=P)
            del hid
            # the model's own logit differences and the part that is no token; an index the kernel refuses is NaN here too
            c_ok, a_none = (c >= 0) & (c < Cn), a == -1
            ok = c_ok & (a_none | ((a >= 0) & (a < Cn)))[:, None]
            cc, ac = c.clamp(0, Cn - 1), a.clamp(0, Cn - 1)
            lg = o['logits']
            nan = torch.full((), float('nan'), dtype=torch.float32, device=dev)
            la = torch.where(a_none, torch.zeros((), device=dev), lg.gather(1, ac[:, None])[:, 0])
            diff = torch.where(ok, lg.gather(1, cc) - la[:, None], nan)
            off = hb[cc].double() - torch.where(a_none, torch.zeros((), dtype=torch.float64, device=dev), hb[ac].double())[:, None]
            if beta is not None:
                g = W[cc] - torch.where(a_none[:, None], torch.zeros((), device=dev), W[ac])[:, None, :]      # (n,K,1024) fp32, as the kernel forms it
                off = off - norms.mean(dim=1)[:, None] * (g.double() * beta.double()).sum(dim=-1)
            parts.append((maps, torch.where(ok, off.float(), nan), c, a, diff))
        if not parts:
            z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device=dev)
            return Attribution(z(0, P, 577, k), z(0, k), z(0, k, dt=torch.int64), z(0, dt=torch.int64), z(0, k))
        return Attribution(*(torch.cat([p[i] for p in parts]) if len(parts) > 1 else parts[0][i] for i in range(5)))

    @torch.no_grad()
    def spread(self, points: Tensor = None, quantiles=(0.5, 0.9), state: dict = None) -> Spread:
        """How far off a guess may be (pg_guess_spread; contract: include/pigeon_hip.h), from the geocell logits of `state` -- default
        `last_state`, what the last forward left behind, with re-encoded rows carrying their exact-tier logits.  With a `temperature`
        other than 1.0 the probabilities are the calibrated softmax(logits / T); the argmax, the top-k, `topk_values`, the refiner's
        inputs and the certainty computations stay the head's own (reference-parity).
          points     (B,2) or (B,G,2) [lng, lat], G candidate guesses per sample; None: the state's own `preds_LLH`
          quantiles  1 .. 4 numbers in (0, 1]
        Returns Spread(expected_km, expected_score, radius_km, quantiles), float64 device tensors: under the head's softmax, the expected
        distance in km and the expected GeoGuessr score (before its rounding) of each point, and per quantile q the radius of the
        smallest circle around the point that holds, whole, cells carrying q of the probability.  "Whole" counts a cell at its
        centroid's distance plus `cell_extent_km`; without a `polygon` column the extents are 0, the mass sits at the centroids, and a
        confident head asked about its own centroid gets a radius of 0 (to the distance kernel's 1e-11 km), not the cell's size.
        Nothing is synchronised; nothing is computed unless this is called."""
        st = self.last_state if state is None else state
        if st is None:
            raise RuntimeError('SuperGuessr.spread: no state -- run a forward first, or pass `state`')
        logits = self._calibrated_logits(st)
        pts = st['preds_LLH'] if points is None else torch.as_tensor(points).to(logits.device, torch.float64)
        ek, es, rk = hip_ops.guess_spread(logits, self.lla_geocells.data, pts.contiguous(), quantiles, extent_km=self.cell_extent_km)
        return Spread(ek, es, rk, tuple(float(q) for q in quantiles))

    @torch.no_grad()
    def confidence(self, state: dict = None) -> Tensor:
        """(B,) fp64: the calibrated probability of the top-1 cell, 1 / sum_c exp((l_c - max l) / T) -- pg_temper_stats's `conf` at
        beta = 1 / `temperature`, one row pass over the logits of `state` (default `last_state`).  NaN for a row with a NaN or +inf
        logit.  Nothing is synchronised; nothing is computed unless this is called."""
        st = self.last_state if state is None else state
        if st is None:
            raise RuntimeError('SuperGuessr.confidence: no state -- run a forward first, or pass `state`')
        r = hip_ops.temper_stats(st['logits'], st['preds_geocell'].contiguous(), [1.0 / self._temperature], conf=True)
        return r['conf'][:, 0]

    def _guess_table(self, candidates, objective: str, device):
        """(candidates (M,2) fp64 on `device`, table (M,C) fp64) of `best_guess`: pg_score_table, built on first use and kept per
        objective until the candidate tensor (its identity, version, storage or device) or the centroids change."""
        src = self.lla_geocells if candidates is None else candidates
        cen = self.lla_geocells
        key = (id(src), src._version, src.data_ptr(), tuple(src.shape), src.dtype, str(src.device), cen._version, cen.data_ptr(), str(device))
        hit = self._guess_tables.get(objective)
        if hit is not None and hit[0] == key:
            return hit[2], hit[3]
        cand = src.detach().to(device, torch.float64).contiguous()
        if cand.dim() != 2 or cand.shape[1] != 2:
            raise ValueError(f'SuperGuessr.best_guess: candidates must be (M,2) [lng, lat], got {tuple(cand.shape)}')
        table = hip_ops.score_table(cand, cen.data.to(device).contiguous(), kind=objective)
        self._guess_tables[objective] = (key, src, cand, table)          # `src` is kept so that its id stays its own
        return cand, table

    @torch.no_grad()
    def best_guess(self, candidates: Tensor = None, objective: str = 'score', incumbent: Tensor = None, state: dict = None) -> BestGuess:
        """The guess chosen by its expectation under the head's softmax (pg_guess_best; contract: include/pigeon_hip.h), from the
        geocell logits of `state` -- default `last_state`, with re-encoded rows carrying their exact-tier logits.  With a `temperature`
        other than 1.0 the expectations are taken under the calibrated softmax(logits / T); the argmax, the top-k, `topk_values`, the
        refiner's inputs and the certainty computations stay the head's own (reference-parity).
          candidates  (M,2) [lng, lat] shared by the batch: a grid, prototype locations, ...; None: the model's own `lla_geocells`
          objective   'score': the largest expected GeoGuessr score (5000 exp(-d / 1492.7), before its rounding); 'km': the smallest
                      expected distance
          incumbent   (B,2) [lng, lat], the guess to beat; None: the state's own `preds_LLH`.  Its expectation is pg_guess_spread's
        The candidates x centroids table is built on first use and cached on the model, per objective, keyed by the candidate
        tensor's identity and version.  Returns BestGuess(index, point, expected, incumbent_expected, taken), device tensors:
        `taken[b]` where the best candidate's expectation is strictly better than the incumbent's (a NaN on either side keeps the
        incumbent), `point[b]` the candidate where taken, else the incumbent.  Nothing is synchronised; nothing is computed unless
        this is called."""
        if objective not in GUESS_OBJECTIVES:
            raise ValueError(f"SuperGuessr.best_guess: objective must be 'score' or 'km', got {objective!r}")
        st = self.last_state if state is None else state
        if st is None:
            raise RuntimeError('SuperGuessr.best_guess: no state -- run a forward first, or pass `state`')
        logits = self._calibrated_logits(st)
        cand, table = self._guess_table(candidates, objective, logits.device)
        score = objective == 'score'
        idx, val = hip_ops.guess_best(logits, table, maximize=score)
        inc = st['preds_LLH'] if incumbent is None else torch.as_tensor(incumbent)
        inc = inc.to(logits.device, torch.float64).contiguous()
        ek, es, _ = hip_ops.guess_spread(logits, self.lla_geocells.data, inc, (1.0,), extent_km=self.cell_extent_km)
        inc_e = es if score else ek
        taken = ((val > inc_e) if score else (val < inc_e)) & (idx >= 0)          # a NaN compares false: the incumbent stays
        if cand.shape[0] == 0:
            return BestGuess(idx, inc, val, inc_e, taken)
        point = torch.where(taken[:, None], cand[idx.clamp(min=0)], inc)
        return BestGuess(idx, point, val, inc_e, taken)

    def _publish(self, st: dict) -> None:
        if 'certain' not in st:                          # a state straight from `encode_head` (no engine behind it)
            st['certain'] = st['tol'] > st['thr']
            st['exact'] = torch.ones_like(st['certain']) if st.get('exact_tier', False) else torch.zeros_like(st['certain'])
        self.last_tol, self.last_margin, self.last_certain = st['tol'], st['margin'], st['certain']
        self._last_exact = st['exact']
        self.last_state = st

    @property
    def last_reencoded(self):
        """(n,) int64: the samples of the last forward that went through the exact tier (a host synchronisation when read)."""
        ex = self._last_exact
        return None if ex is None else torch.nonzero(ex).flatten()

    @property
    def last_bound(self):
        """(B,) fp32: the margin change the threshold stands for, per sample of the last forward (its tier's threshold x `sens`)."""
        st = self.last_state
        if st is None:
            return None
        thr = torch.where(st['exact'], self.certainty.threshold(True), self.certainty.threshold(False))
        return st['sens'] * thr

    def package(self, st: dict, labels: Tensor = None, labels_clf: Tensor = None, labels_multi_task: Tensor = None,
                labels_climate: Tensor = None, labels_month: Tensor = None):
        """State -> the reference's outputs (:459-483).  The state's reference to the input pixels is dropped here (it was only
        needed for a possible re-encode): `last_state` must not keep a whole batch of pixels alive.

        Multi-task (:316-348, :463-464, :477): `preds_mt / preds_climate / preds_month` are the columns of the state's `aux_preds`
        (contiguous copies; `preds_month` None with yfcc), the three losses the reference's expressions through torch's loss modules
        -- logged values like `loss_clf`, no gradients.  `labels_climate` is what torch's CrossEntropyLoss accepts after the
        reference's float cast (:342): (B, 28) class probabilities / one-hot rows.  A loss whose labels were not given is 0 (the
        reference would raise on None there)."""
        self._publish(st)
        st['pixel_values'] = None
        k = self.num_candidates
        geocell_topk = TopK(st['topk_values'][:, :k], st['topk_indices'][:, :k])
        mt = self._multi_task_predictions(st, labels_multi_task, labels_climate, labels_month)
        if not self.training and self.serving:                              # :462-466
            if self.multi_task:
                return st['preds_LLH'], geocell_topk, mt.preds_mt, st['embedding']
            return st['preds_LLH'], geocell_topk, st['embedding']
        dev = st['logits'].device
        loss_clf = None
        if labels_clf is not None:                                          # :456, :474 (logged only)
            label_probs = self._to_one_hot(labels_clf.to(dev))
            if self.should_smooth_labels and labels is not None:            # :469-471 soft labels by distance
                distances = haversine_matrix(labels.to(dev), self.lla_geocells.data.t())
                label_probs = smooth_labels(distances)
            loss_clf = self.loss_fnc(st['logits'], label_probs)
        loss = loss_clf
        if self.multi_task and loss_clf is not None:                        # :477
            loss = loss_clf + mt.loss_reg + mt.loss_climate + mt.loss_month
        return ModelOutput(loss, loss_clf, mt.loss_reg, mt.loss_climate, mt.loss_month, st['preds_LLH'], st['preds_geocell'],
                           mt.preds_mt, mt.preds_climate, mt.preds_month, geocell_topk, st['embedding'])

    def _multi_task_predictions(self, st: dict, labels_multi_task: Tensor = None, labels_climate: Tensor = None,
                                labels_month: Tensor = None) -> MultiTaskPredictions:
        """:316-348 on what pg_aux_heads_forward left in the state."""
        if not self.multi_task:
            return MultiTaskPredictions(0, None, 0, None, 0, None)
        ap = st['aux_preds']
        dev = ap.device
        r, c = NUM_MULTI_TASK_VARIABLES, NUM_MULTI_TASK_VARIABLES + NUM_CLIMATES
        preds_mt, preds_climate = ap[:, :r].contiguous(), ap[:, r:c].contiguous()
        preds_month = None if self.yfcc else ap[:, c:].contiguous()
        loss_reg = loss_climate = loss_month = 0
        if not self.serving:                                                # :340-345
            if labels_multi_task is not None:
                loss_reg = self.loss_fnc_mt(preds_mt, labels_multi_task.to(dev)) * REGRESSION_LOSS_SCALING
            if labels_climate is not None:
                loss_climate = self.loss_fnc_climate(preds_climate, labels_climate.to(dev, dtype=torch.float32)) * CLIMATE_LOSS_SCALING
            if preds_month is not None and labels_month is not None:
                loss_month = self.loss_fnc_month(preds_month, labels_month.to(dev)) * MONTHS_LOSS_SCALING
        return MultiTaskPredictions(loss_reg, preds_mt, loss_climate, preds_climate, loss_month, preds_month)

    def forward(self, pixel_values: Tensor = None, embedding: Tensor = None, heading: Tensor = None,
                labels: Tensor = None, labels_clf: Tensor = None, labels_multi_task: Tensor = None,
                labels_climate: Tensor = None, labels_month: Tensor = None, index: Tensor = None, pixel_bytes: Tensor = None):
        """Inference branch of reference models/super_guessr.py:350-483.

        pixel_values (B,12,336,336) [panorama] or (B,3,336,336); or embedding (B,4,1024)/(B,1024).
        Returns ModelOutput (or, with serving=True in eval mode, the (pred_LLH, topk, embedding) tuple -- multi-task:
        (pred_LLH, topk, preds_mt, embedding) --, :462-466).  `heading` is ignored: the only configuration that accepts
        heading=True is the one in which the reference ignores it too (:273-274).
        `pixel_bytes` (instead of pixel_values / embedding): uint8 (B,12,336,336) or (B,3,336,336), see `encode_head`.
        """
        self._check_pixel_bytes(pixel_bytes, pixel_values, embedding)
        self._assert_requirements(pixel_values if pixel_bytes is None else pixel_bytes, embedding, heading)
        if not self.cell_layer.weight.is_cuda:
            raise RuntimeError('pigeon_amd.SuperGuessr runs on the GPU only: call .to("cuda") first (no CPU fallback)')
        with torch.no_grad():
            # fast pass, tolerance of the top-1 against every cell, exact re-encode of the samples that are not certain
            # (pigeon_amd.deferred, settled before this call returns: one host synchronisation)
            res = self.engine(None).submit(pixel_values, embedding, pixel_bytes=pixel_bytes)[0]
            return self.package(dict(res['state']), labels, labels_clf, labels_multi_task, labels_climate, labels_month)

    def engine(self, refiner=None, **kw):
        """The settle-before-return form of pigeon_amd.deferred.DeferredExact for (this model, `refiner`), built once."""
        from .deferred import DeferredExact
        key = id(refiner)
        hit = self._engines.get(key)
        if hit is None or hit[0] is not refiner:
            self._engines[key] = hit = (refiner, DeferredExact(self, refiner, immediate=True, **kw))
        return hit[1]

    @torch.no_grad()
    def _autocalibrate(self, px: Tensor) -> None:
        """First use without an explicit `calibrate_certainty`: a batch of >= 8 samples calibrates right away; smaller batches (a
        server answering one panorama at a time) are collected until 16 samples have been seen, then calibrate once.  Frozen after."""
        P = self._panels()
        if px.shape[0] == 0:
            return
        if px.shape[0] >= 8 * P and not self._cal_buffer:
            self._calibrate(px)
            return
        self._cal_buffer.append(px.detach().clone())
        if sum(t.shape[0] for t in self._cal_buffer) >= 16 * P:
            if len({t.dtype == torch.uint8 for t in self._cal_buffer}) > 1:    # bytes and floats collected together: all as fp32 pixels
                self._cal_buffer = [hip_ops.bytes_to_pixels(t) if t.dtype == torch.uint8 else t.float() for t in self._cal_buffer]
                px = self._cal_buffer[-1]
            buf, self._cal_buffer = torch.cat([t.to(px.dtype) for t in self._cal_buffer]), []
            self._calibrate(buf)

    @torch.no_grad()
    def _calibrate(self, px: Tensor, max_samples: int = 32) -> dict:
        P = self._panels()
        n = min(max_samples, px.shape[0] // P)
        px = px[:n * P]
        fast_i, exact_i = self._embed(px), self._embed(px, exact=True)
        st = self.certainty.calibrate(fast_i.reshape((-1, P, CLIP_EMBED_DIM)).mean(dim=1), exact_i.reshape((-1, P, CLIP_EMBED_DIM)).mean(dim=1),
                                      fast_images=fast_i, exact_images=exact_i)
        if self.certainty.force_exact:
            print(f'pigeon_amd.SuperGuessr: the 16-bit encoder measures {st["image_rel_err"]:.2e} (worst image '
                  f'{st["worst_image_rel_err"]:.2e}) against the exact encoder on these weights -- outside the 1e-3 embedding '
                  f'contract; every sample will be encoded in the exact mode (about 4x the time per image).')
        return st

    @torch.no_grad()
    def calibrate_certainty(self, pixel_values: Tensor, max_samples: int = 32) -> float:
        """Measure what the 16-bit path's embedding error IS on this model -- once per set of weights -- and set the certainty
        threshold from it: up to `max_samples` samples go through the fast and the exact encoder (`Certainty.calibrate`: the
        systematic part of their difference and the RMS of the rest).  Frozen afterwards: which samples a later forward re-encodes
        does not depend on what earlier batches held.  Returns the total RMS relative difference.  Needs pixels and a base model."""
        if self.base_model is None or pixel_values is None:
            raise ValueError('calibrate_certainty needs pixel_values and a base model')
        dev = self.cell_layer.weight.device
        px = pixel_values.reshape((-1, 3, 336, 336)).to(dev)
        if px.dtype == torch.uint8:
            px = px.float()                              # (pixel_values: numbers, as in `encode_head`)
        return self._calibrate(px, max_samples)['fast_vs_exact_rms']

    # ------------------------------------------------------------------------------------------ calibration as a file
    def _calibration_meta(self, source: str = '') -> dict:
        meta = self._encoder().encoder_config()
        meta['source'] = source
        return meta

    def save_calibration(self, path: str, source: str = '') -> str:
        """Write what `calibrate_certainty` (or the first forwards) measured to `path`, keyed by the encoder's weight fingerprint
        (pg_vit_fingerprint) -- `Certainty.save`.  Needs a base model and a finished calibration."""
        if self.base_model is None:
            raise CalibrationError('save_calibration: no base model -- nothing was measured here')
        if not self.certainty.calibrated:
            raise CalibrationError('save_calibration: not calibrated yet (call calibrate_certainty, or run the first forwards)')
        return self.certainty.save(path, self._encoder().fingerprint(), self._panels(),
                                   self._calibration_meta(source or f'SuperGuessr, {self.certainty.stats.get("samples")} samples'))

    def load_calibration(self, path: str) -> dict:
        """Take bias, tolerance and the `force_exact` verdict from a calibration file instead of measuring them inside a forward.
        The file is checked BEFORE anything on this object changes, and all state is set at once.  Refused (CalibrationError): an
        unreadable file, an unknown `format_version`, a fingerprint that is not this encoder's (both are named), `panels` different
        from this model's.  Order: weights first (`load_state` drops a calibration, loaded or measured), then the calibration.
        With base_model=None (precomputed embeddings) there is no encoder to fingerprint: the file is accepted and sets
        `embedding_rel_tol` -- what caller-supplied embeddings are judged against -- to 1.1 x the file's `image_residual_rms` (the
        per-image error of the 16-bit path that wrote them, after its bias), or to the exact tier's floor when the file says
        `force_exact` (those embeddings were written by the exact encoder).  Returns the file's header."""
        sd, header = Certainty.load(path)
        new = Certainty(self.certainty.kappa, self._rel_tol0, self.certainty.rel_tol_exact, debias=self.certainty.debias)
        new.load_state_dict(sd)
        if self.base_model is None:
            if new.force_exact:
                tol = new.rel_tol_exact
            else:
                resid = new.stats.get('image_residual_rms')
                if resid is None or not (float(resid) > 0.0):
                    raise CalibrationError(f'{path!r}: no image_residual_rms in the file\'s statistics -- cannot set embedding_rel_tol')
                tol = SAFETY * float(resid)                # the safety factor `Certainty.calibrate` puts on rel_tol
            if self._embedding_rel_tol0 is None:
                self._embedding_rel_tol0 = (self._embedding_rel_tol,)
            self.embedding_rel_tol = float(tol)
            self.calibration_header = header
            return header
        require_fingerprint(path, header, self._encoder().fingerprint())
        if header['panels'] != self._panels():
            raise CalibrationError(f'{path!r}: rel_tol was measured on samples of {header["panels"]} images (panels), this model uses {self._panels()}')
        self.certainty = new
        self.calibration_header = header
        self._cal_buffer = []
        self._wnorm = {}
        return header

    def __str__(self):
        shown = (('base_model', self.base_model is not None), ('panorama', self.panorama), ('hierarchical', self.hierarchical),
                 ('multi-task', self.multi_task), ('yfcc', self.yfcc), ('embedding_size', self.hidden_size), ('input_dim', self.input_dim),
                 ('num_geocells', self.num_cells), ('label_smoothing', self.should_smooth_labels), ('uses_headings', self.heading),
                 ('freeze_base', self.freeze_base), ('serving', self.serving))
        width = max(len(k) for k, _ in shown) + 1
        return 'SuperGuessr(\n' + ''.join(f'\t{k.ljust(width)}= {v}\n' for k, v in shown) + ')'
