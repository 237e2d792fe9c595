"""Evaluation entry points behind the reference's names: `evaluate()` (evaluation/evaluate.py:10-85) builds
SuperGuessr + ProtoRefiner, `evaluate_model()` (training/train_eval_loop.py:35-161) runs the batch loop
`model(**data)` -> `refiner(...)` -> collect.  Plus `PanoramaPipeline`, the data-parallel step the benchmark
times: ViT + head on the local shard, ONE all-gather of embeddings / candidates, refinement.

Out of scope here: TensorBoard writers.  The distance / geocell metrics of
evaluation/metrics.py:89-181 are provided under the reference's keys; `Country_accuracy` (:56-88) when the country
polygons are given (pigeon_amd/regions.py: exact point-in-region lookup on the GPU, no geopandas).
"""
from __future__ import annotations

import logging
import os
from typing import Callable, Dict, Optional

import numpy as np
import torch

from .config import DECAY_CONSTANT, EVAL_BATCH_SIZE_PER_GPU
from .deferred import DeferredExact, as_model_output
from .distributed import Communicator
from .geo_utils import haversine_np
from .proto_refiner import ProtoRefiner, load_refiner_cache
from .super_guessr import SuperGuessr

logger = logging.getLogger('train')
LABEL_KEYS = ('labels', 'labels_clf', 'labels_multi_task', 'labels_climate', 'labels_month')      # of a batch, in `package`'s order


def percentage_within_radius(distances: np.ndarray, km: float) -> float:
    """reference evaluation/metrics.py:89-100 (a FRACTION, strict `<`, despite the name)"""
    return (distances < km).sum() / len(distances)


def geoguessr_score(distances: np.ndarray) -> float:
    """reference evaluation/metrics.py:102-114; DECAY_CONSTANT = 1492.7 (config.py:52)"""
    return np.mean(np.round(5000 * np.exp(-distances / DECAY_CONSTANT)))


def topk_geocell_accuracy(cell_labels: np.ndarray, topk_preds: np.ndarray) -> float:
    """reference evaluation/metrics.py:116-136"""
    num_correct = 0
    for label, top5 in zip(cell_labels, topk_preds):
        if label in top5:
            num_correct += 1
    return num_correct / len(cell_labels)


def mae(labels: np.ndarray, preds: np.ndarray) -> float:
    """reference evaluation/metrics.py:22-27"""
    return np.mean(np.abs(labels - preds))


def load_scaler(yfcc: bool = False):
    """The fitted scaler of the six regression targets (reference evaluation/metrics.py:43-44: joblib.load of
    config.SCALER_PATH(_YFCC)), or None when the file is not there."""
    import os
    from . import config as cfg
    path = cfg.SCALER_PATH_YFCC if yfcc else cfg.SCALER_PATH
    if not os.path.exists(path):
        return None
    import joblib
    return joblib.load(path)


def recover_regression_values(values: np.ndarray, yfcc: bool = False, scaler=None) -> np.ndarray:
    """reference evaluation/metrics.py:29-54: undo the scaler, the log transform of every variable but the average temperature,
    and the offsets (elevation 408, or 416 with yfcc; 1 for the other log-transformed ones).  `scaler`: anything with
    `inverse_transform` (default: the file config.SCALER_PATH(_YFCC) names)."""
    if scaler is None:
        scaler = load_scaler(yfcc)
        if scaler is None:
            raise FileNotFoundError('recover_regression_values: no scaler given and no scaler file at config.SCALER_PATH(_YFCC)')
    vals = np.array(scaler.inverse_transform(np.asarray(values)))
    vals[:, :2] = np.exp(vals[:, :2])
    vals[:, 3:] = np.exp(vals[:, 3:])
    return vals - np.array([416 if yfcc else 408, 1, 0, 1, 1, 1]).transpose()


def spread_metrics(radius_km, quantiles, distances, expected_km=None, expected_score=None) -> Dict[str, float]:
    """How the head's probabilities compare with the truth: for every quantile q of `SuperGuessr.spread` (radius_km (N, nq), in the
    order of `quantiles`) `Radius_<100 q>_coverage`, the share of samples whose true distance (`distances` (N,) km) is at most their
    radius -- to be read against q: a calibrated head covers q of the samples -- and `Median_radius_<100 q>_km`; with the two
    expectations also `Mean_expected_km` and `Mean_expected_score`.  A sample whose radius is NaN is not covered."""
    radius_km, distances = np.asarray(radius_km, dtype=np.float64), np.asarray(distances, dtype=np.float64)
    if radius_km.ndim != 2 or radius_km.shape != (distances.shape[0], len(quantiles)):
        raise ValueError(f'spread_metrics: radius_km {radius_km.shape} does not match {distances.shape[0]} samples x {len(quantiles)} quantiles')
    out = {}
    for j, q in enumerate(quantiles):
        tag = f'{100 * float(q):g}'
        out[f'Radius_{tag}_coverage'] = float(np.mean(distances <= radius_km[:, j]))
        out[f'Median_radius_{tag}_km'] = float(np.median(radius_km[:, j]))
    if expected_km is not None:
        out['Mean_expected_km'] = float(np.mean(np.asarray(expected_km, dtype=np.float64)))
    if expected_score is not None:
        out['Mean_expected_score'] = float(np.mean(np.asarray(expected_score, dtype=np.float64)))
    return out


def _final_spread(model: SuperGuessr, st: dict, refined, quantiles):
    """`model.spread` of a settled state at its FINAL guess: the refined point when there is one (fp32 -> fp64, exact), else the
    state's own centroid.  Device tensors only."""
    return model.spread(points=None if refined is None else refined.to(torch.float64), quantiles=quantiles, state=st)


def _final_best_guess(model: SuperGuessr, st: dict, refined, objective: str):
    """`model.best_guess` of a settled state against its FINAL guess as the incumbent (as `_final_spread`).  Device tensors only."""
    return model.best_guess(objective=objective, incumbent=None if refined is None else refined.to(torch.float64), state=st)


def best_guess_metrics(best_llh, distances_fn, labels, taken) -> Dict[str, float]:
    """The existing km and score metrics on the guesses chosen by expectation (`best_llh` (N,2)), and the share of rows changed."""
    d = distances_fn(np.asarray(best_llh), np.asarray(labels))
    return {'Mean_km_error_best': np.mean(d), 'Median_km_error_best': np.median(d), 'Geoguessr_score_best': geoguessr_score(d),
            'Best_guess_changed': float(np.mean(np.asarray(taken, dtype=bool)))}


def neighbour_metrics(nn_lnglat, distances_fn, labels, preds) -> Dict[str, float]:
    """The retrieval baseline: the existing km and score metrics with the NEAREST training row's coordinates (`nn_lnglat` (N,K,2),
    column 0) as the guess, and the share of items on which that guess is closer to the truth than the model's final one."""
    labels = np.asarray(labels)
    d = distances_fn(np.asarray(nn_lnglat)[:, 0, :].astype(np.float64), labels)
    return {'Mean_km_error_nn': np.mean(d), 'Median_km_error_nn': np.median(d), 'Geoguessr_score_nn': geoguessr_score(d),
            'NN_beats_model': float(np.mean(d < distances_fn(np.asarray(preds), labels)))}


def _neighbour_index(refiner, neighbours):
    """`neighbours=K` of evaluate_model / serve: K checked, and the search index over the refiner's bank (borrowed fp32 rows)."""
    from .neighbours import index_of
    return int(neighbours), index_of(refiner, neighbours, 'neighbours=K')


def _class_labels(labels) -> np.ndarray:
    labels = np.asarray(labels)
    return np.argmax(labels, axis=-1) if labels.ndim > 1 else labels          # (N, classes) one-hot / probabilities, or (N,) indices


def compute_geoguessr_metrics(results, scaler=None, countries=None) -> Dict[str, float]:
    """reference evaluation/metrics.py:138-199 on the 11-tuple evaluate_model builds (train_eval_loop.py:138-140):
    the km-error statistics, the Under_*_km fractions, the GeoGuessr score and the geocell (top-k) accuracies, under the
    reference's keys; with multi-task labels (`labels_mt` not None, :184-199) also `Climate_accuracy`, `Month_accuracy` (when there
    are month labels) and -- when a scaler is available: the `scaler` keyword, or the file config.SCALER_PATH(_YFCC) names -- the six
    `Mean_*_error` entries on the recovered regression values.  Climate labels may be class indices or the (N, 28) one-hot rows
    the model's forward takes.  `Country_accuracy` (:178, find_country / country_accuracy :56-88) is added when `countries` is given:
    a `pigeon_amd.regions.RegionBank` of the country polygons (`RegionBank.from_geojson(config.COUNTRY_PATH)`); the lookup runs on
    the GPU (pg_region_locate / _classify / _nearest) and is exact.  Without `countries` the key is left out, as before.
    Everything else is host numpy on the collected predictions, as in the reference."""
    predictions, cell_preds, preds_mt, preds_climate, preds_month, top5_geocells, labels, cell_labels, labels_mt, labels_climate, \
        labels_month = results
    cell_labels = np.asarray(cell_labels)
    if cell_labels.ndim > 1:
        cell_labels = np.argmax(cell_labels, axis=-1)
    distances = haversine_np(np.asarray(predictions), np.asarray(labels))      # dtypes as collected (fp32 preds: np.radians in fp32)
    eval_dict = {'Mean_km_error': np.mean(distances), 'Median_km_error': np.median(distances)}
    for km in (1, 5, 10, 25, 50, 100, 200, 750, 1000, 2500):
        eval_dict[f'Under_{km}_km'] = percentage_within_radius(distances, km)
    if countries is not None:                                                  # :178
        from .regions import country_accuracy
        eval_dict['Country_accuracy'] = country_accuracy(np.asarray(predictions), np.asarray(labels), countries)
    eval_dict['Geoguessr_score'] = geoguessr_score(distances)
    eval_dict['Geocell_accuracy'] = float(np.mean(cell_labels == np.asarray(cell_preds)))      # sklearn accuracy_score
    eval_dict['Geocell_top5_accuracy'] = topk_geocell_accuracy(cell_labels, top5_geocells)
    if labels_mt is not None:                                                  # :184-199
        yfcc = labels_month is None                                            # :163
        if scaler is None:
            scaler = load_scaler(yfcc)
        if scaler is None:
            print('compute_geoguessr_metrics: no regression scaler (config.SCALER_PATH) -- the six Mean_*_error entries are left out')
        else:
            p_mt = recover_regression_values(np.asarray(preds_mt), yfcc, scaler)
            l_mt = recover_regression_values(np.asarray(labels_mt), False, scaler)     # :186 as the reference: the labels without `yfcc`
            for i, name in enumerate(('elevation', 'population', 'temperature', 'temp_diff', 'precipitation', 'prec_diff')):
                eval_dict[f'Mean_{name}_error'] = mae(l_mt[:, i], p_mt[:, i])
        eval_dict['Climate_accuracy'] = float(np.mean(_class_labels(labels_climate) == np.argmax(np.asarray(preds_climate), axis=-1)))
        if not yfcc:
            eval_dict['Month_accuracy'] = float(np.mean(_class_labels(labels_month) == np.argmax(np.asarray(preds_month), axis=-1)))
    return eval_dict


@torch.no_grad()
def certain_forward(model: SuperGuessr, refiner: Optional[ProtoRefiner], pixel_values=None, embedding=None, labels=None,
                    labels_clf=None, labels_multi_task=None, labels_climate=None, labels_month=None, pixel_bytes=None, spread=None,
                    best_guess=None, **_unused):
    """`model(**data)` followed by `refiner(...)` with the reference's discrete outputs (a z ~ 4 statistical statement for the samples called certain, pigeon_amd/certainty.py): one fast pass, the tolerance of every
    discrete decision downstream of the embedding -- the top-1 cell (pg_head_certainty) and, with a refiner, the winning candidate,
    the candidate-set boundary, the nearest prototype and the farthest member (pg_refine_certainty) -- and ONE exact pass
    (pg_vit_forward_precise) over the samples that are not certain, after which their head outputs AND their refinement are
    recomputed.  This is the settle-before-return form of `pigeon_amd.deferred.DeferredExact` (one host synchronisation: how many
    samples are uncertain is data dependent); loops over many batches use the engine's deferred form (`evaluate_model`,
    `PanoramaPipeline.submit`).
    Returns (outputs as `model.forward` returns them, info) with info = dict(certain (B,) bool: every output of the sample is the
    reference's; cause (B,) int32: why a sample was not certain after the fast pass; reencoded (n,) int64; head_tol, refine_tol,
    refine_code (B,) or None; boundary_checked; refined_LLH (B,2) f32 / refined_geocell (B,) i64: the refinement's result -- the
    caller need not run the refiner again; multi-task models: aux_tol (B,) f32 the tolerance of the climate and month argmaxes,
    aux_code (B,) i32 which class sets it -- `head_tol` is already the minimum over the geocell, climate and month decisions).
    `pixel_bytes` (instead of pixel_values / embedding): uint8 (B,12,336,336) or (B,3,336,336) 8-bit pixels (`SuperGuessr.encode_head`);
    every output and every `info` entry equals what the fp32 pixels `table[bytes]` give.
    `spread` (quantiles, e.g. (0.5, 0.9); default None: nothing is computed): adds info['spread'], `SuperGuessr.spread` of the final
    guess -- the refined point with a refiner, else the top-1 centroid -- from the settled state's logits (re-encoded rows: their
    exact-tier logits).
    `best_guess` ('score' | 'km'; default None: nothing is computed): adds info['best_guess'], `SuperGuessr.best_guess` over the model's
    own centroids under that objective, with the final guess -- the refined point with a refiner -- as the incumbent."""
    if pixel_bytes is not None:
        model._check_pixel_bytes(pixel_bytes, pixel_values, embedding)
    res = model.engine(refiner).submit(pixel_values, embedding, pixel_bytes=pixel_bytes)[0]
    out = as_model_output(model, res, labels, labels_clf, labels_multi_task, labels_climate, labels_month)
    st = res['state']
    info = dict(certain=st['certain'], cause=st['cause'], head_tol=st['tol'], refine_tol=st.get('refine_tol'),
                refine_code=st.get('refine_code'), boundary_checked=model.engine(refiner).boundary_checked if refiner is not None else None,
                reencoded=torch.nonzero(st['exact']).flatten(), refined_LLH=st.get('refined_LLH'),
                refined_geocell=st.get('refined_geocell'))
    if 'aux_tol' in st:
        info['aux_tol'], info['aux_code'] = st['aux_tol'], st['aux_code']
    model.last_certain = info['certain']
    if spread is not None:
        info['spread'] = _final_spread(model, st, st.get('refined_LLH') if refiner is not None else None, spread)
    if best_guess is not None:
        info['best_guess'] = _final_best_guess(model, st, st.get('refined_LLH') if refiner is not None else None, best_guess)
    return out, info


IMAGE_KEYS = ('image', 'image_2', 'image_3', 'image_4')


class ImageEvalDataset:
    """The reference's `EvalDataset` (dataset_creation/benchmark/eval_dataset.py) for `evaluate_model`: wraps anything indexable whose
    items hold a raw `image` column, or the four views `image`, `image_2`, `image_3`, `image_4` (PIL images or uint8 (H,W,3) arrays
    of any sizes).  Where the reference's workers run the CLIP processor per item and ship 12 x 336 x 336 floats, a worker here only
    decodes and packs (`packing.pack_images`: the raw views in one uint8 buffer) and passes every other column (`labels`,
    `labels_clf`, ...) through; `collate` joins a batch's items into ONE `PackedImages`, and the process that owns the GPU resizes
    the whole mixed-size batch to 8-bit pixels in one ragged call (`preprocess`) and submits them as `pixel_bytes`.  String keys are
    column reads of the wrapped dataset (`dataset['labels']`, as `evaluate_model` collects the labels for the metrics).
    encoded=True: the image columns hold files (bytes, paths, or the dicts of HF `Image(decode=False)` columns); a worker ships the
    bytes as an `EncodedImages` and the decode runs on the GPU too (`gpu_preprocess(EncodedImages)`, pigeon_amd/jpeg.py).
    equirect=True: every item's single `image` column holds ONE equirectangular panorama (raw, or a file with encoded=True); the four
    views at headings 0 / 90 / 180 / 270 are rendered from it on the GPU (pigeon_amd/panorama.py) in front of the resize."""

    def __init__(self, dataset, encoded: bool = False, equirect: bool = False):
        self.dataset, self.encoded, self.equirect = dataset, encoded, equirect

    def __len__(self) -> int:
        return len(self.dataset)

    def __getitem__(self, idx):
        if isinstance(idx, str):
            return self.dataset[idx]
        from .packing import pack_images
        item = self.dataset[idx]
        if 'image' not in item:
            raise KeyError("ImageEvalDataset: items need an 'image' column (or 'image', 'image_2', 'image_3', 'image_4')")
        if self.equirect and 'image_2' in item:
            raise KeyError("ImageEvalDataset(equirect=True): items hold ONE equirectangular 'image', these also have 'image_2'")
        views = [item[k] for k in (IMAGE_KEYS if 'image_2' in item else IMAGE_KEYS[:1])]
        out = {k: v for k, v in item.items() if 'image' not in k}              # (the reference drops every image column the same way)
        if self.equirect:
            out['equirect'] = True
        if self.encoded:                                           # the files' bytes as they are: the worker does nothing but read
            from .jpeg import EncodedImages, image_bytes
            out['images'] = EncodedImages([image_bytes(v) for v in views])
            return out
        out['images'] = pack_images([v.numpy() if torch.is_tensor(v) else v for v in views])
        return out

    @staticmethod
    def collate(batch):
        """collate_fn: a list of items -> {'images': one PackedImages of the batch's views in item order, 'views': views per item,
        every other key: torch's default collation}."""
        from torch.utils.data import default_collate
        from .packing import concat_packed
        views = {len(b['images']) for b in batch}
        if len(views) != 1:
            raise ValueError(f'ImageEvalDataset: items of one batch hold {sorted(views)} views; every item must have the same number')
        out = default_collate([{k: v for k, v in b.items() if k not in ('images', 'equirect')} for b in batch])
        if any(b.get('equirect') for b in batch):
            out['equirect'] = True
        from .jpeg import EncodedImages
        parts = [b['images'] for b in batch]
        out['images'] = EncodedImages.concat(parts) if isinstance(parts[0], EncodedImages) else concat_packed(parts)
        out['views'] = views.pop()
        return out

    @staticmethod
    def preprocess(data: dict, device) -> dict:
        """Main process: the batch's `PackedImages` -> `pixel_bytes` (B, 3 * views, 336, 336) uint8 on the device, by the ragged
        GPU preprocessing; the other keys as they are."""
        from .clip_embedder import gpu_preprocess
        data = dict(data)
        packed, views = data.pop('images'), int(data.pop('views'))
        if data.pop('equirect', False):                            # one panorama per item: its four views, panorama-major
            from .panorama import HEADINGS, panorama_pixels
            px = panorama_pixels(packed, device, torch.uint8)
            data['pixel_bytes'] = px.reshape((len(packed), 3 * len(HEADINGS), 336, 336))
            return data
        px = gpu_preprocess(packed, device, torch.uint8)
        data['pixel_bytes'] = px.reshape((len(packed) // views, 3 * views, 336, 336))
        return data


def evaluate_model(model: SuperGuessr, dataset, metrics: Optional[Callable] = None, train_args=None,
                   refiner: Optional[ProtoRefiner] = None, yfcc: bool = False, writer=None, step: int = 0,
                   batch_size: Optional[int] = None, num_workers: int = 0, spread=None, best_guess=None, neighbours=None,
                   bootstrap: Optional[int] = None, bootstrap_seed: int = 0, bootstrap_level: float = 0.95, countries=None):
    """reference training/train_eval_loop.py:35-161 (eval loop :77-112).

    dataset items are dicts of forward() keyword arguments (pixel_values | pixel_bytes | embedding, labels, labels_clf, ...), or
    -- an `ImageEvalDataset` -- raw images of any sizes, which are resized to `pixel_bytes` here, a batch at a time on the GPU.
    Returns the dict of concatenated numpy results; if `metrics` is given it is called with the same 11-tuple
    the reference builds (:138-140) and its dict is merged in.
    `spread` (quantiles, e.g. (0.5, 0.9); default None: nothing is computed): `SuperGuessr.spread` of every finished batch's final
    guess, from its final state (rows the exact tier re-encoded: their re-encoded logits), on device tensors without a host
    synchronisation: results['expected_km'], ['expected_score'] (N,), ['radius_km'] (N, nq), ['spread_quantiles']; when the dataset
    has a `labels` column also `spread_metrics`: Radius_<100 q>_coverage, Median_radius_<100 q>_km, Mean_expected_km / _score.
    `best_guess` ('score' | 'km'; default None: nothing is computed): `SuperGuessr.best_guess` of every finished batch over the model's
    centroids, its final guess as the incumbent, on device tensors without a host synchronisation: results['best_LLH'] (N,2),
    ['best_index'], ['best_expected'], ['best_taken'] (N,); when the dataset has a `labels` column also Mean_km_error_best,
    Median_km_error_best, Geoguessr_score_best (the existing metric functions on best_LLH) and Best_guess_changed, the share of rows
    taken.  Every other key is computed as without it.
    `neighbours` (K in 1..64; default None: nothing is computed, nothing is launched): the K nearest rows of the refiner's bank of
    training embeddings for every finished batch's final embedding (`pigeon_amd.neighbours`, exact for the embedding it is given),
    on device tensors without a host synchronisation: results['nn_rows'], ['nn_distance'] (N,K), ['nn_lnglat'] (N,K,2),
    ['nn_certified'] (N,); when the dataset has a `labels` column also Mean_km_error_nn, Median_km_error_nn, Geoguessr_score_nn (the
    nearest row's coordinates as the guess) and NN_beats_model.  Needs a refiner (ValueError without).
    `bootstrap` (R replicates; default None: nothing is computed, nothing is launched, no key is added): the paired bootstrap of
    every metric `metrics` returns and of the best-guess and neighbour metrics (`pigeon_amd.bootstrap`: the per-item columns of
    `metric_columns`, resampled R times on the GPU with `bootstrap_seed`), stored under results['bootstrap']: key -> dict(estimate,
    se, lo, hi) at `bootstrap_level`, the paired differences '<key>_best - <key>' / '<key>_nn - <key>' with share_le_zero, plus
    results['bootstrap_level'].  Needs `metrics`; `countries`: the bank behind `Country_accuracy`, for that metric's column.  In a
    multi-rank run rank 0 bootstraps.  Every other key is computed as without it.
    """
    from torch.utils.data import DataLoader
    if bootstrap is not None:
        if isinstance(bootstrap, bool) or int(bootstrap) != bootstrap or int(bootstrap) < 1:
            raise ValueError(f'evaluate_model: bootstrap must be a positive number of replicates, got {bootstrap!r}')
        if metrics is None:
            raise ValueError('evaluate_model: bootstrap=R resamples the metrics; it needs `metrics`')
        if not 0.0 < float(bootstrap_level) < 1.0:
            raise ValueError(f'evaluate_model: bootstrap_level must lie strictly between 0 and 1, got {bootstrap_level!r}')
    nn_k, nn_index = _neighbour_index(refiner, neighbours) if neighbours is not None else (None, None)
    logger.warning('Starting evaluation ...')
    if batch_size is None:
        batch_size = getattr(train_args, 'per_device_eval_batch_size', EVAL_BATCH_SIZE_PER_GPU)
    from_images = isinstance(dataset, ImageEvalDataset)
    eval_data = DataLoader(dataset, batch_size, shuffle=False, pin_memory=False, num_workers=num_workers,
                           collate_fn=ImageEvalDataset.collate if from_images else None)
    model.eval()
    if refiner is not None:
        refiner.eval()
    combined_preds, combined_geocell_preds, combined_top5_cells, combined_top5_probs = [], [], [], []
    combined_loss = 0.0
    combined_preds_mt, combined_preds_climate, combined_preds_month = [], [], []
    combined_loss_mt = [0.0, 0.0, 0.0]                     # reg, climate, month
    multi_task = bool(getattr(model, 'multi_task', False))
    combined_certain = []
    combined_spread = []
    combined_best = []
    combined_nn = []
    n_seen = 0
    # The reference's loop (:77-112) computes a batch and appends its predictions; the predictions are only read after the loop
    # (:114-140).  Here a batch's rows that the 16-bit encoder cannot settle are queued on the device and re-encoded by the exact
    # encoder 40+ images at a time (pigeon_amd.deferred): a batch is appended when all its rows are settled -- a few iterations
    # late, in order -- and `flush()` settles the rest after the loop.  No host synchronisation per batch.
    engine = DeferredExact(model, refiner)

    def collect(done):
        # device tensors only: a `.cpu()` / `float()` here would wait for the step that has just been queued
        nonlocal combined_loss, n_seen
        for res in done:
            meta = res['meta']
            outputs = as_model_output(model, res, *(meta.get(k) for k in LABEL_KEYS))
            if outputs.loss_clf is not None:
                combined_loss = combined_loss + outputs.loss_clf.detach() * meta['n_keys']   # :81-82 (`len(data)` as the reference)
            # :84-95.  The reference decides with `outputs.loss_reg > 0` -- a comparison of a device value on the host, i.e. a
            # synchronisation per step, which this loop does not do: decided from what the host knows (a multi-task model, and the
            # batch came with regression labels)
            if multi_task and meta.get('labels_multi_task') is not None:
                for i, l in enumerate((outputs.loss_reg, outputs.loss_climate, outputs.loss_month)):
                    combined_loss_mt[i] = combined_loss_mt[i] + (l.detach() if torch.is_tensor(l) else l) * meta['n_keys']
                combined_preds_mt.append(outputs.preds_mt)
                combined_preds_climate.append(outputs.preds_climate)
                if outputs.preds_month is not None:
                    combined_preds_month.append(outputs.preds_month)
            # :98-103: the refinement is the one the engine already ran (and re-ran for the rows the exact tier re-encoded)
            combined_preds.append(res['refined_LLH'] if refiner is not None else outputs.preds_LLH)
            combined_geocell_preds.append(outputs.preds_geocell)                 # :106-112
            top5 = outputs.top5_geocells
            combined_top5_cells.append(top5.indices)
            combined_top5_probs.append(top5.values)
            combined_certain.append(res['certain'])                              # every output of the sample is the reference's
            if spread is not None:
                combined_spread.append(_final_spread(model, res['state'], res['state'].get('refined_LLH') if refiner is not None else None, spread))
            if best_guess is not None:
                combined_best.append(_final_best_guess(model, res['state'], res['state'].get('refined_LLH') if refiner is not None else None, best_guess))
            if nn_index is not None:
                combined_nn.append(nn_index.search(res['state']['embedding'], k=nn_k))
            n_seen += outputs.preds_geocell.shape[0]

    with torch.no_grad():
        for data in eval_data:
            if from_images:
                data = ImageEvalDataset.preprocess(data, model.cell_layer.weight.device)
            # :80 `model(**data)` and :98 `refiner(...)`, with what the refiner will consume checked as well
            keep = dict({k: data.get(k) for k in LABEL_KEYS}, n_keys=len(data))
            collect(engine.submit(data.get('pixel_values'), data.get('embedding'), meta=keep, pixel_bytes=data.get('pixel_bytes')))
        collect(engine.flush())
    dropped = engine.check_nothing_dropped()
    if dropped:
        raise RuntimeError(f'evaluate_model: {dropped} uncertain rows did not fit the exact tier\'s queue (internal sizing error)')
    to_np = lambda parts: np.concatenate([t.cpu().detach().numpy() for t in parts], axis=0)     # noqa: E731
    preds = to_np(combined_preds)
    preds_geocells = to_np(combined_geocell_preds)
    top5_geocells = to_np(combined_top5_cells)
    combined_certain = [t.cpu().numpy() for t in combined_certain]
    results = dict(preds=preds, preds_geocells=preds_geocells, top5_geocells=top5_geocells,
                   top5_probs=to_np(combined_top5_probs), loss_clf=float(combined_loss) / max(n_seen, 1))
    if combined_certain:        # beyond the reference's keys: which samples' outputs are certain to be the fp32 reference's
        results['geocell_certain'] = np.concatenate(combined_certain, axis=0)
        # how many samples are STILL not certain after the exact tier (judged at its floor): their outputs are returned as computed
        results['uncertain_after_exact'] = int((~results['geocell_certain']).sum())
        results['exact_passes'] = [dict(f) for f in engine.flush_log]
    preds_mt = preds_climate = preds_month = None
    if combined_preds_mt:                                                         # :126-135
        preds_mt, preds_climate = to_np(combined_preds_mt), to_np(combined_preds_climate)
        preds_month = to_np(combined_preds_month) if combined_preds_month else None
        results.update(preds_mt=preds_mt, preds_climate=preds_climate, preds_month=preds_month,
                       loss_reg=float(combined_loss_mt[0]) / max(n_seen, 1), loss_climate=float(combined_loss_mt[1]) / max(n_seen, 1),
                       loss_month=float(combined_loss_mt[2]) / max(n_seen, 1))
    if spread is not None:
        results.update(expected_km=to_np([s.expected_km for s in combined_spread]), expected_score=to_np([s.expected_score for s in combined_spread]),
                       radius_km=to_np([s.radius_km for s in combined_spread]), spread_quantiles=tuple(float(q) for q in spread))
        try:
            true_lla = np.asarray(dataset['labels'])
        except (KeyError, IndexError, TypeError, ValueError):
            true_lla = None                                                       # no labels: the three columns only
        if true_lla is not None and len(true_lla) == len(preds):
            results.update(spread_metrics(results['radius_km'], results['spread_quantiles'], haversine_np(preds, true_lla),
                                          results['expected_km'], results['expected_score']))
    if best_guess is not None:
        results.update(best_LLH=to_np([g.point for g in combined_best]), best_index=to_np([g.index for g in combined_best]),
                       best_expected=to_np([g.expected for g in combined_best]), best_taken=to_np([g.taken for g in combined_best]))
        try:
            true_lla = np.asarray(dataset['labels'])
        except (KeyError, IndexError, TypeError, ValueError):
            true_lla = None
        best_extra = {}
        if true_lla is not None and len(true_lla) == len(preds):
            best_extra = best_guess_metrics(results['best_LLH'], haversine_np, true_lla, results['best_taken'])
    nn_extra = {}
    if nn_index is not None:
        results.update(nn_rows=to_np([n.rows for n in combined_nn]), nn_distance=to_np([n.distance for n in combined_nn]),
                       nn_lnglat=to_np([n.lnglat for n in combined_nn]), nn_certified=to_np([n.certified for n in combined_nn]))
        try:
            true_lla = np.asarray(dataset['labels'])
        except (KeyError, IndexError, TypeError, ValueError):
            true_lla = None
        if true_lla is not None and len(true_lla) == len(preds) and len(preds):
            nn_extra = neighbour_metrics(results['nn_lnglat'], haversine_np, true_lla, preds)
    if metrics is not None:                                                       # :122-140
        labels_lla, labels_cell = dataset['labels'], dataset['labels_clf']
        if isinstance(labels_lla, np.ndarray) == False:
            labels_lla, labels_cell = np.asarray(labels_lla), np.asarray(labels_cell)
        labels_mt = labels_climate = labels_month = None
        if preds_mt is not None:
            labels_mt, labels_climate = np.asarray(dataset['labels_multi_task']), np.asarray(dataset['labels_climate'])
            labels_month = np.asarray(dataset['labels_month']) if preds_month is not None else None
        collected = (preds, preds_geocells, preds_mt, preds_climate, preds_month, top5_geocells,
                     labels_lla, labels_cell, labels_mt, labels_climate, labels_month)
        results.update(metrics(collected))
    if best_guess is not None:
        results.update(best_extra)
    results.update(nn_extra)
    if bootstrap is not None and int(os.environ.get('RANK', '0')) == 0:
        from . import bootstrap as boot
        cols, stats = boot.metric_columns(collected, countries=countries, best_LLH=results['best_LLH'] if best_guess is not None and best_extra else None,
                                          best_taken=results['best_taken'] if best_guess is not None and best_extra else None,
                                          nn_lnglat=results['nn_lnglat'] if nn_extra else None)
        stats = {k: s for k, s in stats.items() if k in results or ' - ' in k}      # what this run reports, and the paired differences
        results['bootstrap'] = boot.bootstrap(cols, stats, R=int(bootstrap), seed=bootstrap_seed, level=bootstrap_level,
                                              device=model.cell_layer.weight.device)
        results['bootstrap_level'] = float(bootstrap_level)
    model.train()
    logger.warning('Back to training ...')
    return results


def evaluate(model: str, dataset, yfcc: bool, landmarks: bool, base_model=None, heading: bool = False,
             refine: bool = True, geocell_path: Optional[str] = None, proto_path: Optional[str] = None,
             dataset_path=None, bank=None, head_state: Optional[str] = None, multi_task: bool = False,
             calibration: Optional[str] = None, embedding_rel_tol: Optional[float] = None, country_path: Optional[str] = None,
             bank_rel_tol=None, spread=None, best_guess=None, neighbours=None, temperature=None, bootstrap=None,
             bootstrap_seed: int = 0, bootstrap_level: float = 0.95, refiner_settings=None):
    """reference evaluation/evaluate.py:10-85.

    `base_model`: as in the reference a STRING -- config.CLIP_MODEL for the pretrained tower, or the path of a checkpoint whose
    weights are copied over it by name (`load_state_dict`, :36-40; the pretrained tower is resolved from local files only, see
    `clip_embedder.load_pretrained_clip`) -- or, additionally, a ready module (`HipCLIPVisionModel`, or any module with a
    transformers CLIPVisionModel state dict), or None to evaluate on precomputed embeddings.  `model` is the path of
    the head checkpoint (`full_model.load_state(model)`, :46); evaluate() uses the reference's two refiner
    parameter sets (:73-80): first build -> ProtoRefiner(20, False, 10000, temperature=1); cached prototypes ->
    ProtoRefiner(40, False, 100000, temperature=0.6).  "Cached" means, in this order: a `bank` argument, the packed CSR
    file `<proto_model_path>.npz` this package writes at its first build, or the reference's own pickle at
    `proto_model_path` (`torch.save(refiner, ...)`, read with `load_refiner_cache` -- an existing
    saved_models/refiner/proto.refiner keeps working).
    `multi_task` (the reference's evaluate hard-wires False, :43; its `run.py -m` trains such models): build the model with the
    regression, climate and month heads, so that a multi-task checkpoint loads completely and the multi-task metrics are reported
    when the dataset carries `labels_multi_task` / `labels_climate` / `labels_month`.
    `calibration` (a path; pigeon_amd/certainty.py): if the file exists it is loaded AFTER the weights and before the first batch
    (`SuperGuessr.load_calibration`: a file measured on other weights raises); if not, the run calibrates on its first batch as
    without the argument and rank 0 writes the file at the end (in a multi-rank job: rank 0's own measurement).
    `embedding_rel_tol` (precomputed embeddings, `base_model=None`): the relative error the dataset's embeddings carry, passed to
    `SuperGuessr`.  None: the fast path's tolerance (1e-3, or what a calibration file says) -- right for files written by
    `run.py embed`; embeddings of the exact encoder or of the fp32 reference are declared with 5e-6.
    `bank_rel_tol`: the relative error the prototype bank's rows carry (`ProtoRefiner(bank_rel_tol=...)`): a number, or the path
    of the sidecar `run.py embed` wrote next to the embeddings the bank was built from (`embedding_meta.json`; its
    `embedding_rel_tol` is taken, and a sidecar written with other weights than the loaded tower's ends the run, both fingerprints
    named).  None: what the bank itself records, else exact.
    `country_path`: the GeoJSON of country polygons behind `Country_accuracy` (reference evaluation/metrics.py:17).  None: the file
    config.COUNTRY_PATH names if it exists, else the key is left out as before; a path given explicitly must exist.
    `spread`: quantiles handed to `evaluate_model(spread=...)`; None (default): no spread is computed.
    `best_guess`: 'score' | 'km', handed to `evaluate_model(best_guess=...)`; None (default): nothing is computed.
    `neighbours`: K, handed to `evaluate_model(neighbours=...)` (needs refine=True); None (default): nothing is computed.
    `temperature`: a number, or the path of the sidecar `python -m pigeon_amd.temperature` wrote for this head (loaded AFTER the
    weights; another head's raises, both fingerprints named): `SuperGuessr.temperature`, so the spread and best-guess metrics are
    computed under the calibrated probabilities, and results['Temperature'] is printed with the metrics.  None (default): nothing
    changes.  The accuracy and distance metrics of the model's own guess do not depend on it.
    `bootstrap` / `bootstrap_seed` / `bootstrap_level`: handed to `evaluate_model(bootstrap=...)`: R paired bootstrap replicates of
    every metric, results['bootstrap'], printed as `value [lo, hi]` with the paired differences below.  None (default): nothing
    changes -- no output, no key, no launch.
    `refiner_settings`: the refiner's (topk, temperature, max_refinement) -- a triple, the string `TOPK,TEMPERATURE,MAX_KM`, or the path
    of the sidecar `python -m pigeon_amd.refiner_fit` wrote for this head and this bank (another head's or bank's raises, both
    fingerprints named).  Applied after the refiner is built and printed; topk above the 50 candidates is refused.  None (default):
    nothing changes -- the literals below, the same output, no launch.
    """
    import os
    from . import config as cfg
    countries = None
    if country_path is not None and not os.path.exists(country_path):
        raise FileNotFoundError(f'evaluate: country polygons {country_path!r} do not exist')
    if os.path.exists(country_path or cfg.COUNTRY_PATH):
        from .regions import RegionBank
        countries = RegionBank.from_geojson(country_path or cfg.COUNTRY_PATH)
        print(f'Loaded {len(countries)} country polygons from {country_path or cfg.COUNTRY_PATH}')
    if isinstance(base_model, str):                                               # reference :36-40
        from .clip_embedder import HipCLIPVisionModel, load_pretrained_clip
        from .utils import load_state_dict
        path = base_model
        try:
            base_model = load_pretrained_clip()                                   # CLIP_MODEL, or the directory env PIGEON_CLIP_MODEL names
            if path != cfg.CLIP_MODEL:
                state_dict = torch.load(path, map_location='cpu')
                load_state_dict(base_model, state_dict)
                print(f'Initialized base model with weights from: {path}')
        except RuntimeError as why:
            if path == cfg.CLIP_MODEL or not os.path.exists(path):
                raise
            # no pretrained tower on this machine, but the checkpoint may carry all of it (base_model.* / vision_model.* names)
            state_dict = torch.load(path, map_location='cpu')
            state_dict = {('.'.join(k.split('.')[1:]) if 'base_model' in k.split('.')[0] else k): v for k, v in state_dict.items()}
            keys = {k[len('vision_model.'):] if k.startswith('vision_model.') else k for k in state_dict}
            if 'embeddings.patch_embedding.weight' not in keys or 'encoder.layers.0.mlp.fc2.weight' not in keys:
                raise RuntimeError(f'evaluate: {path!r} does not hold a complete vision tower and the pretrained one is unavailable '
                                   f'({why})') from why
            base_model = HipCLIPVisionModel(state_dict)
            print(f'Initialized base model with weights from: {path} (pretrained tower unavailable: checkpoint only)')
    tol_kw = {} if embedding_rel_tol is None else {'embedding_rel_tol': float(embedding_rel_tol)}
    full_model = SuperGuessr(base_model, panorama=True, hierarchical=False, multi_task=multi_task, heading=heading,
                             freeze_base=True, yfcc=yfcc, num_candidates=50, geocell_path=geocell_path, **tol_kw)
    # the reference's torch.load raises on a missing checkpoint (:46); only the explicit random-init names skip loading
    for ckpt in (head_state, model):
        if ckpt in (None, '', 'none', 'random'):
            continue
        if not os.path.exists(ckpt):
            raise FileNotFoundError(f'evaluate: checkpoint {ckpt!r} does not exist (pass "none" / "random" to evaluate '
                                    f'a randomly initialised head on purpose)')
        full_model.load_state(ckpt)
    full_model.to('cuda')
    print(full_model)
    write_calibration = False
    if calibration:
        if os.path.exists(calibration):                                           # weights first, then the calibration
            header = full_model.load_calibration(calibration)
            print(f'Loaded calibration {calibration} (fingerprint {header["fingerprint"]}, {header["samples"]} samples; {header["source"]})')
        else:
            write_calibration = int(os.environ.get('RANK', '0')) == 0
    if temperature is not None:
        full_model.load_temperature(temperature)
        print(f'Temperature {full_model.temperature:.6g}: spread and best-guess metrics under softmax(logits / T)')
    refiner = None
    bank_tol = _resolve_bank_rel_tol(bank_rel_tol, full_model)
    if refine:
        proto_model_path = cfg.PROTO_MODEL_YFCC_PATH if yfcc else cfg.PROTO_MODEL_PATH
        proto_path = proto_path or (cfg.PROTO_PATH_YFCC if yfcc else cfg.PROTO_PATH)
        dataset_path = dataset_path or (cfg.DATASET_PATH_YFCC if yfcc else cfg.DATASET_PATH)
        if landmarks:
            proto_path, proto_model_path = cfg.PROTO_PATH_LANDMARKS, cfg.PROTO_MODEL_LANDMARKS_PATH
            dataset_path = [cfg.DATASET_PATH_YFCC, cfg.DATASET_PATH_LANDMARKS]
        packed = proto_model_path + '.npz'
        protos = None
        if bank is None and not os.path.exists(packed):
            try:                                                                  # the reference's own cache (:65-69):
                protos = load_refiner_cache(proto_model_path)                     # torch.load(proto_model_path).protos
            except FileNotFoundError:
                pass
        if bank is not None:
            refiner = ProtoRefiner(40, False, 100000, bank=bank, temperature=0.6, bank_rel_tol=bank_tol)
        elif os.path.exists(packed):                                              # cached bank, packed CSR form
            refiner = ProtoRefiner(40, False, 100000, bank=packed, temperature=0.6, verbose=False, bank_rel_tol=bank_tol)
        elif protos is not None:                                                  # cached prototypes (:76-80)
            refiner = ProtoRefiner(40, False, 100000, proto_path=proto_path, dataset_path=dataset_path,
                                   protos=protos, temperature=0.6, verbose=False, bank_rel_tol=bank_tol)
        else:                                                                     # first build (:72-75)
            refiner = ProtoRefiner(20, False, 10000, proto_path=proto_path, dataset_path=dataset_path, temperature=1,
                                   bank_rel_tol=bank_tol)
            os.makedirs(os.path.dirname(packed) or '.', exist_ok=True)
            refiner.host_bank.save(packed)
        if refiner_settings is not None:
            from .refiner_fit import apply_to
            apply_to(refiner, refiner_settings, full_model)
        print(refiner)
        if refiner.bank_rel_tol > 0:
            print(f'Prototype bank declared at a relative error of {refiner.bank_rel_tol:.3g}: the refiner\'s certainty accounts for it')
    metrics = compute_geoguessr_metrics if countries is None else (lambda r: compute_geoguessr_metrics(r, countries=countries))
    results = evaluate_model(full_model, dataset, metrics, None, refiner, spread=spread, best_guess=best_guess, neighbours=neighbours,
                             bootstrap=bootstrap, bootstrap_seed=bootstrap_seed, bootstrap_level=bootstrap_level, countries=countries)
    if 'bootstrap' in results:
        from .bootstrap import report
        print(report(results['bootstrap'], results['bootstrap_level']))
    if temperature is not None:
        results['Temperature'] = full_model.temperature
        print(f"Temperature: {results['Temperature']:.6g}")
    if write_calibration:
        if full_model.base_model is not None and full_model.certainty.calibrated:
            full_model.save_calibration(calibration, source=f'evaluate, first batch, {full_model.certainty.stats.get("samples")} samples')
            print(f'Calibration written to {calibration}')
        else:
            print(f'No calibration written to {calibration}: nothing was measured in this run (no encoder, the exact tier off, '
                  'or fewer than 8 samples)')
    return results


def _resolve_bank_rel_tol(value, model: SuperGuessr) -> Optional[float]:
    """`evaluate(bank_rel_tol=...)`: None, a number (also as a string), or the path of an `embedding_meta.json` sidecar, which must
    have been written with the weights of `model`'s tower (no tower -- precomputed embeddings: nothing to compare with)."""
    if value is None:
        return None
    try:
        return float(value)
    except (TypeError, ValueError):
        pass
    from .certainty import require_fingerprint
    from .embed import load_embedding_meta
    meta = load_embedding_meta(str(value))
    if model.base_model is not None:
        header = dict({'layers': '?', 'ln_fold': '?', 'source': ''}, **meta)
        require_fingerprint(str(value), header, model._encoder().fingerprint())
    return float(meta['embedding_rel_tol'])


class PanoramaPipeline:
    """The data-parallel inference step (BASELINE.json configs[3]/[4]): every rank runs the ViT + geocell head on
    its shard of panoramas, ONE grouped all-gather moves per-image embeddings (B,4,1024) f32 + top-k candidates + initial
    predictions + sample indices to every rank (the reference's accelerator.gather, preprocessing/embed.py:36-37),
    each rank refines its 1/W slice of the gathered batch against its replica of the prototype bank, and a second, tiny
    grouped all-gather concatenates the refined (lng,lat) / geocell of all slices (plus, round 6, the certainty flags and every rank's
    exact-tier queue length), so that every rank -- rank 0 in particular -- holds the whole batch's result as the reference's
    collection loop does (training/train_eval_loop.py:98-112).  All outputs are rank-major; `distributed.restore_order(res['index'],
    ...)` puts them back in sample order.

    Round 6: the step is `pigeon_amd.deferred.DeferredExact.submit` -- no host synchronisation, the rows the 16-bit encoder cannot
    settle wait in a device queue for ONE exact pass per `min_flush` panoramas (default: what fills one round of the CUs with the
    exact encoder's panels -- 7 panoramas on 256 CUs, `deferred.round_quantum`), taken by every rank in the same step on the same
    number of slots.  `submit` returns the steps that became final (a few steps late, in order), `flush` the rest; `step` = submit +
    flush (settled before it returns: the form tests, `smoke()` and single calls use)."""

    def __init__(self, model: SuperGuessr, refiner: Optional[ProtoRefiner], comm: Optional[Communicator] = None,
                 min_flush: Optional[int] = None, max_lag: int = 12, ops=None, pass_quantum: Optional[int] = None):
        self.model, self.refiner = model, refiner
        self.comm = comm or Communicator()
        self.engine = DeferredExact(model, refiner, self.comm, ops=ops, min_flush=min_flush, max_lag=max_lag,
                                    pass_quantum=pass_quantum)
        self.last_info = None            # of the newest result handed out: certain, cause, exact, queued

    @property
    def split_marks(self):
        return self.engine.marks

    @split_marks.setter
    def split_marks(self, v):
        """Set to a list to collect five time stamps per submitted step (see split_ms): compute vs gather(-wait)."""
        self.engine.marks = v

    @staticmethod
    def split_ms(marks):
        """(compute ms, gather ms) of one step's five marks: [start, before gather 1, after it, before gather 2, end].  On the
        device the gather spans include the time this rank WAITS for the slowest rank to arrive at the collective."""
        if isinstance(marks[0], float):
            d = [(b - a) * 1e3 for a, b in zip(marks[:-1], marks[1:])]
        else:
            d = [a.elapsed_time(b) for a, b in zip(marks[:-1], marks[1:])]
        return d[0] + d[2], d[1] + d[3]

    def _note(self, done):
        if done:
            r = done[-1]
            self.last_info = dict(certain=r['certain'], cause=r['cause'], exact=r['exact'], queued=r['queued'], step=r['step'],
                                  boundary_checked=self.engine.boundary_checked)
        return done

    @torch.no_grad()
    def submit(self, pixel_values: torch.Tensor = None, index: Optional[torch.Tensor] = None, meta=None, pixel_bytes: torch.Tensor = None):
        return self._note(self.engine.submit(pixel_values, index=index, meta=meta, pixel_bytes=pixel_bytes))

    @torch.no_grad()
    def flush(self):
        return self._note(self.engine.flush())

    @torch.no_grad()
    def step(self, pixel_values: torch.Tensor = None, index: Optional[torch.Tensor] = None, pixel_bytes: torch.Tensor = None):
        """`pixel_bytes` (instead of pixel_values): uint8 (B,12,336,336) / (B,3,336,336) 8-bit pixels, a quarter of the resident batch."""
        done = self.submit(pixel_values, index, pixel_bytes=pixel_bytes) + self.flush()
        return done[-1]
