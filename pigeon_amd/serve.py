"""The serving endpoint the reference's GeoGuessr bot talks to.

The reference ships only the CLIENT: `bot/chrome_extension/scripts/duel.js:51-64` posts four street-view screenshots
(headings 0 / 90 / 180 / 270 degrees, `chrome.tabs.captureVisibleTab` data URIs) as JSON to
`POST http://127.0.0.1:5000/api/v1/predict` and reads `guess.results.lat` / `guess.results.lng` from the answer
(:66-70); after the round it posts the game state to `POST /api/v1/game` (:86-97) and ignores the body.  The backend
behind that port is not in the repository ("an external server running PIGEON on an NVIDIA A100", bot/README.md).  This
module is that backend over the HIP hot path: decode -> CLIP preprocessing (`pg_prep_forward` on the GPU) ->
`SuperGuessr(serving=True)` (the tuple path, reference models/super_guessr.py:462-466) -> optional `ProtoRefiner`.

    app = make_app(model, refiner)              # model: SuperGuessr(..., panorama=True, serving=True).eval()
    uvicorn.run(app, host="127.0.0.1", port=5000)

`predict_panorama` is the whole request handler without HTTP, so the GPU tests can call it directly.  The model and the
preprocessor are injected: the module itself imports neither torch.cuda nor the HIP library, and the HTTP contract is
tested on CPU with a stub model (tests/test_serve_cpu.py).
"""
from __future__ import annotations

import base64
import io
import json
from typing import Callable, Dict, List, Optional, Sequence

IMAGE_KEYS = ("image", "image_2", "image_3", "image_4")          # duel.js:59-62, in heading order
PANORAMA_KEY = "panorama"                                        # ours: one equirectangular image instead of the four views
SPREAD_QUANTILES = (0.5, 0.9)                                    # of `spread=True`: the radii a response carries


class BadRequest(ValueError):
    pass


def decode_data_uri(uri: str):
    """'data:image/png;base64,....' (or bare base64) -> RGB PIL image."""
    from PIL import Image
    if not isinstance(uri, str) or not uri:
        raise BadRequest("image field must be a non-empty data URI string")
    payload = uri.split(",", 1)[1] if uri.startswith("data:") else uri
    try:
        raw = base64.b64decode(payload, validate=False)
        img = Image.open(io.BytesIO(raw))
        img.load()
    except Exception as e:                                        # PIL raises many types for corrupt input
        raise BadRequest(f"cannot decode image: {e}") from e
    return img.convert("RGB")


def data_uri_bytes(uri: str) -> bytes:
    """'data:image/jpeg;base64,....' (or bare base64) -> the file's bytes, undecoded."""
    if not isinstance(uri, str) or not uri:
        raise BadRequest("image field must be a non-empty data URI string")
    payload = uri.split(",", 1)[1] if uri.startswith("data:") else uri
    try:
        return base64.b64decode(payload, validate=False)
    except Exception as e:
        raise BadRequest(f"cannot decode image: {e}") from e


class EquirectRequest:
    """One equirectangular panorama of a request (`image`: a PIL image, or the file's bytes in the encoded mode) and the compass
    heading of its centre column: `predict_panorama` renders the four views 0 / 90 / 180 / 270 from it on the GPU."""

    def __init__(self, image, centre_heading: float = 0.0):
        self.image, self.centre_heading = image, float(centre_heading)


def panorama_from_request(body: Dict, encoded: bool = False):
    """The four views of one location.  A single-image request (`classic.js` sends only `image`) is answered from that
    view repeated four times: the panorama head averages the four panel embeddings (super_guessr.py:437).
    encoded=True: the views stay the payloads' bytes, for `predict_panorama` to decode on the GPU.
    A body with the key `panorama` (ONE data URI: an equirectangular image) and optionally `panorama_heading` (compass heading of its
    centre column, default 0) gives an EquirectRequest instead, answered like a four-image request; together with any of `image` ..
    `image_4` it is a BadRequest."""
    if isinstance(body, dict) and PANORAMA_KEY in body:
        if any(k in body for k in IMAGE_KEYS):
            raise BadRequest("'panorama' cannot be combined with 'image' .. 'image_4': send the equirectangular image or the four views")
        heading = body.get("panorama_heading", 0.0)
        if isinstance(heading, bool) or not isinstance(heading, (int, float)) or heading != heading or abs(heading) == float("inf"):
            raise BadRequest("'panorama_heading' must be a finite number (degrees)")
        return EquirectRequest((data_uri_bytes if encoded else decode_data_uri)(body[PANORAMA_KEY]), heading)
    if not isinstance(body, dict) or IMAGE_KEYS[0] not in body:
        raise BadRequest("JSON body with an 'image' field expected")
    views = [(data_uri_bytes if encoded else decode_data_uri)(body[k]) for k in IMAGE_KEYS if body.get(k)]
    if len(views) == 1:
        views = views * 4
    if len(views) != 4:
        raise BadRequest(f"1 or 4 images expected, got {len(views)}")
    return views


def predict_panorama(views: Sequence, model, refiner=None, preprocess: Optional[Callable] = None, attribution: bool = False,
                     spread: bool = False, best_guess: bool = False, neighbours: Optional[int] = None, confidence: bool = False) -> Dict:
    """views: four PIL images (or the EquirectRequest of a `panorama` body) -> {'lat', 'lng'} (+ 'geocell_margin', 'geocell_certain', 'reencoded_exact' when the model exposes the
    certainty of its top-1).  `preprocess(list of PIL) -> (4,3,336,336)` defaults to the GPU path.  Views that are all `bytes` (image
    files) go to the same path undecoded: baseline JPEGs are decoded on the GPU (pigeon_amd/jpeg.py: Pillow's pixels, bit for bit),
    anything else by Pillow; a payload neither can read is a BadRequest.  With an injected `preprocess` bytes are decoded first.
    attribution=True adds 'attribution': the top-1 cell against its runner-up as a sum over the views' patches (`model.attribute`,
    pigeon_amd/explain.py `attribution_json`; on the exact tier when this panorama was re-encoded there).
    spread=True adds how far off the answer may be (`model.spread` at the returned point, SPREAD_QUANTILES): 'expected_km',
    'expected_score' (the GeoGuessr score before its rounding) and 'radius_km': {"0.5": km, "0.9": km}, the radii of the circles
    around the answer that hold, whole, cells carrying that share of the head's probability.
    best_guess=True answers with the point of the largest expected GeoGuessr score (`model.best_guess` over the geocell centroids, the
    former answer as the incumbent): 'lat' / 'lng' become the chosen point -- the extension reads nothing else --, the former answer
    moves to 'argmax_lat' / 'argmax_lng', and 'guess_expected_score' and 'guess_changed' are added.  The `spread` keys, when asked
    for as well, still describe the former answer.
    neighbours=K (1..64) adds 'neighbours': [{'lat', 'lng', 'distance', 'row'}, ...], the K training panoramas whose embeddings are
    nearest to this one's (exact search over the refiner's bank, pigeon_amd/neighbours.py), nearest first; it needs a refiner.
    confidence=True adds 'confidence', a float: the probability of the top-1 geocell under softmax(logits / model.temperature)
    (`model.confidence`, one pg_temper_stats row pass); `spread` and `best_guess` integrate over the same calibrated probabilities."""
    import torch
    if confidence and not hasattr(model, "confidence"):
        raise ValueError("predict_panorama(confidence=True): this model has no `confidence` (it needs SuperGuessr.confidence)")
    nn_index = None
    if neighbours is not None:
        from .neighbours import index_of
        nn_index = index_of(refiner, neighbours, "predict_panorama(neighbours=K)")
    if best_guess and not hasattr(model, "best_guess"):
        raise ValueError("predict_panorama(best_guess=True): this model has no `best_guess` (it needs SuperGuessr.best_guess)")
    bg = None
    if spread and not hasattr(model, "spread"):
        raise ValueError("predict_panorama(spread=True): this model has no `spread` (it needs SuperGuessr.spread)")
    sp = None
    if isinstance(views, EquirectRequest):
        # one equirectangular image: its four views are rendered on the GPU (pigeon_amd/panorama.py) into the buffer the resize reads;
        # a file's bytes go there as bytes.  The views exist on the device only, so an injected host `preprocess` cannot take them.
        if preprocess is not None:
            raise BadRequest("a 'panorama' request is rendered by the GPU preprocessing; this server runs with an injected one")
        from .panorama import panorama_pixels
        heading, as_bytes = views.centre_heading, isinstance(views.image, (bytes, bytearray))
        views = views.image
        if as_bytes:
            from .jpeg import EncodedImages
            views = EncodedImages([bytes(views)])
        preprocess = lambda source: panorama_pixels(source, centre_heading=heading)        # noqa: E731
    else:
        views = list(views)
        as_bytes = bool(views) and all(isinstance(v, (bytes, bytearray)) for v in views)
        if as_bytes and preprocess is not None:
            views = [decode_data_uri(base64.b64encode(bytes(v)).decode()) for v in views]
        if preprocess is None:
            from .clip_embedder import gpu_preprocess
            preprocess = gpu_preprocess
            if as_bytes:
                from .jpeg import EncodedImages
                views = EncodedImages(views)
    try:
        px = preprocess(views)                                     # (4,3,336,336), CLIP-normalised
    except (ValueError, OSError) as e:
        if not as_bytes:
            raise
        raise BadRequest(f"cannot decode image: {e}") from e       # a damaged scan / a file Pillow cannot identify or read
    px = px.reshape(1, 12, px.shape[-2], px.shape[-1])             # one panorama, panels along the channel axis (:386-393)
    with torch.no_grad():
        if hasattr(model, "encode_head"):
            # pigeon_amd.SuperGuessr: the same call with the certainty of every discrete output (top-1 cell AND what the refiner below
            # will pick) checked, and the panorama re-encoded in the exact mode if it is not certain (exact_top1, the default)
            from .evaluate import certain_forward
            out, info = certain_forward(model, refiner, pixel_values=px, spread=SPREAD_QUANTILES if spread else None,
                                        best_guess="score" if best_guess else None)
            sp, bg = info.get("spread"), info.get("best_guess")
            pred_llh, topk, embedding = out[0], out[1], out[-1]    # multi-task models put preds_mt in between (:463-464)
            if refiner is not None:
                pred_llh = info["refined_LLH"]                     # the refinement certain_forward ran (once; re-run for re-encoded rows)
        else:
            out = model(pixel_values=px)                           # serving tuple, [lng, lat] order (:455, :462-466)
            pred_llh, topk, embedding = out[0], out[1], out[-1]    # 3 elements, or 4 with preds_mt third (multi-task, :463-464)
            if refiner is not None:
                _, pred_llh, _ = refiner(embedding=embedding, initial_preds=pred_llh, candidate_cells=topk.indices,
                                         candidate_probs=topk.values)
            if spread:
                sp = model.spread(points=pred_llh.reshape(-1, 2).to(torch.float64), quantiles=SPREAD_QUANTILES)
            if best_guess:
                bg = model.best_guess(objective="score", incumbent=pred_llh.reshape(-1, 2).to(torch.float64))
    lng, lat = (float(v) for v in pred_llh.reshape(-1, 2)[0].tolist())
    res = {"lat": lat, "lng": lng}
    if bg is not None:                                             # the chosen point answers; the former answer stays readable
        res["argmax_lat"], res["argmax_lng"] = lat, lng
        res["lng"], res["lat"] = (float(v) for v in bg.point.reshape(-1, 2)[0].tolist())
        res["guess_expected_score"] = float(torch.where(bg.taken, bg.expected, bg.incumbent_expected).reshape(-1)[0])
        res["guess_changed"] = bool(bg.taken.reshape(-1)[0])
    # certainty of the geocell top-1 (pigeon_amd.SuperGuessr, round 4): extra keys, the extension reads lat / lng only
    if getattr(model, "last_certain", None) is not None:
        res["geocell_margin"] = float(model.last_margin.reshape(-1)[0])
        res["geocell_certain"] = bool(model.last_certain.reshape(-1)[0])
        res["reencoded_exact"] = bool(getattr(model, "last_reencoded", None) is not None and model.last_reencoded.numel() > 0)
    if confidence:
        res["confidence"] = float(model.confidence().reshape(-1)[0])
    if sp is not None:                                             # extra keys as well: the extension reads lat / lng only
        res["expected_km"] = float(sp.expected_km.reshape(-1)[0])
        res["expected_score"] = float(sp.expected_score.reshape(-1)[0])
        res["radius_km"] = {f"{q:g}": float(r) for q, r in zip(sp.quantiles, sp.radius_km.reshape(-1, len(sp.quantiles))[0].tolist())}
    if nn_index is not None:
        nn = nn_index.search(embedding.reshape(1, -1, embedding.shape[-1]) if embedding.dim() > 2 else embedding.reshape(1, -1), k=neighbours)
        rows, dist, ll = nn.rows[0].tolist(), nn.distance[0].tolist(), nn.lnglat[0].tolist()
        res["neighbours"] = [{"lat": float(p[1]), "lng": float(p[0]), "distance": float(d), "row": int(r)}
                             for r, d, p in zip(rows, dist, ll) if r >= 0]
    if attribution:
        from .explain import attribution_json
        with torch.no_grad():
            att = model.attribute(pixel_values=px, tier="exact" if res.get("reencoded_exact") else "fast")
        res["attribution"] = attribution_json(att)
    return res


def make_app(model, refiner=None, preprocess: Optional[Callable] = None, game_log: Optional[List] = None, encoded: bool = False,
             spread: bool = False, best_guess: bool = False, neighbours: Optional[int] = None, confidence: bool = False):
    """Starlette application with the two routes the extension calls.  encoded=True: the payloads are handed on as bytes and decoded
    on the GPU (see predict_panorama); the response is the same.  spread=True: every answer carries 'expected_km', 'expected_score'
    and 'radius_km' (see predict_panorama); a model without `spread` is refused here, not per request.  best_guess=True: every answer
    is the point of the largest expected score (see predict_panorama); a model without `best_guess` is refused here as well.  neighbours=K: every answer carries its K nearest
    training panoramas (see predict_panorama); refused here without a refiner bank, and the search index is built here, not per request.
    confidence=True: every answer carries 'confidence', the calibrated top-1 probability (see predict_panorama)."""
    if confidence and not hasattr(model, "confidence"):
        raise ValueError("make_app(confidence=True): this model has no `confidence` (it needs SuperGuessr.confidence)")
    if neighbours is not None:
        from .neighbours import index_of
        index_of(refiner, neighbours, "make_app(neighbours=K)")
    if best_guess and not hasattr(model, "best_guess"):
        raise ValueError("make_app(best_guess=True): this model has no `best_guess` (it needs SuperGuessr.best_guess)")
    if spread and not hasattr(model, "spread"):
        raise ValueError("make_app(spread=True): this model has no `spread` (it needs SuperGuessr.spread)")
    from starlette.applications import Starlette
    from starlette.responses import JSONResponse
    from starlette.routing import Route

    async def predict(request):
        try:
            body = await request.json()
            views = panorama_from_request(body, encoded)
        except (BadRequest, json.JSONDecodeError) as e:
            return JSONResponse({"error": str(e)}, status_code=400)
        attribution = body.get("attribution") is True
        if attribution and not hasattr(model, "attribute"):
            return JSONResponse({"error": "this model has no patch attribution ('attribution': true needs SuperGuessr.attribute)"},
                                status_code=400)
        # called inline on the event loop, on purpose: the handles behind `model` are one per (device, stream) and not
        # thread-safe, so requests are answered one at a time -- a `def` handler would run in Starlette's pool
        try:
            res = predict_panorama(views, model, refiner, preprocess, attribution=attribution, spread=spread, best_guess=best_guess,
                                   neighbours=neighbours, confidence=confidence)
        except BadRequest as e:                                    # (encoded mode: the payloads are only decoded in there)
            return JSONResponse({"error": str(e)}, status_code=400)
        return JSONResponse({"gameID": body.get("gameID"), "roundID": body.get("roundID"), "results": res})

    async def game(request):                                       # duel.js:86-97: fire-and-forget round log
        try:
            body = await request.json()
        except json.JSONDecodeError as e:
            return JSONResponse({"error": str(e)}, status_code=400)
        if game_log is not None:
            game_log.append(body)
        return JSONResponse({"status": "ok"})

    return Starlette(routes=[Route("/api/v1/predict", predict, methods=["POST"]),
                             Route("/api/v1/game", game, methods=["POST"])])


def main(argv=None):
    """python -m pigeon_amd.serve --head <head.model> [--geocells <csv>] [--protos <csv> --dataset <dir>] [--calibration <file>] [--spread] [--guess expected-score] [--neighbours K] [--temperature FILE|NUMBER] [--refiner FILE|TOPK,TEMPERATURE,MAX_KM] [--port 5000]"""
    import os
    ap = _arg_parser()
    args = ap.parse_args(argv)
    if args.neighbours is not None and not args.protos:
        ap.error("--neighbours K searches the refiner's bank of training embeddings: give --protos and --dataset")
    if args.neighbours is not None and not 1 <= args.neighbours <= 64:
        ap.error(f"--neighbours must be in 1..64, got {args.neighbours}")
    if args.calibration and not os.path.exists(args.calibration):
        ap.error(f"--calibration {args.calibration}: no such file (the server only loads a calibration; write one with "
                 "`python -m pigeon_amd.calibrate` or `run.py evaluate --calibration`)")
    import torch
    import uvicorn
    from .clip_embedder import HipCLIPVisionModel
    from .super_guessr import SuperGuessr
    kw = {"geocell_path": args.geocells} if args.geocells else {}
    from .clip_embedder import load_pretrained_clip
    try:
        base = load_pretrained_clip()                                  # CLIP_MODEL from local files (env PIGEON_CLIP_MODEL / HF cache)
    except RuntimeError as why:
        print(f"[serve] no pretrained tower ({why}); using a seeded random-init ViT-L/14-336 with {args.layers} layers")
        base = HipCLIPVisionModel(seed=0, layers=args.layers)
    model = SuperGuessr(base, panorama=True, serving=True, freeze_base=True, exact_top1=args.exact_top1, **kw).to("cuda").eval()
    if args.head:
        model.load_state(args.head)
    if args.calibration:                                               # after the weights: the first request is answered calibrated
        header = model.load_calibration(args.calibration)
        print(f"[serve] calibration {args.calibration}: fingerprint {header['fingerprint']}, {header['samples']} samples; "
              f"{model.certainty.describe()}")
    if args.temperature is not None:                                   # after the weights: a sidecar is keyed to the head
        model.load_temperature(args.temperature)
        print(f"[serve] temperature {model.temperature:.6g}: spread, best guess and `confidence` under softmax(logits / T)")
    refiner = build_refiner(args, model)
    torch.cuda.synchronize()
    uvicorn.run(make_app(model, refiner, encoded=args.encoded, spread=args.spread, best_guess=args.guess == "expected-score",
                         neighbours=args.neighbours, confidence=args.temperature is not None), host=args.host, port=args.port)


def build_refiner(args, model):
    """The server's refiner: the constructor defaults over --protos / --dataset (a packed .npz bank is taken as it is), then --refiner
    (FILE | TOPK,TEMPERATURE,MAX_KM; pigeon_amd/refiner_fit.py) applied and printed.  None without --protos."""
    from .proto_refiner import ProtoRefiner
    if not args.protos:
        if getattr(args, "refiner", None) is not None:
            raise ValueError("--refiner sets the refiner's topk, temperature and max_km: give --protos and --dataset")
        return None
    if str(args.protos).endswith(".npz"):
        refiner = ProtoRefiner(bank=args.protos)
    else:
        refiner = ProtoRefiner(proto_path=args.protos, dataset_path=args.dataset)
    if getattr(args, "refiner", None) is not None:
        from .refiner_fit import apply_to
        apply_to(refiner, args.refiner, model, prefix="[serve] ")
    return refiner


def _arg_parser():
    import argparse
    ap = argparse.ArgumentParser(description=main.__doc__)
    ap.add_argument("--head", default=None, help="SuperGuessr checkpoint (torch.save state dict); random init if omitted")
    ap.add_argument("--geocells", default=None)
    ap.add_argument("--protos", default=None)
    ap.add_argument("--dataset", default=None)
    ap.add_argument("--layers", type=int, default=24)
    ap.add_argument("--no-exact-top1", dest="exact_top1", action="store_false",
                    help="switch the exact mode off (default on: panoramas whose discrete outputs are inside the 16-bit path's error band "
                         "are re-encoded in the encoder's exact mode, so that the answer is the reference's fp32 one)")
    ap.add_argument("--encoded", action="store_true", default=False,
                    help="hand the requests' payloads on as bytes: baseline JPEGs are decoded on the GPU into the buffer the resize reads "
                         "(the same pixels as Pillow's), anything else by Pillow as before")
    ap.add_argument("--spread", action="store_true", default=False,
                    help="add to every answer how far off it may be: expected_km, expected_score and radius_km {\"0.5\", \"0.9\"} "
                         "(SuperGuessr.spread at the returned point); the extension reads lat / lng only")
    ap.add_argument("--guess", choices=("expected-score",), default=None,
                    help="answer with the point of the largest expected GeoGuessr score under the head's probabilities (SuperGuessr.best_guess "
                         "over the geocell centroids): lat / lng become that point, the former answer moves to argmax_lat / argmax_lng")
    ap.add_argument("--neighbours", type=int, default=None, metavar="K",
                    help="add to every answer its K (1..64) nearest training panoramas, neighbours: [{lat, lng, distance, row}, ...] "
                         "(exact search over the refiner's bank of training embeddings); needs --protos and --dataset")
    ap.add_argument("--temperature", default=None, metavar="FILE|NUMBER",
                    help="the temperature of the head's probabilities: a number, or the sidecar `python -m pigeon_amd.temperature` wrote "
                         "for this head (as in `run.py evaluate --temperature`); every answer gains `confidence`, the calibrated "
                         "top-1 probability, and --spread / --guess use the calibrated probabilities")
    ap.add_argument("--refiner", default=None, metavar="FILE|TOPK,TEMPERATURE,MAX_KM",
                    help="the refiner's topk, temperature and veto radius: three numbers, or the sidecar `python -m pigeon_amd.refiner_fit` "
                         "wrote for this head and these prototypes (as in `run.py evaluate --refiner`); needs --protos")
    ap.add_argument("--host", default="127.0.0.1")
    ap.add_argument("--port", type=int, default=5000)
    ap.add_argument("--calibration", default=None, metavar="FILE",
                    help="encoder calibration file (pigeon_amd/certainty.py), LOAD ONLY: it must exist and match the weights.  The first "
                         "request is then answered with the measured tolerance and de-biased embeddings, instead of the uncalibrated "
                         "tolerance until 16 panoramas have come in")
    return ap


if __name__ == "__main__":
    main()
