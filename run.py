"""Command-line entry, same surface as the reference's run.py (:21-93): the mode is the first positional
argument (`pretrain | finetune | embed | evaluate`), then the model name/path.

Only the inference hot path is implemented here: `embed` (multi-GPU CLIP embedding of a dataset,
preprocessing/embed.py) and `evaluate` (SuperGuessr + ProtoRefiner, evaluation/evaluate.py).  `pretrain` and
`finetune` are training and out of scope -> NotImplementedError.

Because the reference's weights / geocells / data are not public (reference README.md:11) every input can be
replaced by seeded synthetic fixtures:  `--synthetic N` embeds / evaluates N synthetic panoramas.

  python run.py embed saved_models/StreetviewCLIP.model -l data/hf_dataset          # weights from a checkpoint
  python run.py embed random --synthetic 64                                        # plumbing check, random ViT
  python run.py evaluate saved_models/head.model -l data/hf_eval -b saved_models/StreetviewCLIP.model
  python run.py evaluate saved_models/head_mt.model -m -l data/hf_eval -b saved_models/StreetviewCLIP.model   (a multi-task checkpoint)
  torchrun --nproc-per-node 8 --master-addr 127.0.0.1 run.py embed random --synthetic 4096
  python run.py embed random --synthetic 64 --calibration cal.npz                  # first run writes cal.npz, later runs load it
  python run.py embed saved_models/StreetviewCLIP.model -l data/hf_dataset --exact  # the exact encoder: embeddings for a prototype bank
  python run.py evaluate saved_models/head.model -l data/hf_pano -b saved_models/StreetviewCLIP.model --raw-images --encoded --equirect
                                                                                   # one equirectangular file per item: views rendered on the GPU
"""
import argparse
import logging
import os

import torch

logger = logging.getLogger('run')


def parse_list(input_list_str):
    return input_list_str.split(',')


argp = argparse.ArgumentParser()
argp.add_argument('function', help='Whether to pretrain, finetune or evaluate a model',
                  choices=['pretrain', 'finetune', 'embed', 'evaluate'])
argp.add_argument('name', help='Path to trained model weights (or "random" for a seeded random-init ViT).')
argp.add_argument('-l', '--load', help='Comma-separated list of processed dataset path.', default=None, type=parse_list)
argp.add_argument('-b', '--base', help='Path to base model.', default=None)
argp.add_argument('-s', '--sample', help='How many examples to sample for training.', default=None)
argp.add_argument('-a', '--auxiliary', action='store_true', default=False)
argp.add_argument('-t', '--test', help='Set flag to evaluate on test set.', action='store_true', default=False)
argp.add_argument('-c', '--classification', action='store_true', default=True)
argp.add_argument('-m', '--multitask', action='store_true', default=False)
argp.add_argument('--heading', action='store_true', default=False)
argp.add_argument('-r', '--resume', action='store_true', default=False)
argp.add_argument('--yfcc', action='store_true', default=False)
argp.add_argument('--landmarks', action='store_true', default=False)
# additions (not in the reference)
argp.add_argument('--synthetic', type=int, default=0, help='use N seeded synthetic panoramas instead of a dataset')
argp.add_argument('--layers', type=int, default=24, help='encoder layers for a "random" model')
argp.add_argument('--out-dir', default='data/landmark_embeddings')
argp.add_argument('--geocells', type=int, default=10000, help='synthetic geocell count')
argp.add_argument('--exact-top1', dest='exact_top1', action='store_true', default=None,
                  help="(default) re-encode the panoramas whose discrete outputs are inside the 16-bit path's error band in the "
                       "encoder's exact mode, so that geocell argmax and refined point are the reference's fp32 ones (PIGEON_EXACT_TOP1=1)")
argp.add_argument('--no-exact-top1', dest='exact_top1', action='store_false',
                  help="the 16-bit path alone (PIGEON_EXACT_TOP1=0): embeddings within 1e-3, discrete outputs not guaranteed")
argp.add_argument('--raw-images', dest='raw_images', action='store_true', default=False,
                  help="embed: items hold one image of any size each (PIL / uint8 array); the DataLoader workers decode and pack, "
                       "the resize + crop + normalise runs on the GPU for the whole mixed-size batch at once (pg_prep_ragged_forward).  "
                       "evaluate: items hold raw `image` (or `image`, `image_2`, `image_3`, `image_4`) columns of any sizes "
                       "(the reference's EvalDataset); they are packed by the workers, resized on the GPU to 8-bit pixels and "
                       "evaluated from those bytes (pigeon_amd.evaluate.ImageEvalDataset)")
argp.add_argument('--encoded', action='store_true', default=False,
                  help="with --raw-images: the items' image columns hold FILES (bytes, paths, or a datasets.Image(decode=False) column); the "
                       "workers only read them, baseline JPEGs are decoded on the GPU into the buffer the resize reads (Pillow's pixels, "
                       "bit for bit), anything else by Pillow in the main process; the count of those and why is printed once")
argp.add_argument('--equirect', action='store_true', default=False,
                  help="evaluate, with --raw-images: every item's single `image` column holds ONE equirectangular panorama (a file with "
                       "--encoded); the four 90-degree views at headings 0 / 90 / 180 / 270 are rendered from it on the GPU at "
                       "round(W / pi) pixels (at least 336) in front of the resize (pigeon_amd/panorama.py)")
argp.add_argument('--calibration', default=None, metavar='FILE',
                  help="encoder calibration file (bias vector, certainty tolerance, exact-encoder verdict; keyed by the weight "
                       "fingerprint).  If FILE exists it is loaded before the first batch -- every rank loads the same one, nothing is "
                       "measured inside a forward, and a file measured on other weights ends the run with an error.  If not, the run "
                       "calibrates on its first batch as without this option and rank 0 writes FILE at the end: `embed` writes the "
                       "vector all ranks already share, `evaluate` rank 0's own.  An explicit calibration run: python -m pigeon_amd.calibrate")


argp.add_argument('--embedding-rel-tol', dest='embedding_rel_tol', type=float, default=None, metavar='TOL',
                  help="evaluate on precomputed embeddings: the relative error they carry, against which their certainty is judged.  "
                       "Default: the 16-bit path's tolerance (1e-3, or what --calibration says), as `embed` writes them; 5e-6 declares "
                       "embeddings of the exact encoder or of the fp32 reference")


argp.add_argument('--exact', action='store_true', default=False,
                  help="embed: every image through the exact encoder (pg_vit_forward_precise, about 3x the time per image): the "
                       "embeddings to build a prototype bank from.  The sidecar embedding_meta.json written next to the .npy files "
                       "then says encoder 'exact' and the exact tier's tolerance")
argp.add_argument('--bank-rel-tol', dest='bank_rel_tol', default=None, metavar='TOL|FILE',
                  help="evaluate: the relative error the prototype bank's embeddings carry -- a number, or the embedding_meta.json "
                       "that `embed` wrote next to the embeddings the bank was built from (a file written with other weights than "
                       "the loaded tower's ends the run).  Default: what the bank records, else exact")


argp.add_argument('--guess', choices=('expected-score', 'expected-km'), default=None,
                  help="evaluate: also choose every guess by its expectation under the head's softmax (SuperGuessr.best_guess over the "
                       "geocell centroids) and report the _best metrics next to the existing ones")
argp.add_argument('--spread', action='store_true', default=False,
                  help="evaluate: how far off every guess may be (SuperGuessr.spread: expected km, expected GeoGuessr score, the radii "
                       "holding 0.5 and 0.9 of the head's probability) and, against the labels, how often the truth lies inside them "
                       "(Radius_50_coverage / Radius_90_coverage, to be read against 0.5 and 0.9)")
argp.add_argument('--temperature', default=None, metavar='FILE|NUMBER',
                  help="evaluate: the temperature of the head's probabilities -- a number, or the sidecar `python -m pigeon_amd.temperature` "
                       "wrote for this head; --spread and --guess are then computed under softmax(logits / T) and `Temperature` is "
                       "printed with the metrics.  The model's own guess and its accuracy do not change")
argp.add_argument('--refiner', default=None, metavar='FILE|TOPK,TEMPERATURE,MAX_KM',
                  help="evaluate: the refiner's topk, temperature and veto radius -- three numbers, or the sidecar "
                       "`python -m pigeon_amd.refiner_fit` wrote for this head and this prototype bank; applied after the refiner is built "
                       "and printed.  Without the flag the built-in settings are used, as before")
argp.add_argument('--bootstrap', type=int, default=None, metavar='R',
                  help="evaluate: R paired bootstrap replicates of every metric on the GPU (pigeon_amd.bootstrap): the metrics are printed as "
                       "`value [lo, hi]`, the paired differences (--guess, --neighbours against the model's own guess) below them")
argp.add_argument('--bootstrap-seed', dest='bootstrap_seed', type=int, default=0, metavar='S')
argp.add_argument('--bootstrap-level', dest='bootstrap_level', type=float, default=0.95, metavar='L')
argp.add_argument('--neighbours', type=int, default=None, metavar='K',
                  help="evaluate: also the K (1..64) nearest training embeddings of every item (exact search over the refiner's bank, "
                       "pigeon_amd.neighbours) and the retrieval baseline's _nn metrics: the nearest row's coordinates as the guess")
argp.add_argument('--countries', default=None, metavar='FILE',
                  help="evaluate: GeoJSON of country polygons (Polygon / MultiPolygon features) for `Country_accuracy`; default: "
                       "config.COUNTRY_PATH if that file exists, else the key is left out")


class _SyntheticImages(torch.utils.data.Dataset):
    def __init__(self, n, panorama):
        self.n, self.panorama = n, panorama

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if isinstance(i, str):                       # column access, as evaluate_model reads dataset['labels'] (train_eval_loop.py:123-124)
            import numpy as np
            return {'labels': np.zeros((self.n, 2)), 'labels_clf': np.zeros(self.n, dtype=np.int64)}[i]
        g = torch.Generator().manual_seed(1234 + i)
        if self.panorama:
            return {'pixel_values': torch.randn((12, 336, 336), generator=g), 'labels': torch.zeros(2, dtype=torch.float64),
                    'labels_clf': torch.tensor(0)}
        return {'image': torch.randn((3, 336, 336), generator=g), 'index': i}


class _SyntheticRawPanoramas(_SyntheticImages):
    """N seeded four-view items of raw uint8 images of mixed sizes, as a dataset with `image` ... `image_4` columns holds them."""
    SIZES = ((336, 336), (400, 640), (512, 384), (337, 500))

    def __init__(self, n, encoded=False):
        super().__init__(n, panorama=True)
        self.encoded = encoded

    def __getitem__(self, i):
        if isinstance(i, str):
            return super().__getitem__(i)
        g = torch.Generator().manual_seed(4321 + i)
        item = {'labels': torch.zeros(2, dtype=torch.float64), 'labels_clf': torch.tensor(0)}
        for v, key in enumerate(('image', 'image_2', 'image_3', 'image_4')):
            h, w = self.SIZES[(i + v) % len(self.SIZES)]
            item[key] = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).numpy()
            if self.encoded:
                item[key] = _jpeg_file(item[key], i + v)
        return item


def _jpeg_file(arr, k):
    """A synthetic image as the dict a datasets.Image(decode=False) column yields: a JPEG file of one of the three samplings."""
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).resize((arr.shape[1] // 8 + 1, arr.shape[0] // 8 + 1)).resize((arr.shape[1], arr.shape[0]), Image.BICUBIC).save(
        buf, 'JPEG', quality=90, subsampling=k % 3)
    return {'bytes': buf.getvalue(), 'path': None}


class _SyntheticEquirect(_SyntheticImages):
    """N seeded equirectangular panoramas of two sizes, one `image` column each: raw uint8 arrays, or JPEG files with encoded."""
    SIZES = ((256, 512), (300, 640))

    def __init__(self, n, encoded=False):
        super().__init__(n, panorama=True)
        self.encoded = encoded

    def __getitem__(self, i):
        if isinstance(i, str):
            return super().__getitem__(i)
        g = torch.Generator().manual_seed(8765 + i)
        h, w = self.SIZES[i % len(self.SIZES)]
        img = torch.randint(0, 256, (h, w, 3), generator=g, dtype=torch.uint8).numpy()
        return {'labels': torch.zeros(2, dtype=torch.float64), 'labels_clf': torch.tensor(0), 'image': _jpeg_file(img, i) if self.encoded else img}


class _SyntheticEncodedImages(_SyntheticRawPanoramas):
    """N seeded single JPEG files of mixed sizes with an index: `embed --raw-images --encoded --synthetic N`."""

    def __getitem__(self, i):
        return {'image': super().__getitem__(i)['image'], 'index': i}


def _vision_model(args):
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    path = args.base if args.function == 'evaluate' else args.name
    if path in (None, 'random') or not os.path.exists(str(path)):
        if path not in (None, 'random'):
            raise FileNotFoundError(path)
        logger.warning('Using a seeded random-init ViT-L/14-336 (%d layers): weights of the reference are not public.', args.layers)
        return HipCLIPVisionModel(seed=0, layers=args.layers)
    sd = torch.load(path, map_location='cpu')
    sd = {('.'.join(k.split('.')[1:]) if 'base_model' in k.split('.')[0] else k): v for k, v in sd.items()}
    return HipCLIPVisionModel(sd)


def main():
    args = argp.parse_args()
    if args.exact_top1 is not None:
        os.environ['PIGEON_EXACT_TOP1'] = '1' if args.exact_top1 else '0'     # read by SuperGuessr / HipCLIPVisionModel at construction
    mode = 'classification' if args.classification else 'regression'
    logger.warning(f'Task: {args.function.capitalize()} Pigeon("{args.name}") via geospatial {mode}.')
    if args.function in ('pretrain', 'finetune'):
        raise NotImplementedError(f'Mode {args.function} is training and not part of the MI355X inference hot path.')

    from pigeon_amd import distributed
    comm = distributed.init_from_env()
    try:
        res = _dispatch(args, comm)
    except BaseException:
        comm.close(rccl=False)  # a failing rank abandons its RCCL communicator (the others may sit in a collective)
        raise
    comm.barrier()
    comm.close()               # every rank: RCCL communicator + control-plane group, before the interpreter unwinds
    return res


def _print_fallbacks(comm):
    from pigeon_amd import jpeg
    if comm.is_main_process and jpeg.fallback_summary():
        print(jpeg.fallback_summary())


def _dispatch(args, comm):
    if args.encoded and not args.raw_images:
        raise SystemExit('--encoded is a mode of --raw-images')
    if args.equirect and not (args.raw_images and args.function == 'evaluate'):
        raise SystemExit('--equirect is a mode of evaluate --raw-images')
    from pigeon_amd import synthetic
    dev = f'cuda:{int(os.environ.get("LOCAL_RANK", "0"))}'
    torch.cuda.set_device(dev)

    if args.function == 'embed':
        if args.resume:
            raise NotImplementedError('Resuming from checkpoint not supported.')
        from pigeon_amd.clip_embedder import CLIPEmbedding
        from pigeon_amd.embed import embed_images
        have_cal = bool(args.calibration) and os.path.exists(args.calibration)
        embedder = CLIPEmbedding(args.name, device=dev, panorama=(not args.yfcc), clip_model=_vision_model(args),
                                 calibration=args.calibration if have_cal else None)
        if have_cal and comm.is_main_process:
            print(f'Loaded calibration {args.calibration} (fingerprint {embedder.calibration_header["fingerprint"]})')
        if args.synthetic:
            dataset = {'train': _SyntheticEncodedImages(args.synthetic, encoded=True) if args.raw_images and args.encoded
                       else _SyntheticImages(args.synthetic, panorama=False)}
        else:
            from datasets import DatasetDict
            dataset = DatasetDict.load_from_disk(args.load[0])
        embed_images(embedder, dataset, comm, out_dir=args.out_dir, num_workers=0 if args.synthetic else 8,
                     raw_images=args.raw_images, exact=args.exact, encoded=args.encoded)
        _print_fallbacks(comm)
        if args.calibration and not have_cal and comm.is_main_process:
            if embedder.guard_stats is not None:
                embedder.save_calibration(args.calibration, source=f'run.py embed, first batch, {embedder.guard_stats["images"]} images')
                print(f'Calibration written to {args.calibration}')
            else:
                print(f'No calibration written to {args.calibration}: nothing was measured in this run')
        if comm.is_main_process:
            print(f'Embeddings written to {args.out_dir}/')
        return args.out_dir

    elif args.function == 'evaluate':
        from pigeon_amd.evaluate import evaluate
        import tempfile
        geocell_path = None
        bank = None
        if args.synthetic:
            tmp = tempfile.mkdtemp(prefix='pigeon_run_')
            geocell_path = os.path.join(tmp, 'geocells.csv')
            synthetic.write_geocell_csv(geocell_path, synthetic.make_geocells(args.geocells, seed=0))
            bank = synthetic.make_bank(args.geocells, 20, seed=2, exact_means=False)
            if args.equirect:
                dataset = _SyntheticEquirect(args.synthetic, args.encoded)
            else:
                dataset = _SyntheticRawPanoramas(args.synthetic, args.encoded) if args.raw_images else _SyntheticImages(args.synthetic, panorama=True)
        else:
            from datasets import DatasetDict
            dataset = DatasetDict.load_from_disk(args.load[0])
            if not args.yfcc:
                dataset = dataset['test'] if args.test else dataset['val']
        if args.raw_images:
            from pigeon_amd.evaluate import ImageEvalDataset
            dataset = ImageEvalDataset(dataset, encoded=args.encoded, equirect=args.equirect)
        results = evaluate(args.name, dataset, yfcc=args.yfcc, base_model=_vision_model(args), refine=True,
                           landmarks=args.landmarks, geocell_path=geocell_path, bank=bank, heading=args.heading,
                           multi_task=args.multitask, calibration=args.calibration, embedding_rel_tol=args.embedding_rel_tol,
                           country_path=args.countries, bank_rel_tol=args.bank_rel_tol, spread=(0.5, 0.9) if args.spread else None,
                           best_guess={'expected-score': 'score', 'expected-km': 'km'}.get(args.guess), neighbours=args.neighbours,
                           temperature=args.temperature, bootstrap=args.bootstrap, bootstrap_seed=args.bootstrap_seed,
                           bootstrap_level=args.bootstrap_level, refiner_settings=args.refiner)
        _print_fallbacks(comm)
        if comm.is_main_process:
            print({k: (v if not hasattr(v, 'shape') or v.shape == () else tuple(v.shape)) for k, v in results.items() if k not in ('exact_passes', 'bootstrap', 'bootstrap_level')})
            if 'Radius_50_coverage' in results:
                print(f"spread: the 50 % radius (median {results['Median_radius_50_km']:.1f} km) holds the truth for "
                      f"{results['Radius_50_coverage']:.1%} of the samples, the 90 % radius (median {results['Median_radius_90_km']:.1f} km) "
                      f"for {results['Radius_90_coverage']:.1%}; mean expected error {results['Mean_expected_km']:.1f} km, mean expected "
                      f"score {results['Mean_expected_score']:.0f}")
            if 'Geoguessr_score_best' in results:
                print(f"guess by {args.guess}: {results['Best_guess_changed']:.1%} of the guesses changed; mean error "
                      f"{results['Mean_km_error']:.1f} -> {results['Mean_km_error_best']:.1f} km, median {results['Median_km_error']:.1f} -> "
                      f"{results['Median_km_error_best']:.1f} km, GeoGuessr score {results['Geoguessr_score']:.0f} -> "
                      f"{results['Geoguessr_score_best']:.0f}")
            if 'Geoguessr_score_nn' in results:
                print(f"nearest training row as the guess: mean error {results['Mean_km_error_nn']:.1f} km, median "
                      f"{results['Median_km_error_nn']:.1f} km, GeoGuessr score {results['Geoguessr_score_nn']:.0f}; closer than the "
                      f"model's guess on {results['NN_beats_model']:.1%} of the items")
            if 'geocell_certain' in results:
                # beyond the reference's output: how many samples' discrete outputs are certain to be the fp32 reference's (a z ~ 4
                # statistical statement, pigeon_amd/certainty.py), and how many are near-ties of the reference itself
                cert = results['geocell_certain']
                print(f"certain: {int(cert.sum())}/{cert.size} samples; still uncertain after the exact tier (returned as computed): "
                      f"{results.get('uncertain_after_exact', 0)}; exact passes: {[f['slots_run'] for f in results.get('exact_passes', [])]} panoramas")
        return results


if __name__ == '__main__':
    main()
