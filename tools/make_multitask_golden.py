"""Writes tests/golden/multitask.npz: what the REAL reference's `SuperGuessr(None, multi_task=True)` computes, in eval mode on the CPU,
from seeded embeddings -- the fixture of tests/test_multitask_cpu.py and tests/test_gpu_multitask.py.

    python tools/make_multitask_golden.py [--out tests/golden/multitask.npz]

Authoring tool: needs the reference tree (oracle/reference_loader.py; `PIGEON_REFERENCE_ROOT`).  Nothing of the reference's program
text goes into the file -- only arrays its model read and wrote.

Two sets:
  a_*   panorama=True, yfcc=False: 48 samples (48, 4, 1024), all three auxiliary layers
  b_*   panorama=False, yfcc=True: 16 samples (16, 1024), no month layer
Per set: the four (three) layers' weights as the reference's constructor initialised them (torch.manual_seed), the geocell centroids
(C = 64), labels, every field of the reference's ModelOutput (`embedding` is the input itself and is not stored twice), the serving
tuple of a `serving=True` copy of the model, the state-dict keys, and the accuracies of the climate / month argmax against the labels.

The embeddings are NOT stored (they are most of a megabyte): they are rows of the seeded stream `stream(seed, n, P)` below --
numpy's frozen legacy generator, whose stream is guaranteed not to change -- and the file keeps the indices of the rows used.  A row of
the stream is used if its geocell, climate AND month margins (top-1 minus top-2 of the exact, float64 outputs) are at least 4 x the
largest rounding bound of the classifier's outputs on that row, bound = (1024 + P + 2) 2^-24 (|mean_p e| |W[a]| + |bias[a]|): then two fp32 evaluations that are each within 2 x bound of
the exact value have the same argmax, so the tests compare the argmax on every row without exclusions.  The first 48 / 16 such rows
are the samples.
"""
import argparse
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import reference_loader  # noqa: E402
from pigeon_amd import synthetic  # noqa: E402

C, N_STREAM = 64, 256
SETS = {'a': dict(panorama=True, yfcc=False, n=48, P=4, seed=4101), 'b': dict(panorama=False, yfcc=True, n=16, P=1, seed=4202)}


def stream(seed: int, n: int, P: int) -> np.ndarray:
    """(n, P, 1024) fp32: the first n rows of the seeded N(0,1) stream (numpy's legacy generator: a frozen stream)."""
    return np.random.RandomState(seed).standard_normal((n, P, 1024)).astype(np.float32)


def rounding_bound(mean_emb: np.ndarray, W: np.ndarray, bias: np.ndarray, P: int) -> np.ndarray:
    """(B, A) float64: (1024 + P + 2) 2^-24 (|e| |W[a]| + |bias[a]|) -- K products, P panel adds, one scale, one bias add, any order."""
    en = np.linalg.norm(mean_emb.astype(np.float64), axis=-1)
    wn = np.linalg.norm(W.astype(np.float64), axis=-1)
    return (1024 + P + 2) * 2.0 ** -24 * (en[:, None] * wn[None, :] + np.abs(bias.astype(np.float64))[None, :])


def top2_margin(x: np.ndarray) -> np.ndarray:
    s = np.sort(x.astype(np.float64), axis=-1)
    return s[:, -1] - s[:, -2]


def one_set(ns, tag: str, panorama: bool, yfcc: bool, n: int, P: int, seed: int) -> dict:
    torch.manual_seed(seed)
    model = ns.SuperGuessr(None, panorama=panorama, multi_task=True, yfcc=yfcc).eval()
    sd = model.state_dict()
    cand = stream(seed, N_STREAM, P)
    emb_all = torch.from_numpy(cand if panorama else cand[:, 0])
    rng = np.random.RandomState(seed + 1)

    def labels_for(m):
        clf = rng.randint(0, C, size=m)
        climate = rng.randint(0, 28, size=m)
        return dict(labels=torch.from_numpy(np.stack([rng.uniform(-180, 180, m), rng.uniform(-90, 90, m)], axis=1)),
                    labels_clf=torch.from_numpy(np.eye(C, dtype=np.float32)[clf]),
                    labels_multi_task=torch.from_numpy(rng.standard_normal((m, 6)).astype(np.float32)),
                    labels_climate=torch.from_numpy(np.eye(28, dtype=np.float32)[climate]),
                    labels_month=torch.from_numpy(rng.randint(0, 12, size=m).astype(np.int64)))

    mean = cand.mean(axis=1, dtype=np.float64).astype(np.float32) if panorama else cand[:, 0]
    ok = np.ones(N_STREAM, dtype=bool)
    classifiers = ('cell', 'climate') + (() if yfcc else ('month',))
    for name in classifiers:                              # margins of the EXACT (float64) outputs
        W, b = sd[f'{name}_layer.weight'].numpy(), sd[f'{name}_layer.bias'].numpy()
        bound = rounding_bound(mean, W, b, P).max(axis=-1)
        margin = top2_margin(mean.astype(np.float64) @ W.astype(np.float64).T + b.astype(np.float64))
        print(f'set {tag} {name}: {int((margin < 4 * bound).sum())} of {N_STREAM} stream rows below 4 x bound; median margin '
              f'{np.median(margin):.3g}, largest bound {bound.max():.3g}')
        ok &= margin >= 4 * bound
    keep = np.nonzero(ok)[0][:n]
    assert keep.size == n, f'set {tag}: only {keep.size} of {N_STREAM} stream rows have clear margins'
    emb = emb_all[keep].contiguous()
    lab = labels_for(n)
    if yfcc:
        lab['labels_month'] = None
    with torch.no_grad():
        out = model(embedding=emb, **lab)
        serving = ns.SuperGuessr(None, panorama=panorama, multi_task=True, yfcc=yfcc, serving=True).eval()
        serving.load_state_dict(sd)
        tup = serving(embedding=emb, labels_clf=lab['labels_clf'])
    assert len(tup) == 4 and torch.equal(tup[2], out.preds_mt) and torch.equal(tup[3], emb) and torch.equal(out.embedding, emb)
    # what the margins promise: the reference's own fp32 argmaxes are the exact ones on every kept row
    m64 = mean[keep].astype(np.float64)
    for name, got in (('cell', out.preds_geocell), ('climate', out.preds_climate.argmax(-1)),
                      ('month', None if yfcc else out.preds_month.argmax(-1))):
        if got is not None:
            W, b = sd[f'{name}_layer.weight'].numpy().astype(np.float64), sd[f'{name}_layer.bias'].numpy().astype(np.float64)
            assert np.array_equal(got.numpy(), (m64 @ W.T + b).argmax(-1)), (tag, name)
    d = {f'{tag}_stream_seed': np.int64(seed), f'{tag}_stream_rows': np.int64(N_STREAM), f'{tag}_stream_index': keep.astype(np.int64),
         f'{tag}_emb_checksum': np.float64(emb.double().sum().item()), f'{tag}_state_keys': np.array(sorted(sd.keys())),
         f'{tag}_panorama': np.bool_(panorama), f'{tag}_yfcc': np.bool_(yfcc)}
    for k, v in sd.items():
        d[f'{tag}_w_{k}'] = v.numpy()
    for k, v in lab.items():
        if v is not None:
            d[f'{tag}_{k}'] = v.numpy()
    for f in out._fields:
        v = getattr(out, f)
        if f == 'embedding' or v is None:
            continue
        if f == 'top5_geocells':
            d[f'{tag}_out_top5_values'], d[f'{tag}_out_top5_indices'] = v.values.numpy(), v.indices.numpy()
        else:
            d[f'{tag}_out_{f}'] = v.numpy() if torch.is_tensor(v) else np.asarray(v)
    d[f'{tag}_serving_len'] = np.int64(len(tup))
    d[f'{tag}_serving_0'], d[f'{tag}_serving_2'] = tup[0].numpy(), tup[2].numpy()
    d[f'{tag}_serving_1_values'], d[f'{tag}_serving_1_indices'] = tup[1].values.numpy(), tup[1].indices.numpy()
    d[f'{tag}_climate_accuracy'] = np.float64(np.mean(out.preds_climate.numpy().argmax(-1) == lab['labels_climate'].numpy().argmax(-1)))
    if out.preds_month is not None:
        d[f'{tag}_month_accuracy'] = np.float64(np.mean(out.preds_month.numpy().argmax(-1) == lab['labels_month'].numpy()))
    return d


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden', 'multitask.npz'))
    args = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix='pigeon_mt_')
    geocells = synthetic.make_geocells(C, seed=11)
    csv = os.path.join(tmp, 'geocells.csv')
    synthetic.write_geocell_csv(csv, geocells)
    ns = reference_loader.load(csv, os.path.join(tmp, 'none.csv'), os.path.join(tmp, 'none'), device='cpu')
    d = {'geocells': geocells}
    for tag, cfg in SETS.items():
        d.update(one_set(ns, tag, **cfg))
    np.savez_compressed(args.out, **d)
    size = os.path.getsize(args.out)
    print(f'{args.out}: {size} bytes, {len(d)} arrays')
    assert size < 1024 * 1024, 'fixture above the 1 MiB limit for committed files'


if __name__ == '__main__':
    main()
