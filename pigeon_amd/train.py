"""Training the geocell head on precomputed embeddings: the reference's `finetune_on_embeddings` (training/train_modes.py:110-133) and
`train_model` (training/train_eval_loop.py:164-253) for the one configuration in which every FLOP of a step is this project's own --
`SuperGuessr(base_model=None, ...)`, whose only trainable layer is `cell_layer = Linear(1024 -> C)`.

A step is two calls into libpigeon_hip.so (csrc/head_train.hip; contract: include/pigeon_hip.h): pg_head_train_loss (panel mean, the
logits inference computes, per-row loss and gradient in fp64) and pg_head_train_update (weight gradient with torch.optim.AdamW's
update as its epilogue).  There is no autograd graph, no gradient buffer and no host synchronisation inside a step.

  python -m pigeon_amd.train -l data/hf_SVCLIP_2203 -o saved_models/head.model            # embeddings written by `run.py embed`
  python -m pigeon_amd.train --synthetic 512 --geocells 257 --epochs 3 -o /tmp/head.model  # seeded, no data needed

Out of scope, each refused by name: gradients into the vision tower (`run.py finetune` / `pretrain` stay as they are), multi_task=True
(the three auxiliary losses), hierarchical=True, gradient accumulation above 1, more than one GPU.
"""
from __future__ import annotations

import argparse
import logging
import os
from typing import Any, Callable, Optional

import torch

from . import hip_ops
from .config import CURRENT_SAVE_PATH, LABEL_SMOOTHING_CONSTANT, TRAIN_ARGS, TrainArgs
from .super_guessr import SuperGuessr

logger = logging.getLogger('train')


class HeadTrainer:
    """AdamW on `model.cell_layer` from embeddings.  Owns the moments m, v and the step count t.

    `step(embedding, labels, labels_clf)`: embedding (B,4,1024) [panorama] or (B,1024); labels (B,2) [lng,lat] are used when the model
    has should_smooth_labels=True (haversine-smoothed targets, tau = config.LABEL_SMOOTHING_CONSTANT), labels_clf (B,) otherwise
    (one-hot targets).  Returns the mean of the per-row losses as a 0-d device tensor; the gradient is that mean's (grad_scale = 1/B).
    A row whose label is not finite (or whose labels_clf is no cell) does not train and makes the returned loss NaN.
    The kernels write the weights through raw pointers, so after every step the version counters of weight and bias are bumped:
    `SuperGuessr.wstats()` and the certainty caches key on them."""

    def __init__(self, model: SuperGuessr, lr: float = 2e-5, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.01,
                 tau: Optional[float] = None):
        if getattr(model, 'base_model', None) is not None:
            raise NotImplementedError('HeadTrainer: a model with a base model (gradients into the vision tower) is not implemented; '
                                      'train on precomputed embeddings with SuperGuessr(base_model=None, ...)')
        if getattr(model, 'multi_task', False):
            raise NotImplementedError('HeadTrainer: multi_task=True (the regression, climate and month losses) is not implemented')
        if getattr(model, 'hierarchical', False):
            raise NotImplementedError('HeadTrainer: hierarchical=True is not implemented')
        W, b = model.cell_layer.weight, model.cell_layer.bias
        if not W.is_cuda:
            raise RuntimeError('HeadTrainer runs on the GPU only: call model.to("cuda") first (no CPU fallback)')
        if W.dtype != torch.float32 or b.dtype != torch.float32 or not W.is_contiguous() or not b.is_contiguous():
            raise ValueError('HeadTrainer: cell_layer.weight and .bias must be contiguous float32 tensors')
        self.model = model
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.tau = float(LABEL_SMOOTHING_CONSTANT if tau is None else tau)
        self.t = 0
        self.m_W, self.v_W = torch.zeros_like(W.data), torch.zeros_like(W.data)
        self.m_b, self.v_b = torch.zeros_like(b.data), torch.zeros_like(b.data)
        self._out = {}                                   # the step's buffers, kept while the batch size stays the same

    def _buffers(self, B: int, dev) -> dict:
        C = self.model.num_cells
        o = self._out
        if o.get('g') is None or o['g'].shape[0] != B or o['g'].device != dev:
            o = self._out = {'xbar': torch.empty((B, hip_ops.HIDDEN), dtype=torch.float32, device=dev),
                             'g': torch.empty((B, C), dtype=torch.float32, device=dev),
                             'loss_rows': torch.empty((B,), dtype=torch.float64, device=dev)}
        return o

    @torch.no_grad()
    def step(self, embedding: torch.Tensor, labels: Optional[torch.Tensor] = None, labels_clf: Optional[torch.Tensor] = None) -> torch.Tensor:
        model = self.model
        W, b = model.cell_layer.weight, model.cell_layer.bias
        dev = W.device
        head_in = model._head_rows(embedding.to(dev, torch.float32))
        B = int(head_in.shape[0])
        llh = clf = None
        if model.should_smooth_labels and labels is not None:
            llh = labels.to(dev, torch.float64).reshape((B, 2)).contiguous()
        elif labels_clf is not None:
            clf = labels_clf.to(dev, torch.int64).reshape((B,)).contiguous()
        else:
            raise ValueError('HeadTrainer.step: labels (should_smooth_labels=True) or labels_clf are needed')
        if B == 0:
            return torch.full((), float('nan'), dtype=torch.float64, device=dev)
        out = hip_ops.head_train_loss(head_in, W.data, b.data, model.lla_geocells.data, llh, clf, tau=self.tau, grad_scale=1.0 / B,
                                      out=self._buffers(B, dev))
        self.t += 1
        hip_ops.head_train_update(out['g'], out['xbar'], W.data, b.data, self.m_W, self.v_W, self.m_b, self.v_b, self.t, lr=self.lr,
                                  beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, weight_decay=self.weight_decay)
        W[:0].zero_(); b[:0].zero_()                     # an in-place operation on an empty view: bumps ._version, moves no byte
        return out['loss_rows'].mean()

    def state_dict(self) -> dict:
        return {'t': self.t, 'lr': self.lr, 'betas': self.betas, 'eps': self.eps, 'weight_decay': self.weight_decay, 'tau': self.tau,
                'm_W': self.m_W.clone(), 'v_W': self.v_W.clone(), 'm_b': self.m_b.clone(), 'v_b': self.v_b.clone()}

    def load_state_dict(self, sd: dict) -> None:
        for k in ('m_W', 'v_W', 'm_b', 'v_b'):
            own = getattr(self, k)
            if tuple(sd[k].shape) != tuple(own.shape):
                raise ValueError(f'HeadTrainer.load_state_dict: {k} has shape {tuple(sd[k].shape)}, this head needs {tuple(own.shape)}')
        for k in ('m_W', 'v_W', 'm_b', 'v_b'):
            getattr(self, k).copy_(sd[k])
        self.t = int(sd['t'])
        self.lr, self.eps, self.weight_decay = float(sd['lr']), float(sd['eps']), float(sd['weight_decay'])
        self.betas, self.tau = (float(sd['betas'][0]), float(sd['betas'][1])), float(sd['tau'])


class ColumnDataset(torch.utils.data.Dataset):
    """Tensors of equal length under their column names: `ds[i]` is the dict of row i (what `model(**data)` takes after collation),
    `ds['labels']` a whole column as numpy (what `evaluate_model` reads), as a datasets.Dataset in torch format behaves."""

    def __init__(self, **columns):
        self.columns = columns
        self.n = len(next(iter(columns.values())))

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        if isinstance(i, str):
            return self.columns[i].numpy()
        return {k: v[i] for k, v in self.columns.items()}


def train_model(loaded_model: Any, dataset, on_embeddings: bool, yfcc: bool, train_args=TRAIN_ARGS, metrics: Optional[Callable] = None,
                patience: Optional[int] = None, should_profile: bool = False, save_path: Optional[str] = None,
                trainer: Optional[HeadTrainer] = None) -> SuperGuessr:
    """reference training/train_eval_loop.py:164-253 for `on_embeddings=True`: per epoch a shuffled pass over dataset['train'] (seeded:
    epoch e draws its permutation from torch.Generator().manual_seed(train_args.seed + e)), `evaluate_model` on dataset['val'], a save
    of `model.state_dict()` to `save_path` (default config.CURRENT_SAVE_PATH, as the reference) when -Geocell_accuracy improves, and
    early stopping after `patience` epochs without improvement.  `train_args` is any object with the fields of `config.TrainArgs`.
    Returns the model (its weights are the last epoch's; the best epoch's are in the file, as in the reference).
    `model.train_log` afterwards: per epoch {'epoch', 'train_loss', 'eval_loss', 'saved'}."""
    from torch.utils.data import DataLoader
    from .evaluate import compute_geoguessr_metrics, evaluate_model
    if not on_embeddings:
        raise NotImplementedError('train_model: on_embeddings=False (gradients into the vision tower) is not implemented; '
                                  '`run.py finetune` stays out of scope')
    acc = getattr(train_args, 'gradient_accumulation_steps', 1)
    if acc is not None and int(acc) > 1:
        raise NotImplementedError(f'train_model: gradient_accumulation_steps = {acc} (above 1) is not implemented')
    if int(os.environ.get('WORLD_SIZE', '1')) > 1:
        raise NotImplementedError('train_model: data-parallel training is not implemented; a step is well under a millisecond of GPU work')
    metrics = compute_geoguessr_metrics if metrics is None else metrics
    save_path = CURRENT_SAVE_PATH if save_path is None else save_path
    model = loaded_model
    if not model.cell_layer.weight.is_cuda:
        model.to('cuda')
    if trainer is None:
        trainer = HeadTrainer(model, lr=train_args.learning_rate)
    train, batch = dataset['train'], int(train_args.per_device_train_batch_size)
    seed = int(getattr(train_args, 'seed', 0))
    logging_steps = max(1, int(getattr(train_args, 'logging_steps', 1) or 1))
    prior_eval_loss, current_patience = None, 0
    model.train_log = []
    logger.warning('Starting training ...')
    model.train()
    for epoch in range(int(train_args.num_train_epochs)):
        order = torch.randperm(len(train), generator=torch.Generator().manual_seed(seed + epoch)).tolist()
        combined_loss, steps = None, 0
        for i, data in enumerate(DataLoader(train, batch, sampler=order, pin_memory=False, num_workers=0)):
            loss = trainer.step(data['embedding'], data.get('labels'), data.get('labels_clf'))
            combined_loss = loss if combined_loss is None else combined_loss + loss      # device tensors: no synchronisation per step
            steps += 1
            if i > 0 and i % logging_steps == 0 and logger.isEnabledFor(logging.DEBUG):
                logger.debug('Loss/train %d: %.6f', epoch * len(order) // batch + i, float(loss))
        results = evaluate_model(model, dataset['val'], metrics, train_args, None, yfcc)
        eval_loss = -float(results['Geocell_accuracy'])                                  # :161
        saved = prior_eval_loss is None or eval_loss < prior_eval_loss
        if saved:                                                                        # :237-242
            os.makedirs(os.path.dirname(os.path.abspath(save_path)), exist_ok=True)
            torch.save(model.state_dict(), save_path)
            prior_eval_loss, current_patience = eval_loss, 0
        else:
            current_patience += 1
        model.train_log.append({'epoch': epoch, 'train_loss': float(combined_loss) / max(steps, 1) if steps else float('nan'),
                                'eval_loss': eval_loss, 'saved': saved})
        logger.warning('epoch %d: train loss %.6f, geocell accuracy %.4f%s', epoch, model.train_log[-1]['train_loss'], -eval_loss,
                       f' -- saved to {save_path}' if saved else '')
        if patience is not None and current_patience == patience:                        # :248-250
            logger.warning(f'Early stopping after {patience} epochs ...')
            break
    return model


def finetune_on_embeddings(dataset, multi_task: bool, heading: bool, yfcc: bool, early_stopping: Optional[int] = None,
                           train_args=TRAIN_ARGS, geocell_path: Optional[str] = None, save_path: Optional[str] = None) -> SuperGuessr:
    """reference training/train_modes.py:110-133: a fresh `SuperGuessr(base_model=None, panorama=not yfcc, should_smooth_labels=True)`
    trained by `train_model`, initialised under torch.manual_seed(train_args.seed).  `geocell_path` / `save_path` override the paths
    the reference takes from its config."""
    if multi_task:
        raise NotImplementedError('finetune_on_embeddings: multi_task=True training (the regression, climate and month losses) is not implemented')
    torch.manual_seed(int(getattr(train_args, 'seed', 0)))           # nn.Linear's initialisation: a run is a function of its seed
    model = SuperGuessr(base_model=None, panorama=(yfcc == False), hierarchical=False, multi_task=False, heading=heading,   # noqa: E712
                        freeze_base=True, should_smooth_labels=True, yfcc=yfcc, geocell_path=geocell_path)
    model.to('cuda')
    print(model)
    return train_model(model, dataset, True, yfcc, train_args, None, early_stopping, save_path=save_path)


def synthetic_dataset(n: int, num_cells: int, seed: int = 0, panorama: bool = True, val_fraction: float = 0.25):
    """A seeded separable set: every geocell has a direction in embedding space, a sample is its cell's direction plus noise (per
    panel), labelled with a point next to the cell's centroid.  -> ({'train': ColumnDataset, 'val': ColumnDataset}, centroids (C,2))"""
    from . import synthetic
    cen = synthetic.make_geocells(num_cells, seed=seed)
    g = torch.Generator().manual_seed(seed + 4711)
    protos = torch.randn((num_cells, hip_ops.HIDDEN), generator=g)
    cells = torch.randint(0, num_cells, (n,), generator=g)
    shape = (n, 4, hip_ops.HIDDEN) if panorama else (n, hip_ops.HIDDEN)
    noise = torch.randn(shape, generator=g) * 0.5
    emb = (protos[cells][:, None, :] if panorama else protos[cells]) + noise
    jitter = (torch.rand((n, 2), generator=g, dtype=torch.float64) - 0.5) * 1e-3
    labels = torch.from_numpy(cen)[cells] + jitter
    n_val = max(1, int(n * val_fraction))
    split = {'train': slice(0, n - n_val), 'val': slice(n - n_val, n)}
    return {k: ColumnDataset(embedding=emb[s].contiguous(), labels=labels[s].contiguous(), labels_clf=cells[s].contiguous())
            for k, s in split.items()}, cen


def main(argv=None):
    argp = argparse.ArgumentParser(description='Train the geocell head on precomputed embeddings (one GPU).')
    argp.add_argument('-l', '--load', default=None, help='dataset directory (datasets.DatasetDict with train / val splits holding '
                                                          'embedding, labels, labels_clf)')
    argp.add_argument('--yfcc', action='store_true', default=False)
    argp.add_argument('-o', '--out', default='saved_models/head.model', help='where the best head is saved')
    argp.add_argument('--epochs', type=int, default=TRAIN_ARGS.num_train_epochs)
    argp.add_argument('--lr', type=float, default=TRAIN_ARGS.learning_rate)
    argp.add_argument('--batch', type=int, default=TRAIN_ARGS.per_device_train_batch_size)
    argp.add_argument('--patience', type=int, default=None)
    argp.add_argument('--seed', type=int, default=TRAIN_ARGS.seed)
    argp.add_argument('--synthetic', type=int, default=0, help='train on N seeded synthetic samples instead of a dataset')
    argp.add_argument('--geocells', type=int, default=10000, help='synthetic geocell count')
    argp.add_argument('--temperature', action='store_true', default=False,
                      help="after training, reload the saved best head, fit its temperature on dataset['val'] (pigeon_amd.temperature) "
                           "and write <out>.temperature.json")
    args = argp.parse_args(argv)
    logging.basicConfig(level=logging.INFO)
    train_args = TrainArgs(num_train_epochs=args.epochs, learning_rate=args.lr, per_device_train_batch_size=args.batch, seed=args.seed)
    geocell_path = None
    if args.synthetic:
        import tempfile
        from . import synthetic
        dataset, cen = synthetic_dataset(args.synthetic, args.geocells, seed=args.seed, panorama=not args.yfcc)
        geocell_path = os.path.join(tempfile.mkdtemp(prefix='pigeon_train_'), 'geocells.csv')
        synthetic.write_geocell_csv(geocell_path, cen)
    elif args.load:
        from datasets import DatasetDict
        dataset = DatasetDict.load_from_disk(args.load)
        dataset.set_format('torch')
    else:
        argp.error('one of -l DATASET and --synthetic N is needed')
    model = finetune_on_embeddings(dataset, multi_task=False, heading=False, yfcc=args.yfcc, early_stopping=args.patience,
                                   train_args=train_args, geocell_path=geocell_path, save_path=args.out)
    for row in model.train_log:
        print(row)
    print(f'Best head saved to {args.out}')
    if args.temperature:
        from . import temperature
        model.load_state(args.out)                                   # the best epoch's weights, not the last epoch's
        val = dataset['val']
        fit = temperature.fit_temperature(model, torch.as_tensor(val['embedding']), torch.as_tensor(val['labels_clf']))
        print(temperature.format_fit(fit))
        print(f"Temperature written to {temperature.save(args.out + '.temperature.json', fit, model)}")
    return model


if __name__ == '__main__':
    main()
