"""Writes tests/golden/head_train.npz: six AdamW steps of the REFERENCE's SuperGuessr(None, panorama=True, should_smooth_labels=True)
on the CPU, in fp32 and after `.double()`, so that the GPU trajectory test has a yardstick that is not this project's own code: the
fp32 reference's deviation from its own fp64 run.  `python tests/make_head_train_golden.py` (needs the reference tree, which
oracle/reference_loader.py imports; none of its text is copied here).

Shapes: B = 8, C = 65, lr = 1e-3, one batch stepped six times.  The file holds the inputs (emb, W0, b0, centroids, labels,
labels_clf, tau, lr), the six losses of both runs and the final W, b of both.  The fp64 run's final W is stored as its difference from
the fp32 run's (`W64_minus_W32`, rounded to fp32: an error of 1e-15 on a difference of 1e-8), which keeps the file under 1 MiB."""
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "head_train.npz")
B, C, LR, STEPS = 8, 65, 1e-3, 6


def main():
    from oracle import reference_loader
    from pigeon_amd import synthetic
    tmp = tempfile.mkdtemp(prefix="pigeon_head_train_")
    cen = synthetic.make_geocells(C, seed=5)
    geo_csv = os.path.join(tmp, "geocells.csv")
    synthetic.write_geocell_csv(geo_csv, cen)
    ns = reference_loader.load(geo_csv, os.path.join(tmp, "none.csv"), os.path.join(tmp, "none"))
    W0, b0 = synthetic.make_head_weights(C, seed=9)
    g = torch.Generator().manual_seed(2024)
    emb = torch.randn((B, 4, 1024), generator=g) * 0.7 + 0.1
    rng = np.random.default_rng(11)
    cells = rng.integers(0, C, B)
    labels = torch.from_numpy(cen[cells] + rng.normal(0, 0.5, (B, 2)))
    labels_clf = torch.from_numpy(cells.astype(np.int64))
    runs = {}
    for name, dt in (("32", torch.float32), ("64", torch.float64)):
        model = ns.SuperGuessr(None, panorama=True, should_smooth_labels=True)
        with torch.no_grad():
            model.cell_layer.weight.copy_(W0)
            model.cell_layer.bias.copy_(b0)
        if dt == torch.float64:
            model.double()
        model.train()
        opt = torch.optim.AdamW(model.parameters(), lr=LR)
        losses = []
        for _ in range(STEPS):
            opt.zero_grad()
            out = model(embedding=emb.to(dt), labels=labels, labels_clf=labels_clf)
            out.loss.backward()
            opt.step()
            losses.append(float(out.loss))
        runs[name] = (np.array(losses, dtype=np.float64), model.cell_layer.weight.detach().numpy().copy(),
                      model.cell_layer.bias.detach().numpy().copy())
    l32, W32, b32 = runs["32"]
    l64, W64, b64 = runs["64"]
    assert W32.dtype == np.float32 and W64.dtype == np.float64
    tau = float(ns.config.LABEL_SMOOTHING_CONSTANT)
    np.savez_compressed(OUT, emb=emb.numpy(), W0=W0.numpy(), b0=b0.numpy(), centroids=cen, labels=labels.numpy(), labels_clf=cells.astype(np.int64),
                        tau=np.float64(tau), lr=np.float64(LR), losses32=l32, losses64=l64, W32=W32, b32=b32,
                        W64_minus_W32=(W64 - W32.astype(np.float64)).astype(np.float32), b64=b64)
    print("head_train: losses fp32", l32, "\n            losses fp64", l64)
    print(f"max|W32 - W64| = {np.abs(W32 - W64).max():.3e} ({np.abs(W32 - W64).max() / LR:.4f} lr), max|b32 - b64| = "
          f"{np.abs(b32 - b64).max():.3e}, max loss deviation {np.abs(l32 - l64).max():.3e}; {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
