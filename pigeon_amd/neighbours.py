"""Which training panoramas look most like this one: exact k-nearest-neighbour search over the bank of training embeddings
(pg_knn_search, csrc/knn.hip).  The retrieval baseline (the nearest row's coordinates as the guess), the retrieval explanation and
the duplicate / contamination check (`--self`) all start here.

The search is exact FOR THE EMBEDDINGS IT IS GIVEN: the k rows of smallest fp32 squared distance, ties to the lower row.  The 16-bit
encoder's own error (about 1e-4 of the norm) is not modelled, and nothing is requeued into the exact encoder.

    python -m pigeon_amd.neighbours --bank DIR --queries emb.npy -k 10 -o nn.npz
    python -m pigeon_amd.neighbours --bank DIR --self -k 5 -o dup.npz
"""
from __future__ import annotations

import argparse
import sys
from typing import NamedTuple, Optional

import numpy as np
import torch

from . import hip_ops

HIDDEN = hip_ops.HIDDEN
K_MAX = 64


class Neighbours(NamedTuple):
    rows: torch.Tensor                    # (B,k) int64 bank rows, -1 past the bank's end
    d2: torch.Tensor                      # (B,k) fp32 squared distances, ascending
    distance: torch.Tensor                # (B,k) fp32 sqrt(d2): the refiner's L2
    lnglat: Optional[torch.Tensor]        # (B,k,2) fp32 [lng,lat] of the rows (NaN where rows == -1), None without coordinates
    certified: torch.Tensor               # (B,) bool: answered by the 16-bit pass and its certificate; False: by the exact tier


def check_k(k, who: str = "neighbours") -> int:
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= K_MAX:
        raise ValueError(f"{who}: k must be an integer in 1..{K_MAX}, got {k!r}")
    return int(k)


def _rows_1024(t: torch.Tensor, name: str, device) -> torch.Tensor:
    """(N,1024) or (N,P,1024) -> (N,1024) fp32 on `device`; panels are averaged as the refiner's bank averages them (the sum of the
    panels in order, times 1/P: pg_proto_build with one member a row)."""
    if not torch.is_tensor(t):
        t = torch.as_tensor(np.asarray(t))
    if t.dim() not in (2, 3) or t.shape[-1] != HIDDEN:
        raise ValueError(f"{name} must be (N,{HIDDEN}) or (N,panels,{HIDDEN}), got {tuple(t.shape)}")
    t = t.to(device=device, dtype=torch.float32).contiguous()
    if t.dim() == 3:
        ar = torch.arange(t.shape[0] + 1, device=t.device, dtype=torch.int64)
        t = hip_ops.proto_build(t, ar, ar[:-1].contiguous())
    return t


class EmbeddingIndex:
    """The bank of training embeddings as a search index.  `embeddings` (N,1024) or (N,4,1024); `lnglat` (N,2) [lng,lat] or None.
    A device fp32 tensor of the right shape is borrowed, not copied; the fp16 copy and the half norms the search needs cost another
    N * 2052 bytes of device memory."""

    def __init__(self, embeddings, lnglat=None, device="cuda"):
        dev = hip_ops.indexed_device(device)
        if dev.type != "cuda":
            raise RuntimeError("pigeon_amd.neighbours runs on the GPU only (no CPU fallback)")
        self.device = dev
        self.embeddings = _rows_1024(embeddings, "embeddings", dev)
        n = int(self.embeddings.shape[0])
        if lnglat is not None:
            lnglat = lnglat if torch.is_tensor(lnglat) else torch.as_tensor(np.asarray(lnglat))
            if lnglat.dim() != 2 or lnglat.shape[0] != n or lnglat.shape[1] < 2:
                raise ValueError(f"lnglat must be ({n},2), got {tuple(lnglat.shape)}")
            lnglat = lnglat[:, :2].to(device=dev, dtype=torch.float32).contiguous()
        self.lnglat = lnglat
        self.bank = hip_ops.knn_prepare(self.embeddings)
        self._queries = 0
        self._certified = torch.zeros((), dtype=torch.int64, device=dev)

    def __len__(self) -> int:
        return int(self.embeddings.shape[0])

    @classmethod
    def from_refiner(cls, refiner, device=None) -> "EmbeddingIndex":
        """The refiner's device bank: train_emb / train_lnglat are borrowed (no fp32 copy)."""
        dev = hip_ops.indexed_device(device if device is not None else getattr(refiner, "_device", "cuda"))
        t = refiner._device_bank(dev).t
        return cls(t["train_emb"], t["train_lnglat"], device=t["train_emb"].device)

    @classmethod
    def from_dataset(cls, path, device="cuda") -> "EmbeddingIndex":
        """A saved dataset's 'train' split (`embedding`, `labels`), a packed bank (.npz with train_emb / train_lnglat) or bare
        embeddings (.npy)."""
        p = str(path)
        if p.endswith(".npy"):
            return cls(np.load(p), None, device=device)
        if p.endswith(".npz"):
            with np.load(p) as z:
                if "train_emb" not in z:
                    raise ValueError(f"{p}: no train_emb array")
                return cls(z["train_emb"], z["train_lnglat"] if "train_lnglat" in z else None, device=device)
        from .proto_refiner import _training_arrays
        emb, lab = _training_arrays(path)
        return cls(emb, lab, device=device)

    def search(self, q, k: int = 10, exclude=None, exact: bool = False) -> Neighbours:
        """q (B,1024) or (B,4,1024).  `exclude` (B,) bank rows that the queries must not return (leave-one-out), -1 for none.
        exact=True takes the exact tier alone: the same answer bit for bit, slower.  No host synchronisation."""
        k = check_k(k, "search")
        q = _rows_1024(q, "q", self.device)
        if exclude is not None:
            exclude = (exclude if torch.is_tensor(exclude) else torch.as_tensor(np.asarray(exclude))).to(self.device, torch.int64).contiguous()
        rows, d2, cert = hip_ops.knn_search(self.bank, q, k, exclude=exclude, mode="exact" if exact else "auto")
        lnglat = None
        if self.lnglat is not None:
            if len(self):
                lnglat = self.lnglat[rows.clamp(min=0)]
                lnglat = torch.where((rows >= 0).unsqueeze(-1), lnglat, torch.full_like(lnglat, float("nan")))
            else:
                lnglat = torch.full((*rows.shape, 2), float("nan"), dtype=torch.float32, device=self.device)
        certified = cert.bool()
        if not exact:
            self._queries += int(q.shape[0])
            self._certified += certified.sum()
        return Neighbours(rows, d2, d2.sqrt(), lnglat, certified)

    @property
    def stats(self) -> dict:
        """Queries searched with exact=False, how many the certificate settled, how many went to the exact tier (reads a device
        counter: one host synchronisation)."""
        c = int(self._certified.item())
        return {"queries": self._queries, "certified": c, "fallback": self._queries - c}


def index_of(refiner, k, who: str = "neighbours") -> EmbeddingIndex:
    """The search index over `refiner`'s bank, built once and kept on the refiner; `k` is checked.  ValueError without a refiner
    that has a bank of training embeddings."""
    check_k(k, who)
    if refiner is None or not hasattr(refiner, "_device_bank"):
        raise ValueError(f"{who} searches the refiner's bank of training embeddings: it needs a refiner with a bank")
    index = getattr(refiner, "_neighbour_index", None)
    if index is None:
        index = EmbeddingIndex.from_refiner(refiner)
        refiner._neighbour_index = index
    return index


# ---------------------------------------------------------------------------------------------------------------------- command line
def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(prog="python -m pigeon_amd.neighbours", description="exact k-nearest training embeddings")
    ap.add_argument("--bank", required=True, help="a saved dataset (its 'train' split), a packed bank .npz or embeddings .npy")
    ap.add_argument("--queries", help="embeddings .npy, (B,1024) or (B,4,1024)")
    ap.add_argument("--self", dest="self_search", action="store_true",
                    help="search the bank against itself, leave-one-out, and report rows with a neighbour at distance 0")
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("-o", "--output", required=True, help="the .npz to write: rows, d2, distance, certified[, lnglat]")
    ap.add_argument("--exact", action="store_true", help="the exact tier only")
    ap.add_argument("--batch", type=int, default=4096, help="queries per search call")
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    if a.self_search == (a.queries is not None):
        ap.error("give exactly one of --queries and --self")
    if not 1 <= a.k <= K_MAX:
        ap.error(f"-k must be in 1..{K_MAX}, got {a.k}")
    if a.batch < 1:
        ap.error(f"--batch must be at least 1, got {a.batch}")
    return a


def main(argv=None) -> int:
    a = parse_args(argv)
    index = EmbeddingIndex.from_dataset(a.bank, device=a.device)
    if index.bank.bad_values:
        print(f"{index.bank.bad_values} bank values are not finite or exceed fp16's range: the exact tier answers every query")
    queries = index.embeddings if a.self_search else torch.as_tensor(np.load(a.queries))
    parts = []
    for s in range(0, int(queries.shape[0]), a.batch):
        e = min(int(queries.shape[0]), s + a.batch)
        ex = torch.arange(s, e, device=index.device, dtype=torch.int64) if a.self_search else None
        parts.append(index.search(queries[s:e], k=a.k, exclude=ex, exact=a.exact))
    if parts:
        cat = lambda f: torch.cat([getattr(p, f) for p in parts]).cpu().numpy()
        out = {f: cat(f) for f in ("rows", "d2", "distance", "certified")}
        if index.lnglat is not None:
            out["lnglat"] = cat("lnglat")
    else:
        out = {"rows": np.zeros((0, a.k), np.int64), "d2": np.zeros((0, a.k), np.float32), "distance": np.zeros((0, a.k), np.float32),
               "certified": np.zeros((0,), bool)}
    np.savez(a.output, **out)
    st = index.stats
    print(f"{out['rows'].shape[0]} queries x {a.k} neighbours over {len(index)} rows -> {a.output}; "
          f"certified {st['certified']}, exact tier {st['fallback']}")
    if a.self_search:
        dup = int((out["d2"][:, 0] == 0).sum()) if out["rows"].shape[0] else 0
        print(f"{dup} rows have a neighbour at distance 0")
    return 0


if __name__ == "__main__":
    sys.exit(main())
