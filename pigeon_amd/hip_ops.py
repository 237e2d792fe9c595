"""Torch-tensor front end of the C ABI: tensors are only containers (device memory + current stream);
every FLOP of the hot path happens inside libpigeon_hip.so."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional

import torch

from . import _lib
from ._lib import Bank, VitCfg, check, load

TOKENS, HIDDEN, MLP, PATCHES, KPAD = 577, 1024, 4096, 576, 640


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_T16 = {torch.float16: _lib.PG_DTYPE_F16, torch.bfloat16: _lib.PG_DTYPE_BF16}
_PIXDT = {torch.float32: _lib.PG_DTYPE_F32, torch.float16: _lib.PG_DTYPE_F16, torch.bfloat16: _lib.PG_DTYPE_BF16}
# what the encoder and the im2col read, what the resize writes: the float formats plus the 8-bit pixel (the byte in front of the
# normalisation table, PG_DTYPE_U8)
_PIXIN = {**_PIXDT, torch.uint8: _lib.PG_DTYPE_U8}
_PREP_OUT = {torch.float32: _lib.PG_DTYPE_F32, torch.float16: _lib.PG_DTYPE_F16, torch.uint8: _lib.PG_DTYPE_U8}
_PG2T = {_lib.PG_DTYPE_F16: torch.float16, _lib.PG_DTYPE_BF16: torch.bfloat16, _lib.PG_DTYPE_F32: torch.float32}


def _dt16(t: torch.Tensor) -> int:
    if t.dtype not in _T16:
        raise _lib.PigeonHipError(f"expected a float16 or bfloat16 tensor, got {t.dtype}")
    return _T16[t.dtype]


def _dev(t: torch.Tensor, dtype=None) -> torch.Tensor:
    if not t.is_cuda:
        raise _lib.PigeonHipError("expected a device tensor")
    if dtype is not None and t.dtype != dtype:
        raise _lib.PigeonHipError(f"expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.PigeonHipError("expected a contiguous tensor")
    return t


def indexed_device(device) -> torch.device:
    """`device` ("cuda", "cuda:1", a torch.device) as a torch.device with its index filled in."""
    dev = torch.device(device)
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def _shape(t: torch.Tensor, name: str, *dims):
    """The C ABI takes pointers plus a few sizes; every other extent is implied.  Refuse a tensor whose shape is not the implied
    one (None = any extent) instead of letting a kernel read past its end."""
    if t.dim() != len(dims) or any(d is not None and int(s) != int(d) for s, d in zip(t.shape, dims)):
        want = "(" + ",".join("*" if d is None else str(int(d)) for d in dims) + ")"
        raise _lib.PigeonHipError(f"{name} must have shape {want}, got {tuple(t.shape)}")
    return t


# ----------------------------------------------------------------------------------------- building blocks
def gemm16(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], out: torch.Tensor, epi: int,
           qscale: float = 1.0, qcols: int = 0, aux: Optional[torch.Tensor] = None, variant: int = 0,
           M: Optional[int] = None):
    """out (epilogue-dependent) <- A[M,K] x W[N,K]^T, both fp16 or both bf16; see pg_op_gemm16."""
    for t in (A, W, out):                                  # row-strided views are fine (padded leading dimensions)
        if not t.is_cuda or t.stride(1) != 1:
            raise _lib.PigeonHipError("gemm16 expects device tensors with unit inner stride")
    if W.dtype != A.dtype:
        raise _lib.PigeonHipError("gemm16: A and W must have the same 16-bit dtype")
    M = A.shape[0] if M is None else M
    K = A.shape[1]
    N = W.shape[0]
    dst = out
    if epi == _lib.EPI_RESID:
        # the residual epilogue's last row tile reads up to 383 rows past row M of `out` (see gemm16_resid_stat / pigeon_hip.h)
        have = out.untyped_storage().nbytes() - out.storage_offset() * out.element_size()
        if have < (M + 384) * out.stride(0) * out.element_size():
            dst = torch.zeros((max(M, out.shape[0]) + 384, out.shape[1]), dtype=out.dtype, device=out.device)[:out.shape[0]]
            dst.copy_(out)
    check(load().pg_op_gemm16_ld(_dt16(A), _p(A), A.stride(0), _p(W), W.stride(0), _p(bias), _p(dst), dst.stride(0), M, N, K,
                                 epi, float(qscale), int(qcols), _p(aux), variant, _stream()), "pg_op_gemm16_ld")
    if dst is not out:
        out.copy_(dst)
    return out


def tune_gemm_tail_rows(rows: int) -> None:
    """pg_tune_gemm_tail_rows: most rows pg_gemm_launch hands to the small-tile tail kernel (0 = never split).  Timing only."""
    check(load().pg_tune_gemm_tail_rows(int(rows)), "pg_tune_gemm_tail_rows")


def tune_gemm_tail_shape(min_k: int, min_n: int) -> None:
    """pg_tune_gemm_tail_shape: the tail split is used for GEMMs with K >= min_k or N >= min_n ((0, 0) = all).  Timing only."""
    check(load().pg_tune_gemm_tail_shape(int(min_k), int(min_n)), "pg_tune_gemm_tail_shape")


def rowstat_cast(x: torch.Tensor, out_dtype: torch.dtype = torch.float16, eps: float = 1e-5):
    """x fp32 (rows,1024) -> (16-bit copy, rowstat (rows,2) = (rstd, mean*rstd))."""
    _dev(x, torch.float32)
    rows = x.numel() // HIDDEN
    x16 = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    rs = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    check(load().pg_op_rowstat_cast(_p(x), _p(x16), _dt16(x16), _p(rs), rows, float(eps), _stream()), "pg_op_rowstat_cast")
    return x16, rs


def gemm16_resid_stat(A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, X: torch.Tensor, variant: int = 0):
    """X += A.W^T + bias in place; returns (x16 copy of the new X, statpart (N/64, M, 2)).

    The persistent kernels fetch the residual rows of a whole 256- / 384-row tile through a buffer descriptor whose row term rides in
    the SGPR offset, which the hardware bounds check does not cover: in the last (partial) tile they READ up to 383 rows past row M of
    X (never write there; the values are discarded).  Inside the encoder those rows are the workspace's next buffer.  Here X must own
    that slack -- if its storage ends earlier the GEMM runs on a padded copy (this wrapper serves tests and tools, not the hot path)."""
    M, K = A.shape
    N = W.shape[0]
    x16 = torch.empty((M, N), dtype=A.dtype, device=A.device)
    part = torch.empty((N // 64, M, 2), dtype=torch.float32, device=A.device)
    have = X.untyped_storage().nbytes() - X.storage_offset() * X.element_size()
    Xr = X
    if have < (M + 384) * X.stride(0) * X.element_size():
        Xr = torch.zeros((M + 384, N), dtype=X.dtype, device=X.device)[:M]
        Xr.copy_(X)
    check(load().pg_op_gemm16_resid_stat(_dt16(A), _p(A), A.stride(0), _p(W), W.stride(0), _p(bias), _p(Xr), Xr.stride(0), _p(x16),
                                         x16.stride(0), _p(part), M, N, K, variant, _stream()), "pg_op_gemm16_resid_stat")
    if Xr is not X:
        X.copy_(Xr)
    return x16, part


def rowstat_finalize(part: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    slots, rows = part.shape[0], part.shape[1]
    rs = torch.empty((rows, 2), dtype=torch.float32, device=part.device)
    check(load().pg_op_rowstat_finalize(_p(part), slots, _p(rs), rows, float(eps), _stream()), "pg_op_rowstat_finalize")
    return rs


def gemm16_ln(A: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, colsum: torch.Tensor, rowstat: torch.Tensor, epi: int,
              qscale: float = 1.0, qcols: int = 0, variant: int = 0) -> torch.Tensor:
    M, K = A.shape
    N = W.shape[0]
    out = torch.empty((M, N), dtype=A.dtype, device=A.device)
    check(load().pg_op_gemm16_ln(_dt16(A), _p(A), A.stride(0), _p(W), W.stride(0), _p(bias), _p(colsum), _p(rowstat), _p(out),
                                 out.stride(0), M, N, K, epi, float(qscale), int(qcols), variant, _stream()), "pg_op_gemm16_ln")
    return out


def layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5,
              out_dtype: torch.dtype = torch.float16, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _dev(x, torch.float32)
    rows = x.numel() // HIDDEN
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    pg = _lib.PG_DTYPE_F32 if out.dtype == torch.float32 else _dt16(out)
    check(load().pg_op_layernorm(_p(x), _p(gamma), _p(beta), _p(out), pg, rows, float(eps), _stream()), "pg_op_layernorm")
    return out


def attention(qkv: torch.Tensor, n_images: int) -> torch.Tensor:
    _dev(qkv)
    out = torch.empty((n_images * TOKENS, HIDDEN), dtype=qkv.dtype, device=qkv.device)
    check(load().pg_op_attention(_dt16(qkv), _p(qkv), _p(out), n_images, _stream()), "pg_op_attention")
    return out


def im2col(pixels: torch.Tensor, out_dtype: torch.dtype = torch.float16) -> torch.Tensor:
    _dev(pixels)
    _shape(pixels, "pixels", None, 3, 336, 336)
    n = pixels.shape[0]
    dt = _PIXIN[pixels.dtype]
    out = torch.empty((n * PATCHES, KPAD), dtype=out_dtype, device=pixels.device)
    check(load().pg_op_im2col(_p(pixels), dt, _p(out), _dt16(out), n, _stream()), "pg_op_im2col")
    return out


def token_mean(x: torch.Tensor) -> torch.Tensor:
    _dev(x, torch.float32)
    n = x.shape[0]
    out = torch.empty((n, HIDDEN), dtype=torch.float32, device=x.device)
    check(load().pg_op_token_mean(_p(x), _p(out), n, _stream()), "pg_op_token_mean")
    return out


def cast_f32(x: torch.Tensor, out_dtype: torch.dtype = torch.float16) -> torch.Tensor:
    _dev(x, torch.float32)
    y = torch.empty(x.shape, dtype=out_dtype, device=x.device)
    check(load().pg_op_cast_f32(_p(x), _p(y), _dt16(y), x.numel(), _stream()), "pg_op_cast_f32")
    return y


# ----------------------------------------------------------------------------------------- around the hot path
def proto_build(train_emb: torch.Tensor, member_off: torch.Tensor, member_idx: torch.Tensor) -> torch.Tensor:
    """(Ntr,1024) or (Ntr,4,1024) fp32 training embeddings + CSR member lists -> (P,1024) fp32 prototype means."""
    _dev(train_emb, torch.float32); _dev(member_off, torch.int64); _dev(member_idx, torch.int64)
    if train_emb.dim() not in (2, 3) or train_emb.shape[-1] != HIDDEN:
        raise _lib.PigeonHipError(f"proto_build: embeddings must be (Ntr,{HIDDEN}) or (Ntr,panels,{HIDDEN}), got {tuple(train_emb.shape)}")
    panels = 1 if train_emb.dim() == 2 else int(train_emb.shape[1])
    if member_off.dim() != 1 or member_off.numel() < 1 or member_idx.dim() != 1:
        raise _lib.PigeonHipError("proto_build: member_off (P+1,) and member_idx (n,) expected")
    P = member_off.numel() - 1
    # one-off bank construction: a host round trip for the CSR invariants is cheap, a member index past the training bank is a
    # read out of bounds in the kernel
    off = member_off.cpu()
    if int(off[0]) != 0 or int(off[-1]) != member_idx.numel() or bool((off[1:] < off[:-1]).any()):
        raise _lib.PigeonHipError("proto_build: member_off must rise from 0 to len(member_idx)")
    if member_idx.numel() and (int(member_idx.min()) < 0 or int(member_idx.max()) >= train_emb.shape[0]):
        raise _lib.PigeonHipError(f"proto_build: member index outside the {train_emb.shape[0]} training rows")
    out = torch.empty((P, HIDDEN), dtype=torch.float32, device=train_emb.device)
    check(load().pg_proto_build(_p(train_emb), panels, train_emb.shape[0], _p(member_off), _p(member_idx), P, _p(out),
                                _stream()), "pg_proto_build")
    return out


def haversine_matrix(x: torch.Tensor, y_rows: torch.Tensor) -> torch.Tensor:
    """x (N,2) fp32/fp64 [lng,lat], y_rows (M,2) fp64 -> (N,M) fp64 km."""
    _dev(x); _dev(y_rows, torch.float64)
    if x.dtype not in (torch.float32, torch.float64):
        raise _lib.PigeonHipError("haversine_matrix: x must be fp32 or fp64")
    _shape(x, "x", None, 2); _shape(y_rows, "y_rows", None, 2)
    N, M = x.shape[0], y_rows.shape[0]
    out = torch.empty((N, M), dtype=torch.float64, device=x.device)
    check(load().pg_haversine_matrix(_p(x), _lib.PG_DTYPE_F64 if x.dtype == torch.float64 else _lib.PG_DTYPE_F32, _p(y_rows),
                                     N, M, _p(out), _stream()), "pg_haversine_matrix")
    return out


def haversine_pairs(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """x (N,2) fp64, y (N,2) fp32/fp64 [lng,lat] degrees -> (N,) fp64 km (row-paired)."""
    _dev(x, torch.float64); _dev(y)
    if y.dtype not in (torch.float32, torch.float64) or x.shape != y.shape or x.dim() != 2 or x.shape[1] != 2:
        raise _lib.PigeonHipError("haversine_pairs: x (N,2) fp64 and y (N,2) fp32/fp64 expected")
    out = torch.empty((x.shape[0],), dtype=torch.float64, device=x.device)
    check(load().pg_haversine_pairs(_p(x), _p(y), _lib.PG_DTYPE_F64 if y.dtype == torch.float64 else _lib.PG_DTYPE_F32,
                                    x.shape[0], _p(out), _stream()), "pg_haversine_pairs")
    return out


def smooth_labels(distances: torch.Tensor, constant: float) -> torch.Tensor:
    _dev(distances, torch.float64)
    _shape(distances, "distances", None, None)
    N, M = distances.shape
    out = torch.empty_like(distances)
    check(load().pg_smooth_labels(_p(distances), N, M, float(constant), _p(out), _stream()), "pg_smooth_labels")
    return out


# ----------------------------------------------------------------------------------------- guess spread
def guess_spread(logits: torch.Tensor, centroids: torch.Tensor, points: torch.Tensor, quantiles=(0.5, 0.9),
                 extent_km: Optional[torch.Tensor] = None, out: Optional[Dict[str, torch.Tensor]] = None):
    """pg_guess_spread: logits (B,C) fp32, centroids (C,2) fp64 [lng,lat], points (B,2) or (B,G,2) fp64, extent_km (C,) fp64 or None,
    quantiles 1 .. 4 numbers in (0, 1] -> (expected_km, expected_score, radius_km), fp64, of shape (B,), (B,), (B,nq) for (B,2) points
    and (B,G), (B,G), (B,G,nq) for (B,G,2) points.  The contract is include/pigeon_hip.h's.  `out` (keys expected_km, expected_score,
    radius_km) supplies the output tensors; no host synchronisation."""
    _dev(logits, torch.float32); _shape(logits, "logits", None, None)
    B, Cn = int(logits.shape[0]), int(logits.shape[1])
    _dev(centroids, torch.float64); _shape(centroids, "centroids", Cn, 2)
    _dev(points, torch.float64)
    flat = points.dim() == 2
    if flat:
        _shape(points, "points", B, 2)
    else:
        _shape(points, "points", B, None, 2)
    G = 1 if flat else int(points.shape[1])
    if extent_km is not None:
        _dev(extent_km, torch.float64); _shape(extent_km, "extent_km", Cn)
    for name, t in (("centroids", centroids), ("points", points), ("extent_km", extent_km)):
        if t is not None and t.device != logits.device:
            raise _lib.PigeonHipError(f"guess_spread: {name} is on {t.device}, logits on {logits.device}")
    qs = [float(q) for q in quantiles]
    if not 1 <= len(qs) <= 4:
        raise _lib.PigeonHipError(f"guess_spread: quantiles must hold 1 .. 4 numbers, got {len(qs)}")
    nq = len(qs)
    shapes = {"expected_km": (B,) if flat else (B, G), "expected_score": (B,) if flat else (B, G),
              "radius_km": (B, nq) if flat else (B, G, nq)}
    if out is None:
        out = {k: torch.empty(s, dtype=torch.float64, device=logits.device) for k, s in shapes.items()}
    for k, s in shapes.items():
        _dev(out[k], torch.float64); _shape(out[k], k, *s)
        if out[k].device != logits.device:
            raise _lib.PigeonHipError(f"guess_spread: {k} is on {out[k].device}, logits on {logits.device}")
    qarr = (C.c_double * nq)(*qs)
    with torch.cuda.device(logits.device):
        check(load().pg_guess_spread(_p(logits), B, Cn, _p(centroids), _p(extent_km), _p(points), G, qarr, nq, _p(out["expected_km"]),
                                     _p(out["expected_score"]), _p(out["radius_km"]), _stream()), "pg_guess_spread")
    return out["expected_km"], out["expected_score"], out["radius_km"]


def guess_spread_plan(C_cells: int) -> dict:
    """pg_guess_spread_plan: where pg_guess_spread keeps the (key, weight) pairs of C cells (host arithmetic, no GPU)."""
    o = (C.c_int32 * 4)()
    check(load().pg_guess_spread_plan(int(C_cells), o), "pg_guess_spread_plan")
    return {"form": int(o[0]), "lds_bytes": int(o[1]), "lds_cells": int(o[2]), "threads": int(o[3])}


# ----------------------------------------------------------------------------------------- guess by expected score
_TABLE_KINDS = {"km": 0, "score": 1}


def score_table(candidates: torch.Tensor, centroids: torch.Tensor, kind: str = "score") -> torch.Tensor:
    """pg_score_table: candidates (M,2) fp64 [lng,lat], centroids (C,2) fp64 -> table (M,C) fp64, candidate-major: the km of
    pg_haversine_matrix (kind='km') or 5000 exp(-km / 1492.7) (kind='score').  No host synchronisation."""
    if kind not in _TABLE_KINDS:
        raise _lib.PigeonHipError(f"score_table: kind must be 'score' or 'km', got {kind!r}")
    _dev(candidates, torch.float64); _shape(candidates, "candidates", None, 2)
    _dev(centroids, torch.float64); _shape(centroids, "centroids", None, 2)
    if centroids.device != candidates.device:
        raise _lib.PigeonHipError(f"score_table: centroids is on {centroids.device}, candidates on {candidates.device}")
    M, Cn = int(candidates.shape[0]), int(centroids.shape[0])
    table = torch.empty((M, Cn), dtype=torch.float64, device=candidates.device)
    with torch.cuda.device(candidates.device):
        check(load().pg_score_table(_p(candidates), M, _p(centroids), Cn, _TABLE_KINDS[kind], _p(table), _stream()), "pg_score_table")
    return table


def guess_best(logits: torch.Tensor, table: torch.Tensor, maximize: bool = True, return_expected: bool = False):
    """pg_guess_best: logits (B,C) fp32, table (M,C) fp64 -> (best_idx int64 (B,), best_value fp64 (B,)[, expected fp64 (B,M)]): per
    row the candidate whose expectation under the row's softmax is largest (maximize) or smallest, the first among equals, -1 / NaN
    for a row the contract answers with NaN.  The contract is include/pigeon_hip.h's.  No host synchronisation."""
    _dev(logits, torch.float32); _shape(logits, "logits", None, None)
    B, Cn = int(logits.shape[0]), int(logits.shape[1])
    _dev(table, torch.float64); _shape(table, "table", None, Cn)
    if table.device != logits.device:
        raise _lib.PigeonHipError(f"guess_best: table is on {table.device}, logits on {logits.device}")
    M = int(table.shape[0])
    idx = torch.empty((B,), dtype=torch.int32, device=logits.device)
    val = torch.empty((B,), dtype=torch.float64, device=logits.device)
    exp = torch.empty((B, M), dtype=torch.float64, device=logits.device) if return_expected else None
    with torch.cuda.device(logits.device):
        check(load().pg_guess_best(_p(logits), B, Cn, _p(table), M, 1 if maximize else 0, _p(idx), _p(val), _p(exp), _stream()),
              "pg_guess_best")
    if M == 0:                                             # a no-op in the library: nothing to choose from
        idx.fill_(-1); val.fill_(float("nan"))
    idx = idx.to(torch.int64)
    return (idx, val, exp) if return_expected else (idx, val)


def guess_best_plan(B: int, C_cells: int, M: int) -> dict:
    """pg_guess_best_plan: what pg_guess_best does with B rows, C cells and M candidates (host arithmetic, no GPU)."""
    o = (C.c_int32 * 8)()
    check(load().pg_guess_best_plan(int(B), int(C_cells), int(M), o), "pg_guess_best_plan")
    return {"form": int(o[0]), "rows_per_tile": int(o[1]), "candidates_per_tile": int(o[2]), "cells_per_step": int(o[3]),
            "workgroups": int(o[4]), "scratch_bytes": int(o[5]), "threads": int(o[6]), "candidate_tiles": int(o[7])}


# ----------------------------------------------------------------------------------------- calibrated head probabilities
def temper_stats(logits: torch.Tensor, labels: torch.Tensor, betas, row_stats: bool = False, conf: bool = False, state: bool = False,
                 out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, torch.Tensor]:
    """pg_temper_stats: logits (N,C) fp32, labels (N,) int64, betas 1 .. 16 finite positive numbers (host) -> dict(totals (K,3) fp64,
    counts (2,) int64) plus, where asked for, row_stats (N,K,3) fp64, conf (N,K) fp64 and state (N,) uint8.  The contract is
    include/pigeon_hip.h's.  `out` supplies output tensors by those names (a name in `out` is asked for).  No host synchronisation."""
    _dev(logits, torch.float32); _shape(logits, "logits", None, None)
    N, Cn = int(logits.shape[0]), int(logits.shape[1])
    _dev(labels, torch.int64); _shape(labels, "labels", N)
    if labels.device != logits.device:
        raise _lib.PigeonHipError(f"temper_stats: labels is on {labels.device}, logits on {logits.device}")
    bs = [float(b) for b in betas]
    K = len(bs)
    if not 1 <= K <= 16:
        raise _lib.PigeonHipError(f"temper_stats: betas must hold 1 .. 16 numbers, got {K}")
    out = dict(out) if out is not None else {}
    shapes = {"totals": ((K, 3), torch.float64), "counts": ((2,), torch.int64)}
    for name, want, shape, dt in (("row_stats", row_stats, (N, K, 3), torch.float64), ("conf", conf, (N, K), torch.float64),
                                  ("state", state, (N,), torch.uint8)):
        if want or name in out:
            shapes[name] = (shape, dt)
    for name, (shape, dt) in shapes.items():
        if name not in out:
            out[name] = torch.empty(shape, dtype=dt, device=logits.device)
        _dev(out[name], dt); _shape(out[name], name, *shape)
        if out[name].device != logits.device:
            raise _lib.PigeonHipError(f"temper_stats: {name} is on {out[name].device}, logits on {logits.device}")
    barr = (C.c_double * K)(*bs)
    with torch.cuda.device(logits.device):
        check(load().pg_temper_stats(_p(logits), N, Cn, _p(labels), barr, K, _p(out.get("row_stats")), _p(out.get("conf")),
                                     _p(out.get("state")), _p(out["totals"]), _p(out["counts"]), _stream()), "pg_temper_stats")
    return {k: out[k] for k in shapes}


def temper_logits(logits: torch.Tensor, beta: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pg_temper_logits: logits (N,C) fp32 -> logits * float32(beta), one rounded multiplication an element; `out` may be `logits`.
    No host synchronisation."""
    _dev(logits, torch.float32); _shape(logits, "logits", None, None)
    N, Cn = int(logits.shape[0]), int(logits.shape[1])
    if out is None:
        out = torch.empty_like(logits)
    _dev(out, torch.float32); _shape(out, "out", N, Cn)
    if out.device != logits.device:
        raise _lib.PigeonHipError(f"temper_logits: out is on {out.device}, logits on {logits.device}")
    with torch.cuda.device(logits.device):
        check(load().pg_temper_logits(_p(logits), N, Cn, float(beta), _p(out), _stream()), "pg_temper_logits")
    return out


def temper_plan(N: int, C_cells: int, K: int) -> dict:
    """pg_temper_plan: what pg_temper_stats does with N rows, C cells and K betas (host arithmetic, no GPU)."""
    o = (C.c_int32 * 4)()
    check(load().pg_temper_plan(int(N), int(C_cells), int(K), o), "pg_temper_plan")
    return {"threads": int(o[0]), "betas_per_pass": int(o[1]), "totals_workgroups": int(o[2]), "scratch_bytes": int(o[3])}


# ----------------------------------------------------------------------------------------- bootstrap intervals
def _boot_seed(seed) -> int:
    seed = int(seed)
    if not 0 <= seed < 2 ** 64:
        raise _lib.PigeonHipError(f"bootstrap: seed must be 0 .. 2^64 - 1, got {seed}")
    return seed


def bootstrap_indices(N: int, seed: int, r: int, j0: int, count: int, device="cuda") -> torch.Tensor:
    """pg_bootstrap_indices: idx(r, j0 + i) for i < count, (count,) int64 on `device`: the index stream of the resampling contract
    (include/pigeon_hip.h).  No host synchronisation."""
    dev = indexed_device(device)
    if int(count) < 0:
        raise _lib.PigeonHipError(f"bootstrap_indices: count = {count}")
    out = torch.empty((int(count),), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(load().pg_bootstrap_indices(int(N), _boot_seed(seed), int(r), int(j0), int(count), _p(out), _stream()), "pg_bootstrap_indices")
    return out


def bootstrap_means(x: torch.Tensor, R: int, seed: int = 0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pg_bootstrap_means: x (M,N) fp64, one per-item column a row -> (R,M) fp64, the mean of every column over each of R resamples
    of the N items (the same items for every column).  No host synchronisation."""
    _dev(x, torch.float64); _shape(x, "x", None, None)
    M, N = int(x.shape[0]), int(x.shape[1])
    if out is None:
        out = torch.empty((max(int(R), 0), M), dtype=torch.float64, device=x.device)
    _dev(out, torch.float64); _shape(out, "out", int(R), M)
    if out.device != x.device:
        raise _lib.PigeonHipError(f"bootstrap_means: out is on {out.device}, x on {x.device}")
    with torch.cuda.device(x.device):
        check(load().pg_bootstrap_means(_p(x), M, N, int(R), _boot_seed(seed), _p(out), _stream()), "pg_bootstrap_means")
    return out


def bootstrap_quantiles(rank: torch.Tensor, sorted_cols: torch.Tensor, R: int, q, seed: int = 0,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pg_bootstrap_quantiles: rank (M,N) int32 (every item's position in its column sorted ascending, stable), sorted_cols (M,N) fp64
    (the sorted columns), q 1 .. 16 numbers in [0, 1] (host) -> (R,M,Q) fp64: numpy.quantile(..., method='linear') of every column
    over each of R resamples.  No host synchronisation."""
    _dev(rank, torch.int32); _shape(rank, "rank", None, None)
    M, N = int(rank.shape[0]), int(rank.shape[1])
    _dev(sorted_cols, torch.float64); _shape(sorted_cols, "sorted", M, N)
    if sorted_cols.device != rank.device:
        raise _lib.PigeonHipError(f"bootstrap_quantiles: sorted is on {sorted_cols.device}, rank on {rank.device}")
    qs = [float(v) for v in q]
    Q = len(qs)
    if not 1 <= Q <= 16:
        raise _lib.PigeonHipError(f"bootstrap_quantiles: q must hold 1 .. 16 numbers, got {Q}")
    if out is None:
        out = torch.empty((max(int(R), 0), M, Q), dtype=torch.float64, device=rank.device)
    _dev(out, torch.float64); _shape(out, "out", int(R), M, Q)
    if out.device != rank.device:
        raise _lib.PigeonHipError(f"bootstrap_quantiles: out is on {out.device}, rank on {rank.device}")
    qarr = (C.c_double * Q)(*qs)
    with torch.cuda.device(rank.device):
        check(load().pg_bootstrap_quantiles(_p(rank), _p(sorted_cols), M, N, int(R), _boot_seed(seed), qarr, Q, _p(out), _stream()),
              "pg_bootstrap_quantiles")
    return out


def bootstrap_plan(N: int, R: int, M: int, Q: int = 1) -> dict:
    """pg_bootstrap_plan: what the bootstrap kernels do with N items, R replicates, M columns and Q quantiles (host arithmetic, no GPU)."""
    o = (C.c_int32 * 8)()
    check(load().pg_bootstrap_plan(int(N), int(R), int(M), int(Q), o), "pg_bootstrap_plan")
    return {"bins": int(o[0]), "shift": int(o[1]), "passes": int(o[2]), "columns_per_workgroup": int(o[3]), "threads": int(o[4]),
            "lds_bytes": int(o[5]), "max_n": int(o[6]), "workgroups": int(o[7])}


# ----------------------------------------------------------------------------------------- nearest rows of the embedding bank
KNN_MODES = {"auto": 0, "exact": 1, "filter": 2}


class KnnBank:
    """What pg_knn_search reads of a bank: the caller's fp32 rows (borrowed, not copied) and pg_knn_prepare's fp16 copy, half
    squared norms and statistics.  `bad_values`, `xmax` and `max_abs` read the statistics back (one host synchronisation each)."""

    def __init__(self, x: torch.Tensor, x16: Optional[torch.Tensor], hn: Optional[torch.Tensor], stats: Optional[torch.Tensor]):
        self.x, self.x16, self.hn, self.stats = x, x16, hn, stats
        self.n = int(x.shape[0])

    def struct(self) -> _lib.KnnBank:
        return _lib.KnnBank(x=self.x.data_ptr() if self.n else None, x16=None if self.x16 is None else self.x16.data_ptr(),
                            hn=None if self.hn is None else self.hn.data_ptr(), stats=None if self.stats is None else self.stats.data_ptr(),
                            n=self.n)

    def _stat_f32(self, i: int) -> float:
        return float(self.stats[i:i + 1].to(torch.int32).view(torch.float32).item())

    @property
    def bad_values(self) -> int:
        return int(self.stats[1].item())

    @property
    def xmax(self) -> float:
        """The largest row norm among the rows fp16 can hold (from the fp32 half squared norm)."""
        return (2.0 * self._stat_f32(0)) ** 0.5

    @property
    def max_abs(self) -> float:
        return self._stat_f32(2)


def knn_prepare(x: torch.Tensor) -> KnnBank:
    """pg_knn_prepare: x (N,1024) fp32 -> KnnBank with x16 (N,1024) fp16, hn (N,) fp32 and stats (4,) int64 on x's device; another
    N * 2052 bytes.  x is kept by reference.  No host synchronisation."""
    _dev(x, torch.float32); _shape(x, "x", None, HIDDEN)
    N = int(x.shape[0])
    x16 = torch.empty((N, HIDDEN), dtype=torch.float16, device=x.device)
    hn = torch.empty((N,), dtype=torch.float32, device=x.device)
    stats = torch.empty((4,), dtype=torch.int64, device=x.device)
    with torch.cuda.device(x.device):
        check(load().pg_knn_prepare(_p(x), N, _p(x16), _p(hn), _p(stats), _stream()), "pg_knn_prepare")
    return KnnBank(x, x16, hn, stats)


def knn_workspace_bytes(n: int, B: int, k: int) -> int:
    out = C.c_size_t(0)
    check(load().pg_knn_workspace_bytes(int(n), int(B), int(k), C.byref(out)), "pg_knn_workspace_bytes")
    return int(out.value)


def knn_search(bank: KnnBank, q: torch.Tensor, k: int, exclude: Optional[torch.Tensor] = None, mode: str = "auto",
               workspace: Optional[torch.Tensor] = None):
    """pg_knn_search: q (B,1024) fp32 -> (idx (B,k) int64, d2 (B,k) fp32, certified (B,) uint8): the k bank rows of smallest exact
    d2 per query, ascending, ties to the lower row, -1 / +inf past the bank's end.  exclude (B,) int64: a row query b must not
    return.  mode 'auto' (16-bit pass, certificate, exact tier for the rest), 'exact' (the exact tier only) or 'filter' (the 16-bit
    pass alone: a diagnostic).  The contract is include/pigeon_hip.h's.  No host synchronisation."""
    if not isinstance(bank, KnnBank):
        raise _lib.PigeonHipError(f"knn_search: bank must be a KnnBank (knn_prepare), got {type(bank).__name__}")
    if mode not in KNN_MODES:
        raise _lib.PigeonHipError(f"knn_search: mode must be one of {sorted(KNN_MODES)}, got {mode!r}")
    _dev(q, torch.float32); _shape(q, "q", None, HIDDEN)
    _dev(bank.x, torch.float32); _shape(bank.x, "bank.x", None, HIDDEN)
    _same_device("knn_search", "bank.x", bank.x, q=q, exclude=exclude, x16=bank.x16, hn=bank.hn, stats=bank.stats, workspace=workspace)
    B, k = int(q.shape[0]), int(k)
    if mode != "exact" and (bank.x16 is None or bank.hn is None or bank.stats is None):
        raise _lib.PigeonHipError(f"knn_search: mode {mode!r} needs a bank from knn_prepare (x16, hn, stats)")
    if bank.x16 is not None:
        _dev(bank.x16, torch.float16); _shape(bank.x16, "bank.x16", bank.n, HIDDEN)
        _dev(bank.hn, torch.float32); _shape(bank.hn, "bank.hn", bank.n)
        _dev(bank.stats, torch.int64); _shape(bank.stats, "bank.stats", 4)
    if exclude is not None:
        _dev(exclude, torch.int64); _shape(exclude, "exclude", B)
    need = knn_workspace_bytes(bank.n, B, k)                  # refuses k, B and n by name
    if workspace is None:
        workspace = torch.empty((need + 256,), dtype=torch.uint8, device=q.device)
    else:
        _dev(workspace, torch.uint8)
    off = (-workspace.data_ptr()) % 256
    ws_bytes = max(0, workspace.numel() - off)
    idx = torch.empty((B, k), dtype=torch.int64, device=q.device)
    d2 = torch.empty((B, k), dtype=torch.float32, device=q.device)
    cert = torch.empty((B,), dtype=torch.uint8, device=q.device)
    s = bank.struct()
    with torch.cuda.device(q.device):
        check(load().pg_knn_search(C.byref(s), _p(q), B, k, _p(exclude), KNN_MODES[mode], _p(idx), _p(d2), _p(cert),
                                   C.c_void_p(workspace.data_ptr() + off), ws_bytes, _stream()), "pg_knn_search")
    return idx, d2, cert


def knn_plan(n: int, B: int, k: int) -> dict:
    """pg_knn_plan: what pg_knn_search does with n rows, B queries and k neighbours (host arithmetic, no GPU)."""
    o = (C.c_int32 * 8)()
    check(load().pg_knn_plan(int(n), int(B), int(k), o), "pg_knn_plan")
    return {"candidates": int(o[0]), "rows_per_tile": int(o[1]), "queries_per_tile": int(o[2]), "spans": int(o[3]), "lds_bytes": int(o[4]),
            "tiles_per_span": int(o[5]), "exact_rows_per_tile": int(o[6]), "exact_spans": int(o[7])}


def tune_knn_spans(spans: int) -> None:
    """pg_tune_knn_spans: force the number of spans of both passes (0 = the defaults)."""
    check(load().pg_tune_knn_spans(int(spans)), "pg_tune_knn_spans")


# ----------------------------------------------------------------------------------------- training the head
def _same_device(who: str, ref_name: str, ref: torch.Tensor, **tensors):
    for name, t in tensors.items():
        if t is not None and t.device != ref.device:
            raise _lib.PigeonHipError(f"{who}: {name} is on {t.device}, {ref_name} on {ref.device}")


def head_train_loss(emb: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, centroids: Optional[torch.Tensor],
                    labels_llh: Optional[torch.Tensor] = None, labels_clf: Optional[torch.Tensor] = None, tau: float = 75.0,
                    grad_scale: float = 1.0, out: Optional[Dict[str, torch.Tensor]] = None, want_logits: bool = False):
    """pg_head_train_loss: emb (B,P,1024) or (B,1024) fp32 with P = 1 or 4, W (C,1024) fp32, bias (C,) fp32, centroids (C,2) fp64
    [lng,lat], labels_llh (B,2) fp64 (smoothed targets) or else labels_clf (B,) int64 (one-hot targets) -> dict of xbar (B,1024) fp32,
    g (B,C) fp32 (the gradient over the logits times grad_scale), loss_rows (B,) fp64 and, with want_logits or an `out` that holds
    one, logits (B,C) fp32.  The contract is include/pigeon_hip.h's.  `out` supplies the output tensors; no host synchronisation."""
    who = "head_train_loss"
    _dev(emb, torch.float32)
    if emb.dim() == 2:
        _shape(emb, "emb", None, HIDDEN)
        P = 1
    else:
        _shape(emb, "emb", None, None, HIDDEN)
        P = int(emb.shape[1])
    if P not in (1, 4):
        raise _lib.PigeonHipError(f"{who}: emb holds {P} panels per sample; 1 or 4 expected")
    B = int(emb.shape[0])
    _dev(W, torch.float32); _shape(W, "W", None, HIDDEN)
    Cn = int(W.shape[0])
    _dev(bias, torch.float32); _shape(bias, "bias", Cn)
    if labels_llh is None and labels_clf is None:
        raise _lib.PigeonHipError(f"{who}: one of labels_llh and labels_clf is needed")
    if labels_llh is not None:
        if centroids is None:
            raise _lib.PigeonHipError(f"{who}: smoothed targets need centroids")
        _dev(labels_llh, torch.float64); _shape(labels_llh, "labels_llh", B, 2)
        labels_clf = None
    else:
        _dev(labels_clf, torch.int64); _shape(labels_clf, "labels_clf", B)
    if centroids is not None:
        _dev(centroids, torch.float64); _shape(centroids, "centroids", Cn, 2)
    _same_device(who, "emb", emb, W=W, bias=bias, centroids=centroids, labels_llh=labels_llh, labels_clf=labels_clf)
    shapes = {"xbar": ((B, HIDDEN), torch.float32), "g": ((B, Cn), torch.float32), "loss_rows": ((B,), torch.float64)}
    if want_logits or (out is not None and "logits" in out):
        shapes["logits"] = ((B, Cn), torch.float32)
    if out is None:
        out = {}
    res = {}
    for k, (s, dt) in shapes.items():
        t = out.get(k)
        if t is None:
            t = torch.empty(s, dtype=dt, device=emb.device)
        _dev(t, dt); _shape(t, k, *s)
        _same_device(who, "emb", emb, **{k: t})
        res[k] = t
    with torch.cuda.device(emb.device):
        check(load().pg_head_train_loss(_p(emb), B, P, _p(W), _p(bias), _p(centroids), Cn, _p(labels_llh), _p(labels_clf), float(tau),
                                        float(grad_scale), _p(res["xbar"]), _p(res["g"]), _p(res["loss_rows"]), _p(res.get("logits")),
                                        _stream()), "pg_head_train_loss")
    return res


def head_train_update(g: torch.Tensor, xbar: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, m_W: torch.Tensor, v_W: torch.Tensor,
                      m_b: torch.Tensor, v_b: torch.Tensor, step: int, lr: float = 2e-5, beta1: float = 0.9, beta2: float = 0.999,
                      eps: float = 1e-8, weight_decay: float = 0.01, dW_out: Optional[torch.Tensor] = None,
                      db_out: Optional[torch.Tensor] = None) -> None:
    """pg_head_train_update: g (B,C), xbar (B,1024) as pg_head_train_loss wrote them; W, m_W, v_W (C,1024) and bias, m_b, v_b (C,)
    fp32, updated IN PLACE through their raw pointers by torch.optim.AdamW's rule (the caller bumps version counters); dW_out (C,1024)
    / db_out (C,) fp32 receive the gradient when given.  The contract is include/pigeon_hip.h's.  No host synchronisation."""
    who = "head_train_update"
    _dev(g, torch.float32); _shape(g, "g", None, None)
    B, Cn = int(g.shape[0]), int(g.shape[1])
    _dev(xbar, torch.float32); _shape(xbar, "xbar", B, HIDDEN)
    for name, t in (("W", W), ("m_W", m_W), ("v_W", v_W)):
        _dev(t, torch.float32); _shape(t, name, Cn, HIDDEN)
    for name, t in (("bias", bias), ("m_b", m_b), ("v_b", v_b)):
        _dev(t, torch.float32); _shape(t, name, Cn)
    if dW_out is not None:
        _dev(dW_out, torch.float32); _shape(dW_out, "dW_out", Cn, HIDDEN)
    if db_out is not None:
        _dev(db_out, torch.float32); _shape(db_out, "db_out", Cn)
    _same_device(who, "g", g, xbar=xbar, W=W, bias=bias, m_W=m_W, v_W=v_W, m_b=m_b, v_b=v_b, dW_out=dW_out, db_out=db_out)
    with torch.cuda.device(g.device):
        check(load().pg_head_train_update(_p(g), _p(xbar), B, Cn, _p(W), _p(bias), _p(m_W), _p(v_W), _p(m_b), _p(v_b), int(step), float(lr),
                                          float(beta1), float(beta2), float(eps), float(weight_decay), _p(dW_out), _p(db_out), _stream()),
              "pg_head_train_update")


def head_train_plan(C_cells: int) -> dict:
    """pg_head_train_plan: where pg_head_train_loss keeps a row's targets for C cells (host arithmetic, no GPU)."""
    o = (C.c_int32 * 4)()
    check(load().pg_head_train_plan(int(C_cells), o), "pg_head_train_plan")
    return {"form": int(o[0]), "lds_bytes": int(o[1]), "lds_cells": int(o[2]), "threads": int(o[3])}


# ----------------------------------------------------------------------------------------- prototype cluster table
def _cell_tables(who: str, cell_off: torch.Tensor, mat_off: Optional[torch.Tensor]):
    """The CSR invariants of a packed batch of cells, on the host (the C calls read both tables there): cell_off rises from 0, cell c's
    matrix has room for its n x n elements.  Returns (cell_off, mat_off) as contiguous int64 CPU tensors; mat_off=None packs densely."""
    if cell_off.dtype != torch.int64 or cell_off.dim() != 1 or cell_off.numel() < 1:
        raise _lib.PigeonHipError(f"{who}: cell_off must be an int64 vector of C + 1 entries")
    off = cell_off.cpu().contiguous()
    n = off[1:] - off[:-1]
    if int(off[0]) != 0 or bool((n < 0).any()):
        raise _lib.PigeonHipError(f"{who}: cell_off must rise from 0")
    if mat_off is None:
        mo = torch.zeros_like(off)
        torch.cumsum(n * n, 0, out=mo[1:])
    else:
        if mat_off.dtype != torch.int64 or mat_off.shape != cell_off.shape:
            raise _lib.PigeonHipError(f"{who}: mat_off must be an int64 vector as long as cell_off")
        mo = mat_off.cpu().contiguous()
        if int(mo[0]) < 0 or bool(((mo[1:] - mo[:-1]) < n * n).any()):
            raise _lib.PigeonHipError(f"{who}: mat_off must leave every cell room for its n x n matrix")
    return off, mo


def haversine_blocks(pts: torch.Tensor, cell_off: torch.Tensor, zero_as: float = 1e-5):
    """pg_haversine_blocks: pts (N,2) fp64 [lng,lat] on the device, cell_off (C+1,) int64 -> (dist, mat_off): the cells' own n x n
    distance matrices in km, packed densely (cell c at dist[mat_off[c]:mat_off[c+1]], row-major), exactly symmetric (the upper
    triangle is haversine_matrix's, bit for bit), zeros and identical points as `zero_as`.  One launch."""
    _dev(pts, torch.float64)
    _shape(pts, "pts", None, 2)
    off, mo = _cell_tables("haversine_blocks", cell_off, None)
    if int(off[-1]) != pts.shape[0]:
        raise _lib.PigeonHipError(f"haversine_blocks: cell_off ends at {int(off[-1])}, pts has {pts.shape[0]} rows")
    out = torch.empty((int(mo[-1]),), dtype=torch.float64, device=pts.device)
    check(load().pg_haversine_blocks(_p(pts), _p(off), _p(mo), off.numel() - 1, float(zero_as), _p(out), _stream()),
          "pg_haversine_blocks")
    return out, mo


def optics_graph(dist: torch.Tensor, cell_off: torch.Tensor, mat_off: torch.Tensor, min_samples: int) -> Dict[str, torch.Tensor]:
    """pg_optics_graph: dist fp64 on the device (the packed matrices), cell_off / mat_off (C+1,) int64 -> ordering, core, reach, pred,
    packed by cell_off; ordering and pred are local to the cell.  sklearn's compute_optics_graph(metric='precomputed'), bit for bit."""
    _dev(dist, torch.float64)
    if dist.dim() != 1:
        raise _lib.PigeonHipError(f"optics_graph: dist must be the flat packed matrices, got shape {tuple(dist.shape)}")
    off, mo = _cell_tables("optics_graph", cell_off, mat_off)
    if int(mo[-1]) > dist.numel():
        raise _lib.PigeonHipError(f"optics_graph: mat_off ends at {int(mo[-1])}, dist has {dist.numel()} elements")
    min_samples = int(min_samples)
    n = off[1:] - off[:-1]
    if min_samples < 2:
        raise _lib.PigeonHipError(f"optics_graph: min_samples must be at least 2 (got {min_samples})")
    if n.numel() and int(n.min()) < min_samples:
        raise _lib.PigeonHipError(f"optics_graph: cell {int(n.argmin())} has {int(n.min())} points, fewer than min_samples = {min_samples}")
    N = int(off[-1])
    ordering = torch.empty((N,), dtype=torch.int64, device=dist.device)
    pred = torch.empty((N,), dtype=torch.int64, device=dist.device)
    core = torch.empty((N,), dtype=torch.float64, device=dist.device)
    reach = torch.empty((N,), dtype=torch.float64, device=dist.device)
    check(load().pg_optics_graph(_p(dist), _p(off), _p(mo), off.numel() - 1, min_samples, _p(ordering), _p(core), _p(reach), _p(pred),
                                 _stream()), "pg_optics_graph")
    return {"ordering": ordering, "core": core, "reach": reach, "pred": pred}


def optics_plan(n: int, min_samples: int) -> dict:
    """pg_optics_plan: what pg_optics_graph does with a cell of n points under the current knobs (host arithmetic, no GPU)."""
    out = (C.c_int32 * 4)()
    check(load().pg_optics_plan(int(n), int(min_samples), out), "pg_optics_plan")
    return {"form": int(out[0]), "threads": int(out[1]), "lds_points": int(out[2]), "max_points": int(out[3])}


def tune_optics_lds_points(max_points: int) -> None:
    """pg_tune_optics_lds_points: the largest cell whose ordering state stays in LDS (0 = the default).  Bit-identical either way."""
    check(load().pg_tune_optics_lds_points(int(max_points)), "pg_tune_optics_lds_points")


# ----------------------------------------------------------------------------------------- point-in-region lookup
class RegionBankHandle:
    """pg_region_bank over numpy CSR arrays (pigeon_amd/regions.py RegionBank builds them): keeps the host offset arrays alive,
    uploads the device copies at the first use that needs them (`device=None`: no GPU is touched; pg_region_plan reads the host side only)."""

    def __init__(self, region_off, ring_off, xy, ring_bbox, region_bbox):
        import numpy as np
        self.region_off = np.ascontiguousarray(region_off, dtype=np.int64)
        self.ring_off = np.ascontiguousarray(ring_off, dtype=np.int64)
        self.host = (np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2), np.ascontiguousarray(ring_bbox, dtype=np.float64).reshape(-1, 4),
                     np.ascontiguousarray(region_bbox, dtype=np.float64).reshape(-1, 4))
        self.num_regions, self.num_rings, self.num_vertices = self.region_off.size - 1, self.ring_off.size - 1, self.host[0].shape[0]
        self.dev = None
        self.struct = _lib.RegionBankStruct(None, None, None, None, None, self.region_off.ctypes.data, self.ring_off.ctypes.data,
                                            self.num_regions, self.num_rings, self.num_vertices)

    def on_device(self, device="cuda"):
        if self.dev is None:
            _lib.require_gpu()
            self.dev = [torch.from_numpy(a).to(device) for a in (self.region_off, self.ring_off) + self.host]
            s = self.struct
            s.region_off, s.ring_off, s.xy, s.ring_bbox, s.region_bbox = (t.data_ptr() or None for t in self.dev)
        return self


def _region_points(who: str, pts: torch.Tensor) -> torch.Tensor:
    _dev(pts, torch.float64)
    return _shape(pts, f"{who}: pts", None, 2)


def _host_i32(who: str, name: str, v, n: int):
    import numpy as np
    a = np.ascontiguousarray(v.cpu().numpy() if torch.is_tensor(v) else v)
    if a.shape != (n,) or a.dtype.kind not in "iu":
        raise _lib.PigeonHipError(f"{who}: {name} must be {n} integers, got shape {a.shape} of {a.dtype}")
    if a.size and (int(a.min()) < -2**31 or int(a.max()) >= 2**31):
        raise _lib.PigeonHipError(f"{who}: {name} does not fit 32 bits")
    return np.ascontiguousarray(a, dtype=np.int32)


def region_locate(bank: RegionBankHandle, pts: torch.Tensor, start=None):
    """pg_region_locate: pts (N,2) fp64 on the device, start (N) host integers or None -> (cover (N) int32, state (N) uint8) on the
    device: the lowest region >= start[i] that is not certainly OUTSIDE and its state (1 INSIDE, 2 AMBIGUOUS); -1 / 0 if none."""
    _region_points("region_locate", pts)
    n = pts.shape[0]
    st = None if start is None else _host_i32("region_locate", "start", start, n)
    cover = torch.empty((n,), dtype=torch.int32, device=pts.device)
    state = torch.empty((n,), dtype=torch.uint8, device=pts.device)
    check(load().pg_region_locate(C.byref(bank.on_device(pts.device).struct), _p(pts), None if st is None else st.ctypes.data, n, _p(cover),
                                  _p(state), _stream()), "pg_region_locate")
    return cover, state


def region_classify(bank: RegionBankHandle, pts: torch.Tensor, region) -> torch.Tensor:
    """pg_region_classify: the state (0 OUTSIDE, 1 INSIDE, 2 AMBIGUOUS) of point i against region[i] (host integers; -1: OUTSIDE)."""
    _region_points("region_classify", pts)
    n = pts.shape[0]
    rg = _host_i32("region_classify", "region", region, n)
    state = torch.empty((n,), dtype=torch.uint8, device=pts.device)
    check(load().pg_region_classify(C.byref(bank.on_device(pts.device).struct), _p(pts), rg.ctypes.data, n, _p(state), _stream()),
          "pg_region_classify")
    return state


def region_nearest(bank: RegionBankHandle, pts: torch.Tensor):
    """pg_region_nearest: (idx (N) int32, dist (N) fp64) on the device: the region whose boundary is nearest (planar, degrees; ties to
    the lower index) and that distance."""
    _region_points("region_nearest", pts)
    n = pts.shape[0]
    idx = torch.empty((n,), dtype=torch.int32, device=pts.device)
    dist = torch.empty((n,), dtype=torch.float64, device=pts.device)
    check(load().pg_region_nearest(C.byref(bank.on_device(pts.device).struct), _p(pts), n, _p(idx), _p(dist), _stream()), "pg_region_nearest")
    return idx, dist


def region_plan(bank: RegionBankHandle) -> dict:
    """pg_region_plan: how the three calls map points onto the device for this bank (host arithmetic, no GPU)."""
    out = (C.c_int32 * 4)()
    check(load().pg_region_plan(C.byref(bank.struct), out), "pg_region_plan")
    return {"form": int(out[0]), "threads": int(out[1]), "max_ring_edges": int(out[2]), "wave_edges": int(out[3])}


def tune_region_wave_edges(max_edges: int) -> None:
    """pg_tune_region_wave_edges: the largest ring (edges) of a bank that is still served by one wave per point (negative = the default)."""
    check(load().pg_tune_region_wave_edges(int(max_edges)), "pg_tune_region_wave_edges")


# ----------------------------------------------------------------------------------------- image preprocessing
def norm_lut() -> torch.Tensor:
    """pg_prep_norm_lut: the (3, 256) fp32 normalisation table ((v / 255) - mean[c]) / std[c], every value a pixel can take.  A host
    tensor from a host call (no GPU needed); `norm_lut()[c][bytes]` is the fp32 pixel of a byte of channel c."""
    out = (C.c_float * 768)()
    check(load().pg_prep_norm_lut(out), "pg_prep_norm_lut")
    return torch.tensor(list(out), dtype=torch.float32).view(3, 256)


def bytes_to_pixels(pixel_bytes: torch.Tensor) -> torch.Tensor:
    """(..., 3, 336, 336) uint8 -> fp32 pixel values through the table: what the encoder computes from, for tests and tools (the
    product path never materialises it)."""
    lut = norm_lut().to(pixel_bytes.device)
    idx = pixel_bytes.long() + (torch.arange(3, device=pixel_bytes.device) * 256).view(3, 1, 1)
    return lut.view(-1)[idx]


class _Handle:
    """Owner of one library handle `_h`: `close` (and collection) destroys it, once, through the library function `_destroy` names."""
    _destroy = ""

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            getattr(load(), self._destroy)(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _prep_out_dtype(out_dtype: torch.dtype) -> int:
    if out_dtype not in _PREP_OUT:
        raise _lib.PigeonHipError("preprocess output dtype must be float32 or float16 (or uint8: the resized bytes)")
    return _PREP_OUT[out_dtype]


def _items_header(items, nbytes: int):
    """A plan's ctypes descriptor array as the uint8 array the head of its buffer must hold."""
    import numpy as np
    return np.frombuffer(items, dtype=np.uint8, count=nbytes) if nbytes else np.zeros(0, dtype=np.uint8)


class Preprocessor(_Handle):
    """CLIP preprocessing on the GPU for one input geometry: (N,H,W,3) uint8 RGB -> (N,3,336,336) pixel_values,
    bit-exact with `CLIPProcessor(images=pil)` (Pillow fixed-point bicubic + numpy float32 normalisation)."""
    _destroy = "pg_prep_destroy"

    def __init__(self, in_h: int, in_w: int, device: int = 0):
        _lib.require_gpu()
        self._h = C.c_void_p()
        check(load().pg_prep_create(C.byref(self._h), int(device), int(in_h), int(in_w)), "pg_prep_create")
        self.in_h, self.in_w, self.device = int(in_h), int(in_w), int(device)
        geo = (C.c_int32 * 6)()
        check(load().pg_prep_geometry(self._h, geo), "pg_prep_geometry")
        self.resized_h, self.resized_w, self.top, self.left, self.row0, self.nrows = [int(x) for x in geo]
        self._ws = None

    def forward(self, images_u8: torch.Tensor, out_dtype: torch.dtype = torch.float32) -> torch.Tensor:
        _dev(images_u8, torch.uint8)
        if images_u8.dim() != 4 or tuple(images_u8.shape[1:]) != (self.in_h, self.in_w, 3):
            raise _lib.PigeonHipError(f"images must be (N,{self.in_h},{self.in_w},3) uint8, got {tuple(images_u8.shape)}")
        dt = _prep_out_dtype(out_dtype)
        n = images_u8.shape[0]
        need = C.c_size_t()
        check(load().pg_prep_workspace_bytes(self._h, n, C.byref(need)), "pg_prep_workspace_bytes")
        if self._ws is None or self._ws.numel() < need.value or self._ws.device != images_u8.device:
            self._ws = torch.empty(need.value, dtype=torch.uint8, device=images_u8.device)
        out = torch.empty((n, 3, 336, 336), dtype=out_dtype, device=images_u8.device)
        check(load().pg_prep_forward(self._h, _p(images_u8), n, _p(out), dt, _p(self._ws), self._ws.numel(), _stream()), "pg_prep_forward")
        return out

    __call__ = forward


class RaggedPlan:
    """What pg_prep_ragged_plan makes of a list of (height, width): one descriptor per image (`items`, a ctypes array of
    _lib.PrepItem; `header()` = the same bytes as a uint8 array, what the head of the packed buffer must hold) and the sizes of the
    packed buffer and of the workspace.  Host data only."""

    def __init__(self, sizes, items, packed_bytes: int, workspace_bytes: int):
        self.sizes, self.items = sizes, items
        self.n = len(sizes)
        self.packed_bytes, self.workspace_bytes = int(packed_bytes), int(workspace_bytes)
        self.header_bytes = self.n * _lib.PREP_ITEM_BYTES

    def header(self):
        return _items_header(self.items, self.header_bytes)


def ragged_plan(sizes) -> RaggedPlan:
    """pg_prep_ragged_plan: the layout of a batch of images of the given (height, width) pairs.  No HIP call: needs the library,
    not a GPU."""
    sizes = [(int(h), int(w)) for h, w in sizes]
    n = len(sizes)
    hw = (C.c_int32 * (2 * n))(*[v for s in sizes for v in s])
    items = (_lib.PrepItem * n)()
    packed, ws = C.c_size_t(), C.c_size_t()
    check(load().pg_prep_ragged_plan(n, hw, items, C.byref(packed), C.byref(ws)), "pg_prep_ragged_plan")
    return RaggedPlan(sizes, items, packed.value, ws.value)


class RaggedPreprocessor(_Handle):
    """CLIP preprocessing on the GPU for a batch of images of DIFFERENT sizes in one packed buffer (layout: pigeon_hip.h,
    pg_prep_ragged_forward): the same bits per image as `Preprocessor(h, w)` on it alone, in three launches per call."""
    _destroy = "pg_prep_ragged_destroy"

    def __init__(self, device: int = 0):
        _lib.require_gpu()
        self._h = C.c_void_p()
        check(load().pg_prep_ragged_create(C.byref(self._h), int(device)), "pg_prep_ragged_create")
        self.device = int(device)
        self._ws = None

    plan = staticmethod(ragged_plan)

    def forward(self, packed_u8: torch.Tensor, plan: RaggedPlan, out_dtype: torch.dtype = torch.float32,
                header_written: bool = False) -> torch.Tensor:
        """packed_u8: DEVICE 1-D uint8 of plan.packed_bytes bytes.  The kernels read the descriptors from its head: they are copied
        there from the plan unless the caller says it has written them already (`header_written`, what gpu_preprocess does on the
        host side of its one copy)."""
        _dev(packed_u8, torch.uint8)
        if packed_u8.dim() != 1 or packed_u8.numel() != plan.packed_bytes:
            raise _lib.PigeonHipError(f"packed buffer must be 1-D uint8 of {plan.packed_bytes} bytes, got {tuple(packed_u8.shape)}")
        if packed_u8.device.index != self.device:
            raise _lib.PigeonHipError(f"packed buffer is on {packed_u8.device}, the preprocessor on cuda:{self.device}")
        dt = _prep_out_dtype(out_dtype)
        out = torch.empty((plan.n, 3, 336, 336), dtype=out_dtype, device=packed_u8.device)
        if plan.n == 0:
            return out
        if self._ws is None or self._ws.numel() < plan.workspace_bytes:
            self._ws = torch.empty(plan.workspace_bytes, dtype=torch.uint8, device=packed_u8.device)
        if not header_written:
            packed_u8[:plan.header_bytes].copy_(torch.from_numpy(plan.header().copy()))
        check(load().pg_prep_ragged_forward(self._h, _p(packed_u8), plan.packed_bytes, plan.items, plan.n, _p(out), dt,
                                            _p(self._ws), self._ws.numel(), _stream()), "pg_prep_ragged_forward")
        return out

    __call__ = forward


# ----------------------------------------------------------------------------------------- JPEG decoding
class JpegEntropyError(ValueError):
    """A supported file whose scan is damaged; `index` is the image's place in the batch."""

    def __init__(self, index: int, message: str):
        super().__init__(message)
        self.index = int(index)


def default_jpeg_threads() -> int:
    """Workers of the host stage: the CPUs this process may run on, 16 at the most (never the machine's count)."""
    import os
    return max(1, min(16, len(os.sched_getaffinity(0))))


def jpeg_probe(data) -> "_lib.JpegInfo":
    """pg_jpeg_probe: the header of one file (bytes).  `.reason` 0 = decoded on the GPU, else why not (`jpeg_reason`).  Host only."""
    if not isinstance(data, (bytes, bytearray, memoryview)):
        raise _lib.PigeonHipError(f"jpeg_probe expects bytes, got {type(data).__name__}")
    data = bytes(data)
    info = _lib.JpegInfo()
    check(load().pg_jpeg_probe(data if data else b"\0", len(data), C.byref(info)), "pg_jpeg_probe")
    return info


def jpeg_reason(code: int) -> str:
    """Short name of a PG_JPEG_R_* code ("progressive", "components", ...); the library's sentence is `jpeg_reason_text`."""
    return _lib.JPEG_REASONS[code] if 0 <= int(code) < len(_lib.JPEG_REASONS) else f"reason_{int(code)}"


def jpeg_reason_text(code: int) -> str:
    return load().pg_jpeg_reason(int(code)).decode()


class JpegPlan:
    """What pg_jpeg_plan makes of a list of probed headers: one pg_jpeg_item per image (`items`), the ragged resize's plan for the same
    sizes (`prep`, a RaggedPlan: same integers as `ragged_plan`) and the sizes of the coefficient buffer and the plane workspace."""

    def __init__(self, infos, items, prep: "RaggedPlan", coef_bytes: int, workspace_bytes: int):
        self.infos, self.items, self.prep = infos, items, prep
        self.n = len(items)
        self.coef_bytes, self.workspace_bytes = int(coef_bytes), int(workspace_bytes)
        self.header_bytes = self.n * _lib.JPEG_ITEM_BYTES

    def header(self):
        return _items_header(self.items, self.header_bytes)


def jpeg_plan(infos) -> JpegPlan:
    """pg_jpeg_plan.  `infos`: a list of _lib.JpegInfo; one with reason != 0 is an image the caller supplies the pixels of (its height
    and width must be set).  Host only."""
    n = len(infos)
    arr = (_lib.JpegInfo * n)(*infos)
    items, prep_items = (_lib.JpegItem * n)(), (_lib.PrepItem * n)()
    coef, ws, packed, prep_ws = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    check(load().pg_jpeg_plan(n, arr, items, prep_items, C.byref(coef), C.byref(ws), C.byref(packed), C.byref(prep_ws)), "pg_jpeg_plan")
    prep = RaggedPlan([(int(i.height), int(i.width)) for i in infos], prep_items, packed.value, prep_ws.value)
    return JpegPlan(list(infos), items, prep, coef.value, ws.value)


def jpeg_entropy_decode(files, plan: JpegPlan, coef: torch.Tensor, threads: Optional[int] = None) -> None:
    """pg_jpeg_entropy_decode: the files' coefficients (and the descriptors, in the head) into the HOST uint8 tensor `coef` of
    plan.coef_bytes bytes; fills the plan's items with the quantisation tables.  ctypes releases the GIL for the call.  Raises
    JpegEntropyError (a ValueError) carrying the index of the first damaged file.  Host only."""
    if not torch.is_tensor(coef) or coef.is_cuda or coef.dtype != torch.uint8 or coef.dim() != 1 or not coef.is_contiguous() \
            or coef.numel() != plan.coef_bytes:
        raise _lib.PigeonHipError(f"coefficient buffer must be a contiguous 1-D uint8 host tensor of {plan.coef_bytes} bytes")
    if len(files) != plan.n:
        raise _lib.PigeonHipError(f"{len(files)} files for a plan of {plan.n} images")
    if plan.n == 0:
        return
    keep = [bytes(f) if plan.items[i].ncomp else b"" for i, f in enumerate(files)]
    ptrs = (C.c_void_p * plan.n)(*[C.cast(C.c_char_p(b), C.c_void_p) for b in keep])
    sizes = (C.c_size_t * plan.n)(*[len(b) for b in keep])
    bad = C.c_int(-1)
    rc = load().pg_jpeg_entropy_decode(plan.n, ptrs, sizes, plan.items, C.c_void_p(coef.data_ptr()), plan.coef_bytes,
                                       int(default_jpeg_threads() if threads is None else threads), C.byref(bad))
    if rc != 0 and bad.value >= 0:
        raise JpegEntropyError(bad.value, load().pg_last_error().decode())
    check(rc, "pg_jpeg_entropy_decode")


def jpeg_forward(coef_dev: torch.Tensor, plan: JpegPlan, packed_dev: torch.Tensor, workspace: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pg_jpeg_forward: coefficients on the device -> RGB at every decoded image's place in `packed_dev` (1-D uint8 of
    plan.prep.packed_bytes bytes) and the resize's descriptors in its head.  The head of `coef_dev` is (re)written from the plan's
    items, which are what the call checks.  Returns packed_dev."""
    _dev(coef_dev, torch.uint8)
    _dev(packed_dev, torch.uint8)
    if coef_dev.dim() != 1 or coef_dev.numel() != plan.coef_bytes:
        raise _lib.PigeonHipError(f"coefficient buffer must be 1-D uint8 of {plan.coef_bytes} bytes, got {tuple(coef_dev.shape)}")
    if packed_dev.dim() != 1 or packed_dev.numel() != plan.prep.packed_bytes:
        raise _lib.PigeonHipError(f"packed buffer must be 1-D uint8 of {plan.prep.packed_bytes} bytes, got {tuple(packed_dev.shape)}")
    if packed_dev.device != coef_dev.device:
        raise _lib.PigeonHipError("coefficient and packed buffers are on different devices")
    if plan.n == 0:
        return packed_dev
    with torch.cuda.device(coef_dev.device):
        if workspace is None:
            workspace = torch.empty(max(plan.workspace_bytes, 16), dtype=torch.uint8, device=coef_dev.device)
        _dev(workspace, torch.uint8)
        coef_dev[:plan.header_bytes].copy_(torch.from_numpy(plan.header().copy()))
        check(load().pg_jpeg_forward(_p(coef_dev), plan.coef_bytes, plan.items, plan.prep.items, plan.n, _p(packed_dev),
                                     plan.prep.packed_bytes, _p(workspace), workspace.numel(), _stream()), "pg_jpeg_forward")
    return packed_dev


# ----------------------------------------------------------------------------------------- equirectangular panoramas
class EquirectPlan:
    """What pg_equirect_plan makes of a list of views: one pg_eq_item per view (`items`), the ragged resize's plan for n images of
    size x size (`prep`, a RaggedPlan: same integers as `ragged_plan`) and the bytes the source buffer must at least hold."""

    def __init__(self, items, prep: "RaggedPlan", src_bytes: int):
        self.items, self.prep = items, prep
        self.n = len(items)
        self.src_bytes = int(src_bytes)


def equirect_plan(views, src_offs) -> EquirectPlan:
    """pg_equirect_plan.  `views`: a list of (src_h, src_w, src_index, size, rot, inv_f) with `rot` nine floats (row-major, camera ->
    panorama) and inv_f = tan(fov / 2) / (size / 2); `src_offs`: byte offset of every panorama in the source buffer.  Host only."""
    n = len(views)
    arr = (_lib.EqView * n)()
    for v, (h, w, k, s, rot, inv_f) in zip(arr, views):
        rot = [float(r) for r in (rot.reshape(-1).tolist() if hasattr(rot, "reshape") else rot)]
        if len(rot) != 9:
            raise _lib.PigeonHipError(f"a view's rotation must have 9 entries, got {len(rot)}")
        v.src_h, v.src_w, v.src_index, v.size, v.inv_f = int(h), int(w), int(k), int(s), float(inv_f)
        v.rot[:] = rot
    offs = [int(o) for o in src_offs]
    if any(o < 0 for o in offs):
        raise _lib.PigeonHipError("equirect_plan: a source offset is negative")
    offs_c = (C.c_uint64 * max(len(offs), 1))(*offs)
    items, prep_items = (_lib.EqItem * n)(), (_lib.PrepItem * n)()
    packed, prep_ws = C.c_size_t(), C.c_size_t()
    check(load().pg_equirect_plan(n, arr, len(offs), offs_c, items, prep_items, C.byref(packed), C.byref(prep_ws)), "pg_equirect_plan")
    prep = RaggedPlan([(int(v.size), int(v.size)) for v in arr], prep_items, packed.value, prep_ws.value)
    src_bytes = max([int(it.src_off) + int(it.src_h) * int(it.src_w) * 3 for it in items], default=0)
    return EquirectPlan(items, prep, src_bytes)


def equirect_forward(src_dev: torch.Tensor, plan: EquirectPlan, packed_dev: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pg_equirect_forward: the panoramas in `src_dev` (DEVICE 1-D uint8; a packed buffer of the JPEG stage or of host pixels will do,
    its head is not read) -> every view's RGB at its place in `packed_dev` (1-D uint8 of plan.prep.packed_bytes bytes, made here if
    None) and the resize's descriptors in its head.  Returns packed_dev."""
    _dev(src_dev, torch.uint8)
    if src_dev.dim() != 1 or src_dev.numel() < plan.src_bytes:
        raise _lib.PigeonHipError(f"source buffer must be 1-D uint8 of at least {plan.src_bytes} bytes, got {tuple(src_dev.shape)}")
    if packed_dev is None:
        packed_dev = torch.empty(plan.prep.packed_bytes, dtype=torch.uint8, device=src_dev.device)
    _dev(packed_dev, torch.uint8)
    if packed_dev.dim() != 1 or packed_dev.numel() != plan.prep.packed_bytes:
        raise _lib.PigeonHipError(f"packed buffer must be 1-D uint8 of {plan.prep.packed_bytes} bytes, got {tuple(packed_dev.shape)}")
    if packed_dev.device != src_dev.device:
        raise _lib.PigeonHipError("source and packed buffers are on different devices")
    if plan.n == 0:
        return packed_dev
    with torch.cuda.device(src_dev.device):
        check(load().pg_equirect_forward(_p(src_dev), src_dev.numel(), plan.items, plan.prep.items, plan.n, _p(packed_dev),
                                         plan.prep.packed_bytes, _stream()), "pg_equirect_forward")
    return packed_dev


# ----------------------------------------------------------------------------------------- ViT encoder handle
class VitEncoder(_Handle):
    """Owns a pg_vit handle: 16-bit-packed weights (fp16 or bf16) resident in HBM, forward = ViT-L/14-336 + token mean.

    state_dict keys may be in either transformers layout (vision_model.* or flat); values are CPU or device
    tensors of any float dtype (converted to fp32 on the host, then packed by the library).
    """
    _destroy = "pg_vit_destroy"

    def __init__(self, state_dict: Dict[str, torch.Tensor], device: int = 0, max_chunk: int = 0,
                 layers: Optional[int] = None, mma_dtype: Optional[str] = None, precise: bool = False):
        """mma_dtype: None (library default: fp16, or env PIGEON_MMA_DTYPE=bf16), 'f16' or 'bf16'.
        precise: also pack the split-fp16 weight copy of the exact mode (`forward_precise`; 3x the 16-bit weight memory)."""
        _lib.require_gpu()
        lib = load()
        keys = [k[len("vision_model."):] if k.startswith("vision_model.") else k for k in state_dict]
        if layers is None:
            layers = 0
            while f"encoder.layers.{layers}.layer_norm1.weight" in keys:
                layers += 1
        if layers < 1:
            raise _lib.PigeonHipError("state dict holds no encoder layers")
        self.layers = layers
        self.device = device
        pgdt = {None: 0, "f16": _lib.PG_DTYPE_F16, "fp16": _lib.PG_DTYPE_F16, "bf16": _lib.PG_DTYPE_BF16}[mma_dtype]
        cfg = VitCfg(layers, 336, 14, 1024, 16, 4096, 1e-5, max_chunk, pgdt, 1 if precise else 0)
        self.precise = bool(precise)
        self._ws_precise = None
        h = C.c_void_p()
        torch.cuda.set_device(device)
        check(lib.pg_vit_create(C.byref(h), device, C.byref(cfg)), "pg_vit_create")
        self._h = h
        for name, t in state_dict.items():
            if not torch.is_tensor(t) or not t.is_floating_point():
                continue                                   # e.g. embeddings.position_ids (int64 buffer)
            a = t.detach().to("cpu", torch.float32).contiguous()
            shape = (C.c_int64 * max(a.dim(), 1))(*(list(a.shape) or [1]))
            check(lib.pg_vit_load_weight(h, name.encode(), C.c_void_p(a.data_ptr()), _lib.PG_DTYPE_F32, shape,
                                         max(a.dim(), 1)), f"pg_vit_load_weight({name})")
        check(lib.pg_vit_finalize(h), "pg_vit_finalize")
        self.mma_dtype = {_lib.PG_DTYPE_F16: "f16", _lib.PG_DTYPE_BF16: "bf16"}[lib.pg_vit_mma_dtype(h)]
        self._ws = None
        self.max_chunk = max_chunk if max_chunk > 0 else 512

    def _workspace(self, n: int) -> torch.Tensor:
        need = C.c_size_t()
        check(load().pg_vit_workspace_bytes(self._h, n, C.byref(need)), "pg_vit_workspace_bytes")
        if self._ws is None or self._ws.numel() < need.value:
            self._ws = None
            self._ws = torch.empty(need.value + 256, dtype=torch.uint8, device=f"cuda:{self.device}")
        return self._ws

    def forward(self, pixels: torch.Tensor, return_hidden: bool = False):
        """pixels (N,3,336,336) fp32/fp16/bf16, or uint8 (the bytes Preprocessor writes with out_dtype=torch.uint8: looked up in the
        normalisation table by the im2col), on the device -> (N,1024) fp32 [, (N,577,1024) fp32]."""
        _dev(pixels)
        if pixels.dim() != 4 or tuple(pixels.shape[1:]) != (3, 336, 336):
            raise _lib.PigeonHipError(f"pixels must be (N,3,336,336), got {tuple(pixels.shape)}")
        if pixels.dtype not in _PIXIN:
            raise _lib.PigeonHipError("pixels must be fp32, fp16 or bf16, or uint8 bytes")
        n = pixels.shape[0]
        ws = self._workspace(n)
        off = (-ws.data_ptr()) % 256
        emb = torch.empty((n, HIDDEN), dtype=torch.float32, device=pixels.device)
        hid = torch.empty((n, TOKENS, HIDDEN), dtype=torch.float32, device=pixels.device) if return_hidden else None
        dt = _PIXIN[pixels.dtype]
        check(load().pg_vit_forward_hidden(self._h, _p(pixels), dt, n, _p(emb), _p(hid),
                                           C.c_void_p(ws.data_ptr() + off), ws.numel() - off, _stream()),
              "pg_vit_forward")
        return (emb, hid) if return_hidden else emb

    __call__ = forward

    def forward_precise(self, pixels: torch.Tensor, return_hidden: bool = False, out: Optional[torch.Tensor] = None):
        """The exact mode (pg_vit_forward_precise): same contract as `forward`, near-fp32 arithmetic (split-fp16 GEMM operands,
        fp32 attention / LayerNorm / QuickGELU), ~5x the time per image.  Needs `precise=True` at construction."""
        if not self.precise:
            raise _lib.PigeonHipError("forward_precise: the encoder was built without precise=True (no split-weight copy)")
        _dev(pixels)
        if pixels.dim() != 4 or tuple(pixels.shape[1:]) != (3, 336, 336):
            raise _lib.PigeonHipError(f"pixels must be (N,3,336,336), got {tuple(pixels.shape)}")
        if pixels.dtype not in _PIXIN:
            raise _lib.PigeonHipError("pixels must be fp32, fp16 or bf16, or uint8 bytes")
        n = pixels.shape[0]
        need = C.c_size_t()
        check(load().pg_vit_precise_workspace_bytes(self._h, n, C.byref(need)), "pg_vit_precise_workspace_bytes")
        if self._ws_precise is None or self._ws_precise.numel() < need.value + 256:
            self._ws_precise = None
            self._ws_precise = torch.empty(need.value + 256, dtype=torch.uint8, device=f"cuda:{self.device}")
        ws = self._ws_precise
        off = (-ws.data_ptr()) % 256
        if out is not None:
            _dev(out, torch.float32); _shape(out, "out", n, HIDDEN)
        emb = out if out is not None else torch.empty((n, HIDDEN), dtype=torch.float32, device=pixels.device)
        hid = torch.empty((n, TOKENS, HIDDEN), dtype=torch.float32, device=pixels.device) if return_hidden else None
        check(load().pg_vit_forward_precise(self._h, _p(pixels), _PIXIN[pixels.dtype], n, _p(emb), _p(hid),
                                            C.c_void_p(ws.data_ptr() + off), ws.numel() - off, _stream()), "pg_vit_forward_precise")
        return (emb, hid) if return_hidden else emb

    def fingerprint(self):
        """pg_vit_fingerprint -> (int, int): 128 bits over every device buffer the FAST encoder reads (packed 16-bit weights, folded
        column sums and biases, LayerNorm parameters, class and position embeddings) plus layer count, operand dtype and LayerNorm
        fold.  The same with and without `precise`.  The key of a stored calibration (pigeon_amd/certainty.py).  Synchronises."""
        out = (C.c_uint64 * 2)()
        check(load().pg_vit_fingerprint(self._h, out), "pg_vit_fingerprint")
        return int(out[0]), int(out[1])

    def param(self, group: int, slot: int, dtype: torch.dtype = torch.uint8) -> torch.Tensor:
        """pg_vit_param_read (test / debug, not for the hot path): the device buffer (group, slot) of pg_vit_fingerprint's numbering,
        continued by the exact tier's buffers and the normalisation table (include/pigeon_hip.h), as a flat CPU tensor of `dtype`
        (the bytes reinterpreted; empty where this handle has no such buffer).  Synchronous."""
        n = C.c_size_t()
        check(load().pg_vit_param_read(self._h, group, slot, None, 0, C.byref(n)), "pg_vit_param_read")
        out = torch.empty(n.value, dtype=torch.uint8)
        if n.value:
            check(load().pg_vit_param_read(self._h, group, slot, C.c_void_p(out.data_ptr()), n.value, C.byref(n)), "pg_vit_param_read")
        return out.view(dtype)

    def graph(self, on: Optional[bool] = None):
        """Switch the encoder's hipGraph replay on / off (None: query only) -> (replays, captures) since creation."""
        r, c = C.c_int64(), C.c_int64()
        check(load().pg_vit_graph(self._h, -1 if on is None else int(bool(on)), C.byref(r), C.byref(c)), "pg_vit_graph")
        return int(r.value), int(c.value)

    # ---- per-kernel-class timing for bench.py ----
    def profile_enable(self, on: bool = True, classes=None):
        """classes: None = every kernel class, else an iterable of class names (_lib.PROF_CLASSES) to bracket with events."""
        v = 1 if on else 0
        if on and classes is not None:
            v = 0
            for c in classes:
                v |= 1 << (_lib.PROF_CLASSES.index(c) + 1)
        check(load().pg_vit_profile_enable(self._h, v), "pg_vit_profile_enable")

    def profile_reset(self):
        check(load().pg_vit_profile_reset(self._h), "pg_vit_profile_reset")

    def profile_read(self):
        n = len(_lib.PROF_CLASSES)
        launches = (C.c_int64 * n)()
        ms = (C.c_double * n)()
        check(load().pg_vit_profile_read(self._h, launches, ms), "pg_vit_profile_read")
        return {name: (int(launches[i]), float(ms[i])) for i, name in enumerate(_lib.PROF_CLASSES)}

    # ---- fp16 saturation counter (debug) ----
    def saturation_check(self, on: bool = True):
        check(load().pg_vit_saturation_check(self._h, 1 if on else 0), "pg_vit_saturation_check")

    def saturation_read(self, reset: bool = True) -> int:
        """16-bit activations found sitting exactly on the fp16 limit +-65504 (= clamped conversions) since the last reset."""
        n = C.c_int64()
        check(load().pg_vit_saturation_read(self._h, C.byref(n), 1 if reset else 0), "pg_vit_saturation_read")
        return int(n.value)

    def range_alarm_read(self, reset: bool = True) -> int:
        """Rows of the residual stream whose sum of squares reached 65504^2 since the last reset (always-on, fp16 operands):
        0 means no 16-bit copy of a residual row can have been clamped.  Synchronises the device."""
        n = C.c_int64()
        check(load().pg_vit_range_alarm_read(self._h, C.byref(n), 1 if reset else 0), "pg_vit_range_alarm_read")
        return int(n.value)


# ----------------------------------------------------------------------------------------- head
def head_forward(emb: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, centroids: torch.Tensor, k: int):
    """emb (B,P,1024) or (B,1024) fp32; returns dict(logits, topk_values, topk_indices, preds_geocell, preds_LLH)."""
    _dev(emb, torch.float32); _dev(W, torch.float32); _dev(bias, torch.float32); _dev(centroids, torch.float64)
    if emb.dim() not in (2, 3):
        raise _lib.PigeonHipError(f"emb must be (B,{HIDDEN}) or (B,P,{HIDDEN}), got {tuple(emb.shape)}")
    B = emb.shape[0]
    P = emb.shape[1] if emb.dim() == 3 else 1
    _shape(emb, "emb", *((B, P, HIDDEN) if emb.dim() == 3 else (B, HIDDEN)))
    Cn = W.shape[0]
    _shape(W, "W", Cn, HIDDEN); _shape(bias, "bias", Cn); _shape(centroids, "centroids", Cn, 2)
    if not 1 <= int(k) <= Cn:
        raise _lib.PigeonHipError(f"head: k = {k} candidates of {Cn} geocells")
    dev = emb.device
    logits = torch.empty((B, Cn), dtype=torch.float32, device=dev)
    tv = torch.empty((B, k), dtype=torch.float32, device=dev)
    ti = torch.empty((B, k), dtype=torch.int64, device=dev)
    am = torch.empty((B,), dtype=torch.int64, device=dev)
    llh = torch.empty((B, 2), dtype=torch.float64, device=dev)
    check(load().pg_head_forward(_p(emb), B, P, _p(W), _p(bias), _p(centroids), Cn, k, _p(logits), _p(tv), _p(ti),
                                 _p(am), _p(llh), _stream()), "pg_head_forward")
    return dict(logits=logits, topk_values=tv, topk_indices=ti, preds_geocell=am, preds_LLH=llh)


def head_margin(logits: torch.Tensor, emb: torch.Tensor, W: torch.Tensor):
    """Certainty inputs of the top-1 (pg_head_margin): logits (B,C) fp32 as written by head_forward, emb (B,P,1024) or (B,1024),
    W (C,1024).  Returns (margin (B,) fp32 = logit(top1) - logit(top2), sens (B,) fp32 = |mean_p emb| |W[top1] - W[top2]| / 32,
    top2 (B,) int64)."""
    _dev(logits, torch.float32); _dev(emb, torch.float32); _dev(W, torch.float32)
    B, Cn = logits.shape
    P = emb.shape[1] if emb.dim() == 3 else 1
    _shape(emb, "emb", *((B, P, HIDDEN) if emb.dim() == 3 else (B, HIDDEN)))
    _shape(W, "W", Cn, HIDDEN)
    margin = torch.empty((B,), dtype=torch.float32, device=logits.device)
    sens = torch.empty((B,), dtype=torch.float32, device=logits.device)
    top2 = torch.empty((B,), dtype=torch.int64, device=logits.device)
    check(load().pg_head_margin(_p(logits), B, Cn, _p(emb), P, _p(W), _p(margin), _p(sens), _p(top2), _stream()), "pg_head_margin")
    return margin, sens, top2


def head_certainty(logits: torch.Tensor, emb: torch.Tensor, W: torch.Tensor, topk_idx: torch.Tensor,
                   drift: Optional[torch.Tensor], wstats: torch.Tensor):
    """pg_head_certainty: tolerance of the top-1 against every cell.  logits (B,C) as written by head_forward, emb (B,P,1024) or
    (B,1024), topk_idx (B,kx) int64 from the same head_forward call, drift (1024,) fp32 or None, wstats (2,) fp32 = [largest row
    norm of W, max_c |W[c].drift| (0 without drift)].  Returns (tol (B,) f32, code (B,) i32, margin (B,) f32, sens (B,) f32)."""
    _dev(logits, torch.float32); _dev(emb, torch.float32); _dev(W, torch.float32); _dev(topk_idx, torch.int64)
    _dev(wstats, torch.float32)
    B, Cn = logits.shape
    P = emb.shape[1] if emb.dim() == 3 else 1
    _shape(emb, "emb", *((B, P, HIDDEN) if emb.dim() == 3 else (B, HIDDEN)))
    _shape(W, "W", Cn, HIDDEN); _shape(topk_idx, "topk_idx", B, None); _shape(wstats, "wstats", 2)
    kx = topk_idx.shape[1]
    if drift is not None:
        _dev(drift, torch.float32); _shape(drift, "drift", HIDDEN)
    dev = logits.device
    tol = torch.empty((B,), dtype=torch.float32, device=dev)
    code = torch.empty((B,), dtype=torch.int32, device=dev)
    margin = torch.empty((B,), dtype=torch.float32, device=dev)
    sens = torch.empty((B,), dtype=torch.float32, device=dev)
    check(load().pg_head_certainty(_p(logits), B, Cn, _p(emb), P, _p(W), _p(topk_idx), kx, _p(drift), _p(wstats), _p(tol), _p(code),
                                   _p(margin), _p(sens), _stream()), "pg_head_certainty")
    return tol, code, margin, sens


def aux_heads_forward(emb: torch.Tensor, W: torch.Tensor, bias: torch.Tensor, n_reg: int, n_climate: int, n_month: int,
                      drift: Optional[torch.Tensor] = None, row_tol: Optional[torch.Tensor] = None):
    """pg_aux_heads_forward: the auxiliary heads of SuperGuessr(multi_task=True) in one launch.  emb (B,P,1024) or (B,1024) fp32,
    W (A,1024) / bias (A,) fp32 with rows [regression | climate | month], A = n_reg + n_climate + n_month <= 64, drift (1024,) fp32 or
    None, row_tol (B,) fp32 or None: lowered IN PLACE to the minimum of itself and the returned tolerance.  Returns dict(preds (B,A)
    f32, cls (B,2) i64 = [argmax climate, argmax month] (-1: no such classifier), tol (B,) f32, code (B,) i32 = 1 + climate class /
    101 + month class that sets tol, 0 = none)."""
    _dev(emb, torch.float32); _dev(W, torch.float32); _dev(bias, torch.float32)
    if emb.dim() not in (2, 3):
        raise _lib.PigeonHipError(f"emb must be (B,{HIDDEN}) or (B,P,{HIDDEN}), got {tuple(emb.shape)}")
    B = emb.shape[0]
    P = emb.shape[1] if emb.dim() == 3 else 1
    _shape(emb, "emb", *((B, P, HIDDEN) if emb.dim() == 3 else (B, HIDDEN)))
    n_reg, n_climate, n_month = int(n_reg), int(n_climate), int(n_month)
    if min(n_reg, n_climate, n_month) < 0:
        raise _lib.PigeonHipError(f"aux_heads: negative output count (n_reg={n_reg} n_climate={n_climate} n_month={n_month})")
    A = n_reg + n_climate + n_month
    _shape(W, "W", A, HIDDEN); _shape(bias, "bias", A)
    if drift is not None:
        _dev(drift, torch.float32); _shape(drift, "drift", HIDDEN)
    if row_tol is not None:
        _dev(row_tol, torch.float32); _shape(row_tol, "row_tol", B)
    dev = emb.device
    preds = torch.empty((B, A), dtype=torch.float32, device=dev)
    cls = torch.empty((B, 2), dtype=torch.int64, device=dev)
    tol = torch.empty((B,), dtype=torch.float32, device=dev)
    code = torch.empty((B,), dtype=torch.int32, device=dev)
    check(load().pg_aux_heads_forward(_p(emb), B, P, _p(W), _p(bias), n_reg, n_climate, n_month, _p(drift), _p(preds), _p(cls),
                                      _p(tol), _p(code), _p(row_tol), _stream()), "pg_aux_heads_forward")
    return dict(preds=preds, cls=cls, tol=tol, code=code)


def embedding_debias(emb: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """pg_embedding_debias, in place: emb[r] -= |emb[r]| * bias for every row of the (n,1024) fp32 matrix `emb` (contiguous; any
    leading shape).  bias (1024,) fp32: the calibrated systematic part of the 16-bit encoder's error (pigeon_amd/certainty.py)."""
    _dev(emb, torch.float32); _dev(bias, torch.float32); _shape(bias, "bias", HIDDEN)
    if emb.dim() < 1 or emb.shape[-1] != HIDDEN or not emb.is_contiguous():
        raise ValueError(f"embedding_debias: emb must be contiguous (..., {HIDDEN}), got {tuple(emb.shape)}")
    n = emb.numel() // HIDDEN
    check(load().pg_embedding_debias(_p(emb), n, HIDDEN, _p(bias), _stream()), "pg_embedding_debias")
    return emb


def _arg(t, name: str, dtype: torch.dtype) -> torch.Tensor:
    """A contiguous device tensor of `dtype`, or a PigeonHipError that names the argument."""
    if not torch.is_tensor(t):
        raise _lib.PigeonHipError(f"{name} must be a tensor, got {type(t).__name__}")
    if not t.is_cuda:
        raise _lib.PigeonHipError(f"{name} must be a device tensor, got one on {t.device}")
    if t.dtype != dtype:
        raise _lib.PigeonHipError(f"{name} must have dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise _lib.PigeonHipError(f"{name} must be contiguous, got strides {tuple(t.stride())} for shape {tuple(t.shape)}")
    return t


def token_attribution(hidden: torch.Tensor, W: torch.Tensor, cells: torch.Tensor, against: Optional[torch.Tensor] = None,
                      panels: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pg_token_attribution: each of K head directions as a sum over tokens.  hidden (n,577,1024) fp32 (last_hidden_state of
    n = B * panels images), W (C,1024) fp32, cells (B,K) int64 with 1 <= K <= 16, against (B,) int64 or None (an entry of -1: none).
    Returns maps (B,panels,577,K) fp32:  maps[b,p,t,k] = hidden[b*panels+p,t] . (W[cells[b,k]] - W[against[b]]) / (577 panels), so
    that maps.sum((1,2)) is the token part of logit[cells[b,k]] - logit[against[b]] of the mean-pooled linear head.  An index outside
    [0, C) makes its column (cells) or its sample (against) NaN; it is never dereferenced.  All tensors on the device.  `out`
    (B,panels,577,K) fp32: write there instead of a fresh tensor."""
    _arg(hidden, "hidden", torch.float32); _arg(W, "W", torch.float32); _arg(cells, "cells", torch.int64)
    if hidden.dim() != 3 or tuple(hidden.shape[1:]) != (TOKENS, HIDDEN):
        raise _lib.PigeonHipError(f"hidden must have shape (*,{TOKENS},{HIDDEN}), got {tuple(hidden.shape)}")
    _shape(W, "W", None, HIDDEN)
    n, P, Cn = int(hidden.shape[0]), int(panels), int(W.shape[0])
    if P < 1 or n % P != 0:
        raise _lib.PigeonHipError(f"panels = {panels}: hidden holds {n} images, not a multiple of it (PG_EINVAL)")
    if Cn < 1:
        raise _lib.PigeonHipError("W must have at least one row (PG_EINVAL)")
    B = n // P
    _shape(cells, "cells", B, None)
    K = int(cells.shape[1])
    if not 1 <= K <= 16:
        raise _lib.PigeonHipError(f"cells must have 1..16 columns (K), got {K} (PG_EINVAL)")
    if against is not None:
        _arg(against, "against", torch.int64); _shape(against, "against", B)
    if out is None:
        out = torch.empty((B, P, TOKENS, K), dtype=torch.float32, device=hidden.device)
    _arg(out, "out", torch.float32); _shape(out, "out", B, P, TOKENS, K)
    for name, t in (("W", W), ("cells", cells), ("against", against), ("out", out)):
        if t is not None and t.device != hidden.device:
            raise _lib.PigeonHipError(f"{name} is on {t.device}, hidden on {hidden.device}")
    with torch.cuda.device(hidden.device):
        check(load().pg_token_attribution(_p(hidden), n, P, _p(W), Cn, _p(cells), _p(against), K, _p(out), _stream()),
              "pg_token_attribution")
    return out


def fingerprint(t: torch.Tensor, seed: int = 0):
    """pg_fingerprint -> (int, int): the 128-bit digest (csrc/fingerprint.hip) of the bytes of the contiguous device tensor `t`, which
    must start on a 16-byte boundary (PigeonHipError otherwise).  Synchronises the current stream: the result is a host value."""
    _dev(t)
    out = (C.c_uint64 * 2)()
    with torch.cuda.device(t.device):
        check(load().pg_fingerprint(_p(t), t.numel() * t.element_size(), C.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), out, _stream()),
              "pg_fingerprint")
    return int(out[0]), int(out[1])


# ----------------------------------------------------------------------------------------- deferred exact tier (csrc/requeue.hip)
def head_wstats(W: torch.Tensor, drift: Optional[torch.Tensor]) -> torch.Tensor:
    """pg_head_wstats: (2,) fp32 = [largest row norm of W, max over cells of |W[c].drift| (0 without drift)]."""
    _dev(W, torch.float32); _shape(W, "W", None, HIDDEN)
    if drift is not None:
        _dev(drift, torch.float32); _shape(drift, "drift", HIDDEN)
    out = torch.empty((2,), dtype=torch.float32, device=W.device)
    check(load().pg_head_wstats(_p(W), W.shape[0], _p(drift), _p(out), _stream()), "pg_head_wstats")
    return out


def requeue_append(head_tol: torch.Tensor, refine_tol: Optional[torch.Tensor], refine_code: Optional[torch.Tensor], thr: float,
                   force_all: bool = False, dst_base: int = 0, flushed: int = 0, cap: int = 0,
                   counters: Optional[torch.Tensor] = None, slot_dst: Optional[torch.Tensor] = None):
    """pg_requeue_append.  Returns (certain (B,) uint8, cause (B,) int32, row_slot (B,) int32 or None without a queue)."""
    _dev(head_tol, torch.float32)
    B = head_tol.numel()
    if refine_tol is not None:
        _dev(refine_tol, torch.float32); _shape(refine_tol, "refine_tol", B)
    if refine_code is not None:
        _dev(refine_code, torch.int32); _shape(refine_code, "refine_code", B)
    dev = head_tol.device
    certain = torch.empty((B,), dtype=torch.uint8, device=dev)
    cause = torch.empty((B,), dtype=torch.int32, device=dev)
    row_slot = None
    if cap > 0:
        _dev(counters, torch.int64); _shape(counters, "counters", 2)
        _dev(slot_dst, torch.int64); _shape(slot_dst, "slot_dst", cap)
        row_slot = torch.empty((B,), dtype=torch.int32, device=dev)
    check(load().pg_requeue_append(_p(head_tol), _p(refine_tol), _p(refine_code), B, float(thr), 1 if force_all else 0, int(dst_base),
                                   int(flushed), int(cap), _p(counters), _p(slot_dst), _p(row_slot), _p(certain), _p(cause), _stream()),
          "pg_requeue_append")
    return certain, cause, row_slot


def rows_to_slots(src: torch.Tensor, row_slot: torch.Tensor, dst: torch.Tensor) -> None:
    """pg_rows_to_slots: dst[row_slot[r]] = src[r] for the rows with a slot; src (B, ...) and dst (cap, ...) share the row shape."""
    _dev(src); _dev(dst); _dev(row_slot, torch.int32)
    if src.dtype != dst.dtype or tuple(src.shape[1:]) != tuple(dst.shape[1:]):
        raise _lib.PigeonHipError(f"rows_to_slots: rows of {src.dtype} {tuple(src.shape[1:])} into {dst.dtype} {tuple(dst.shape[1:])}")
    B = src.shape[0]
    _shape(row_slot, "row_slot", B)
    rb = (src.numel() // max(B, 1)) * src.element_size()
    check(load().pg_rows_to_slots(_p(src), rb, _p(row_slot), B, _p(dst), _stream()), "pg_rows_to_slots")


def requeue_take(slot_dst: torch.Tensor, head: int, n_valid: int, n_pad: int) -> torch.Tensor:
    """pg_requeue_take -> (n_pad,) int64 ring rows of the slots [head, head + n_pad) (mod cap), -1 beyond the first n_valid."""
    _dev(slot_dst, torch.int64)
    out = torch.empty((n_pad,), dtype=torch.int64, device=slot_dst.device)
    check(load().pg_requeue_take(_p(slot_dst), slot_dst.numel(), int(head), int(n_valid), int(n_pad), _p(out), _stream()), "pg_requeue_take")
    return out


def scatter_rows(src: torch.Tensor, dst_row: torch.Tensor, dst: torch.Tensor, remap=None) -> None:
    """pg_scatter_rows: dst[dst_row[i]] = src[i] (dst_row[i] < 0: skipped).  remap = (wb, b, off): dst_row addresses the gathered ring,
    dst is a local-only array (see include/pigeon_hip.h)."""
    _dev(src); _dev(dst); _dev(dst_row, torch.int64)
    n = src.shape[0]
    _shape(dst_row, "dst_row", n)
    if src.dtype != dst.dtype or tuple(src.shape[1:]) != tuple(dst.shape[1:]):
        raise _lib.PigeonHipError(f"scatter_rows: rows of {src.dtype} {tuple(src.shape[1:])} into {dst.dtype} {tuple(dst.shape[1:])}")
    rb = 1
    for d in src.shape[1:]:
        rb *= int(d)
    rb *= src.element_size()
    wb, b, off = remap if remap is not None else (0, 0, 0)
    check(load().pg_scatter_rows(_p(src), rb, _p(dst_row), n, _p(dst), dst.shape[0], int(wb), int(b), int(off), _stream()), "pg_scatter_rows")


# ----------------------------------------------------------------------------------------- exact-mode building blocks
def x3_split(x: torch.Tensor, gelu: bool = False) -> torch.Tensor:
    """fp32 (rows,cols) -> fp16 triple (rows, 3 cols) = [hi | lo | hi 2^-8]; gelu: through QuickGELU first."""
    _dev(x, torch.float32)
    rows, cols = x.shape
    y = torch.empty((rows, 3 * cols), dtype=torch.float16, device=x.device)
    check(load().pg_op_x3_split(_p(x), _p(y), rows, cols, 1 if gelu else 0, _stream()), "pg_op_x3_split")
    return y


def gemm16_parts(A: torch.Tensor, W: torch.Tensor, bias: Optional[torch.Tensor], S: int) -> torch.Tensor:
    """pg_op_gemm16_parts: A (M, S*Kp), W (N, S*Kp) 16-bit -> (S, M, N) fp32, part p = A[:, p Kp:(p+1) Kp] x W[:, p Kp:(p+1) Kp]^T
    (+ bias for p = 0), all parts in one persistent launch."""
    _dev(A); _dev(W)
    if W.dtype != A.dtype or A.shape[1] != W.shape[1] or A.shape[1] % S:
        raise _lib.PigeonHipError("gemm16_parts: A and W must share dtype and a K' divisible by S")
    M, Kt = A.shape
    N = W.shape[0]
    out = torch.empty((S, M, N), dtype=torch.float32, device=A.device)
    check(load().pg_op_gemm16_parts(_dt16(A), _p(A), A.stride(0), _p(W), W.stride(0), _p(bias), _p(out), M, N, Kt // S, S, _stream()),
          "pg_op_gemm16_parts")
    return out


def x3_layernorm(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5) -> torch.Tensor:
    _dev(x, torch.float32)
    rows = x.numel() // HIDDEN
    y = torch.empty((rows, 3 * HIDDEN), dtype=torch.float16, device=x.device)
    check(load().pg_op_x3_layernorm(_p(x), _p(gamma), _p(beta), _p(y), rows, float(eps), _stream()), "pg_op_x3_layernorm")
    return y


def x3_pack_weight(W: torch.Tensor) -> torch.Tensor:
    """Host-side mirror of the library's weight triple (vit_weights.hip pack_x3), for the building-block tests: W fp32 (N,K) ->
    fp16 (N,3K) = [Wh | Wh | (W - Wh) 2^8], both conversions saturating at +-65504 as the library's (tests/test_gpu_weights.py holds
    the two equal bit for bit)."""
    Wh = W.clamp(-65504.0, 65504.0).to(torch.float16)
    Wl = ((W - Wh.float()) * 256.0).clamp(-65504.0, 65504.0).to(torch.float16)
    return torch.cat([Wh, Wh, Wl], dim=1).contiguous()


def attention_f32(qkv: torch.Tensor, n_images: int) -> torch.Tensor:
    _dev(qkv, torch.float32)
    _shape(qkv, "qkv", n_images * TOKENS, 3 * HIDDEN)
    out = torch.empty((n_images * TOKENS, HIDDEN), dtype=torch.float32, device=qkv.device)
    check(load().pg_op_attention_f32(_p(qkv), _p(out), n_images, _stream()), "pg_op_attention_f32")
    return out


# ----------------------------------------------------------------------------------------- refiner
class DeviceBank:
    """CSR prototype bank resident in HBM (see include/pigeon_hip.h pg_bank)."""

    FIELDS = [("proto_emb", torch.float32), ("cell_off", torch.int64), ("proto_lnglat", torch.float32),
              ("proto_count", torch.int32), ("member_off", torch.int64), ("member_idx", torch.int64),
              ("train_emb", torch.float32), ("train_lnglat", torch.float32)]

    def __init__(self, arrays, device="cuda"):
        self.t = {}
        for name, dt in self.FIELDS:
            a = getattr(arrays, name) if not isinstance(arrays, dict) else arrays[name]
            t = torch.as_tensor(a) if not torch.is_tensor(a) else a
            self.t[name] = t.to(device=device, dtype=dt).contiguous()
        self.num_cells = self.t["cell_off"].numel() - 1
        self.num_protos = self.t["proto_emb"].shape[0]
        self.num_train = self.t["train_emb"].shape[0]
        t = self.t                                            # the CSR arrays must fit each other: the kernels index by them
        _shape(t["proto_emb"], "proto_emb", self.num_protos, HIDDEN); _shape(t["proto_lnglat"], "proto_lnglat", self.num_protos, 2)
        _shape(t["proto_count"], "proto_count", self.num_protos); _shape(t["member_off"], "member_off", self.num_protos + 1)
        _shape(t["cell_off"], "cell_off", self.num_cells + 1); _shape(t["member_idx"], "member_idx", None)
        _shape(t["train_emb"], "train_emb", self.num_train, HIDDEN); _shape(t["train_lnglat"], "train_lnglat", self.num_train, 2)
        self.struct = Bank(*[C.c_void_p(self.t[n].data_ptr()) for n, _ in self.FIELDS],
                           self.num_cells, self.num_protos, self.num_train)


def refine_forward(bank: DeviceBank, q: torch.Tensor, init_llh: torch.Tensor, cand: torch.Tensor,
                   cand_prob: Optional[torch.Tensor], topk: int, temperature: float, max_refine_km: float,
                   return_scratch: bool = False):
    """Returns (preds_LLH (B,2) f32, preds_geocell (B,) i64, choice (B,) i32) [, scratch (B,topk,4) f32 =
    (score, lng, lat, bank rows streamed) per (query, candidate)]."""
    _dev(q, torch.float32); _dev(init_llh, torch.float64); _dev(cand, torch.int64)
    if cand_prob is not None:
        _dev(cand_prob, torch.float32)
    if q.dim() not in (2, 3) or cand.dim() != 2:
        raise _lib.PigeonHipError(f"refine: q must be (B,{HIDDEN}) or (B,P,{HIDDEN}) and cand (B,k), got {tuple(q.shape)} / {tuple(cand.shape)}")
    B = q.shape[0]
    P = q.shape[1] if q.dim() == 3 else 1
    k = cand.shape[1]
    _shape(q, "q", *((B, P, HIDDEN) if q.dim() == 3 else (B, HIDDEN)))
    _shape(init_llh, "init_llh", B, 2); _shape(cand, "cand", B, k)
    if cand_prob is not None:
        _shape(cand_prob, "cand_prob", B, k)
    if not 1 <= int(topk) <= k:
        raise _lib.PigeonHipError(f"refine: topk = {topk} of k = {k} candidates")
    dev = q.device
    scratch = torch.empty((B, topk, 4), dtype=torch.float32, device=dev)
    out_llh = torch.empty((B, 2), dtype=torch.float32, device=dev)
    out_cell = torch.empty((B,), dtype=torch.int64, device=dev)
    out_choice = torch.empty((B,), dtype=torch.int32, device=dev)
    check(load().pg_refine_forward(C.byref(bank.struct), _p(q), B, P, _p(init_llh), _p(cand), _p(cand_prob), k, topk,
                                   float(temperature), float(max_refine_km), _p(scratch), _p(out_llh), _p(out_cell),
                                   _p(out_choice), _stream()), "pg_refine_forward")
    if return_scratch:
        return out_llh, out_cell, out_choice, scratch
    return out_llh, out_cell, out_choice


def refine_forward_ex(bank: DeviceBank, q: torch.Tensor, init_llh: torch.Tensor, cand: torch.Tensor,
                      cand_prob: Optional[torch.Tensor], topk: int, n_eval: int, temperature: float, max_refine_km: float):
    """pg_refine_forward_ex: refine_forward's selection over the first `topk` candidates, with `n_eval` >= topk candidates evaluated and
    the 12-float records pg_refine_certainty needs.  Returns (preds_LLH, preds_geocell, choice, refined, scratch12 (B,n_eval,12))."""
    _dev(q, torch.float32); _dev(init_llh, torch.float64); _dev(cand, torch.int64)
    if cand_prob is not None:
        _dev(cand_prob, torch.float32)
    if q.dim() not in (2, 3) or cand.dim() != 2:
        raise _lib.PigeonHipError(f"refine: q must be (B,{HIDDEN}) or (B,P,{HIDDEN}) and cand (B,k), got {tuple(q.shape)} / {tuple(cand.shape)}")
    B = q.shape[0]
    P = q.shape[1] if q.dim() == 3 else 1
    k = cand.shape[1]
    _shape(q, "q", *((B, P, HIDDEN) if q.dim() == 3 else (B, HIDDEN)))
    _shape(init_llh, "init_llh", B, 2); _shape(cand, "cand", B, k)
    if cand_prob is not None:
        _shape(cand_prob, "cand_prob", B, k)
    if not 1 <= int(topk) <= int(n_eval) <= k:
        raise _lib.PigeonHipError(f"refine_ex: topk = {topk}, n_eval = {n_eval} of k = {k} candidates")
    dev = q.device
    scratch = torch.empty((B, n_eval, 12), dtype=torch.float32, device=dev)
    out_llh = torch.empty((B, 2), dtype=torch.float32, device=dev)
    out_cell = torch.empty((B,), dtype=torch.int64, device=dev)
    out_choice = torch.empty((B,), dtype=torch.int32, device=dev)
    out_refined = torch.empty((B,), dtype=torch.int32, device=dev)
    check(load().pg_refine_forward_ex(C.byref(bank.struct), _p(q), B, P, _p(init_llh), _p(cand), _p(cand_prob), k, int(topk), int(n_eval),
                                      float(temperature), float(max_refine_km), _p(scratch), _p(out_llh), _p(out_cell),
                                      _p(out_choice), _p(out_refined), _stream()), "pg_refine_forward_ex")
    return out_llh, out_cell, out_choice, out_refined, scratch


def refine_certainty(bank: DeviceBank, q: torch.Tensor, cand: torch.Tensor, cand_prob: Optional[torch.Tensor], topk: int,
                     scratch12: torch.Tensor, W: torch.Tensor, drift: Optional[torch.Tensor], wstats: torch.Tensor,
                     temperature: float, refined: torch.Tensor, choice: torch.Tensor, bank_sigma: float = 0.0):
    """pg_refine_certainty over the records refine_forward_ex left.  Returns (tol (B,) f32, code (B,) i32).
    bank_sigma = kappa x the relative error the bank's rows carry (0: an exact bank, pg_refine_certainty as before; > 0:
    pg_refine_certainty_bank, same meaning of tol and code)."""
    bank_sigma = float(bank_sigma)
    if not (0.0 <= bank_sigma < float("inf")):
        raise _lib.PigeonHipError(f"refine_certainty: bank_sigma = {bank_sigma!r} (must be finite and >= 0)")
    _dev(q, torch.float32); _dev(cand, torch.int64); _dev(scratch12, torch.float32); _dev(W, torch.float32)
    _dev(wstats, torch.float32); _dev(refined, torch.int32); _dev(choice, torch.int32)
    B = q.shape[0]
    P = q.shape[1] if q.dim() == 3 else 1
    k = cand.shape[1]
    n_eval = scratch12.shape[1]
    _shape(q, "q", *((B, P, HIDDEN) if q.dim() == 3 else (B, HIDDEN)))
    _shape(cand, "cand", B, k); _shape(scratch12, "scratch12", B, n_eval, 12); _shape(W, "W", None, HIDDEN)
    _shape(refined, "refined", B); _shape(choice, "choice", B); _shape(wstats, "wstats", 2)
    if cand_prob is not None:
        _dev(cand_prob, torch.float32); _shape(cand_prob, "cand_prob", B, k)
    if drift is not None:
        _dev(drift, torch.float32); _shape(drift, "drift", HIDDEN)
    tol = torch.empty((B,), dtype=torch.float32, device=q.device)
    code = torch.empty((B,), dtype=torch.int32, device=q.device)
    args = (C.byref(bank.struct), _p(q), B, P, _p(cand), _p(cand_prob), k, int(topk), int(n_eval), _p(scratch12), _p(W), W.shape[0],
            _p(drift), _p(wstats), float(temperature), _p(refined), _p(choice), _p(tol), _p(code))
    if bank_sigma == 0.0:
        check(load().pg_refine_certainty(*args, _stream()), "pg_refine_certainty")
    else:
        check(load().pg_refine_certainty_bank(*args, bank_sigma, _stream()), "pg_refine_certainty_bank")
    return tol, code


# ----------------------------------------------------------------------------------------- refiner grid sweep (csrc/refine_sweep.hip)
SWEEP_CHOICE_BYTES = 256 << 20                       # refine_sweep keeps a chunk's choice bytes under this


def _sweep_grid(topks, temps, max_kms):
    ks = [int(v) for v in topks]
    ts = [float(v) for v in temps]
    rs = [float(v) for v in max_kms]
    return ks, ts, rs, (C.c_int32 * max(len(ks), 1))(*ks), (C.c_float * max(len(ts), 1))(*ts), (C.c_double * max(len(rs), 1))(*rs)


def refine_sweep_choice(scratch: torch.Tensor, cand_prob: Optional[torch.Tensor], init_llh: torch.Tensor, topks, temps, max_kms,
                        veto_km: bool = False, out: Optional[torch.Tensor] = None):
    """pg_refine_sweep: the selection of refine_forward at every point of the grid topks x temps x max_kms (host sequences), from the
    records `scratch` (B,n_eval,4 or 12) fp32 that refine_forward / refine_forward_ex left.  cand_prob (B,k) fp32 or None, init_llh
    (B,2) fp64.  Returns choice (G,B) uint8 with g = (iK * nT + iT) * nR + iR: the candidate in bits 0-5, bit 7 = the veto fired;
    with veto_km=True also the (B,n_eval) fp64 veto distances.  A temperature is the float32 the kernel sees.  No host synchronisation."""
    _arg(scratch, "scratch", torch.float32); _arg(init_llh, "init_llh", torch.float64)
    if scratch.dim() != 3 or scratch.shape[2] not in (4, 12):
        raise _lib.PigeonHipError(f"scratch must have shape (B,n_eval,4) or (B,n_eval,12), got {tuple(scratch.shape)}")
    B, n_eval, SC = (int(v) for v in scratch.shape)
    _shape(init_llh, "init_llh", B, 2)
    k = 0
    if cand_prob is not None:
        _arg(cand_prob, "cand_prob", torch.float32); _shape(cand_prob, "cand_prob", B, None)
        k = int(cand_prob.shape[1])
    ks, ts, rs, ka, ta, ra = _sweep_grid(topks, temps, max_kms)
    G = len(ks) * len(ts) * len(rs)
    if out is None:
        out = torch.empty((G, B), dtype=torch.uint8, device=scratch.device)
    _arg(out, "out", torch.uint8); _shape(out, "out", G, B)
    vk = torch.empty((B, n_eval), dtype=torch.float64, device=scratch.device) if veto_km else None
    for name, t in (("cand_prob", cand_prob), ("init_llh", init_llh), ("out", out)):
        if t is not None and t.device != scratch.device:
            raise _lib.PigeonHipError(f"refine_sweep: {name} is on {t.device}, scratch on {scratch.device}")
    with torch.cuda.device(scratch.device):
        check(load().pg_refine_sweep(_p(scratch), SC, B, n_eval, _p(cand_prob), k, _p(init_llh), ka, len(ks), ta, len(ts), ra, len(rs),
                                     _p(out), _p(vk), _stream()), "pg_refine_sweep")
    return (out, vk) if veto_km else out


def refine_sweep_totals(choice: torch.Tensor, values: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pg_refine_sweep_totals: choice (G,B) uint8, values (B,n_eval,V) fp64 with V 1 .. 16 -> (G,V+2) fp64: per grid point the sum over
    rows of the chosen candidate's values, the rows whose choice is not candidate 0 and the vetoed rows.  No host synchronisation."""
    _arg(choice, "choice", torch.uint8); _arg(values, "values", torch.float64)
    _shape(choice, "choice", None, None)
    G, B = int(choice.shape[0]), int(choice.shape[1])
    _shape(values, "values", B, None, None)
    n_eval, V = int(values.shape[1]), int(values.shape[2])
    if out is None:
        out = torch.empty((G, V + 2), dtype=torch.float64, device=choice.device)
    _arg(out, "out", torch.float64); _shape(out, "out", G, V + 2)
    if values.device != choice.device or out.device != choice.device:
        raise _lib.PigeonHipError(f"refine_sweep_totals: values on {values.device}, out on {out.device}, choice on {choice.device}")
    with torch.cuda.device(choice.device):
        check(load().pg_refine_sweep_totals(_p(choice), G, B, n_eval, _p(values), V, _p(out), _stream()), "pg_refine_sweep_totals")
    return out


def refine_sweep_plan(B: int, n_eval: int, G: int, V: int) -> dict:
    """pg_refine_sweep_plan: what the sweep does with B rows, n_eval candidates, G grid points and V columns (host arithmetic, no GPU)."""
    o = (C.c_int64 * 4)()
    check(load().pg_refine_sweep_plan(int(B), int(n_eval), int(G), int(V), o), "pg_refine_sweep_plan")
    return {"rows_per_workgroup": int(o[0]), "lds_bytes": int(o[1]), "row_groups": int(o[2]), "choice_bytes": int(o[3])}


def refine_sweep(scratch: torch.Tensor, cand_prob: Optional[torch.Tensor], init_llh: torch.Tensor, values: torch.Tensor, topks, temps,
                 max_kms, max_choice_bytes: int = SWEEP_CHOICE_BYTES) -> torch.Tensor:
    """The totals (G,V+2) fp64 of every grid point over all B rows: refine_sweep_choice + refine_sweep_totals over chunks of rows, a
    multiple of the workgroup's rows each, sized so that a chunk's G x rows choice bytes stay under `max_choice_bytes`; the chunks'
    totals are added in chunk order in fp64.  No host synchronisation."""
    B, n_eval = int(scratch.shape[0]), int(scratch.shape[1])
    ks, ts, rs = list(topks), list(temps), list(max_kms)
    G = len(ks) * len(ts) * len(rs)
    V = int(values.shape[2]) if values.dim() == 3 else 0
    if B == 0 or G == 0:
        return refine_sweep_totals(refine_sweep_choice(scratch, cand_prob, init_llh, ks, ts, rs), values)
    unit = refine_sweep_plan(B, n_eval, G, V)["rows_per_workgroup"]
    rows = max(unit, (int(max_choice_bytes) // G) // unit * unit)
    total = None
    for s in range(0, B, rows):
        e = min(B, s + rows)
        ch = refine_sweep_choice(scratch[s:e], None if cand_prob is None else cand_prob[s:e], init_llh[s:e], ks, ts, rs)
        part = refine_sweep_totals(ch, values[s:e])
        total = part if total is None else total + part
        del ch
    return total


def tune_gemm_raster(gn: int) -> None:
    """pg_tune_gemm_raster: N tiles per raster group of the 384 x 256 GEMM (0 default, -1 all).  Timing only."""
    check(load().pg_tune_gemm_raster(int(gn)), "pg_tune_gemm_raster")


def tune_exact_fusion(on: bool) -> None:
    """pg_tune_exact_fusion: the exact pass's activation splits inside their producers (default on).  Bit-identical either way."""
    check(load().pg_tune_exact_fusion(1 if on else 0), "pg_tune_exact_fusion")


def tune_gemm_mid(on) -> None:
    """pg_tune_gemm_mid: the routing of GEMM launches of up to ~64 images between the 384 x 256 / 256 x 256 persistent kernels and the
    128 x 128 small-batch kernel (True / 1: on, the default; False / 0: a variant means its own kernel; 2: only the 128 x 128 kernel
    as an alternative -- the A/B arm).  Timing only: all kernels give the same bits for a row."""
    mode = 2 if (not isinstance(on, bool) and on == 2) else (1 if on else 0)
    check(load().pg_tune_gemm_mid(mode), "pg_tune_gemm_mid")


# ----------------------------------------------------------------------------------------- exact-mode plan and the blocks it is made of
def vit_precise_plan(n_images: int) -> dict:
    """pg_vit_precise_plan: what forward_precise does with a batch of n_images under the current knobs (host arithmetic, no GPU)."""
    out = (C.c_int32 * 8)()
    check(load().pg_vit_precise_plan(int(n_images), out), "pg_vit_precise_plan")
    return dict(qkv=out[0], out=out[1], fc1=out[2], fc2=out[3], fc1_fused=bool(out[4]), attn_x3=bool(out[5]), chunk=out[6], chunks=out[7])


def tune_exact_products(n: int) -> None:
    """pg_tune_exact_products: 3 (the exact tier) or 2 partial products per weight GEMM of the exact pass."""
    check(load().pg_tune_exact_products(int(n)), "pg_tune_exact_products")


def x3_im2col(pixels: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pixels (n,3,336,336) fp32 / fp16 / bf16 -> the patch matrix's fp16 triple (n*576, 3*640)."""
    _dev(pixels); _shape(pixels, "pixels", None, 3, 336, 336)
    n = pixels.shape[0]
    if out is None:
        out = torch.empty((n * PATCHES, 3 * KPAD), dtype=torch.float16, device=pixels.device)
    _dev(out, torch.float16)
    if out.numel() < n * PATCHES * 3 * KPAD:
        raise _lib.PigeonHipError("x3_im2col: output too small")
    check(load().pg_op_x3_im2col(_p(pixels), _PIXIN[pixels.dtype], _p(out), n, _stream()), "pg_op_x3_im2col")
    return out


def sum_parts(parts: torch.Tensor, dst: torch.Tensor, resid: bool, n: Optional[int] = None) -> torch.Tensor:
    """pg_op_sum_parts: parts (S, part_elems) fp32; dst[:n] = (resid ? dst[:n] : 0) + ((p0 + p1) + p2 ...), in place on dst."""
    _dev(parts, torch.float32); _dev(dst, torch.float32)
    S, pe = parts.shape[0], parts[0].numel()
    n = pe if n is None else int(n)
    if dst.numel() < n:
        raise _lib.PigeonHipError("sum_parts: dst too small")
    check(load().pg_op_sum_parts(_p(parts), S, pe, _p(dst), n, 1 if resid else 0, _stream()), "pg_op_sum_parts")
    return dst


def preln(x: torch.Tensor, cls: torch.Tensor, pos0: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, rows: Optional[int] = None,
          eps: float = 1e-5, stat_dtype: Optional[torch.dtype] = None, x16: Optional[torch.Tensor] = None,
          rowstat: Optional[torch.Tensor] = None):
    """pg_op_preln in place on x (>= rows, 1024) fp32.  stat_dtype (or x16 / rowstat buffers): also -> (x16, rowstat)."""
    _dev(x, torch.float32)
    for t in (cls, pos0, gamma, beta):
        _dev(t, torch.float32)
        if t.numel() < HIDDEN:
            raise _lib.PigeonHipError("preln: parameter vectors need 1024 elements")
    rows = x.numel() // HIDDEN if rows is None else int(rows)
    if x.numel() < rows * HIDDEN:
        raise _lib.PigeonHipError("preln: x too small")
    if stat_dtype is not None and x16 is None:
        x16 = torch.empty((rows, HIDDEN), dtype=stat_dtype, device=x.device)
        rowstat = torch.empty((rows, 2), dtype=torch.float32, device=x.device)
    if x16 is not None and (x16.numel() < rows * HIDDEN or rowstat.numel() < rows * 2):
        raise _lib.PigeonHipError("preln: x16 / rowstat too small")
    check(load().pg_op_preln(_p(x), _p(cls), _p(pos0), _p(gamma), _p(beta), rows, float(eps), _p(x16),
                             _dt16(x16) if x16 is not None else 0, _p(rowstat), _stream()), "pg_op_preln")
    return (x16, rowstat) if x16 is not None else None


def attention_x3(qkv: torch.Tensor, n_images: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """pg_op_attention_x3: fp32 QKV (n*577, 3072) -> the fp16 triple (n*577, 3072) of softmax(q k^T / 8) v."""
    _dev(qkv, torch.float32)
    _shape(qkv, "qkv", n_images * TOKENS, 3 * HIDDEN)
    if out is None:
        out = torch.empty((n_images * TOKENS, 3 * HIDDEN), dtype=torch.float16, device=qkv.device)
    _dev(out, torch.float16)
    if out.numel() < n_images * TOKENS * 3 * HIDDEN:
        raise _lib.PigeonHipError("attention_x3: output too small")
    check(load().pg_op_attention_x3(_p(qkv), _p(out), n_images, _stream()), "pg_op_attention_x3")
    return out
