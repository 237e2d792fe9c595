"""Exact-input references for the GEMM epilogues and the attention kernels (helper module: no tests, no fixtures).

An fp32 accumulator is exact, in ANY summation order and whatever the matrix pipe does internally, when every operand is a small
integer and every partial sum stays below 2^24.  With such inputs the value an epilogue has to write is known exactly, so the
comparison is an equality against an fp64 computation at any shape -- a dropped K slab, a tile written to the wrong rows, a bias taken
from the neighbouring column tile each change an integer.

The fp64 restatements below are written from the definitions in include/pigeon_hip.h ("Building-block ops") and from
modeling_clip's QuickGELU (x * sigmoid(1.702 x)), not from the kernels' sources.  Everything is torch on whatever device the case
lives on (the fp64 matmul runs in row chunks, on the GPU through torch.float64 when the case is there: a different implementation from
the kernels under test).

A GEMM "case" is a GemmCase; `outputs` are the buffers a kernel (or an emulation of one) wrote, INCLUDING their guard rows, which were
pre-filled with SENTINEL and must still hold it.  compare_gemm returns a list of human-readable findings (empty = equal)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, List, Optional

import torch

EPI_QKV, EPI_GELU, EPI_RESID, EPI_PATCH, EPI_F32, EPI_RESID_STAT, EPI_QKV_LN, EPI_GELU_LN, EPI_GELU_X3 = range(9)
EPI_NAMES = ("QKV", "GELU", "RESID", "PATCH", "F32", "RESID_STAT", "QKV_LN", "GELU_LN", "GELU_X3")
TOKENS, PATCHES, HEADS, HDIM, HIDDEN = 577, 576, 16, 64, 1024
SENTINEL = 7.0            # guard rows (and PATCH's class-token rows) are pre-filled with it; no exact-input result is checked against it
GUARD_ROWS = 389          # >= 384: the fp32 residual epilogues may READ up to 383 rows past row M (pigeon_hip.h, memory contract)
U32 = 2.0 ** -24          # unit roundoff of fp32
_SIG16 = {torch.float16: 11, torch.bfloat16: 8}      # significand bits (with the hidden one)


# ================================================================================================================ GEMM cases
@dataclass
class GemmCase:
    epi: int
    M: int                # rows of A (PATCH: images * 576)
    N: int
    K: int
    dtype: torch.dtype    # 16-bit operand type
    A: torch.Tensor       # (M, K)
    W: torch.Tensor       # (N, K)
    bias: Optional[torch.Tensor] = None      # (N,) fp32
    qscale: float = 1.0
    qcols: int = 0
    pos: Optional[torch.Tensor] = None       # (577, N) fp32            PATCH
    X0: Optional[torch.Tensor] = None        # (M, N) fp32              RESID / RESID_STAT: the residual stream before the call
    rowstat: Optional[torch.Tensor] = None   # (M, 2) fp32 (rstd, mean * rstd)   *_LN
    colsum: Optional[torch.Tensor] = None    # (N,) fp32                *_LN
    exact_inputs: bool = True

    @property
    def out_rows(self) -> int:
        if self.epi != EPI_PATCH:
            return self.M
        return (self.M - 1) // PATCHES * TOKENS + 1 + (self.M - 1) % PATCHES + 1      # the last patch row's token row, + 1

    @property
    def out_cols(self) -> int:
        return 3 * self.N if self.epi == EPI_GELU_X3 else self.N

    @property
    def out_dtype(self) -> torch.dtype:
        if self.epi in (EPI_RESID, EPI_PATCH, EPI_F32, EPI_RESID_STAT):
            return torch.float32
        return torch.float16 if self.epi == EPI_GELU_X3 else self.dtype


def _randint(lo, hi, shape, gen, device):
    return torch.randint(lo, hi + 1, shape, generator=gen, device=device, dtype=torch.int16)


def make_exact_gemm_case(epi: int, M: int, N: int, K: int, dtype: torch.dtype, seed: int, device="cpu") -> GemmCase:
    """Integer inputs for which every epilogue's pre-rounding value is exact in fp32, in any order and with or without FMA contraction.

    A, W integer in [-3, 3] (exact in fp16 and bf16): |acc| <= 9 K.  bias, position embedding integer in [-64, 64]; the residual X
    integer in [-1000, 1000]; colsum integer in [-200, 200]; mean * rstd integer in [-4, 4]; rstd and qscale powers of two
    (1, 1/2, 1/4, 1/8; 1/8).  Every intermediate is then a multiple of 2^-6 below 2^17: 23 bits, inside fp32's 24.  Raises where
    that would not hold."""
    if 9 * K + 1000 + 64 + 4 * 200 >= 2 ** 17:
        raise ValueError(f"K = {K}: partial sums would leave the exact range")
    if epi == EPI_GELU_X3 and dtype != torch.float16:
        raise ValueError("GELU_X3 exists for fp16 only")
    g = torch.Generator(device=device).manual_seed(seed)
    c = GemmCase(epi, M, N, K, dtype, _randint(-3, 3, (M, K), g, device).to(dtype), _randint(-3, 3, (N, K), g, device).to(dtype))
    if epi != EPI_PATCH:
        c.bias = _randint(-64, 64, (N,), g, device).float()
    if epi in (EPI_QKV, EPI_QKV_LN):
        c.qscale, c.qcols = 0.125, min(1024, N // 2)
    if epi == EPI_PATCH:
        c.pos = _randint(-64, 64, (TOKENS, N), g, device).float()
    if epi in (EPI_RESID, EPI_RESID_STAT):
        c.X0 = _randint(-1000, 1000, (M, N), g, device).float()
    if epi in (EPI_QKV_LN, EPI_GELU_LN):
        rstd = torch.pow(2.0, -_randint(0, 3, (M,), g, device).float())
        c.rowstat = torch.stack([rstd, _randint(-4, 4, (M,), g, device).float()], dim=1).contiguous()
        c.colsum = _randint(-200, 200, (N,), g, device).float()
    return c


def make_gauss_gemm_case(epi: int, M: int, N: int, K: int, dtype: torch.dtype, seed: int, device="cpu") -> GemmCase:
    """Gaussian operands of the model's scale (activations ~ N(0, 1), weights ~ N(0, 0.03^2)) rounded to the operand type: rounding
    inside the accumulation is exercised, the answer is no longer exact (see gemm_acc_bound)."""
    g = torch.Generator(device=device).manual_seed(seed)
    rn = lambda *s: torch.randn(s, generator=g, device=device)
    c = GemmCase(epi, M, N, K, dtype, rn(M, K).to(dtype), (rn(N, K) * 0.03).to(dtype), exact_inputs=False)
    if epi != EPI_PATCH:
        c.bias = rn(N)
    if epi in (EPI_QKV, EPI_QKV_LN):
        c.qscale, c.qcols = math.log2(math.e) / 8.0, min(1024, N // 2)
    if epi == EPI_PATCH:
        c.pos = rn(TOKENS, N)
    if epi in (EPI_RESID, EPI_RESID_STAT):
        c.X0 = rn(M, N)
    if epi in (EPI_QKV_LN, EPI_GELU_LN):
        c.rowstat = torch.stack([0.5 + 1.5 * torch.rand(M, generator=g, device=device), rn(M)], dim=1).contiguous()
        c.colsum = rn(N)
    return c


def alloc_outputs(c: GemmCase) -> Dict[str, torch.Tensor]:
    """The buffers a launch of case c writes, each with GUARD_ROWS sentinel rows behind it; RESID / RESID_STAT start from X0."""
    dev = c.A.device
    out = torch.full((c.out_rows + GUARD_ROWS, c.out_cols), SENTINEL, dtype=c.out_dtype, device=dev)
    if c.X0 is not None:
        out[:c.M] = c.X0
    bufs = {"out": out}
    if c.epi == EPI_RESID_STAT:
        bufs["x16"] = torch.full((c.M + GUARD_ROWS, c.N), SENTINEL, dtype=c.dtype, device=dev)
        bufs["part"] = torch.full((c.N // 64 + 1, c.M, 2), SENTINEL, dtype=torch.float32, device=dev)     # one guard SLOT
    return bufs


# ---------------------------------------------------------------------------------------------------------------- fp64 epilogues
def quick_gelu64(v: torch.Tensor) -> torch.Tensor:
    """modeling_clip QuickGELUActivation: x * sigmoid(1.702 x), fp64."""
    return v * torch.sigmoid(1.702 * v)


def pre_activation64(c: GemmCase, acc: torch.Tensor, rows: torch.Tensor) -> torch.Tensor:
    """The value the epilogue forms from the accumulator of A's rows `rows` (an index tensor) before any scaling / activation /
    residual add, fp64."""
    if c.epi in (EPI_QKV_LN, EPI_GELU_LN):
        rs = c.rowstat[rows].double()
        return rs[:, :1] * acc - rs[:, 1:2] * c.colsum.double()[None, :] + c.bias.double()[None, :]
    if c.epi == EPI_PATCH:
        return acc + c.pos.double()[1 + rows % PATCHES]
    return acc + c.bias.double()[None, :] if c.bias is not None else acc


def half_ulp16(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Half a unit in the last place of the 16-bit type at magnitude |x| (fp64 in, fp64 out; fp16's subnormal spacing as floor)."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -140)))
    if dtype == torch.float16:
        e = e.clamp_min(-14.0)
    return torch.pow(2.0, e - _SIG16[dtype])


def gelu_fast_bound(v: torch.Tensor, v_err: Optional[torch.Tensor] = None) -> torch.Tensor:
    """|y_kernel - y| for y = v * sigmoid(1.702 v) formed in fp32 as  t = c v;  e = v_exp_f32(t);  s = 1 + e;  r = v_rcp_f32(s);
    y = v r  (two multiplies, one add at half an ulp = U32 relative each; v_exp_f32 and v_rcp_f32 at one ulp = 2 U32 each).

      y = v / (1 + e):   dy/y = d(mul) + d(rcp) + d(add) - e/(1+e) * (d(exp) + ln2 * dt)
      dt: the constant c = fp32(1.702 log2 e) and the product c v are each rounded once: |dt| <= 2 U32 |t|, |t| = 1.702 log2(e) |v|
      => |dy| <= |y| U32 (1 + 2 + 1 + w (2 + 2 ln2 |t|)),   w = e / (1 + e) = sigmoid(-1.702 v)
    plus (|v| + 1) 2^-126 for results / reciprocals below the smallest normal fp32 being flushed to zero.  An error v_err of v itself
    (Gaussian inputs: the accumulation's) passes through |dy/dv| <= 1.1."""
    t = 1.702 * math.log2(math.e) * v.abs()
    w = torch.sigmoid(-1.702 * v)
    b = quick_gelu64(v).abs() * U32 * (4.0 + w * (2.0 + 2.0 * math.log(2.0) * t)) + (v.abs() + 1.0) * 2.0 ** -126
    return b if v_err is None else b + 1.1 * v_err


def gelu_ieee_bound(v: torch.Tensor) -> torch.Tensor:
    """The exact tier's form v / (1 + expf(-1.702 v)): the product 1.702 v (constant and product rounded: 2 U32 |t|), expf within one
    ulp (2 U32), the add and the IEEE division at half an ulp each:  |dy| <= |y| U32 (1 + 1 + w (2 + 2 |t|)),  t = 1.702 v."""
    t = 1.702 * v.abs()
    w = torch.sigmoid(-1.702 * v)
    return quick_gelu64(v).abs() * U32 * (2.0 + w * (2.0 + 2.0 * t)) + (v.abs() + 1.0) * 2.0 ** -126


def sumsq_bound(sq_sum: torch.Tensor) -> torch.Tensor:
    """fp32 sum of 64 squares, any association: each square rounded once, 63 additions:  |err| <= gamma_64 S <= 65 U32 S."""
    return 65.0 * U32 * sq_sum


# ---------------------------------------------------------------------------------------------------------------- the comparator
def _first(mask: torch.Tensor, limit: int = 4):
    idx = mask.nonzero()[:limit]
    return [tuple(int(x) for x in r) for r in idx.cpu()]


def _where(c: GemmCase, row: int, col: int) -> str:
    return (f"row {row} (384-row tile {row // 384} +{row % 384}, 256-row tile {row // 256} +{row % 256}, 16-row block {row % 256 // 16}) "
            f"col {col} (256-col tile {col // 256} +{col % 256}, 64-col slot {col // 64})")


def slab_guess(c: GemmCase, row: int, col: int, diff: float) -> str:
    """Which 32-wide K slabs explain an error `diff` = got - expected of the accumulator at (row, col): dropped (-slab) or counted twice."""
    a = c.A[row].double().reshape(-1, 32)
    w = c.W[col].double().reshape(-1, 32)
    s = (a * w).sum(1)
    hit = [f"slab {int(i)} dropped" for i in (s == -diff).nonzero().flatten()[:3] if diff != 0]
    hit += [f"slab {int(i)} twice" for i in (s == diff).nonzero().flatten()[:3] if diff != 0]
    return ", ".join(hit) if hit else "no single 32-wide K slab explains it"


def _report(c, name, bad, got, want, r0, scale_for_slab=None, limit=4) -> List[str]:
    out = []
    for (i, j) in _first(bad, limit):
        row, col = r0 + i, j
        g, w = float(got[i, j]), float(want[i, j])
        msg = f"{EPI_NAMES[c.epi]} {name}: got {g!r} want {w!r} at " + _where(c, row, col % c.N)
        if scale_for_slab is not None and c.exact_inputs and math.isfinite(g):
            sc = float(scale_for_slab[i, j]) if torch.is_tensor(scale_for_slab) else float(scale_for_slab)
            if sc != 0.0:
                msg += "; " + slab_guess(c, row, col % c.N, (g - w) / sc)
        out.append(msg)
    if bad.any():
        rows = bad.any(1).nonzero().flatten()
        out.append(f"{EPI_NAMES[c.epi]} {name}: {int(bad.sum())} wrong elements in rows {r0 + int(rows[0])} .. {r0 + int(rows[-1])} of chunk [{r0}, {r0 + bad.shape[0]})")
    return out


def _require_exact32(v: torch.Tensor, what: str):
    if not bool((v.float().double() == v).all()):
        raise ValueError(f"exact-input precondition broken: {what} is not representable in fp32")


def compare_gemm(c: GemmCase, outputs: Dict[str, torch.Tensor], chunk: int = 16384, limit: int = 4, guard: bool = True,
                 also_within=None) -> List[str]:
    """Everything a launch of case c must have written, against fp64, in row chunks.  Exact inputs: equality wherever the value is
    exact (QKV, QKV_LN, RESID, PATCH, F32, X / x16 / column sums of RESID_STAT, sums of squares up to 2^24), the derived per-element
    bounds elsewhere (GELU forms, larger sums of squares).  Gaussian inputs (c.exact_inputs False): every value within
    gemm_acc_bound carried through the epilogue.  Guard rows, PATCH's class-token rows and the partials' guard slot must still hold
    SENTINEL (guard=False: the buffers were not made by alloc_outputs and end at row M).  also_within = (rtol, atol) additionally holds
    an fp32 `out` to |got - want| <= atol + rtol |want|."""
    f: List[str] = []
    out = outputs["out"]
    M, N = c.M, c.N
    Wd = c.W.double()
    absW = Wd.abs() if not c.exact_inputs else None
    for r0 in range(0, M, chunk):
        r1 = min(M, r0 + chunk)
        Ad = c.A[r0:r1].double()
        acc = Ad @ Wd.t()
        v = pre_activation64(c, acc, torch.arange(r0, r1, device=acc.device))
        verr = None
        scale = 1.0
        if c.exact_inputs:
            _require_exact32(v, "the epilogue's pre-activation value")
        else:
            verr = gemm_acc_bound(c, Ad.abs() @ absW.t(), acc, r0, r1)
        if c.epi in (EPI_QKV_LN, EPI_GELU_LN):
            scale = c.rowstat[r0:r1, :1].double().expand(-1, N)
        if c.epi in (EPI_QKV, EPI_QKV_LN):
            q = torch.ones(N, dtype=torch.float64, device=v.device)
            q[:c.qcols] = float(torch.tensor(c.qscale, dtype=torch.float32))
            v = v * q
            got = out[r0:r1].double()
            if c.exact_inputs:
                want = v.float().to(c.dtype).double()
                f += _report(c, "out", got != want, got, want, r0, (scale * q).expand(r1 - r0, N), limit)
            else:
                tol = verr * q + 2 * U32 * v.abs() + half_ulp16(v.abs() + verr * q, c.dtype)      # + the qscale product, the constant's rounding
                f += _report(c, "out", ~((got - v).abs() <= tol), got, v, r0, None, limit)
        elif c.epi in (EPI_GELU, EPI_GELU_LN):
            y = quick_gelu64(v)
            e = gelu_fast_bound(v, verr)
            tol = e + half_ulp16(y.abs() + e, c.dtype)
            got = out[r0:r1].double()
            f += _report(c, "out", ~((got - y).abs() <= tol), got, y, r0, None, limit)
        elif c.epi == EPI_GELU_X3:
            y = quick_gelu64(v)
            e = gelu_ieee_bound(v)
            t = out[r0:r1]
            hi, lo, hs = t[:, :N].double(), t[:, N:2 * N].double(), t[:, 2 * N:]
            f += _report(c, "hi", ~((hi - y).abs() <= e + half_ulp16(y.abs() + e, torch.float16)), hi, y, r0, None, limit)
            # lo = fp16(g - hi): relative 2^-11 of |g - hi| <= 2^-11 |g|, or fp16's subnormal spacing
            f += _report(c, "hi+lo", ~((hi + lo - y).abs() <= e + 2.0 ** -22 * y.abs() + 2.0 ** -25), hi + lo, y, r0, None, limit)
            want_hs = (t[:, :N].float() * 2.0 ** -8).half()
            f += _report(c, "hi*2^-8", hs != want_hs, hs.double(), want_hs.double(), r0, None, limit)
        elif c.epi == EPI_PATCH:
            orow = torch.arange(r0, r1, device=v.device)
            orow = orow // PATCHES * TOKENS + 1 + orow % PATCHES
            got = out[orow].double()
            f += _cmp32(c, "out", got, v, verr, r0, limit)
        else:                                               # F32, RESID, RESID_STAT
            x = v + c.X0[r0:r1].double() if c.X0 is not None else v
            if c.exact_inputs:
                _require_exact32(x, "the new residual value")
            xerr = None if verr is None else verr + U32 * (v.abs() + x.abs())
            got = out[r0:r1].double()
            f += _cmp32(c, "out", got, x, xerr, r0, limit)
            if also_within is not None:
                f += _report(c, "out (rtol, atol)", ~((got - x).abs() <= also_within[1] + also_within[0] * x.abs()), got, x, r0, None, limit)
            if c.epi == EPI_RESID_STAT:
                f += _compare_stat(c, outputs, x, xerr, r0, r1, limit)
        if len(f) > 40:
            f.append("... (stopped after 40 findings)")
            return f
    # what must NOT have been written
    if not guard:
        return f
    if c.epi == EPI_PATCH:
        cls = out[:c.out_rows:TOKENS]
        if not bool((cls == SENTINEL).all()):
            f.append(f"PATCH: class-token rows written (images {_first((cls != SENTINEL).any(1, keepdim=True))})")
    for name, buf, rows in (("out", out, c.out_rows), ("x16", outputs.get("x16"), M)):
        if buf is not None and not bool((buf[rows:] == SENTINEL).all()):
            f.append(f"{EPI_NAMES[c.epi]} {name}: guard rows past row {rows} written at (row - {rows}, col) {_first(buf[rows:] != SENTINEL)}")
    if c.epi == EPI_RESID_STAT and not bool((outputs["part"][N // 64] == SENTINEL).all()):
        f.append(f"RESID_STAT part: guard slot {N // 64} written at (row, which) {_first(outputs['part'][N // 64] != SENTINEL)}")
    return f


def _cmp32(c, name, got, want, err, r0, limit):
    if err is None:
        return _report(c, name, got != want, got, want, r0, 1.0, limit)
    return _report(c, name, ~((got - want).abs() <= err + U32 * want.abs()), got, want, r0, None, limit)


def _compare_stat(c, outputs, x, xerr, r0, r1, limit):
    """x16 = the 16-bit copy of the new rows; part[slot, row] = (sum, sum of squares) of the row's 64 columns of that slot -- SLOT-major
    (N/64, M, 2).  Exact inputs: the copy and the sums are exact; a sum of squares is exact when it stays below 2^24 (all partial
    sums of non-negative integers do then), else within sumsq_bound."""
    f = []
    N = c.N
    got16 = outputs["x16"][r0:r1].double()
    part = outputs["part"][:N // 64, r0:r1].double().permute(1, 0, 2)          # (rows, slots, 2)
    xs = x.reshape(r1 - r0, N // 64, 64)
    s1, s2 = xs.sum(2), (xs * xs).sum(2)
    if c.exact_inputs:
        want16 = x.float().to(c.dtype).double()
        f += _report(c, "x16", got16 != want16, got16, want16, r0, 1.0, limit)
        bad1 = part[:, :, 0] != s1
        exact2 = s2 <= 2.0 ** 24
        bad2 = torch.where(exact2, part[:, :, 1] != s2, ~((part[:, :, 1] - s2).abs() <= sumsq_bound(s2)))
    else:
        tol16 = xerr + half_ulp16(x.abs() + xerr, c.dtype)
        f += _report(c, "x16", ~((got16 - x).abs() <= tol16), got16, x, r0, None, limit)
        e64 = xerr.reshape(r1 - r0, N // 64, 64)
        bad1 = ~((part[:, :, 0] - s1).abs() <= e64.sum(2) + 65.0 * U32 * xs.abs().sum(2))
        bad2 = ~((part[:, :, 1] - s2).abs() <= (2 * xs.abs() * e64 + e64 * e64).sum(2) + sumsq_bound(s2))
    for which, bad, want in (("sum", bad1, s1), ("sum of squares", bad2, s2)):
        for (i, s) in _first(bad, limit):
            f.append(f"RESID_STAT part[{s}, {r0 + i}] {which}: got {float(part[i, s, 0 if which == 'sum' else 1])!r} want {float(want[i, s])!r}"
                     f" (row {r0 + i}: 384-row tile {(r0 + i) // 384}, 256-row tile {(r0 + i) // 256}; slot-major index)")
    return f


# ---------------------------------------------------------------------------------------------------------------- Gaussian bounds
def ideal_out64(c: GemmCase, rows: torch.Tensor) -> torch.Tensor:
    """The unrounded value of `out` for A's rows `rows` (an index tensor), fp64 (RESID_STAT: the new X; GELU_X3: the activation)."""
    v = pre_activation64(c, c.A[rows].double() @ c.W.double().t(), rows)
    if c.epi in (EPI_QKV, EPI_QKV_LN):
        v[:, :c.qcols] *= float(torch.tensor(c.qscale, dtype=torch.float32))
    if c.epi in (EPI_GELU, EPI_GELU_LN, EPI_GELU_X3):
        v = quick_gelu64(v)
    return v + c.X0[rows].double() if c.X0 is not None else v


def sequential_out32(c: GemmCase, rows: torch.Tensor) -> torch.Tensor:
    """`out` for A's rows `rows` from a plain fp32 accumulation in sequential K order (k = 0, 1, 2, ...: the worst reasonable order)
    and the epilogue in plain fp32 torch arithmetic, rounded to the output type: the yardstick of the Gaussian RMS test."""
    a, w = c.A[rows].float(), c.W.float().t().contiguous()
    acc = torch.zeros((a.shape[0], c.N), dtype=torch.float32, device=a.device)
    for k in range(c.K):
        acc += a[:, k:k + 1] * w[k:k + 1]
    if c.epi in (EPI_QKV_LN, EPI_GELU_LN):
        rs = c.rowstat[rows]
        v = rs[:, :1] * acc - rs[:, 1:2] * c.colsum[None, :] + c.bias[None, :]
    elif c.epi == EPI_PATCH:
        v = acc + c.pos[1 + rows % PATCHES]
    else:
        v = acc + c.bias[None, :]
    if c.epi in (EPI_QKV, EPI_QKV_LN):
        v[:, :c.qcols] *= c.qscale
    if c.epi in (EPI_GELU, EPI_GELU_LN):
        v = v * torch.sigmoid(1.702 * v)
    if c.X0 is not None:
        v = c.X0[rows] + v
    return v.to(c.out_dtype)


def gemm_acc_bound(c: GemmCase, absprod: torch.Tensor, acc: torch.Tensor, r0: int, r1: int) -> torch.Tensor:
    """Textbook worst case of a K-term fp32 dot product in any order, K U32 (|A| |W|^T), carried to the pre-activation value: the
    LayerNorm fold multiplies it by rstd and adds three more fp32 operations on (rstd acc, mean rstd colsum, bias); the others one add."""
    e = c.K * U32 * absprod
    if c.epi in (EPI_QKV_LN, EPI_GELU_LN):
        rs = c.rowstat[r0:r1].double()
        t1, t2 = (rs[:, :1] * acc).abs(), (rs[:, 1:2] * c.colsum.double()[None, :]).abs()
        return rs[:, :1] * e + 3 * U32 * (t1 + t2 + c.bias.double().abs()[None, :])
    other = c.pos.double().abs().max() if c.epi == EPI_PATCH else (c.bias.double().abs()[None, :] if c.bias is not None else 0.0)
    return e + U32 * (acc.abs() + other)


# ================================================================================================================ attention
def _v_values(n: int, dtype: torch.dtype, device, span: int) -> torch.Tensor:
    """V (n, 577, 16, 64) of integers in [-span, span], a different residue for neighbouring images, keys, heads and columns, so a value
    read from a wrong key / head / column / image differs from the right one (as distinct as `span` allows)."""
    img = torch.arange(n, device=device).view(n, 1, 1, 1)
    key = torch.arange(TOKENS, device=device).view(1, TOKENS, 1, 1)
    head = torch.arange(HEADS, device=device).view(1, 1, HEADS, 1)
    col = torch.arange(HDIM, device=device).view(1, 1, 1, HDIM)
    m = 2 * span + 1
    v = (key * 37 + head * 101 + col * 7 + img * 13 + (key * col) % 11) % m - span
    return v.to(dtype)


def _span(dtype):
    # fp16 holds integers up to 2048, bf16 up to 256; fp32 (the exact tier, split in two fp16 halves) 577 * 14000 < 2^24
    return {torch.float16: 1019, torch.bfloat16: 125, torch.float32: 13998}[dtype]


def _codes(n: int, seed: int, device) -> torch.Tensor:
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randint(0, 2, (n, TOKENS, HEADS, HDIM), generator=g) * 2 - 1).to(device)


def _pack_qkv(q, k, v, dtype) -> torch.Tensor:
    n = q.shape[0]
    return torch.cat([t.reshape(n * TOKENS, HIDDEN).to(dtype) for t in (q, k, v)], dim=1).contiguous()


def attention_uniform_case(n: int, dtype: torch.dtype, seed: int = 1, device="cpu"):
    """Q = 0: every probability is exactly 1, the row sum exactly 577, O the exact integer sum of V over the keys.  Returns
    (qkv (n*577, 3072), sum of V over keys as fp64 (n, 16, 64))."""
    v = _v_values(n, dtype, device, _span(dtype))
    k = _codes(n, seed, device)
    q = torch.zeros_like(k)
    vs = v.double().sum(1)
    if float(vs.abs().max()) >= 2.0 ** 24:
        raise ValueError("uniform attention case: the sum of V leaves the exact range")
    return _pack_qkv(q, k, v, dtype), vs


def onehot_targets(kind: str, device="cpu") -> torch.Tensor:
    """pi (577,): the key each query attends to.
    'spread': pi(i) = (37 i + 63) mod 577 -- 37 is coprime to 577, so pi is a permutation (every key, hence keys 0, 63, 64, 575, 576
    and every key tile, is a target; every query, hence query 576 and the last block 512..575, has one) and neighbouring queries of a
    16-query block land 37 keys apart: in different 64-key tiles.
    'last': every query's target is key 576, the single-key step after the nine matrix-pipe tiles."""
    i = torch.arange(TOKENS, device=device)
    if kind == "last":
        return torch.full_like(i, TOKENS - 1)
    pi = (37 * i + 63) % TOKENS
    assert int(pi[0]) == 63 and sorted(pi.tolist()) == list(range(TOKENS))
    for qb in range(0, TOKENS - 1, 16):
        assert len(set((pi[qb:qb + 16] // 64).tolist())) >= 4
    return pi


def attention_onehot_case(n: int, dtype: torch.dtype, kind: str, qfactor: float, score_div: float, seed: int = 2, device="cpu"):
    """K rows are +-1 code vectors, Q row i = qfactor * K[pi(i)]: the target's score is 64 qfactor / score_div, every other lower by
    the gap asserted here (>= 160 in the units the kernel's softmax sees; exp2(-160) and exp(-160) are below fp32's smallest
    subnormal, 2^-149, so every other key's weight is exactly 0), and the output row must EQUAL V[pi(i)].  Raises if the gap is smaller.
    Returns (qkv, expected (n*577, 1024) in `dtype`, gap)."""
    pi = onehot_targets(kind, device)
    k = _codes(n, seed, device)
    q = qfactor * k[:, pi]
    v = _v_values(n, dtype, device, _span(dtype))
    s = torch.einsum("nihd,njhd->nhij", q.double(), k.double()) / score_div
    tgt = s.gather(3, pi.view(1, 1, TOKENS, 1).expand(n, HEADS, TOKENS, 1))
    s.scatter_(3, pi.view(1, 1, TOKENS, 1).expand(n, HEADS, TOKENS, 1), float("-inf"))
    gap = float((tgt.squeeze(3) - s.max(3).values).min())
    if not (gap >= 160.0 and bool((tgt == 64 * qfactor / score_div).all())):
        raise ValueError(f"one-hot attention case: score gap {gap} < 160")
    return _pack_qkv(q, k, v, dtype), v[:, pi].reshape(n * TOKENS, HIDDEN).to(dtype), gap


def attention_staircase_case(n: int, dtype: torch.dtype, step: float, score_mul: float, seed: int = 3, device="cpu"):
    """The maximum of key tile t exceeds tile t-1's by `step` (in the units the kernel's softmax sees): 7.9 -- the lazy softmax keeps
    its reference until the steps add up to more than 8 -- or 8.1 -- a rescale at every tile; key 576 tops the staircase.  Only 3 of
    the 64 dimensions are non-zero (d 0: the 8-per-tile ramp, d 1: the -/+0.1 per tile and a per-query tilt, d 2: a small per-key
    wiggle), so the fp32 score error term of the bound stays far below P's rounding.  score_mul: what Q carries so that the
    kernel's softmax sees these scores (1 for pg_op_attention, 8 for pg_op_attention_f32, which divides by 8).  V Gaussian.
    Returns (qkv, q, k, v) with q, k, v the ROUNDED operands as fp64 (n, 577, 16, 64); the caller checks the steps on them."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    tile = (torch.arange(TOKENS) // 64).double()                                # 0..9 (tile 9 = key 576 alone)
    q = torch.zeros((n, TOKENS, HEADS, HDIM), dtype=torch.float64)
    k = torch.zeros_like(q)
    q[..., 0] = score_mul
    q[..., 1] = score_mul
    q[..., 2] = score_mul * (torch.rand((n, TOKENS, HEADS), generator=g, dtype=torch.float64) * 0.5 + 0.5)
    k[..., 0] = (8.0 * tile).view(1, TOKENS, 1)
    k[..., 1] = ((step - 8.0) * tile).view(1, TOKENS, 1)
    k[..., 2] = -torch.rand((n, TOKENS, HEADS), generator=g, dtype=torch.float64) * 3.0      # each tile: scores within 3 below its top ...
    top = torch.arange(TOKENS) % 64 == (torch.arange(TOKENS) // 64 * 7) % 64
    top[TOKENS - 1] = True
    k[:, top, :, 2] = 0.0                                                                     # ... which one key per tile reaches
    v = torch.randn((n, TOKENS, HEADS, HDIM), generator=g, dtype=torch.float64)
    q, k, v = [t.to(dtype).to(device) for t in (q, k, v)]
    return _pack_qkv(q, k, v, dtype), q.double(), k.double(), v.double()


def staircase_steps(q, k, score_div: float) -> torch.Tensor:
    """Differences between consecutive key tiles' maxima, per (image, head, query): (n, 16, 577, 9), fp64, from the rounded operands."""
    s = torch.einsum("nihd,njhd->nhij", q, k) / score_div
    pad = torch.full(s.shape[:3] + (640 - TOKENS,), float("-inf"), dtype=s.dtype, device=s.device)
    tmax = torch.cat([s, pad], 3).reshape(s.shape[:3] + (10, 64)).max(4).values
    return tmax[..., 1:] - tmax[..., :-1]


def attention_ref64(q, k, v, score_div: float, base2: bool):
    """softmax(q k^T / score_div) v per (image, head) in fp64 (base 2 for pg_op_attention, whose Q carries log2 e); returns
    (out (n*577, 1024), softmax . |V| (same shape), scores)."""
    n = q.shape[0]
    s = torch.einsum("nihd,njhd->nhij", q, k) / score_div
    p = torch.softmax(s * (math.log(2.0) if base2 else 1.0), dim=3)
    o = torch.einsum("nhij,njhd->nihd", p, v).reshape(n * TOKENS, HIDDEN)
    oa = torch.einsum("nhij,njhd->nihd", p, v.abs()).reshape(n * TOKENS, HIDDEN)
    return o, oa, s


def staircase_eps(dtype, q, k, score_div: float) -> float:
    """eps_p of the staircase bound  |out - ref| <= 2 eps_p (softmax . |V|) + u_out |ref| + 577 2^-24 max|V|  -- the relative error of one
    probability as the PV product sees it:
      * P rounded to the operand type: 2^-12 (fp16) / 2^-9 (bf16); the exact tier's attention (dtype fp32): 2^-22, two fp16 halves.
        (Round-to-nearest's worst case for ONE value is twice that, 2^-11 / 2^-8; the tighter figure is kept on purpose: a bound
        that is stricter than the worst case allows can only fail too early, never hide an error.);
      * its exponent: the fp32 score is a sum of the D non-zero products seeded with -m, D + 1 additions of terms bounded by
        |m| + sum |q_d k_d| <= 2 max sum |q_d k_d|: |ds| <= (D + 1) 2^-24 * 2 max sum |q k| (+ 2^-22 of it where the operands are
        split in halves and the lo.lo product is dropped); an error ds of the exponent is a relative error <= ds of P (ln2 ds in base 2);
      * the exponential itself: one ulp, 2^-23;
      * at most nine rescales of O and of the row sum: exp2 (2^-23) and the product (2^-24) each.
    The factor 2 in front: numerator and row sum each carry eps_p."""
    p_round = {torch.float16: 2.0 ** -12, torch.bfloat16: 2.0 ** -9, torch.float32: 2.0 ** -22}[dtype]
    D = int((q.abs().amax((0, 1, 2)) > 0).sum())
    smax = float(torch.einsum("nihd,njhd->nhij", q.abs(), k.abs()).max()) / score_div
    ds = ((D + 1) * U32 + (2.0 ** -22 if dtype == torch.float32 else 0.0)) * 2 * smax
    return p_round + ds + 2.0 ** -23 + 9 * (2.0 ** -23 + 2.0 ** -24)


def staircase_tol(dtype, q, k, v, score_div: float, base2: bool):
    """(reference, per-element tolerance) of the staircase case; see staircase_eps."""
    o, oa, _ = attention_ref64(q, k, v, score_div, base2)
    u_out = U32 if dtype == torch.float32 else 2.0 ** -_SIG16[dtype]
    return o, 2 * staircase_eps(dtype, q, k, score_div) * oa + u_out * o.abs() + TOKENS * U32 * float(v.abs().max())


def ulp32(x: torch.Tensor) -> torch.Tensor:
    return torch.pow(2.0, torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126))) - 23)


def attention_where(row: int, col: int) -> str:
    tok = row % TOKENS
    return (f"image {row // TOKENS} query {tok} (128-query block {tok // 128}, 16-query block {tok % 128 // 16}, lane row {tok % 16}) "
            f"head {col // HDIM} column {col % HDIM} (16-column block {col % HDIM // 16})")


def compare_attention(got: torch.Tensor, want: torch.Tensor, tol=None, limit: int = 4, guard: Optional[torch.Tensor] = None) -> List[str]:
    """got (n*577, 1024) against want: equal (tol None) or |got - want| <= tol (a tensor or a number); the guard region behind the output
    must still hold SENTINEL.  Findings name image / query block / head / column; with a tolerance also the worst row."""
    g, w = got.double(), want.double()
    err = (g - w).abs()
    bad = (g != w) if tol is None else ~(err <= tol)
    f = [f"attention: got {float(g[i, j])!r} want {float(w[i, j])!r} at " + attention_where(i, j) for (i, j) in _first(bad, limit)]
    if f:
        rows = bad.any(1).nonzero().flatten()
        worst = int(torch.nan_to_num(err, nan=float("inf")).max(1).values.argmax())
        f.append(f"attention: {int(bad.sum())} wrong elements in {len(rows)} rows; worst row {worst} = " + attention_where(worst, 0).split(" head")[0])
    if guard is not None and not bool((guard == SENTINEL).all()):
        f.append(f"attention: guard region behind the output written at {_first(guard != SENTINEL)}")
    return f
