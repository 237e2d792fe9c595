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


# ================================================================================================================ the exact tier's triple
# csrc/x3.h: the triple of an fp32 value v is fully determined --
#     hi = fp16_rne(clamp(v, +-65504)),   lo = fp16_rne(v - hi)  (the fp32 difference is exact),   hs = fp16_rne(hi * 2^-8)
# -- so a kernel that writes it from a KNOWN fp32 value is compared bit for bit, fp16-subnormal halves, ties and the saturation included.
F16_MAX = 65504.0
SEGMENTS = ("hi", "lo", "hi*2^-8")


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t if t.dtype == torch.int16 else t.view(torch.int16)


def _halves(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.float16) if t.dtype == torch.int16 else t


def triple_ref(v: torch.Tensor):
    """(hi, lo, hs) of the fp32 tensor v as int16 bit patterns, with torch's own conversions (round to nearest even, subnormals kept) on
    whatever device v lives on.  |v| must stay below 1.3e5: beyond, v - hi itself overflows fp16 (outside the kernels' contract)."""
    v = v.float()
    hi = v.clamp(-F16_MAX, F16_MAX).half()
    lo = (v - hi.float()).half()
    hs = (hi.float() * 2.0 ** -8).half()
    return _bits(hi), _bits(lo), _bits(hs)


def compare_triple(got: torch.Tensor, v: torch.Tensor, C: int, seg: Optional[int] = None, limit: int = 4, where=None,
                   guard: bool = True) -> List[str]:
    """got (rows + guard rows, 3 seg) fp16 / int16 against the triple of v (rows, C) fp32, bit for bit.  Segment s occupies columns
    [s seg, s seg + C); with seg > C (the patch matrix: C = 588, seg = 640) the columns between the segments must be zero.  Rows past
    v's must still hold SENTINEL (guard=False: there are none).  Findings name segment, row and column (+ where(row, col))."""
    seg = C if seg is None else seg
    rows = v.shape[0]
    f: List[str] = []
    if got.dim() != 2 or got.shape[1] != 3 * seg or got.shape[0] < rows or v.shape[1] != C:
        return [f"triple: buffer of shape {tuple(got.shape)} for values {tuple(v.shape)}, C = {C}, segment stride {seg}"]
    g = _bits(got)
    for s, want in enumerate(triple_ref(v)):
        have = g[:rows, s * seg:s * seg + C]
        bad = have != want
        for (i, j) in _first(bad, limit):
            f.append(f"triple {SEGMENTS[s]}: got 0x{int(have[i, j]) & 0xffff:04x} ({float(_halves(have)[i, j])!r}) want 0x{int(want[i, j]) & 0xffff:04x} "
                     f"({float(_halves(want)[i, j])!r}) for v = {float(v[i, j])!r} at segment {s} row {i} col {j} (4-col group {j // 4})"
                     + (" " + where(i, j) if where else ""))
        if bad.any():
            r = bad.any(1).nonzero().flatten()
            f.append(f"triple {SEGMENTS[s]}: {int(bad.sum())} wrong elements in rows {int(r[0])} .. {int(r[-1])}")
        if seg > C:
            pad = g[:rows, s * seg + C:(s + 1) * seg]
            if bool((pad != 0).any()):
                f.append(f"triple {SEGMENTS[s]}: columns between the segments not zero at (row, pad col) {_first(pad != 0, limit)}")
    if guard and got.shape[0] > rows:
        gr = _halves(got[rows:])
        if not bool((gr == SENTINEL).all()):
            f.append(f"triple: guard rows past row {rows} written at (row - {rows}, col) {_first(gr != SENTINEL, limit)}")
    return f


def triple_consistent(got: torch.Tensor, C: int, rows: Optional[int] = None, limit: int = 4):
    """A triple whose fp32 value the host cannot reproduce (LayerNorm, QuickGELU, attention) still has to be A triple:
         hs == fp16(hi * 2^-8) bit for bit;   |lo| <= ulp16(hi) / 2  (hi is the NEAREST fp16);
         fp16(hi + lo) == hi  (hi + lo is exact in fp32: at most 23 bits apart) -- except where |lo| is exactly half an ulp: lo is itself
         rounded to 11 bits, which can carry a value just inside the half ulp onto the tie, and a tie may round to the other neighbour.
    Returns (findings, hi + lo as fp64 (rows, C)): the reconstructed value then goes to a value comparator with triple_recon_bound."""
    rows = got.shape[0] if rows is None else rows
    t = _halves(got[:rows])
    hi, lo, hs = t[:, :C], t[:, C:2 * C], t[:, 2 * C:3 * C]
    f: List[str] = []
    want_hs = (hi.float() * 2.0 ** -8).half()
    hu = half_ulp16(hi.double(), torch.float16)                      # 2^-25 for a subnormal or zero hi
    s = hi.float() + lo.float()
    checks = (("hi*2^-8 != fp16(hi * 2^-8)", _bits(hs) != _bits(want_hs)),
              ("|lo| > ulp16(hi) / 2", ~(lo.double().abs() <= hu)),
              ("fp16(hi + lo) != hi", ~(s.half() == hi) & (lo.double().abs() != hu)))
    for name, bad in checks:
        for (i, j) in _first(bad, limit):
            f.append(f"triple inconsistent, {name}: hi {float(hi[i, j])!r} lo {float(lo[i, j])!r} hs {float(hs[i, j])!r} at row {i} col {j} (4-col group {j // 4})")
        if bad.any():
            f.append(f"triple inconsistent, {name}: {int(bad.sum())} elements")
    return f, hi.double() + lo.double()


def triple_recon_bound(v: torch.Tensor) -> torch.Tensor:
    """|v - (hi + lo)| for |v| <= 65504:  v - hi is exact and at most ulp16(hi) / 2 <= 2^-11 |hi|; rounding it to lo costs half an ulp of
    lo, 2^-11 |lo| <= 2^-22 |hi| <= 2^-22 (1 + 2^-11) |v|, or half the subnormal quantum, 2^-25, where lo is subnormal:
    max(2^-21 |v|, 2^-25) with a factor 2 to spare on the relative term."""
    return torch.maximum(v.abs() * 2.0 ** -21, torch.full_like(v, 2.0 ** -25))


SPECIALS = (0.0, -0.0, 2.0 ** -24, -(2.0 ** -24), 3 * 2.0 ** -25, 2.0 ** -25, 1.0e-6, 3.0e-5, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -25, 6.1e-5,
            1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, -(1.0 + 2.0 ** -11), 1.0 + 2.0 ** -11 + 2.0 ** -23, 2048.0 + 1.0, 2048.0 + 3.0,
            65504.0, -65504.0, 65519.9, 65520.0, -65520.0, 7.0e4, -1.0e5, 65503.99, 0.1, 1.0 / 3.0)


def triple_values(rows: int, cols: int, seed: int, device="cpu", specials: bool = True) -> torch.Tensor:
    """fp32 (rows, cols): Gaussian times a log-uniform scale over 1e-6 .. 3e4 (every fp16 binade, the subnormal range included), and
    SPECIALS -- +-0, the fp16 subnormal range, exact ties (1 + 2^-11 rounds down to even, 1 + 3 2^-11 up), the saturation edge (65504,
    65519.9, 65520, 7e4, -1e5) -- planted at the start of the first row, at the end of the last row (the ragged end of a grid-stride
    loop) and in the middle."""
    g = torch.Generator(device=device).manual_seed(seed)
    mag = torch.pow(10.0, torch.rand((rows, cols), generator=g, device=device) * (math.log10(3.0e4) + 6.0) - 6.0)
    v = (torch.randn((rows, cols), generator=g, device=device) * mag).clamp(-6.0e4, 6.0e4)
    if specials:
        sp = torch.tensor(SPECIALS, dtype=torch.float32, device=device)
        k = min(len(sp), cols)
        v[0, :k] = sp[:k]
        v[rows - 1, cols - k:] = sp[:k]
        v[rows // 2, cols // 2 - k // 2:cols // 2 - k // 2 + k] = sp[:k].flip(0)
    return v.contiguous()


# ================================================================================================================ LayerNorm and row statistics
# The row kernels (csrc/rowops.hip, csrc/precise.hip) state their arithmetic: a wave owns a 1024-float row, 16 values per lane;
#   mean   = tree sum / 1024          in-lane (a + b) + (c + d), four of those added in sequence, then six butterfly levels: no value
#                                     passes through more than 12 additions; the division by 1024 is exact
#   var    = sum (x - mean)^2 / 1024  TWO passes: the deviations from the computed mean, squared, 16 in sequence per lane + 6 levels
#   rstd   = 1 / sqrtf(var + eps)
#   y      = (x - mean) * rstd * g + b
# gamma_d = d u / (1 - d u) bounds the relative error of any quantity that went through d roundings (u = 2^-24).
LN_SUM_DEPTH = 12            # additions on the longest path of the row sum
LN_SQ_DEPTH = 25             # (x - mean) rounded (twice: it is squared) + the square + 16 + 6 additions


def _gamma(d: int) -> float:
    return d * U32 / (1.0 - d * U32)


def _rstd_interval(var, dvar, eps: float):
    """rstd = (var + eps)^-1/2 and the most the computed 1 / sqrtf(var_c + eps32) can differ from it, given |var_c - var| <= dvar and
    var_c >= 0 (a sum of squares; rowstat_finalize clamps): eps arrives as fp32 (|eps32 - eps| <= u eps), the addition rounds once,
    sqrtf and the division are taken at one ulp each ((1 + 2u)^2 < 1 + 5u; they are correctly rounded in this build: a factor 2 to
    spare).  The interval is carried exactly, not to first order: with dvar close to var + eps the upper end is what it is."""
    eps32 = float(torch.tensor(eps, dtype=torch.float32))
    rstd = (var + eps).rsqrt()
    t_lo = ((var - dvar).clamp_min(0.0) + eps32) * (1.0 - U32)
    t_hi = (var + dvar + eps32) * (1.0 + U32)
    k = 1.0 + 5.0 * U32
    return rstd, torch.maximum(t_lo.rsqrt() * k - rstd, rstd - t_hi.rsqrt() / k)


def _two_pass_stats(x: torch.Tensor, eps: float):
    """fp64 (mean, deviations, rstd) of the rows of x and the bounds (dm, dr) of the kernels' computed mean and rstd:
         |mean_c - mean| <= dm = gamma_12 mean|x|
         var_c = (1/n) sum (x - mean_c)^2 (1 + theta), |theta| <= gamma_25, and (1/n) sum (x - mean_c)^2 = var + (mean - mean_c)^2 EXACTLY
         (the deviations from the true mean sum to zero)  =>  |var_c - var| <= dm^2 + gamma_25 (var + dm^2): no cancellation term --
         that is what the second pass buys."""
    xd = x.double()
    m = xd.mean(1, keepdim=True)
    dev = xd - m
    var = (dev * dev).mean(1, keepdim=True)
    dm = _gamma(LN_SUM_DEPTH) * xd.abs().mean(1, keepdim=True)
    rstd, dr = _rstd_interval(var, dm * dm + _gamma(LN_SQ_DEPTH) * (var + dm * dm), eps)
    return m, dev, rstd, dm, dr


def layernorm_bound(x: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, eps: float = 1e-5):
    """(y, bound): LayerNorm of the fp32 rows x in fp64 and, per element, the most the kernels' fp32 result can differ from it.
         d_c = fl(x - mean_c):                |d_c - dev| <= E_d = dm + u (|dev| + dm)
         p_c = fl(fl(d_c rstd_c) g):          |p_c - dev rstd g| <= |g| [ E_d (rstd + dr) (1 + u)^2 + |dev| ((rstd + dr) (1 + u)^2 - rstd) ] = E_p
         y_c = fl(p_c + b):                   |y_c - y| <= E_p + u (|y| + E_p)
    (four roundings; with the multiply and the add contracted into an FMA there are three, which the same expression covers), plus
    2^-124 for results below the smallest normal fp32.  A 16-bit output adds half_ulp16(|y| + bound), a triple triple_recon_bound."""
    m, dev, rstd, dm, dr = _two_pass_stats(x, eps)
    g, b = gamma.double()[None, :], beta.double()[None, :]
    y = dev * rstd * g + b
    e_d = dm + U32 * (dev.abs() + dm)
    k = (rstd + dr) * (1.0 + U32) ** 2
    e_p = g.abs() * (e_d * k + dev.abs() * (k - rstd))
    return y, e_p + U32 * (y.abs() + e_p) + 2.0 ** -124


def rowstat_bound(x: torch.Tensor, eps: float = 1e-5):
    """((rstd, mean rstd), (bound, bound)) per row for the two-pass statistics (rowstat_cast_kernel, preln_kernel's STAT form):
    rstd as in layernorm_bound; the product fl(mean_c rstd_c) lies within (|mean| + dm) (rstd + dr) (1 + u) - |mean| rstd of mean rstd."""
    m, _, rstd, dm, dr = _two_pass_stats(x, eps)
    return (rstd[:, 0], (m * rstd)[:, 0]), (dr[:, 0], ((m.abs() + dm) * (rstd + dr) * (1.0 + U32) - m.abs() * rstd)[:, 0])


def rowstat_finalize_bound(part: torch.Tensor, eps: float = 1e-5, n: int = HIDDEN):
    """The same pair from per-slice partials part (slots, rows, 2) = (sum, sum of squares), as rowstat_finalize_kernel computes it -- ONE
    pass:  s1, s2 = the partials added in slot order;  mean = s1 / n;  var = max(s2 / n - mean^2, 0).  Against fp64 on the same partials:
         |mean_c - mean| <= dm = gamma_slots sum|p1| / n,      |s2 / n - E2| <= dE = gamma_slots sum|p2| / n
         |fl(mean_c^2) - mean^2| <= dm (2 |mean| + dm) + u (|mean| + dm)^2
         the subtraction rounds once:  u (E2 + dE + (1 + u) (|mean| + dm)^2)
    The last two lines are the CANCELLATION term: u (E2 + mean^2) stands against var = E2 - mean^2, so a row with |mean| >> std has a
    bound on var (and through _rstd_interval on rstd) that is (E2 + mean^2) / var times the two-pass one -- it is carried as such, not
    folded into a constant.  Returns ((rstd, mean rstd), (bound, bound))."""
    p = part.double()
    slots = part.shape[0]
    m = (p[:, :, 0].sum(0) / n)[:, None]
    e2 = (p[:, :, 1].sum(0) / n)[:, None]
    var = (e2 - m * m).clamp_min(0.0)
    dm = _gamma(slots) * (p[:, :, 0].abs().sum(0) / n)[:, None]
    de = _gamma(slots) * (p[:, :, 1].abs().sum(0) / n)[:, None]
    mm = (m.abs() + dm) ** 2
    dvar = de + dm * (2.0 * m.abs() + dm) + U32 * mm + U32 * (e2 + de + (1.0 + U32) * mm)
    rstd, dr = _rstd_interval(var, dvar, eps)
    return (rstd[:, 0], (m * rstd)[:, 0]), (dr[:, 0], ((m.abs() + dm) * (rstd + dr) * (1.0 + U32) - m.abs() * rstd)[:, 0])


ROW_KINDS = ("gaussian", "mean >> std", "constant", "outlier", "small")


def ln_rows(rows: int, seed: int, device="cpu", kind0: int = 0) -> torch.Tensor:
    """fp32 (rows, 1024); row r is of kind ROW_KINDS[(r + kind0) % 5]: Gaussian (mean 0.5, std 3); |mean| >> std (mean +-50, std 0.1 -- the
    trained-tower regime, where a one-pass variance loses its digits); constant (variance exactly 0); Gaussian with one 3e3 outlier;
    Gaussian of scale 1e-2."""
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn((rows, HIDDEN), generator=g, device=device)
    r = torch.arange(rows, device=device)
    kind = ((r + kind0) % 5)[:, None]
    sign = (1.0 - 2.0 * ((r // 5) % 2).float())[:, None]
    const = (torch.tensor([50.0, -3.25, 0.0, 1.0e-3, 1.0 / 3.0, -777.0], device=device)[(r // 5) % 6])[:, None]
    col = torch.arange(HIDDEN, device=device)[None, :]
    spike = (col == ((r * 37) % HIDDEN)[:, None]).float() * 3.0e3
    x = torch.where(kind == 0, x * 3.0 + 0.5, torch.where(kind == 1, sign * 50.0 + 0.1 * x, torch.where(
        kind == 2, const.expand(rows, HIDDEN), torch.where(kind == 3, x + spike, x * 1.0e-2))))
    return x.contiguous()


def ln_affine(seed: int, device="cpu"):
    """Jittered LayerNorm parameters: gamma = 1 + 0.1 N(0, 1), beta = 0.05 N(0, 1) -- a parameter read from the neighbouring lane shows."""
    g = torch.Generator(device=device).manual_seed(seed)
    return (1.0 + 0.1 * torch.randn(HIDDEN, generator=g, device=device)).contiguous(), (0.05 * torch.randn(HIDDEN, generator=g, device=device)).contiguous()


def _ln_where(row: int, col: int, kind0: Optional[int]) -> str:
    k = "" if kind0 is None else f", a '{ROW_KINDS[(row + kind0) % 5]}' row"
    return f"row {row} (token {row % TOKENS} of image {row // TOKENS}{k}) col {col} (lane {col % 256 // 4}, load {col // 256})"


def compare_values(name: str, got: torch.Tensor, want: torch.Tensor, tol: torch.Tensor, r0: int = 0, kind0: Optional[int] = None,
                   limit: int = 4) -> List[str]:
    """|got - want| <= tol per element (a NaN or Inf anywhere fails); findings name the row, its kind and the column."""
    g = got.double()
    err = (g - want).abs()
    bad = ~(err <= tol)
    f = [f"{name}: got {float(g[i, j])!r} want {float(want[i, j])!r} (bound {float(tol[i, j] if tol.dim() == 2 else tol):.3e}) at " + _ln_where(r0 + i, j, kind0)
         for (i, j) in _first(bad, limit)]
    if f:
        rows = bad.any(1).nonzero().flatten()
        f.append(f"{name}: {int(bad.sum())} elements outside their bound in rows {r0 + int(rows[0])} .. {r0 + int(rows[-1])}")
    return f


def compare_layernorm(got: torch.Tensor, x: torch.Tensor, gamma, beta, eps: float, out, kind0: Optional[int] = None,
                      chunk: int = 16384, limit: int = 4, name: str = "layernorm", worst: Optional[list] = None) -> List[str]:
    """got = what a LayerNorm kernel wrote for the rows x (+ sentinel guard rows behind them), per element within layernorm_bound.
    out: torch.float32 / float16 / bfloat16 (+ half an ulp of the type at |y| + bound) or "x3": a triple (rows, 3072), which must be
    triple_consistent and whose hi + lo gets triple_recon_bound on top.  No element is excluded.  worst (a list): receives the largest
    error / bound ratio."""
    rows = x.shape[0]
    f: List[str] = []
    for r0 in range(0, rows, chunk):
        r1 = min(rows, r0 + chunk)
        y, b = layernorm_bound(x[r0:r1], gamma, beta, eps)
        if out == "x3":
            fc, val = triple_consistent(got[r0:r1], HIDDEN, limit=limit)
            f += [f"{name} rows {r0}..: {m}" for m in fc]
            b = b + triple_recon_bound(y.abs() + b)
        else:
            val = got[r0:r1].double()
            if out != torch.float32:
                b = b + half_ulp16(y.abs() + b, out)
        f += compare_values(name, val, y, b, r0, kind0, limit)
        if worst is not None:
            worst.append(float(torch.nan_to_num((val - y).abs() / b, nan=float("inf")).max()))
        if len(f) > 40:
            return f
    gr = got[rows:]
    if gr.numel() and not bool((_halves(gr).double() == SENTINEL).all()):
        f.append(f"{name}: guard rows past row {rows} written at (row - {rows}, col) {_first(_halves(gr).double() != SENTINEL, limit)}")
    return f


def compare_rowstat(name: str, got: torch.Tensor, ref, bound, kind0: Optional[int] = None, limit: int = 4) -> List[str]:
    """got (rows, 2) = (rstd, mean rstd) against (ref, bound) of rowstat_bound / rowstat_finalize_bound."""
    f = []
    for c, what in enumerate(("rstd", "mean*rstd")):
        err = (got[:, c].double() - ref[c]).abs()
        bad = ~(err <= bound[c])
        for (i,) in _first(bad, limit):
            k = "" if kind0 is None else f" ('{ROW_KINDS[(i + kind0) % 5]}')"
            f.append(f"{name} {what}: got {float(got[i, c])!r} want {float(ref[c][i])!r} (bound {float(bound[c][i]):.3e}) at row {i}{k}, 256-row block {i // 256} +{i % 256}")
        if bad.any():
            f.append(f"{name} {what}: {int(bad.sum())} rows outside their bound")
    return f


def statparts_of(x: torch.Tensor, slots: int = 16) -> torch.Tensor:
    """(slots, rows, 2) fp32: per 64-column slice (sum, sum of squares) of the rows x, formed in fp64 and rounded once -- the layout the
    RESID_STAT epilogue hands rowstat_finalize (slot-major)."""
    xs = x.double().reshape(x.shape[0], slots, -1)
    return torch.stack([xs.sum(2), (xs * xs).sum(2)], dim=2).permute(1, 0, 2).float().contiguous()


# ================================================================================================================ im2col, sum of parts
PATCH_K, PATCH_KPAD = 588, 640


def im2col_ref(pixels: torch.Tensor) -> torch.Tensor:
    """(n, 3, 336, 336) -> (n 576, 588) fp32: row = image 576 + py 24 + px, column k = c 196 + ky 14 + kx (Conv2d's weight flattened),
    through torch's unfold on the pixels widened to fp32 (exact for every pixel type)."""
    n = pixels.shape[0]
    u = torch.nn.functional.unfold(pixels.float(), kernel_size=14, stride=14)            # (n, 588, 576)
    return u.transpose(1, 2).reshape(n * PATCHES, PATCH_K).contiguous()


def im2col_where(row: int, col: int) -> str:
    p = row % PATCHES
    return f"(image {row // PATCHES} patch row {p // 24} patch col {p % 24}; channel {col // 196} ky {col % 196 // 14} kx {col % 14})"


def compare_im2col(got: torch.Tensor, pixels: torch.Tensor, limit: int = 4) -> List[str]:
    """got (n 576 + guard rows, 640) 16-bit against unfold rounded to got's type: equal, pad columns 588..639 zero, guard rows untouched."""
    want = im2col_ref(pixels)
    if got.dtype == torch.float16:
        want = want.clamp(-F16_MAX, F16_MAX)
    want = want.to(got.dtype)
    rows = want.shape[0]
    f = []
    bad = _bits(got[:rows, :PATCH_K]) != _bits(want)
    for (i, j) in _first(bad, limit):
        f.append(f"im2col: got {float(got[i, j])!r} want {float(want[i, j])!r} at row {i} col {j} " + im2col_where(i, j))
    if bad.any():
        f.append(f"im2col: {int(bad.sum())} wrong elements")
    if bool((_bits(got[:rows, PATCH_K:]) != 0).any()):
        f.append(f"im2col: pad columns not zero at (row, col - 588) {_first(_bits(got[:rows, PATCH_K:]) != 0, limit)}")
    if got.shape[0] > rows and not bool((got[rows:].float() == SENTINEL).all()):
        f.append(f"im2col: guard rows written at {_first(got[rows:].float() != SENTINEL, limit)}")
    return f


def representable_pixels(n: int, seed: int, device="cpu") -> torch.Tensor:
    """fp32 pixels (n, 3, 336, 336) that are exact in fp16 AND bf16 (multiples of 1/16 in [-8, 8)): every (pixel type, operand type) pair
    then has one right answer.  Neighbouring pixels, rows, channels and images differ."""
    g = torch.Generator(device=device).manual_seed(seed)
    return (torch.randint(-128, 128, (n, 3, 336, 336), generator=g, device=device).float() / 16.0).contiguous()


def sum_parts_ref(parts: torch.Tensor, dst0: Optional[torch.Tensor]) -> torch.Tensor:
    """((p0 + p1) + p2) ... in fp32, then dst0 + that: the additions of sum_parts_kernel in its order, with torch on the CPU (IEEE
    single additions, nothing to contract)."""
    p = parts.detach().cpu().float()
    acc = p[0].clone()
    for k in range(1, p.shape[0]):
        acc = acc + p[k]
    return acc if dst0 is None else dst0.detach().cpu().float() + acc
