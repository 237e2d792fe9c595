"""The fast tier's 16-bit chain restated in fp64 (torch only; test infrastructure, no kernel and no product code is used).

pg_vit_forward / pg_vit_forward_hidden is the ViT-L/14-336 encoder with 16-bit MFMA operands.  `fast_hidden` is the same network in
fp64 arithmetic that rounds ONLY where the product rounds -- read from csrc/vit.hip (the chain), csrc/vit_weights.hip (the load-time packing of the
weights), csrc/gemm_epi.h (the epilogues), csrc/rowops.hip (im2col, pre-LayerNorm, LayerNorm, row statistics, token mean) and
csrc/attention.hip:

  patch      im2col pixels and patch weights rounded to 16 bit; X = acc + position (fp32 store); class row = cls + pos[0] (one fp32
             addition); pre-LayerNorm in place (fp32 store)
  QKV / fc1  separate chain: A = round16(LN(x) gamma + beta), W = round16(W), y = acc + b
             folded chain:   A = round16(x) -- the RAW residual row --, W' = round16(gamma o W), colsum = sum_k W' (of the ROUNDED
             values), c = beta.W^T + b, and y = rstd acc - (mean rstd) colsum + c with (rstd, mean rstd) of the fp32 row, stored fp32
  attention  Q scaled by log2(e) / 8 BEFORE its rounding; K, V rounded; softmax in base 2; P rounded to the operand type for keys
             0 .. 575 (they go through the MFMAs, and the row sum is the sum of the ROUNDED P: it comes out of the matrix pipe too)
             against the lazy reference maximum -- that of the query's first 64-key tile, raised only where a later tile exceeds it by
             more than 2^8 --, key 576 is a VALU step whose p stays fp32; the output rounded
  fc1        QuickGELU of y, rounded
  out / fc2  x = x + (acc + b), ONE rounding to fp32 per GEMM (the residual stream is fp32; the last layer's fc2 writes no 16-bit copy)
  embedding  the token mean, rounded to fp32

A value the product holds in fp32 before it rounds it to 16 bit is rounded fp64 -> fp32 -> 16 bit here too (and fp16 saturates at
+-65504 as pack16x2 does).  NOT modelled, and what the factor 2 of the bounds pays for: the fp32 accumulation order inside the MFMAs,
v_exp_f32 and the reciprocals, the one-pass (sum, sum of squares) form of the folded statistics in fp32, the fp32 rescales of the
attention's accumulators when the reference maximum is raised.

`compare_hidden` is the comparator of tests/test_gpu_fast_tier.py: every row of every image, and every embedding, against the fp64
oracle; tests/test_fastref_cpu.py shows that the restatement is the network and that the comparator sees the mistakes it is meant for."""
import math
from typing import Callable, Dict, List, Optional

import torch
import torch.nn.functional as F

TOKENS, PATCHES, HEADS, HDIM, HIDDEN, MLP = 577, 576, 16, 64, 1024, 4096
F16_MAX = 65504.0
LN_EPS = 1e-5
EMB_TOL = 1e-3            # the project's contract for a fast-tier embedding (BASELINE.json north_star)
LOG2E = math.log2(math.e)
ATT_LAZY_THR = 8.0        # csrc/attention_common.h: the softmax reference is raised when a tile's maximum exceeds it by more than 2^8
# kQScale of csrc/vit.hip: 0.125f * 1.4426950408889634f, a product of two floats
QSCALE_F32 = float(torch.tensor(0.125, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32))


def _strip(sd):
    return {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in sd.items()}


class _Rounding:
    """The two roundings of the chain: r16 (an MFMA operand / a 16-bit store) and r32 (an fp32 store); both the identity when off."""

    def __init__(self, dtype: Optional[torch.dtype]):
        assert dtype in (None, torch.float16, torch.bfloat16)
        self.dtype = dtype

    def r16(self, x: torch.Tensor) -> torch.Tensor:
        if self.dtype is None:
            return x
        y = x.to(torch.float32)
        if self.dtype == torch.float16:
            y = y.clamp(-F16_MAX, F16_MAX)
        return y.to(self.dtype).to(torch.float64)

    def r32(self, x: torch.Tensor) -> torch.Tensor:
        return x if self.dtype is None else x.to(torch.float32).to(torch.float64)


def _ln_stats(x: torch.Tensor):
    """(mean, rstd) of every row, biased variance, as layernorm_kernel / preln_kernel / rowstat_finalize_kernel mean them."""
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    return mean, 1.0 / torch.sqrt(var + LN_EPS)


def _layernorm(x, g, b):
    mean, rstd = _ln_stats(x)
    return (x - mean) * rstd * g + b


class _Weights:
    """The parameters as pg_vit_finalize packs them (fold_ln, host_cvt), in fp64 on `device`; built once per (chain, type)."""

    def __init__(self, sd: Dict[str, torch.Tensor], ln_fold: bool, R: _Rounding, device):
        sd = {k: v.to(device=device, dtype=torch.float64) for k, v in _strip(sd).items() if torch.is_tensor(v) and v.is_floating_point()}
        self.layers = 0
        while f"encoder.layers.{self.layers}.layer_norm1.weight" in sd:
            self.layers += 1
        self.ln_fold = ln_fold
        self.wpatch = R.r16(sd["embeddings.patch_embedding.weight"].reshape(HIDDEN, -1))
        self.cls, self.pos = sd["embeddings.class_embedding"], sd["embeddings.position_embedding.weight"]
        self.preg, self.preb = sd["pre_layrnorm.weight"], sd["pre_layrnorm.bias"]
        self.L = []
        for i in range(self.layers):
            p = f"encoder.layers.{i}."
            wqkv = torch.cat([sd[p + f"self_attn.{n}_proj.weight"] for n in "qkv"], 0)
            bqkv = torch.cat([sd[p + f"self_attn.{n}_proj.bias"] for n in "qkv"], 0)
            l = dict(wo=R.r16(sd[p + "self_attn.out_proj.weight"]), bo=sd[p + "self_attn.out_proj.bias"],
                     w2=R.r16(sd[p + "mlp.fc2.weight"]), b2=sd[p + "mlp.fc2.bias"])
            for name, W, b, g, be in (("qkv", wqkv, bqkv, sd[p + "layer_norm1.weight"], sd[p + "layer_norm1.bias"]),
                                      ("fc1", sd[p + "mlp.fc1.weight"], sd[p + "mlp.fc1.bias"], sd[p + "layer_norm2.weight"], sd[p + "layer_norm2.bias"])):
                if ln_fold:                                    # fold_ln: W' = cvt(W gamma), colsum of the rounded W', c = beta.W^T + b (both stored fp32)
                    wf = R.r16(W * g[None, :])
                    l[name] = dict(w=wf, colsum=R.r32(wf.sum(1)), c=R.r32(W @ be + b))
                else:
                    l[name] = dict(w=R.r16(W), b=b, g=g, be=be)
            self.L.append(l)


def _attention(q, k, v, R: _Rounding):
    """q (already scaled by log2(e) / 8 and rounded), k, v: (n, 577, 1024) -> the attention output (n, 577, 1024), rounded."""
    n = q.shape[0]
    q, k, v = [t.view(n, TOKENS, HEADS, HDIM).transpose(1, 2) for t in (q, k, v)]
    s = q @ k.transpose(-1, -2)                                    # base-2 scores
    # The reference each P is rounded against (att8_softmax): the maximum of the query's first 64-key tile, raised to a later tile's
    # maximum only where that exceeds it by more than ATT_LAZY_THR.  P of tile t is rounded as exp2(s - m_t); a later raise rescales
    # the fp32 accumulators, not the rounded values: the weight of a key is round16(exp2(s - m_t)) exp2(m_t - top).
    tiles = s[..., :TOKENS - 1].reshape(n, HEADS, TOKENS, 9, 64).max(-1).values
    m, refs = tiles[..., 0], []
    for t in range(9):
        if t:
            m = torch.where(tiles[..., t] - m > ATT_LAZY_THR, tiles[..., t], m)
        refs.append(m)
    mk = torch.stack(refs, -1).repeat_interleave(64, dim=-1)       # (n, 16, 577, 576): the reference in force at each key
    top = s.max(-1, keepdim=True).values
    pm = R.r16(torch.exp2(s[..., :TOKENS - 1] - mk)) * torch.exp2(mk - top)   # keys 0 .. 575: the P operand of the PV MFMA
    pl = torch.exp2(s[..., TOKENS - 1:] - top)                     # key 576: fp32 on the VALU
    o = (pm @ v[:, :, :TOKENS - 1] + pl * v[:, :, TOKENS - 1:]) / (pm.sum(-1, keepdim=True) + pl)
    return R.r16(o.transpose(1, 2).reshape(n, TOKENS, HIDDEN))


def _forward_chunk(W: _Weights, px: torch.Tensor, R: _Rounding, exact_scale: bool, rowstat_hook, detail):
    n = px.shape[0]
    a = R.r16(F.unfold(px.to(torch.float64), 14, stride=14).transpose(1, 2))        # (n, 576, 588), k = c 196 + ky 14 + kx
    x = torch.empty((n, TOKENS, HIDDEN), dtype=torch.float64, device=px.device)
    x[:, 1:] = R.r32(a @ W.wpatch.t() + W.pos[1:][None])
    x[:, 0] = R.r32(W.cls + W.pos[0])
    x = R.r32(_layernorm(x, W.preg, W.preb))
    qs = LOG2E / 8.0 if exact_scale else QSCALE_F32

    def ln_gemm(x, l, layer, name):
        """QKV / fc1 before their activation: the value the epilogue holds in fp32."""
        if not W.ln_fold:
            return R.r16(_layernorm(x, l["g"], l["be"])) @ l["w"].t() + l["b"]
        mean, rstd = _ln_stats(x)
        rstd, mrs = R.r32(rstd), R.r32(mean * rstd)               # rowstat [M][2] fp32
        if rowstat_hook is not None:
            rstd, mrs = rowstat_hook(layer, name, rstd, mrs)
        return rstd * (R.r16(x) @ l["w"].t()) - mrs * l["colsum"] + l["c"]

    for i, l in enumerate(W.L):
        y = ln_gemm(x, l["qkv"], i, "qkv")
        q, k, v = R.r16(y[..., :HIDDEN] * qs), R.r16(y[..., HIDDEN:2 * HIDDEN]), R.r16(y[..., 2 * HIDDEN:])
        o = _attention(q, k, v, R)
        x = R.r32(x + (o @ l["wo"].t() + l["bo"]))
        y = ln_gemm(x, l["fc1"], i, "fc1")
        g = R.r16(y * torch.sigmoid(1.702 * y))
        if detail is not None and i + 1 == W.layers:
            detail.setdefault("before_last_fc2", []).append(x.clone())
        x = R.r32(x + (g @ l["w2"].t() + l["b2"]))
    return x


@torch.no_grad()
def fast_hidden(sd: Dict[str, torch.Tensor], pixels: torch.Tensor, ln_fold: bool = True, dtype: Optional[torch.dtype] = torch.float16,
                chunk: int = 8, rowstat_hook: Optional[Callable] = None, detail: Optional[dict] = None):
    """The fast tier's last hidden state (n, 577, 1024) and its token mean (n, 1024), both fp64 tensors on the pixels' device.

    ln_fold: the LayerNorm-folded chain (the product default) or the separate-LayerNorm chain (PIGEON_LN_FOLD=0).
    dtype:   torch.float16 / torch.bfloat16: the operand type; None: every rounding switched off (the plain network in fp64).
    chunk:   images per pass (at most 8: the attention scores of one image are 43 MB in fp64).
    rowstat_hook(layer, "qkv" | "fc1", rstd, mrs) -> (rstd, mrs): folded chain only, for planting a mistake in a test.
    detail:  a dict that receives "before_last_fc2" (n, 577, 1024): the residual stream the last fc2 adds to."""
    assert 1 <= chunk <= 8 and pixels.dim() == 4 and tuple(pixels.shape[1:]) == (3, 336, 336)
    R = _Rounding(dtype)
    W = _Weights(sd, ln_fold, R, pixels.device)
    hs = [_forward_chunk(W, pixels[i:i + chunk], R, dtype is None, rowstat_hook, detail) for i in range(0, pixels.shape[0], chunk)]
    h = torch.cat(hs, 0)
    if detail is not None:
        detail["before_last_fc2"] = torch.cat(detail["before_last_fc2"], 0)
    return h, R.r32(h.mean(1))


# ------------------------------------------------------------------------------------------------ errors, bounds, the comparator
def row_errors(h: torch.Tensor, ref: torch.Tensor) -> torch.Tensor:
    """(n, 577): ||h - ref|| / ||ref|| of every hidden row; computed image by image (fp64 copies of one image at a time)."""
    out = torch.empty(h.shape[:2], dtype=torch.float64, device=ref.device)
    for i in range(h.shape[0]):
        r = ref[i].to(torch.float64)
        out[i] = (h[i].to(device=ref.device, dtype=torch.float64) - r).norm(dim=1) / r.norm(dim=1)
    return out


def emb_errors(e: torch.Tensor, ref_e: torch.Tensor) -> torch.Tensor:
    r = ref_e.to(torch.float64)
    return (e.to(device=r.device, dtype=torch.float64) - r).norm(dim=1) / r.norm(dim=1)


def bounds(rest_h: torch.Tensor, rest_e: torch.Tensor, ref_h: torch.Tensor, cap_emb: bool = True) -> dict:
    """The bounds a kernel is held to, from the RESTATEMENT's error against the fp64 oracle (never from a kernel's):
    row_tol = 2 max E_row, emb_tol = min(2 max E_emb, EMB_TOL) (cap_emb=False: bf16, which has its own documented floor).
    The factor 2 is the margin the project gives a kernel over a plain statement of the same arithmetic
    (test_launch_gaussian_512_images: kernel <= 2 x sequential fp32); it pays for what the restatement does not model."""
    er, ee = row_errors(rest_h, ref_h), emb_errors(rest_e, ref_h.mean(1))
    emb_tol = 2.0 * float(ee.max())
    return dict(row_tol=2.0 * float(er.max()), emb_tol=min(emb_tol, EMB_TOL) if cap_emb else emb_tol,
                row_max=float(er.max()), row_median=float(er.median()), row_min=float(er.min()), emb_max=float(ee.max()), emb_min=float(ee.min()))


def compare_hidden(got: torch.Tensor, ref: torch.Tensor, row_tol: float, emb_tol: float, emb: Optional[torch.Tensor] = None,
                   label: str = "", limit: int = 8, worst: Optional[dict] = None) -> List[str]:
    """got (n, 577, 1024) against the fp64 reference `ref` (at least n images): EVERY row of EVERY image within row_tol, every embedding
    (`emb` as delivered, else got's token mean) within emb_tol of ref's token mean, relative 2-norms; NaN fails.  Returns the findings:
    the first `limit` bad rows by position -- image, token, row of the batch and 256-row tile, the geometry of the persistent GEMMs --, a
    count with the extent of the rest, and the bad embeddings.  worst: receives 'row' and 'emb', the largest errors seen."""
    n = got.shape[0]
    assert tuple(got.shape[1:]) == (TOKENS, HIDDEN) and ref.shape[0] >= n and tuple(ref.shape[1:]) == (TOKENS, HIDDEN)
    er = torch.nan_to_num(row_errors(got, ref[:n]), nan=float("inf"))
    e = got.to(torch.float64).mean(1) if emb is None else emb
    ee = torch.nan_to_num(emb_errors(e, ref[:n].to(torch.float64).mean(1)), nan=float("inf"))
    if worst is not None:
        worst["row"], worst["emb"] = float(er.max()), float(ee.max())
    found, pre = [], (label + ": " if label else "")
    bad = (~(er <= row_tol)).nonzero()
    for (i, t) in bad[:limit].tolist():
        r = i * TOKENS + t
        found.append(f"{pre}image {i} token {t} (row {r}, 256-row tile {r // 256} +{r % 256}) hidden-row error {float(er[i, t]):.3e} > {row_tol:.3e}")
    if bad.shape[0] > limit:
        rows = bad[:, 0] * TOKENS + bad[:, 1]
        found.append(f"{pre}{bad.shape[0]} bad rows in all, in {int(bad[:, 0].unique().numel())} images, rows {int(rows.min())} .. {int(rows.max())} "
                     f"(256-row tiles {int(rows.min()) // 256} .. {int(rows.max()) // 256}), worst {float(er.max()):.3e}")
    for i in (~(ee <= emb_tol)).nonzero().flatten()[:limit].tolist():
        found.append(f"{pre}image {i} embedding error {float(ee[i]):.3e} > {emb_tol:.3e}")
    return found
