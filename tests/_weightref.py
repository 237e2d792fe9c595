"""numpy restatement of what pg_vit_finalize leaves on the device and of pg_vit_fingerprint, written from the comments of
include/pigeon_hip.h, csrc/vit_handle.h and csrc/vit_weights.hip (the fingerprint's buffer order, seeds and table) and from the
transformers state-dict layout -- not from the packing code.  Everything here is host arithmetic on a few dozen MB; every buffer
can be compared with the library's bit for bit (tests/test_gpu_weights.py), and tests/test_weightref_cpu.py shows that these buffers
are the network and that a comparison against them reports the slips it is meant for.

Buffers, in the fingerprint's numbering (group 0 = the embeddings, group l + 1 = encoder layer l; seed = (group << 8) | slot):

    group 0      0 patch weight 16-bit [1024][640] (588 columns, zero padded)   1 class embedding   2 position embedding [577][1024]
                 3 pre_layrnorm weight   4 its bias   | 5 patch triple [1024][3 * 640] (precise)   6 the normalisation table (not restated:
                 the library's own pg_prep_norm_lut is the reference)
    group l + 1  0 q|k|v weight 16-bit [3072][1024]   1 its bias   2 its column sums (fold only)   3 out_proj weight   4 its bias
                 5 fc1 weight [4096][1024]   6 its bias   7 its column sums (fold only)   8 fc2 weight [1024][4096]   9 its bias
                 10..13 layer_norm1 weight, bias, layer_norm2 weight, bias
                 | 14..17 the triples of q|k|v, out_proj, fc1, fc2   18 the raw q|k|v bias   19 the raw fc1 bias (precise)

With the fold, a folded weight is W' = cvt(fp32(W * gamma)) (ONE fp32 rounding, then the 16-bit one), its column sums are the sums of
the ROUNDED W' over k, and its bias is beta . W^T + b accumulated in double over k in order.  A triple is [Wh | Wh | f16((W - Wh) 2^8)]
of the UNFOLDED weight.  fp16 conversions saturate at +-65504 and round to nearest even; bf16 rounds to nearest even on the bit pattern.

`WeightRef` keeps each step in a method of its own, so that a test can derive a deliberately wrong variant by overriding one."""
import math

import numpy as np

import _fpref

D, F, TOKENS, PATCH_K, PATCH_KPAD = 1024, 4096, 577, 588, 640
PG_DTYPE_BF16, PG_DTYPE_F16 = 1, 2
MAGIC = int.from_bytes(b"PGVITFP1", "little")
EMBED_FP_SLOTS, LAYER_FP_SLOTS = 5, 14                          # the slots below these are the fingerprint's; the rest continue the numbering
EMBED_SLOTS, LAYER_SLOTS = 7, 20
NAMES = {0: ["patch", "class_embedding", "position_embedding", "pre_layrnorm.weight", "pre_layrnorm.bias", "patch triple", "norm table"]}
LAYER_NAMES = ["wqkv", "bqkv", "qkv colsum", "wo", "bo", "w1", "b1", "fc1 colsum", "w2", "b2", "ln1.weight", "ln1.bias", "ln2.weight",
               "ln2.bias", "wqkv triple", "wo triple", "w1 triple", "w2 triple", "bqkv raw", "b1 raw"]


def slot_name(group, slot):
    return NAMES[0][slot] if group == 0 else f"layer {group - 1} {LAYER_NAMES[slot]}"


def f32(a):
    return np.ascontiguousarray(np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, dtype=np.float32))


def f16_bits(x):
    """fp32 -> fp16 bits: clip to +-65504, then IEEE round to nearest even (NaN stays NaN, -0 stays -0, below 2^-25 flushes to +-0)."""
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.clip(x, np.float32(-65504.0), np.float32(65504.0)).astype(np.float16).view(np.uint16)


def bf16_bits(x):
    """fp32 -> bf16 bits: round to nearest even on the integer pattern (+-Inf stay, a carry out of the mantissa may reach Inf); a NaN
    keeps its upper 16 bits with the quiet bit set."""
    u = np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = ((u + 0x7FFF + ((u >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) & np.uint64(0xFFFF)
    return np.where(nan, (u >> np.uint64(16)) | np.uint64(0x40), r).astype(np.uint16)


def bits_to_f64(dtype, b):
    b = np.ascontiguousarray(b, dtype=np.uint16)
    if dtype == "f16":
        return b.view(np.float16).astype(np.float64)
    return (b.astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def rows_sum_exactly_in_double(v64):
    """Per row of float64 values: True where a double sum of the row is exact IN ANY ORDER -- every term is a multiple of the row's
    smallest quantum and every partial sum fits 53 bits: (largest exponent - smallest non-zero exponent) + 8 mantissa bits + 10 bits
    for up to 1024 terms <= 52.  Rows with a non-finite term are True (their sum is that Inf / NaN in any order, as long as the row
    holds one kind of it -- the planted inputs keep each extreme in a row of its own)."""
    v = np.abs(np.asarray(v64, dtype=np.float64))
    fin = np.isfinite(v).all(axis=1)
    _, e = np.frexp(np.where(np.isfinite(v), v, 0.0))
    nz = v != 0
    big = np.where(nz, e, -10 ** 6).max(axis=1)
    small = np.where(nz, e, 10 ** 6).min(axis=1)
    return ~fin | ~nz.any(axis=1) | (big - small + 8 + 10 <= 52)


class WeightRef:
    def __init__(self, state_dict, layers, dtype="f16", fold=True, precise=False):
        assert dtype in ("f16", "bf16")
        self.layers, self.dtype, self.fold_on, self.precise = int(layers), dtype, bool(fold), bool(precise)
        self.sd = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v for k, v in state_dict.items()}

    # ---- the steps
    def f16(self, x):
        return f16_bits(x)

    def cvt(self, x):
        return self.f16(x) if self.dtype == "f16" else bf16_bits(x)

    def scaled(self, W, gamma):
        """16-bit bits of gamma o W: the fp32 product (one rounding), then the conversion."""
        with np.errstate(over="ignore", invalid="ignore"):
            return self.cvt(np.float32(W) * np.float32(gamma)[None, :])

    def colsum(self, w16, W, gamma):
        """float32 of the exact sum over k of the ROUNDED row (math.fsum: the correctly rounded double of the exact sum, which IS the
        exact sum wherever rows_sum_exactly_in_double holds -- always for fp16: multiples of 2^-24 below 2^16, 1024 of them)."""
        v = bits_to_f64(self.dtype, w16)
        out = np.empty(v.shape[0], dtype=np.float64)
        for n, row in enumerate(v.tolist()):
            try:
                out[n] = math.fsum(row)
            except (ValueError, OverflowError):                 # +Inf and -Inf in one row
                out[n] = math.nan
        with np.errstate(over="ignore", invalid="ignore"):
            return out.astype(np.float32)

    def cbias(self, W, b, beta):
        """beta . W^T + b in double, k in order (each product of two fp32 values is exact in double), then float32."""
        Wt = np.ascontiguousarray(np.float64(W).T)
        b64 = np.float64(beta)
        c = np.zeros(W.shape[0], dtype=np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            for k in range(W.shape[1]):
                c += b64[k] * Wt[k]
            return (c + np.float64(b)).astype(np.float32)

    def qkv(self, q, k, v):
        return np.concatenate([q, k, v], axis=0)

    def padded(self, w16, kpad):
        out = np.zeros((w16.shape[0], kpad), dtype=np.uint16)
        out[:, :w16.shape[1]] = w16
        return out

    def triple(self, W, kpad=None):
        """[Wh | Wh | f16((W - float(Wh)) * 256)], each segment zero padded from K to kpad columns; the same saturating conversion twice."""
        W = np.float32(W)
        hb = self.f16(W)
        with np.errstate(over="ignore", invalid="ignore"):
            lo = self.f16((W - hb.view(np.float16).astype(np.float32)) * np.float32(256.0))
        kpad = kpad or W.shape[1]
        return np.concatenate([self.padded(hb, kpad), self.padded(hb, kpad), self.padded(lo, kpad)], axis=1)

    def in_fingerprint(self, group, slot):
        return slot < (EMBED_FP_SLOTS if group == 0 else LAYER_FP_SLOTS)

    # ---- the buffers
    def p(self, name):
        return f32(self.sd[name])

    def buffers(self):
        """[(group, slot, seed, ndarray)] in order: uint16 arrays for the 16-bit buffers, float32 for the others; a slot this
        configuration does not have is left out."""
        out = []

        def add(g, s, a):
            out.append((g, s, (g << 8) | s, np.ascontiguousarray(a)))

        wp = self.p("embeddings.patch_embedding.weight").reshape(D, PATCH_K)
        add(0, 0, self.padded(self.cvt(wp), PATCH_KPAD))
        add(0, 1, self.p("embeddings.class_embedding").reshape(D))
        add(0, 2, self.p("embeddings.position_embedding.weight").reshape(TOKENS, D))
        add(0, 3, self.p("pre_layrnorm.weight"))
        add(0, 4, self.p("pre_layrnorm.bias"))
        if self.precise:
            add(0, 5, self.triple(wp, PATCH_KPAD))
        for l in range(self.layers):
            pre, g = f"encoder.layers.{l}.", l + 1
            P = lambda n: self.p(pre + n)
            wqkv = self.qkv(*(P(f"self_attn.{x}_proj.weight") for x in "qkv"))
            bqkv = self.qkv(*(P(f"self_attn.{x}_proj.bias") for x in "qkv"))
            w1, b1 = P("mlp.fc1.weight"), P("mlp.fc1.bias")
            for s0, W, b, ln in ((0, wqkv, bqkv, "layer_norm1"), (5, w1, b1, "layer_norm2")):
                if self.fold_on:
                    gamma, beta = P(ln + ".weight"), P(ln + ".bias")
                    w16 = self.scaled(W, gamma)
                    add(g, s0, w16)
                    add(g, s0 + 1, self.cbias(W, b, beta))
                    add(g, s0 + 2, self.colsum(w16, W, gamma))
                else:
                    add(g, s0, self.cvt(W))
                    add(g, s0 + 1, b)
                if s0 == 0:
                    add(g, 3, self.cvt(P("self_attn.out_proj.weight")))
                    add(g, 4, P("self_attn.out_proj.bias"))
            add(g, 8, self.cvt(P("mlp.fc2.weight")))
            add(g, 9, P("mlp.fc2.bias"))
            for s, n in ((10, "layer_norm1.weight"), (11, "layer_norm1.bias"), (12, "layer_norm2.weight"), (13, "layer_norm2.bias")):
                add(g, s, P(n))
            if self.precise:
                add(g, 14, self.triple(wqkv))
                add(g, 15, self.triple(P("self_attn.out_proj.weight")))
                add(g, 16, self.triple(w1))
                add(g, 17, self.triple(P("mlp.fc2.weight")))
                add(g, 18, bqkv)
                add(g, 19, b1)
        return out

    # ---- the fingerprint
    def table(self, bufs):
        """The 'PGVITFP1' table of 64-bit words over the buffers of the fingerprint's slots among `bufs`, in their order."""
        fp = [(g, s, seed, a) for (g, s, seed, a) in bufs if self.in_fingerprint(g, s)]
        t = [MAGIC, self.layers, PG_DTYPE_F16 if self.dtype == "f16" else PG_DTYPE_BF16, 1 if self.fold_on else 0, len(fp)]
        for (_, _, seed, a) in fp:
            t += [seed, a.nbytes, *_fpref.fingerprint(a, seed)]
        return np.array(t, dtype=np.uint64)

    def fingerprint(self, bufs=None):
        return _fpref.fingerprint(self.table(self.buffers() if bufs is None else bufs).astype("<u8"), 0)


def restate(state_dict, layers, dtype="f16", fold=True, precise=False, cls=WeightRef):
    """-> ([(group, slot, seed, ndarray)], (fp0, fp1))"""
    r = cls(state_dict, layers, dtype, fold, precise)
    bufs = r.buffers()
    return bufs, r.fingerprint(bufs)


def first_difference(got, want):
    """got, want: arrays of one buffer (any shapes of equal size, 16- or 32-bit) compared as integers -> None, or (row, column, got
    bits, wanted bits) of the first differing element in `want`'s 2-D shape."""
    w = np.ascontiguousarray(want)
    wi = w.view(np.uint16 if w.itemsize == 2 else np.uint32).reshape(w.shape[0], -1)
    gi = np.ascontiguousarray(got).view(wi.dtype).reshape(-1)
    if gi.size != wi.size:
        return (-1, -1, gi.size, wi.size)
    bad = np.flatnonzero(gi != wi.reshape(-1))
    if bad.size == 0:
        return None
    i = int(bad[0])
    return (i // wi.shape[1], i % wi.shape[1], int(gi[i]), int(wi.reshape(-1)[i]))


def differing(a, b):
    """Names of the buffers in which two restatements' lists differ (a slot missing on one side counts)."""
    da, db = {(g, s): x for g, s, _, x in a}, {(g, s): x for g, s, _, x in b}
    out = []
    for key in sorted(set(da) | set(db)):
        if key not in da or key not in db or first_difference(da[key], db[key]) is not None:
            out.append(slot_name(*key))
    return out


# ------------------------------------------------------------------------------------------------ planted inputs
# Columns that carry planted values (the last one is the matrix's last column: K - 1, next to the patch weight's padding), and the
# LayerNorm gammas of the first 16 of them: powers of two, so that W * gamma is exact and a tie stays a tie through the fold.
PLANT_COLS = [0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 89, 144, 233, 377, 500, -1]
PLANT_GAMMA = [2.0, 0.5, -2.0, -0.5, 2.0, 0.5, -1.0, 1.0, 1.0, -1.0, 1.0, -1.0, 1.0, -1.0, -1.0, -1.0]
_T = 2.0 ** -24                                                  # fp16's subnormal quantum
ROW_FINE = [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), -(1 + 3 * 2.0 ** -11),         # fp16 ties: to even downwards, upwards
            1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8),             # bf16 ties, both directions
            _T, 1.5 * _T, 0.5 * _T, 0.5 * _T * (1 + 2.0 ** -10), -0.25 * _T, 2.0 ** -15 + _T,     # subnormals, their ties, below 2^-25
            0.0, -0.0]                                                                            # ... and the two zeros
ROW_LARGE = [40000.0, 65504.0, -40000.0, 1e5, 65519.996, -70000.0, 65536.0, 65520.0,              # |W| < 65504 < |W gamma| in columns 0 and 2
             -65520.0, 70000.0, 65535.0, -65504.0, 65519.996, -1e5, 131072.0, 65472.0]
ROW_HUGE = [1e30, -1e30, 2.0 ** 100, -2.0 ** 110, 2.0 ** 120, 1e32, -1e35, float(np.finfo(np.float32).max),
            1e38, 3e30, -2.0 ** 101, 2.0 ** 127, 1e31, -1e33, 1e34, -1e36]
# (row, values, keep the rest of the row): the large and huge rows are zero elsewhere, so that a bf16 row sums exactly in double
PLANT_ROWS = [(3, ROW_FINE, True), (4, ROW_LARGE, False), (5, ROW_HUGE, False), (6, [None] * 7 + [math.inf], True),
              (7, [None] * 8 + [-math.inf], True)]
MATRICES = ["self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.out_proj.weight",
            "mlp.fc1.weight", "mlp.fc2.weight"]
NAN_AT = ("encoder.layers.1.mlp.fc2.weight", 900, 4000)


def plant(state_dict):
    """A copy (torch tensors, flat key layout) of `state_dict` with the values above written into rows of their own of every GEMM
    weight -- in another block of rows per matrix and layer -- and power-of-two gammas on their columns; one NaN, in fc2 of layer 1."""
    import torch
    sd = {(k[len("vision_model."):] if k.startswith("vision_model.") else k): v.detach().clone().to(torch.float32) for k, v in state_dict.items()}
    layers = 0
    while f"encoder.layers.{layers}.layer_norm1.weight" in sd:
        layers += 1

    def put(name, base):
        w = sd[name].numpy().reshape(sd[name].shape[0], -1)
        for (r, vals, keep) in PLANT_ROWS:
            if not keep:
                w[base + r, :] = 0.0
            for c, v in zip(PLANT_COLS, vals):
                if v is not None:
                    w[base + r, c] = np.float32(v)

    put("embeddings.patch_embedding.weight", 40)
    for l in range(layers):
        pre = f"encoder.layers.{l}."
        for ln in ("layer_norm1", "layer_norm2"):
            g, b = sd[pre + ln + ".weight"].numpy(), sd[pre + ln + ".bias"].numpy()
            g[PLANT_COLS] = np.float32(PLANT_GAMMA)
            assert (b[PLANT_COLS] != 0).all()                   # (an Inf weight times a zero beta would be a NaN bias)
        for i, m in enumerate(MATRICES):
            put(pre + m, 16 * i + 128 * l)
    name, r, c = NAN_AT
    if name in sd:
        sd[name][r, c] = math.nan
    return sd
