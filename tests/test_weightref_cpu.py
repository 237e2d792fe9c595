"""tests/_weightref.py on the CPU: the restatement of pg_vit_finalize's buffers is the network, its conversions give hand-derived bit
patterns on the planted values, a comparison against it reports the slips it is meant for, and the fingerprints of the calibration
tests' tower are pinned as literals (tests/test_gpu_weights.py holds the library to the same ones)."""
import math

import numpy as np
import pytest

import _weightref as R

# pg_vit_fingerprint of make_vit_weights(seed=11, layers=2, affine_jitter=True) as "%016x%016x", per (operand dtype, LayerNorm fold):
# the meaning of a stored calibration's key.  Computed with the restatement; a change here invalidates every stored calibration.
PINNED = {("f16", True): "2ba26d258475fb70dd433d8ead9d9d8e", ("f16", False): "6d73f3768d079f2652d9e9092447ced1",
          ("bf16", True): "a60ffe6f41354e3c7a6967b6089bb860", ("bf16", False): "52f9663d54bfde681f61bdd5c375b754"}


@pytest.fixture(scope="module")
def sd2():
    from pigeon_amd import synthetic
    return synthetic.make_vit_weights(seed=11, layers=2, affine_jitter=True)


@pytest.fixture(scope="module")
def planted(sd2):
    return R.plant(sd2)


# ------------------------------------------------------------------------------------------------ 1. the restatement is the network
@pytest.mark.parametrize("dtype,u", [("f16", 2.0 ** -11), ("bf16", 2.0 ** -8)])
@pytest.mark.parametrize("which", ["qkv", "fc1"])
def test_folded_buffers_are_layernorm_then_linear(sd2, dtype, u, which):
    """rstd (x . W'^T - mean colsum) + cbias against LN(x) . W^T + b, in fp64, on 200 rows of non-zero mean and 256 output rows:
    equal to the fp32 roundings of colsum and cbias once W' stands for gamma o W, and within the rounding of W' alone of the network."""
    r = R.WeightRef(sd2, 2, dtype, fold=True)
    pre = "encoder.layers.1."
    if which == "qkv":
        W = r.qkv(*(r.p(pre + f"self_attn.{x}_proj.weight")[100:185] for x in "qkv"))
        b = r.qkv(*(r.p(pre + f"self_attn.{x}_proj.bias")[100:185] for x in "qkv"))
        gamma, beta = r.p(pre + "layer_norm1.weight"), r.p(pre + "layer_norm1.bias")
    else:
        W, b = r.p(pre + "mlp.fc1.weight")[1000:1256], r.p(pre + "mlp.fc1.bias")[1000:1256]
        gamma, beta = r.p(pre + "layer_norm2.weight"), r.p(pre + "layer_norm2.bias")
    w16 = r.scaled(W, gamma)
    Wr = R.bits_to_f64(dtype, w16)
    cs, cb = np.float64(r.colsum(w16, W, gamma)), np.float64(r.cbias(W, b, beta))
    rng = np.random.default_rng(3)
    x = rng.standard_normal((200, R.D)) * 2.0 + rng.standard_normal((200, 1)) * 3.0
    mean = x.mean(axis=1, keepdims=True)
    rstd = 1.0 / np.sqrt(x.var(axis=1, keepdims=True) + 1e-5)
    xn = (x - mean) * rstd
    W64, g64 = np.float64(W), np.float64(gamma)
    network = (xn * g64 + np.float64(beta)) @ W64.T + np.float64(b)
    restated = rstd * (x @ Wr.T - mean * cs) + cb
    with_rounded_w = xn @ Wr.T + np.float64(beta) @ W64.T + np.float64(b)
    # the two fp32 roundings (colsum, cbias) and fp64 noise of a 1024-term product
    tol_a = np.abs(mean * rstd) * np.abs(cs) * 2.0 ** -24 + np.abs(cb) * 2.0 ** -24 + 1e-11 * (np.abs(x) @ np.abs(Wr).T) * np.abs(rstd)
    assert (np.abs(restated - with_rounded_w) <= tol_a).all(), float((np.abs(restated - with_rounded_w) / tol_a).max())
    # the rounding of W' alone: each element within u (+ the fp32 product's rounding) of gamma o W, or half an fp16 subnormal quantum
    tol_b = np.abs(xn) @ (np.abs(W64 * g64) * (u + 2.0 ** -23) + 2.0 ** -25).T + tol_a
    err = np.abs(restated - network)
    assert (err <= tol_b).all(), float((err / tol_b).max())
    assert err.max() > 0.01 * tol_b.max() / math.sqrt(R.D)       # ... and the bound is of the size of what it bounds


def test_triple_reconstructs_the_weight(sd2):
    r = R.WeightRef(sd2, 2, "f16", precise=True)
    W = r.p("encoder.layers.0.mlp.fc2.weight")[:300]
    t = r.triple(W).view(np.float16).astype(np.float64)
    K = W.shape[1]
    assert t.shape == (300, 3 * K) and np.array_equal(t[:, :K], t[:, K:2 * K])
    rec = t[:, :K] + t[:, 2 * K:] / 256.0
    # 2^-22 relative; where the low half is an fp16 subnormal, half its quantum: 2^-25 / 256
    assert (np.abs(rec - W) <= np.maximum(2.0 ** -22 * np.abs(W), 2.0 ** -33)).all()
    P = r.triple(r.p("embeddings.patch_embedding.weight").reshape(R.D, R.PATCH_K)[:8], R.PATCH_KPAD)
    assert P.shape == (8, 3 * R.PATCH_KPAD) and not P.reshape(8, 3, R.PATCH_KPAD)[:, :, R.PATCH_K:].any()


# ------------------------------------------------------------------------------------------------ 2. the planted values
def _bits(bufs, group, slot):
    return [a for g, s, _, a in bufs if (g, s) == (group, slot)][0]


def test_planted_values_convert_as_derived_by_hand(planted):
    """The unfolded out_proj weight of layer 0 (rows 48 + 3 .. 48 + 7 carry the planted values): bit patterns worked out by hand."""
    cols = R.PLANT_COLS
    f16 = _bits(R.restate(planted, 1, "f16", fold=False)[0], 1, 3)
    bf16 = _bits(R.restate(planted, 1, "bf16", fold=False)[0], 1, 3)
    fine, large, huge, pinf, ninf = (48 + r for r, _, _ in R.PLANT_ROWS)
    assert f16[fine, cols].tolist() == [0x3C00, 0x3C02, 0xBC00, 0xBC02,      # ties of 1 + {1, 3} 2^-11: to the even neighbour
                                        0x3C04, 0x3C0C, 0xBC04, 0xBC0C,      # 1 + {1, 3} 2^-8 are fp16 numbers
                                        0x0001, 0x0002, 0x0000, 0x0001, 0x8000, 0x0201,      # subnormals: 1, tie 1.5 -> 2, tie 0.5 -> 0, just above -> 1, -0
                                        0x0000, 0x8000]
    assert bf16[fine, cols].tolist() == [0x3F80, 0x3F80, 0xBF80, 0xBF80,     # below bf16's half quantum 2^-9
                                         0x3F80, 0x3F82, 0xBF80, 0xBF82,     # ties of 1 + {1, 3} 2^-8: to the even neighbour
                                         0x3380, 0x33C0, 0x3300, 0x3300, 0xB280, 0x3800,      # no flush: 2^-24, 1.5 2^-24, 2^-25, 2^-25 (1 + 2^-10) -> 2^-25, -2^-26, 2^-15
                                         0x0000, 0x8000]
    MAXH = 0x7BFF
    assert f16[large, cols].tolist() == [0x78E2, MAXH, 0xF8E2, MAXH, MAXH, 0x8000 | MAXH, MAXH, MAXH, 0x8000 | MAXH, MAXH, MAXH, 0x8000 | MAXH,
                                         MAXH, 0x8000 | MAXH, MAXH, 0x7BFE]
    assert all(v == (MAXH | (0x8000 if x < 0 else 0)) for v, x in zip(f16[huge, cols].tolist(), R.ROW_HUGE))
    assert f16[pinf, cols[7]] == MAXH and f16[ninf, cols[8]] == 0x8000 | MAXH
    assert bf16[pinf, cols[7]] == 0x7F80 and bf16[ninf, cols[8]] == 0xFF80 and bf16[huge, cols[7]] == 0x7F80      # FLT_MAX carries into Inf
    assert not f16[large, 4].any() and not f16[huge, 6].any()                # the rest of those rows is zero
    # the fold: |W| = 40000 is in range, |W gamma| = 80000 is not; a zero times a negative gamma changes its sign
    folded = _bits(R.restate(planted, 1, "f16", fold=True)[0], 1, 0)
    q_large, q_fine = 0 + 4, 0 + 3
    assert folded[q_large, cols[0]] == MAXH and folded[q_large, cols[2]] == MAXH
    assert folded[q_fine, cols[14]] == 0x8000 and folded[q_fine, cols[15]] == 0x0000
    # the NaN: fc2 of layer 1, nowhere else
    two = R.restate(planted, 2, "f16", fold=True, precise=True)[0]
    name, r, c = R.NAN_AT
    for g, s, _, a in two:
        v = a.view(np.float16) if a.dtype == np.uint16 else a
        where = np.argwhere(np.isnan(v)).tolist()
        if (g, s) == (2, 8):
            assert where == [[r, c]] and a[r, c] == 0x7E00
        elif (g, s) == (2, 17):
            assert where == [[r, c], [r, R.F + c], [r, 2 * R.F + c]]
        else:
            assert where == [], R.slot_name(g, s)


def test_planted_bf16_rows_sum_exactly_in_double(planted):
    """The condition under which `float32(double sum in any order)` is THE column sum (tests/test_gpu_weights.py asserts it again on
    its inputs): every folded bf16 row spans at most 52 - 18 binades."""
    bufs, _ = R.restate(planted, 2, "bf16", fold=True)
    seen = 0
    for g, s, _, a in bufs:
        if g and s in (0, 5):
            ok = R.rows_sum_exactly_in_double(R.bits_to_f64("bf16", a))
            assert ok.all(), (R.slot_name(g, s), np.flatnonzero(~ok)[:5])
            seen += 1
    assert seen == 4
    bad = np.zeros((2, 1024))
    bad[0, :2], bad[1, :2] = (2.0 ** 40, 2.0 ** 6), (2.0 ** 40, 2.0 ** 5)
    assert R.rows_sum_exactly_in_double(bad).tolist() == [True, False]         # frexp exponents 41 and 7 / 6: 34 + 18 = 52 < 35 + 18


# ------------------------------------------------------------------------------------------------ 3. the comparator reports the slips
class ColsumOfUnrounded(R.WeightRef):
    def colsum(self, w16, W, gamma):
        return (np.float64(W) * np.float64(gamma)).sum(axis=1).astype(np.float32)


class BiasInFp32(R.WeightRef):
    def cbias(self, W, b, beta):
        c = np.zeros(W.shape[0], dtype=np.float32)
        Wt = np.ascontiguousarray(np.float32(W).T)
        with np.errstate(over="ignore", invalid="ignore"):
            for k in range(W.shape[1]):
                c += np.float32(beta[k]) * Wt[k]
            return c + np.float32(b)


class GammaAfterRounding(R.WeightRef):
    def scaled(self, W, gamma):
        with np.errstate(over="ignore", invalid="ignore"):
            return self.cvt(np.float32(R.bits_to_f64(self.dtype, self.cvt(W))) * np.float32(gamma)[None, :])


class Truncating(R.WeightRef):
    def f16(self, x):
        with np.errstate(over="ignore", invalid="ignore"):
            v = np.clip(np.float32(x), np.float32(-65504.0), np.float32(65504.0))
            h = v.astype(np.float16)
            away = np.abs(h.astype(np.float32)) > np.abs(v)
            return np.where(away, np.nextafter(h, np.float16(0)), h).astype(np.float16).view(np.uint16)

    def cvt(self, x):
        return self.f16(x) if self.dtype == "f16" else (np.ascontiguousarray(np.float32(x)).view(np.uint32) >> 16).astype(np.uint16)


class NotSaturating(R.WeightRef):
    def f16(self, x):
        with np.errstate(over="ignore", invalid="ignore"):
            return np.float32(x).astype(np.float16).view(np.uint16)


class QVK(R.WeightRef):
    def qkv(self, q, k, v):
        return np.concatenate([q, v, k], axis=0)


class DirtyPadding(R.WeightRef):
    def padded(self, w16, kpad):
        out = super().padded(w16, kpad)
        out[:, w16.shape[1]:] = w16[:, :1]
        return out


W16 = ["patch", "layer 0 wqkv", "layer 0 wo", "layer 0 w1", "layer 0 w2"]
TRIPLES = ["patch triple", "layer 0 wqkv triple", "layer 0 wo triple", "layer 0 w1 triple", "layer 0 w2 triple"]
COLSUMS = ["layer 0 qkv colsum", "layer 0 fc1 colsum"]
MUTANTS = {
    "colsum of the unrounded weights": (ColsumOfUnrounded, "f16", COLSUMS),
    "bias accumulated in fp32": (BiasInFp32, "f16", ["layer 0 bqkv", "layer 0 b1"]),
    "gamma applied after rounding": (GammaAfterRounding, "f16", ["layer 0 wqkv", "layer 0 w1"] + COLSUMS),
    "truncation, fp16": (Truncating, "f16", W16 + TRIPLES + COLSUMS),
    "truncation, bf16": (Truncating, "bf16", W16 + COLSUMS),
    "no saturation": (NotSaturating, "f16", W16 + TRIPLES + COLSUMS),
    "q|v|k": (QVK, "f16", ["layer 0 wqkv", "layer 0 bqkv", "layer 0 qkv colsum", "layer 0 wqkv triple", "layer 0 bqkv raw"]),
    "non-zero padding": (DirtyPadding, "f16", ["patch", "patch triple"]),
}


@pytest.fixture(scope="module")
def base(planted):
    """The restatement of layer 0 of the planted tower (one layer: every kind of buffer, half the arithmetic), per operand dtype."""
    return {dt: R.restate(planted, 1, dt, fold=True, precise=dt == "f16") for dt in ("f16", "bf16")}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_each_slip_shows_in_its_buffers(planted, base, name):
    cls, dt, where = MUTANTS[name]
    bufs, fp = R.restate(planted, 1, dt, fold=True, precise=dt == "f16", cls=cls)
    assert sorted(R.differing(bufs, base[dt][0])) == sorted(where)
    assert fp != base[dt][1]
    # the report names the first differing element
    g, s = [(g, s) for g, s, _, _ in bufs if R.slot_name(g, s) == where[0]][0]
    d = R.first_difference(_bits(bufs, g, s), _bits(base[dt][0], g, s))
    assert d is not None and d[2] != d[3]


def test_saturation_shows_only_on_the_planted_rows(planted, base):
    """(What the suite's embedding bounds cannot see: without the planted rows the two conversions agree everywhere.)"""
    bufs, _ = R.restate(planted, 1, "f16", fold=True, precise=True, cls=NotSaturating)
    got, want = _bits(bufs, 1, 3), _bits(base["f16"][0], 1, 3)
    rows = sorted(set(np.argwhere(got != want)[:, 0].tolist()))
    assert rows == [48 + 4, 48 + 5, 48 + 6, 48 + 7]


def test_a_dropped_or_swapped_table_entry_changes_the_fingerprint(planted, base):
    bufs, fp = base["f16"]
    r = R.WeightRef(planted, 1, "f16", fold=True, precise=True)
    assert r.fingerprint(bufs) == fp
    i = [k for k, b in enumerate(bufs) if (b[0], b[1]) == (1, 7)][0]
    dropped = bufs[:i] + bufs[i + 1:]
    swapped = bufs[:i - 1] + [bufs[i], bufs[i - 1]] + bufs[i + 1:]
    reseeded = bufs[:i] + [(1, 7, bufs[i][2] + 1, bufs[i][3])] + bufs[i + 1:]
    seen = {fp}
    for other in (dropped, swapped, reseeded):
        v = r.fingerprint(other)
        assert v not in seen
        seen.add(v)
    # the exact tier's buffers are not part of it
    assert r.fingerprint([b for b in bufs if r.in_fingerprint(b[0], b[1])]) == fp
    assert R.restate(planted, 1, "f16", fold=True, precise=False)[1] == fp
    t = r.table(bufs)
    assert t[0] == 0x3150465449564750 and t[:5].tolist()[1:] == [1, 2, 1, 5 + 14] and t.size == 5 + 4 * 19


def test_key_layouts_and_conversions_of_special_values(sd2):
    pre = {"vision_model." + k: v for k, v in sd2.items()}
    a, b = R.restate(sd2, 1, "bf16", fold=False), R.restate(pre, 1, "bf16", fold=False)
    assert a[1] == b[1] and R.differing(a[0], b[0]) == []
    nan = np.array([0x7FC00000, 0xFF800001, 0x7F800001], dtype=np.uint32).view(np.float32)
    assert R.bf16_bits(nan).tolist() == [0x7FC0, 0xFFC0, 0x7FC0]                       # a NaN is quieted, never rounded into Inf
    assert R.f16_bits(nan[:1]).tolist() == [0x7E00]


# ------------------------------------------------------------------------------------------------ 4. pinned fingerprints
@pytest.mark.parametrize("dtype,fold", list(PINNED))
def test_pinned_fingerprints(sd2, dtype, fold):
    _, fp = R.restate(sd2, 2, dtype, fold)
    assert "%016x%016x" % fp == PINNED[(dtype, fold)]
    assert len(set(PINNED.values())) == 4
