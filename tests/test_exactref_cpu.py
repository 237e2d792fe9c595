"""The exact-input comparators of tests/_exactref.py have teeth, shown without a GPU: a stand-in for the kernels (numpy fp32, another
summation order: 32-wide K slabs, last slab first) is accepted for every epilogue, and each subtly wrong variant of it -- the mistakes a
tiled GEMM or a flash-attention kernel actually makes -- is rejected.  Plus the planner's invariants over every row count."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import _exactref as X

F16, BF16 = torch.float16, torch.bfloat16
FC2_CLASS, QKV_CLASS = (1024, 4096), (3072, 1024)            # (N, K): fc2's 64 K tiles, QKV's 12 column tiles
M_CPU = 300                                                   # one whole 256-row tile + a ragged one of 44 rows


# ================================================================================================================ GEMM stand-in
def _f32(t):
    return t.float().cpu().numpy()


def emulate_gemm(c, mutant=None):
    """Case c through a numpy fp32 stand-in of a tiled GEMM kernel; `mutant` names one deliberate mistake.  Returns the output buffers
    (with guard rows) as compare_gemm takes them."""
    A, W = _f32(c.A), _f32(c.W)
    M, N, K = c.M, c.N, c.K
    acc = np.zeros((M, N), np.float32)
    slabs = [(s, A[:, 32 * s:32 * s + 32] @ W[:, 32 * s:32 * s + 32].T) for s in reversed(range(K // 32))]
    for s, p in slabs:
        acc += p
    blk = (slice(16, 32), slice(256 + 16, 256 + 32))           # one 16 x 16 block of output tile (0, 1)
    mid = dict(slabs)[K // 64]
    if mutant == "slab_dropped":
        acc[blk] -= mid[blk]
    if mutant == "slab_twice":
        acc[blk] += mid[blk]
    if mutant == "blocks_swapped":
        acc[[*range(16, 32), *range(48, 64)], 256:512] = acc[[*range(48, 64), *range(16, 32)], 256:512]
    bias = None if c.bias is None else _f32(c.bias).copy()
    if mutant == "bias_of_previous_tile":
        bias[512:768] = bias[256:512]
    one = np.float32(1.0)
    if c.epi in (X.EPI_QKV_LN, X.EPI_GELU_LN):
        rs = _f32(c.rowstat)
        v = rs[:, :1] * acc - rs[:, 1:2] * _f32(c.colsum)[None, :] + bias[None, :]
    elif c.epi == X.EPI_PATCH:
        v = acc + _f32(c.pos)[1 + np.arange(M) % X.PATCHES]
    else:
        v = acc + bias[None, :] if bias is not None else acc
    bufs = X.alloc_outputs(c)
    out = bufs["out"]
    rows = M
    if mutant == "tail_unwritten":
        rows = M // 256 * 256
    to16 = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dt)
    if c.epi in (X.EPI_QKV, X.EPI_QKV_LN):
        qc = c.qcols + (1 if mutant == "qcols_plus_one" else 0)
        v[:, :qc] *= np.float32(c.qscale)
        res = to16(v, c.dtype)
    elif c.epi in (X.EPI_GELU, X.EPI_GELU_LN):
        with np.errstate(over="ignore"):
            e = np.exp2(np.float32(-1.702 * math.log2(math.e)) * v, dtype=np.float32)
        res = to16(v * (one / (one + e)), c.dtype)
    elif c.epi == X.EPI_GELU_X3:
        with np.errstate(over="ignore"):
            g = v / (one + np.exp(np.float32(-1.702) * v, dtype=np.float32))
        hi = torch.from_numpy(g).half()
        lo = (torch.from_numpy(g) - hi.float()).half()
        res = torch.cat([hi, lo, (hi.float() * 2.0 ** -8).half()], dim=1)
    elif c.epi in (X.EPI_RESID, X.EPI_RESID_STAT):
        res = torch.from_numpy(_f32(c.X0) + v)
    else:
        res = torch.from_numpy(v)
    if c.epi == X.EPI_PATCH:
        r = np.arange(M)
        orow = r // X.PATCHES * X.TOKENS + 1 + r % X.PATCHES
        if mutant == "patch_rows_shifted":
            orow = orow - 1                                      # the class-token offset of the image forgotten
        out[torch.from_numpy(orow[:rows])] = res[:rows]
    else:
        out[:rows] = res[:rows]
        if mutant == "row_past_M":
            out[M] = res[M - 1]
    if c.epi == X.EPI_RESID_STAT:
        bufs["x16"][:rows] = res[:rows].to(c.dtype)
        xs = res.numpy().reshape(M, N // 64, 64)
        part = np.stack([xs.sum(2, dtype=np.float32), (xs * xs).sum(2, dtype=np.float32)], axis=2)      # (M, slots, 2): token-major
        if mutant == "stat_token_major":
            bufs["part"][:N // 64] = torch.from_numpy(np.ascontiguousarray(part)).reshape(N // 64, M, 2)
        elif mutant == "stat_stride_of_main_rows":
            # a launch cut at row 256: the main kernel strides its slots by ITS row count instead of the full M
            flat = bufs["part"].reshape(-1)
            slot_major = torch.from_numpy(part.transpose(1, 0, 2).copy())
            bufs["part"][:N // 64, 256:] = slot_major[:, 256:]
            flat[:N // 64 * 256 * 2] = slot_major[:, :256].reshape(-1)
        else:
            bufs["part"][:N // 64, :rows] = torch.from_numpy(part.transpose(1, 0, 2)[:, :rows].copy())
    return bufs


def _case(epi, N, K, dtype=F16, seed=5):
    M = X.PATCHES if epi == X.EPI_PATCH else M_CPU
    return X.make_exact_gemm_case(epi, M, N, K, dtype, seed)


@pytest.mark.parametrize("dtype", [F16, BF16], ids=["fp16", "bf16"])
@pytest.mark.parametrize("epi", range(9), ids=X.EPI_NAMES)
def test_emulation_with_another_summation_order_is_accepted(epi, dtype):
    if epi == X.EPI_GELU_X3 and dtype == BF16:
        with pytest.raises(ValueError):                       # the builder refuses what does not exist; nothing is dropped silently
            _case(epi, 512, 256, dtype)
        return
    for (N, K) in ((512, 640), (1024, 2048)):
        c = _case(epi, N, K, dtype, seed=epi + 11)
        assert X.compare_gemm(c, emulate_gemm(c)) == []


# mutant -> the epilogues it is tried on (every generic mistake on an exact, an fp32-residual and a bounded epilogue)
GENERIC = (X.EPI_QKV, X.EPI_RESID_STAT, X.EPI_GELU_LN, X.EPI_F32, X.EPI_GELU_X3)
MUTANTS = {
    "slab_dropped": GENERIC, "slab_twice": GENERIC, "blocks_swapped": GENERIC, "tail_unwritten": GENERIC + (X.EPI_PATCH,),
    "row_past_M": GENERIC,
    "bias_of_previous_tile": (X.EPI_QKV, X.EPI_GELU, X.EPI_RESID, X.EPI_F32, X.EPI_RESID_STAT, X.EPI_QKV_LN, X.EPI_GELU_LN, X.EPI_GELU_X3),
    "qcols_plus_one": (X.EPI_QKV, X.EPI_QKV_LN),
    "patch_rows_shifted": (X.EPI_PATCH,),
    "stat_token_major": (X.EPI_RESID_STAT,),
    "stat_stride_of_main_rows": (X.EPI_RESID_STAT,),
}


@pytest.mark.parametrize("shape", [FC2_CLASS, QKV_CLASS], ids=["K4096", "N3072"])
@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_gemm_mutant_is_rejected(mutant, shape, capsys):
    N, K = shape
    for epi in MUTANTS[mutant]:
        c = _case(epi, N, K, seed=31 + epi)
        assert X.compare_gemm(c, emulate_gemm(c)) == [], "the unmutated emulation must pass first"
        found = X.compare_gemm(c, emulate_gemm(c, mutant))
        assert found, (mutant, X.EPI_NAMES[epi], shape)
        if mutant in ("slab_dropped", "slab_twice") and epi in (X.EPI_QKV, X.EPI_F32, X.EPI_RESID_STAT):
            # a failure reads as a location: the 16 x 16 block, and the K slab that explains the difference
            what = f"slab {K // 64} " + ("dropped" if mutant == "slab_dropped" else "twice")
            assert any("row 16 " in m and "col 272 " in m and what in m for m in found), found[:3]


def test_builder_raises_instead_of_dropping_a_case():
    with pytest.raises(ValueError):
        X.make_exact_gemm_case(X.EPI_F32, 16, 256, 16384, F16, 0)            # 9 K leaves the exact range
    c = _case(X.EPI_F32, 256, 128)
    c.bias[0] = 2.0 ** -30                                                   # acc + bias is no longer an fp32 number
    with pytest.raises(ValueError):
        X.compare_gemm(c, emulate_gemm(c))


def test_gaussian_bound_accepts_fp32_and_rejects_a_dropped_slab():
    for epi in (X.EPI_QKV_LN, X.EPI_RESID_STAT, X.EPI_GELU_LN, X.EPI_PATCH):
        c = X.make_gauss_gemm_case(epi, X.PATCHES if epi == X.EPI_PATCH else M_CPU, 512, 1024, F16, 3)
        assert X.compare_gemm(c, emulate_gemm(c)) == []
        assert X.compare_gemm(c, emulate_gemm(c, "blocks_swapped"))


# ================================================================================================================ attention stand-in
def emulate_attention(qkv, n, score_div=1.0, base2=True, p_dtype=None, out_dtype=None, mutant=None):
    """Flash-style attention in torch fp32 the way the kernels walk it: 64-key tiles, a running reference maximum raised only when
    a tile exceeds it by more than 8, key 576 as a last single-key step, P rounded to p_dtype.  `mutant` names one mistake."""
    T, H, D = X.TOKENS, X.HEADS, X.HDIM
    x = qkv.float().reshape(n, T, 3, H, D)
    q, k, v = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)      # (n, H, T, D)
    if mutant == "heads_swapped":
        v = v.clone(); v[:, [2, 3]] = v[:, [3, 2]]
    if mutant == "v_untransposed_block":
        v = v.clone(); v[:, 5, 64:80, 16:32] = v[:, 5, 64:80, 16:32].transpose(-1, -2).clone()
    if mutant == "query_576_is_575":
        q = q.clone(); q[:, :, 576] = q[:, :, 575]
    ex = (lambda t: torch.exp2(t)) if base2 else (lambda t: torch.exp(t))
    s_all = q @ k.transpose(-1, -2) / score_div
    m = torch.full((n, H, T), float("-inf"))
    O = torch.zeros((n, H, T, D))
    l = torch.zeros((n, H, T))
    for t in range(10):
        j0, j1 = 64 * t, min(T, 64 * t + 64)
        if t == 9 and mutant == "key_576_ignored":
            break
        s = s_all[..., j0:j1]
        tm = s.max(-1).values
        raise_m = (tm > m + 8.0) if t else torch.ones_like(tm, dtype=torch.bool)
        new_m = torch.where(raise_m, tm, m)
        alpha = torch.where(torch.isinf(m), torch.zeros_like(m), ex(m - new_m))
        if mutant != "no_rescale":
            O = O * alpha[..., None]
        l = l * alpha
        m = new_m
        p = ex(s - m[..., None])
        if p_dtype is not None:
            p = p.to(p_dtype).float()
        if mutant == "tile_skipped" and t == 4:
            p[:, 7, 32:48] = 0.0                                  # head 7, one 16-query block
        O = O + p @ v[:, :, j0:j1]
        l = l + p.sum(-1) * (4.0 if (t == 9 and mutant == "key_576_four_times") else 1.0)
    out = (O / l[..., None]).transpose(1, 2).reshape(n * T, H * D)
    return out.to(out_dtype or qkv.dtype)


ATT_MUTANTS = ("key_576_ignored", "key_576_four_times", "tile_skipped", "no_rescale", "heads_swapped", "query_576_is_575", "v_untransposed_block")


def _att_cases(dtype):
    """(name, qkv, want, tol, emulation kwargs) for n = 2: uniform, one-hot spread / last, in the form the kernel of `dtype` takes."""
    n = 2
    f32 = dtype == torch.float32
    kw = dict(score_div=8.0, base2=False) if f32 else dict(score_div=1.0, base2=True, p_dtype=dtype)
    qkv, vs = X.attention_uniform_case(n, dtype)
    mean = (vs / 577.0).unsqueeze(1).expand(n, X.TOKENS, X.HEADS, X.HDIM).reshape(n * X.TOKENS, X.HIDDEN)
    tol = 2 * X.ulp32(mean) if f32 else 2 * X.half_ulp16(mean, dtype)          # 2 ulp of fp32 / 1 ulp of the 16-bit type
    cases = [("uniform", qkv, mean, tol, kw)]
    for kind in ("spread", "last"):
        qkv, want, gap = X.attention_onehot_case(n, dtype, kind, 128.0 if f32 else 16.0, 8.0 if f32 else 1.0)
        assert gap >= 160.0
        cases.append(("onehot_" + kind, qkv, want, None, kw))
    return n, cases


@pytest.mark.parametrize("dtype", [F16, BF16, torch.float32], ids=["fp16", "bf16", "fp32"])
def test_attention_emulation_accepted_and_every_mutant_rejected(dtype):
    n, cases = _att_cases(dtype)
    caught = {m: [] for m in ATT_MUTANTS}
    for name, qkv, want, tol, kw in cases:
        assert X.compare_attention(emulate_attention(qkv, n, **kw), want, tol) == [], name
        for m in ATT_MUTANTS:
            if X.compare_attention(emulate_attention(qkv, n, mutant=m, **kw), want, tol):
                caught[m].append(name)
    assert all(caught.values()), {m: c for m, c in caught.items() if not c}
    # the cases are built for these: the uniform one counts keys, the one-hot ones place them
    assert "uniform" in caught["key_576_four_times"] and "onehot_last" in caught["key_576_ignored"]
    assert "onehot_last" in caught["no_rescale"] and "onehot_spread" in caught["query_576_is_575"]


def test_onehot_targets_cover_what_they_claim():
    pi = X.onehot_targets("spread")
    assert {0, 63, 64, 575, 576} <= set(pi.tolist()) and len(set(pi.tolist())) == 577
    assert set((pi[512:576] // 64).tolist()) == set(range(9)) | ({9} if 576 in pi[512:576].tolist() else set())
    assert bool((X.onehot_targets("last") == 576).all())


@pytest.mark.parametrize("dtype,step", [(F16, 7.9), (F16, 8.1), (BF16, 7.9), (BF16, 8.1)])
def test_staircase_case_has_the_steps_it_claims(dtype, step):
    qkv, q, k, v = X.attention_staircase_case(1, dtype, step, 1.0)
    d = X.staircase_steps(q, k, 1.0)
    assert bool(((d > 7.8) & (d < 8.0)).all()) if step < 8 else bool(((d > 8.0) & (d < 8.2)).all()), (float(d.min()), float(d.max()))
    o, tol = X.staircase_tol(dtype, q, k, v, 1.0, True)
    assert X.compare_attention(emulate_attention(qkv, 1, p_dtype=dtype), o, tol) == []
    assert X.compare_attention(emulate_attention(qkv, 1, p_dtype=dtype, mutant="no_rescale"), o, tol)


# ================================================================================================================ planner invariants
PRODUCT_LAUNCHES = {"patch": (X.EPI_PATCH, 1024, 640), "qkv": (X.EPI_QKV_LN, 3072, 1024), "out": (X.EPI_RESID_STAT, 1024, 1024),
                    "fc1": (X.EPI_GELU_LN, 4096, 1024), "fc2": (X.EPI_RESID_STAT, 1024, 4096)}
TILE_ROWS = {0: 384, 1: 256, 2: 128, 3: 32, 4: 256}         # pg_gemm_plan's kernel code -> tile height
TAIL_ROWS = 768


def sweep_rows():
    ms = set(range(1, 4097)) | set(range(577, 300001, 577)) | {300000}
    for base in (256, 384):
        for m in range(base, 300001, base):
            ms.update(range(max(1, m - 2), min(300000, m + 2) + 1))
    return sorted(ms)


def test_plan_invariants_over_every_row_count(hip_lib):
    L = hip_lib
    k, rows, rest = C.c_int(), C.c_int(), C.c_int()
    ms = sweep_rows()
    seen_split = set()
    try:
        assert L.pg_tune_gemm_tail_rows(TAIL_ROWS) == 0
        for mid in (1, 2, 0):
            assert L.pg_tune_gemm_mid(mid) == 0
            for name, (epi, N, K) in PRODUCT_LAUNCHES.items():
                for M in ms:
                    assert L.pg_gemm_plan(0, epi, M, N, K, C.byref(k), C.byref(rows), C.byref(rest)) == 0, (name, M)
                    kk, r, rs = k.value, rows.value, rest.value
                    assert 0 <= r <= M and kk in TILE_ROWS and rs in (-1, 2, 3), (name, mid, M, kk, r, rs)
                    assert (rs == -1) == (r == M), (name, mid, M, kk, r, rs)
                    if rs != -1:
                        assert r > 0 and r % TILE_ROWS[kk] == 0 and M - r <= TAIL_ROWS, (name, mid, M, kk, r, rs)
                        seen_split.add(name)
    finally:
        L.pg_tune_gemm_mid(1)
    assert {"fc1", "fc2"} <= seen_split                      # the sweep does reach the split (the invariants are not vacuous)


# ================================================================================================================ the exact tier's streaming kernels
# numpy stand-ins of csrc/precise.hip / csrc/rowops.hip's row kernels (numpy's own float16 / float32 conversions and another, equally
# valid summation tree: pairwise halving, depth 10) pass the comparators of _exactref.py with NO element excluded, and each mistake such
# a kernel can make is rejected with a message that names the place.
F32 = np.float32


def emulate_triple(v, C, mutant=None, seg=None, guard=3):
    """v (rows, C) fp32 numpy -> (rows + guard, 3 seg) fp16 torch buffer as a split kernel writes it (guard rows = SENTINEL)."""
    seg = C if seg is None else seg
    v = np.ascontiguousarray(v, dtype=F32)
    with np.errstate(over="ignore", invalid="ignore"):
        vc = v if mutant == "no_saturation" else np.clip(v, -65504.0, 65504.0).astype(F32)
        hi = vc.astype(np.float16)
        if mutant == "truncation":                              # round toward zero instead of to nearest even
            over = np.abs(hi.astype(F32)) > np.abs(vc)
            hi = np.where(over, np.nextafter(hi, np.float16(0)), hi).astype(np.float16)
        lo = (v - (vc if mutant == "lo_from_unrounded" else hi.astype(F32))).astype(np.float16)
        if mutant == "lo_subnormal_flushed":
            lo = np.where(np.abs(lo.astype(F32)) < 2.0 ** -14, np.float16(0), lo).astype(np.float16)
        hs = ((v if mutant == "hs_from_v" else hi.astype(F32)) * F32(2.0 ** -8)).astype(np.float16)
    segs = [hi, hs, lo] if mutant == "lo_hs_swapped" else [hi, lo, hs]
    out = np.full((v.shape[0] + guard, 3 * seg), X.SENTINEL, np.float16)
    out[:v.shape[0]] = 0 if mutant != "pad_not_zeroed" else X.SENTINEL
    for s, a in enumerate(segs):
        out[:v.shape[0], s * seg:s * seg + C] = a
    if mutant == "group_at_neighbours_offset":                  # row 2, segment lo: the 4-column group 9 lands on group 10's columns
        out[2, seg + 40:seg + 44] = lo[2, 36:40]
    if mutant == "row_past_end":
        out[v.shape[0], :C] = hi[-1]
    return torch.from_numpy(out)


TRIPLE_MUTANTS = {   # mutant -> words its finding must contain
    "truncation": ("triple hi",), "no_saturation": ("triple hi", "65520"), "lo_from_unrounded": ("triple lo",), "hs_from_v": ("triple hi*2^-8",),
    "lo_subnormal_flushed": ("triple lo",), "lo_hs_swapped": ("triple lo", "triple hi*2^-8"),
    "group_at_neighbours_offset": ("segment 1 row 2 col 40 (4-col group 10)",), "row_past_end": ("guard rows",),
}


def test_triple_standin_accepted_and_every_mutant_rejected():
    C = 1024
    v = X.triple_values(7, C, 3).numpy()
    tv = torch.from_numpy(v)
    assert X.compare_triple(emulate_triple(v, C), tv, C) == []
    # the planted values do what they are planted for (numpy's conversions: an implementation that is not torch's)
    t = emulate_triple(np.array([[1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65519.9, 65520.0, 7.0e4, -1.0e5, 2.0 ** -24, -0.0]], F32), 8, guard=0).float()
    assert t[0, :8].tolist() == [1.0, 1 + 2.0 ** -9, 65504.0, 65504.0, 65504.0, -65504.0, 2.0 ** -24, 0.0]
    assert t[0, 8:16].tolist()[:6] == [2.0 ** -11, -(2.0 ** -11), 15.8984375, 16.0, 4496.0, -34496.0]
    assert int(emulate_triple(np.array([[-0.0] * 4], F32), 4, guard=0).view(torch.int16)[0, 0]) == -32768          # -0 keeps its sign in hi
    for m, words in TRIPLE_MUTANTS.items():
        found = X.compare_triple(emulate_triple(v, C, m), tv, C)
        assert found, m
        for w in words:
            assert any(w in line for line in found), (m, w, found[:3])
    # the consistency check (for triples whose value the host cannot reproduce) sees the same mistakes where they break the triple's own
    # structure, and passes the honest one on the values inside fp16's range
    inside = np.clip(v, -6.0e4, 6.0e4)
    f, val = X.triple_consistent(emulate_triple(inside, C, guard=0), C)
    assert f == [] and bool(((val - torch.from_numpy(inside).double()).abs() <= X.triple_recon_bound(torch.from_numpy(inside).double())).all())
    for m in ("truncation", "hs_from_v", "lo_hs_swapped"):
        assert X.triple_consistent(emulate_triple(inside, C, m, guard=0), C)[0], m


def _pairwise(a):
    """fp32 pairwise sum over the last axis (a power of two long): another valid tree, depth log2(n)."""
    a = a.astype(F32)
    while a.shape[-1] > 1:
        a = (a[..., 0::2] + a[..., 1::2]).astype(F32)
    return a[..., 0]


def emulate_layernorm(x, g, b, eps=1e-5, mutant=None, const_rows=None):
    x, g, b = [np.ascontiguousarray(t, dtype=F32) for t in (x, g, b)]
    n = F32(x.shape[1])
    mean = (_pairwise(x) / n).astype(F32)[:, None]
    d = (x - mean).astype(F32)
    var = (_pairwise((d * d).astype(F32)) / (F32(1023.0) if mutant == "divisor_1023" else n)).astype(F32)[:, None]
    if mutant == "one_pass":
        var = np.maximum((_pairwise((x * x).astype(F32)) / n).astype(F32)[:, None] - (mean * mean).astype(F32), F32(0)).astype(F32)
    e = np.full_like(var, F32(eps))
    if mutant == "eps_dropped":
        e[const_rows] = 0
    with np.errstate(divide="ignore", invalid="ignore"):
        rstd = (F32(1) / np.sqrt((var + e).astype(F32))).astype(F32)
        if mutant == "gamma_of_next_lane":
            g = np.roll(g, -4)
        return ((((d * rstd).astype(F32) * g[None, :]).astype(F32)) + b[None, :]).astype(F32), mean[:, 0], rstd[:, 0]


def _ln_buffer(y, out, guard=3):
    y = torch.from_numpy(y)
    if out == "x3":
        return emulate_triple(y.numpy(), X.HIDDEN, guard=guard)
    buf = torch.full((y.shape[0] + guard, X.HIDDEN), X.SENTINEL, dtype=out)
    buf[:y.shape[0]] = y.clamp(-65504.0, 65504.0).to(out) if out == F16 else y.to(out)
    return buf


LN_ROWS = 45          # nine of each row kind
LN_MUTANTS = ("one_pass", "divisor_1023", "eps_dropped", "gamma_of_next_lane")


@pytest.mark.parametrize("out", [torch.float32, F16, BF16, "x3"], ids=["f32", "f16", "bf16", "x3"])
def test_layernorm_standin_accepted_and_every_mutant_rejected(out):
    x = X.ln_rows(LN_ROWS, 8)
    g, b = X.ln_affine(9)
    kinds = np.arange(LN_ROWS) % 5
    y, _, _ = emulate_layernorm(x.numpy(), g.numpy(), b.numpy())
    worst = []
    assert X.compare_layernorm(_ln_buffer(y, out), x, g, b, 1e-5, out, kind0=0, worst=worst) == []
    assert 0.0 < max(worst) < 1.0
    # torch's own fp32 LayerNorm (yet another summation order) is inside the bound too
    assert X.compare_layernorm(_ln_buffer(torch.nn.functional.layer_norm(x, (1024,), g, b, 1e-5).numpy(), out), x, g, b, 1e-5, out, kind0=0) == []
    for m in LN_MUTANTS:
        ym, _, _ = emulate_layernorm(x.numpy(), g.numpy(), b.numpy(), mutant=m, const_rows=kinds == 2)
        found = X.compare_layernorm(_ln_buffer(ym, out), x, g, b, 1e-5, out, kind0=0, limit=100)
        assert found, (m, out)
        named = " ".join(found)
        if m == "one_pass":
            assert "'mean >> std' row" in named, found[:3]
        if m == "eps_dropped":
            assert "'constant' row" in named and all("'constant' row" in l for l in found if " at row " in l and "triple inconsistent" not in l), found[:3]
    # a stale guard row
    buf = _ln_buffer(y, out)
    buf[LN_ROWS, 5] = 1.0
    assert any("guard rows" in l for l in X.compare_layernorm(buf, x, g, b, 1e-5, out))


def test_one_pass_variance_is_what_the_finalize_bound_allows_and_the_two_pass_bound_does_not():
    """rowstat_finalize really is one-pass: its stand-in passes rowstat_finalize_bound (which carries the cancellation term) on every row
    kind, and the SAME numbers fail the two-pass bound on the |mean| >> std (and constant) rows, only there -- the two bounds are not interchangeable."""
    x = X.ln_rows(LN_ROWS, 12)
    part = X.statparts_of(x)
    p = part.numpy()
    s1 = np.zeros(LN_ROWS, F32); s2 = np.zeros(LN_ROWS, F32)
    for i in range(p.shape[0]):
        s1 = (s1 + p[i, :, 0]).astype(F32); s2 = (s2 + p[i, :, 1]).astype(F32)
    mean = (s1 / F32(1024)).astype(F32)
    var = np.maximum((s2 / F32(1024)).astype(F32) - (mean * mean).astype(F32), F32(0)).astype(F32)
    rstd = (F32(1) / np.sqrt((var + F32(1e-5)).astype(F32))).astype(F32)
    got = torch.from_numpy(np.stack([rstd, (mean * rstd).astype(F32)], 1))
    ref, bound = X.rowstat_finalize_bound(part)
    assert X.compare_rowstat("finalize", got, ref, bound, kind0=0) == []
    ref2, bound2 = X.rowstat_bound(x)
    found = X.compare_rowstat("two-pass", got, ref2, bound2, kind0=0, limit=100)
    # (a constant row is the limit of that regime: its variance is ALL cancellation)
    assert any("'mean >> std'" in l for l in found) and all("'mean >> std'" in l or "'constant'" in l for l in found if " at row " in l), found[:3]
    assert float((bound[0] / bound2[0])[1::5].min()) > 100.0          # the cancellation term, not a constant
    # the two-pass stand-in is inside the two-pass bound; a rowstat computed from the row BEFORE it was rewritten is not
    _, m2, r2 = emulate_layernorm(x.numpy(), np.ones(1024), np.zeros(1024))
    assert X.compare_rowstat("cast", torch.from_numpy(np.stack([r2, (m2 * r2).astype(F32)], 1)), ref2, bound2, kind0=0) == []
    assert X.compare_rowstat("cast", torch.from_numpy(np.stack([np.roll(r2, 1), (m2 * r2).astype(F32)], 1)), ref2, bound2, kind0=0)


def emulate_preln(x, cls, pos0, g, b, mutant=None):
    x = x.copy()
    t0 = np.arange(x.shape[0]) % X.TOKENS == 0
    if mutant != "class_row_from_stale_x":
        x[t0] = (cls + pos0).astype(F32)[None, :]
    return emulate_layernorm(x, g, b)[0]


def test_preln_standin_accepted_and_stale_class_row_rejected():
    rows = 2 * X.TOKENS + 3                                     # two images and the start of a third: class rows 0, 577, 1154
    x = X.ln_rows(rows, 21)
    x[::X.TOKENS] = 1234.5                                      # what the patch GEMM leaves there is NOT the class token: a sentinel
    g, b = X.ln_affine(22)
    gen = torch.Generator().manual_seed(23)
    cls, pos0 = torch.randn(1024, generator=gen) * 0.03, torch.randn(1024, generator=gen) * 0.02
    want_in = x.clone()
    want_in[::X.TOKENS] = cls + pos0                            # one fp32 addition: the row the kernel normalises
    y = emulate_preln(x.numpy(), cls.numpy(), pos0.numpy(), g.numpy(), b.numpy())
    assert X.compare_layernorm(_ln_buffer(y, torch.float32), want_in, g, b, 1e-5, torch.float32, kind0=0, name="preln") == []
    bad = emulate_preln(x.numpy(), cls.numpy(), pos0.numpy(), g.numpy(), b.numpy(), "class_row_from_stale_x")
    found = X.compare_layernorm(_ln_buffer(bad, torch.float32), want_in, g, b, 1e-5, torch.float32, kind0=0, name="preln", limit=5000)
    rows_named = {int(l.split(" at row ")[1].split(" ")[0]) for l in found if " at row " in l}
    assert rows_named == {0, 577, 1154}, sorted(rows_named)[:8]
    assert any("token 0 of image 2" in l for l in found)


def test_sum_parts_reference_pins_the_order():
    g = torch.Generator().manual_seed(31)
    for S in (2, 3, 4, 6):
        parts = torch.randn((S, 1000), generator=g) * torch.tensor([1.0, 300.0, 0.01, 7.0, 1e3, 1e-3][:S])[:, None]
        dst0 = torch.randn(1000, generator=g)
        p = parts.numpy()
        acc = p[0].copy()
        for k in range(1, S):
            acc = (acc + p[k]).astype(F32)
        for resid in (False, True):
            want = X.sum_parts_ref(parts, dst0 if resid else None)
            assert torch.equal(torch.from_numpy((dst0.numpy() + acc).astype(F32) if resid else acc), want)
        rev = p[S - 1].copy()
        for k in range(S - 2, -1, -1):
            rev = (rev + p[k]).astype(F32)
        if S > 2:                                                 # (two parts: the addition commutes; from three on the order shows)
            assert not torch.equal(torch.from_numpy(rev), X.sum_parts_ref(parts, None)), "the inputs must tell the orders apart"
        twice = ((dst0.numpy() + acc).astype(F32) + dst0.numpy()).astype(F32)
        assert not torch.equal(torch.from_numpy(twice), X.sum_parts_ref(parts, dst0))


def emulate_im2col(px, mutant=None):
    n = px.shape[0]
    a = px.reshape(n, 3, 24, 14, 24, 14)                        # (img, c, py, ky, px, kx)
    order = (0, 2, 4, 1, 5, 3) if mutant == "ky_kx_transposed" else (0, 2, 4, 1, 3, 5)
    return np.ascontiguousarray(a.transpose(order).reshape(n * 576, 588))


@pytest.mark.parametrize("mutant", [None, "ky_kx_transposed", "pad_not_zeroed"])
def test_im2col_standin_and_mutants(mutant):
    px = X.representable_pixels(2, 41)
    vals = emulate_im2col(px.numpy(), mutant)
    for dt in (F16, BF16):                                       # the fast path's patch matrix
        buf = torch.full((2 * 576 + 3, 640), X.SENTINEL, dtype=dt)
        buf[:2 * 576, :588] = torch.from_numpy(vals).to(dt)
        if mutant != "pad_not_zeroed":
            buf[:2 * 576, 588:] = 0
        found = X.compare_im2col(buf, px.to(dt))
        assert bool(found) == (mutant is not None), (mutant, found[:2])
        if mutant == "ky_kx_transposed":
            assert any("ky 0 kx 1" in l for l in found), found[:2]     # the first element that moves
        if mutant == "pad_not_zeroed":
            assert any("pad columns" in l for l in found)
    # the exact tier's: three segments of 588 at stride 640
    ref = X.im2col_ref(px)
    buf = emulate_triple(vals, 588, "pad_not_zeroed" if mutant == "pad_not_zeroed" else None, seg=640)
    found = X.compare_triple(buf, ref, 588, seg=640, where=X.im2col_where)
    assert bool(found) == (mutant is not None), (mutant, found[:2])
    if mutant == "pad_not_zeroed":
        assert any("columns between the segments" in l for l in found)
    if mutant == "ky_kx_transposed":
        assert any("ky 0 kx 1" in l for l in found), found[:2]
