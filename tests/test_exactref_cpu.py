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
