"""Exact-input tests of every GEMM epilogue and of the attention kernels at the product's shapes (run with -m gpu on an MI355X).

The A == B tests of test_gpu_parity.py compare kernels that share gemm_epi.h, the slab geometry, the K order and the planner: a
mistake they share is invisible there.  Here each kernel is compared with an independent fp64 statement of the operation
(tests/_exactref.py) on inputs for which the answer is EXACT -- small integers, partial sums below 2^24, powers of two for the
scales -- so the comparison is an equality at any shape and any row count the planner produces; the epilogues that are not exact
(the GELU forms, large sums of squares) get a per-element bound derived from their operations, and Gaussian inputs at the 512-image
shapes exercise the rounding that exact inputs cannot.  tests/test_exactref_cpu.py shows that these comparators reject the mistakes
they are meant for.

No input here is NaN, Inf or outside a kernel's contract, and every buffer a kernel may touch past its last row is owned by the test."""
import ctypes as C

import pytest
import torch

import _exactref as X

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
TAIL_ROWS = 768                                                    # pg_tune_gemm_tail_rows' default, set explicitly by the fixture
# name -> (epilogue, N, K, variant, rows per image).  Variant 0 = the product's default path; the exact tier's two launch on 36.
# Leading dimensions as csrc/vit.hip and csrc/vit_precise.hip pass them: lda = ldw = K (the patch matrix's K is already padded from 588 to 640), ldc = N.
LAUNCHES = {
    "patch": (X.EPI_PATCH, 1024, 640, 0, 576), "qkv_ln": (X.EPI_QKV_LN, 3072, 1024, 0, 577), "out": (X.EPI_RESID_STAT, 1024, 1024, 0, 577),
    "fc1_ln": (X.EPI_GELU_LN, 4096, 1024, 0, 577), "fc2": (X.EPI_RESID_STAT, 1024, 4096, 0, 577),
    "qkv": (X.EPI_QKV, 3072, 1024, 0, 577), "fc1": (X.EPI_GELU, 4096, 1024, 0, 577), "fc2_resid": (X.EPI_RESID, 1024, 4096, 0, 577),
    "exact_f32": (X.EPI_F32, 1024, 3072, 36, 577), "exact_gelu_x3": (X.EPI_GELU_X3, 4096, 3072, 36, 577),
}
PRODUCT = ("patch", "qkv_ln", "out", "fc1_ln", "fc2")
VARIANTS = (8, 33, 36, 56, 70, 71)


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops
    _lib.require_gpu()                       # fails loudly if the HIP library / GPU is missing -- no fallback
    L = _lib.load()
    _lib.check(L.pg_tune_gemm_tail_rows(TAIL_ROWS), "pg_tune_gemm_tail_rows")
    return dict(lib=_lib, ops=hip_ops, L=L)


def _variant(epi, variant):
    """What to pass for `variant`: pg_op_gemm16_resid_stat / pg_op_gemm16_ln read 0 as 36, the encoder's own launches (pg_gemm_launch
    with 0) as the product default 56 -- the product path of those three epilogues is asked for by its number."""
    return variant if variant or epi not in (X.EPI_RESID_STAT, X.EPI_QKV_LN, X.EPI_GELU_LN) else 56


def plan(env, variant, epi, M, N, K):
    """pg_gemm_plan -> (kernel, rows_main, rest), or None where the launch refuses the variant / shape / epilogue (PG_EINVAL)."""
    k, r, s = C.c_int(-9), C.c_int(-9), C.c_int(-9)
    rc = env["L"].pg_gemm_plan(_variant(epi, variant), epi, M, N, K, C.byref(k), C.byref(r), C.byref(s))
    if rc == -1:
        return None
    assert rc == 0, rc
    return k.value, r.value, s.value


def launch(env, c, variant):
    """Case c through the C ABI into buffers of its own (alloc_outputs: sentinel guard rows behind every output)."""
    ops, lib, L = env["ops"], env["lib"], env["L"]
    b = X.alloc_outputs(c)
    p, st, dt, v = ops._p, ops._stream(), ops._dt16(c.A), _variant(c.epi, variant)
    out = b["out"]
    if c.epi == X.EPI_RESID_STAT:
        lib.check(L.pg_op_gemm16_resid_stat(dt, p(c.A), c.A.stride(0), p(c.W), c.W.stride(0), p(c.bias), p(out), out.stride(0), p(b["x16"]),
                                            b["x16"].stride(0), p(b["part"]), c.M, c.N, c.K, v, st), "pg_op_gemm16_resid_stat")
    elif c.epi in (X.EPI_QKV_LN, X.EPI_GELU_LN):
        lib.check(L.pg_op_gemm16_ln(dt, p(c.A), c.A.stride(0), p(c.W), c.W.stride(0), p(c.bias), p(c.colsum), p(c.rowstat), p(out),
                                    out.stride(0), c.M, c.N, c.K, c.epi, float(c.qscale), int(c.qcols), v, st), "pg_op_gemm16_ln")
    else:
        lib.check(L.pg_op_gemm16_ld(dt, p(c.A), c.A.stride(0), p(c.W), c.W.stride(0), p(c.bias), p(out), out.stride(0), c.M, c.N, c.K,
                                    c.epi, float(c.qscale), int(c.qcols), p(c.pos), v, st), "pg_op_gemm16_ld")
    torch.cuda.synchronize()
    return b


def run_exact_cell(env, name, M, dtype, variant=None, seed=0):
    epi, N, K, v0, _ = LAUNCHES[name]
    v = v0 if variant is None else variant
    c = X.make_exact_gemm_case(epi, M, N, K, dtype, 1000 + seed + M % 997, DEV)
    found = X.compare_gemm(c, launch(env, c, v))
    return [f"[{name} M={M} {str(dtype)[6:]} variant {v} plan {plan(env, v, epi, M, N, K)}] {m}" for m in found]


# ================================================================================================================ GEMM, exact inputs
CELLS = [(n, i, F16) for n in LAUNCHES for i in (1, 4, 16, 64, 256, 512)] + \
        [(n, i, BF16) for n in LAUNCHES if n != "exact_gelu_x3" for i in (1, 16, 64)]


@pytest.mark.parametrize("name,images,dtype", CELLS, ids=[f"{n}-{i}img-{str(d)[6:]}" for n, i, d in CELLS])
def test_launch_exact(env, name, images, dtype):
    """The product's five launches as the encoder makes them, the non-folded chain's QKV / GELU / RESID and the exact tier's F32 /
    GELU_X3, at 1 .. 512 images: every output element equals the fp64 value (QKV, QKV_LN, RESID, PATCH, F32, the X / x16 / column sums
    of RESID_STAT) or lies within the epilogue's own arithmetic error, per element (_exactref.gelu_fast_bound, gelu_ieee_bound,
    sumsq_bound hold the derivations); guard rows, PATCH's class-token rows and the partials' guard slot untouched.  Where the planner
    cuts a RESID_STAT launch the partials keep the full M as their row stride: the comparison covers the rows on both sides of the cut."""
    epi, N, K, v, rpi = LAUNCHES[name]
    M = images * rpi
    assert plan(env, v, epi, M, N, K) is not None, "the product's own launch must be accepted"
    found = run_exact_cell(env, name, M, dtype)
    assert not found, "\n".join(found)


def planner_edges(env, name):
    """Row counts around every point where the plan of launch `name` changes, taken from pg_gemm_plan now (the GPU's CU count, the
    current knobs): M - 1, M, M + 1 for each M in 2 .. 64 images at which (kernel, rest, rows_main of a split) differs from M - 1's, and
    rows_main + 1, rows_main + tail_rows, rows_main + tail_rows + 1 around the 256- and 512-image steps."""
    epi, N, K, v, rpi = LAUNCHES[name]
    sig = lambda p: (p[0], p[2], p[1] if p[2] != -1 else None)
    ms, prev = set(), None
    for M in range(1, 64 * rpi + 2):
        s = sig(plan(env, v, epi, M, N, K))
        if prev is not None and s != prev:
            ms.update((M - 1, M, M + 1))
        prev = s
    for images in (256, 512):
        rm = plan(env, v, epi, images * rpi, N, K)[1]
        ms.update((rm + 1, rm + TAIL_ROWS, rm + TAIL_ROWS + 1))
    return sorted(ms)


@pytest.mark.parametrize("name", PRODUCT)
def test_planner_edges_exact(env, name, capsys):
    """Every row count at which the planner changes its mind (kernel, split, where it cuts), one below and one above -- most of them not
    multiples of 16 -- through the same exact comparison.  A RESID_STAT launch that is cut must be among them for fc2."""
    epi, N, K, v, _ = LAUNCHES[name]
    ms = planner_edges(env, name)
    plans = {M: plan(env, v, epi, M, N, K) for M in ms}
    with capsys.disabled():
        print(f"\nplanner edges [{name}]: " + ", ".join(f"{M}:{plans[M]}" for M in ms))
    assert ms and any(M % 16 for M in ms)
    if name in ("fc1_ln", "fc2"):
        assert any(p[2] != -1 for p in plans.values()), "no split launch among the edges"
    found = []
    for M in ms:
        found += run_exact_cell(env, name, M, F16, seed=1)
        assert len(found) < 30, "\n".join(found)
    assert not found, "\n".join(found)


@pytest.mark.parametrize("variant", VARIANTS)
def test_every_variant_exact(env, variant, capsys):
    """Every explicit variant on one many-round ragged shape (73 939 rows: 289 panels of 256, 193 of 384, the last ones ragged, an odd
    row count) per epilogue it accepts -- asked of pg_gemm_plan, not hard-coded."""
    M = 3 * 256 * 96 + 211
    found, ran = [], []
    for name in ("qkv", "fc1", "fc2_resid", "patch", "exact_f32", "fc2", "qkv_ln", "fc1_ln", "exact_gelu_x3"):
        epi, N, K, _, _ = LAUNCHES[name]
        if plan(env, variant, epi, M, N, K) is None:
            continue
        ran.append(X.EPI_NAMES[epi])
        found += run_exact_cell(env, name, M, F16, variant=variant, seed=2)
    with capsys.disabled():
        print(f"\nvariant {variant}: epilogues {ran}")
    assert len(ran) >= 4 and not found, "\n".join(found)


# ================================================================================================================ GEMM, Gaussian inputs
@pytest.mark.parametrize("name,dtype", [("patch", F16), ("qkv_ln", BF16), ("out", F16), ("fc1_ln", BF16), ("fc2", F16)])
def test_launch_gaussian_512_images(env, name, dtype, capsys):
    """Exact inputs do not exercise rounding.  The five product launches at 512 images on Gaussian operands:
      * per element, |got - fp64| <= K 2^-24 (|A| |W|^T) carried through the epilogue + the output's half ulp (_exactref.gemm_acc_bound
        -- the textbook worst case of a K-term fp32 dot product in any order; loose);
      * per 256-column tile, the RMS error against fp64 is at most twice that of a plain fp32 accumulation in sequential K order with
        the same epilogue (the worst reasonable order; the factor 2 is for the matrix pipe's internal rounding not being IEEE).  The
        sequential yardstick is computed on ~37 000 rows -- every 8th plus the last 384, the ragged tiles -- not on all 295 424."""
    epi, N, K, v, rpi = LAUNCHES[name]
    M = 512 * rpi
    c = X.make_gauss_gemm_case(epi, M, N, K, dtype, 77, DEV)
    b = launch(env, c, v)
    found = X.compare_gemm(c, b)
    assert not found, "\n".join(found)
    rows = torch.unique(torch.cat([torch.arange(0, M, 8, device=DEV), torch.arange(M - 384, M, device=DEV)]))
    orow = rows // X.PATCHES * X.TOKENS + 1 + rows % X.PATCHES if epi == X.EPI_PATCH else rows
    ref = X.ideal_out64(c, rows)
    rms = lambda t: ((t.double() - ref) ** 2).reshape(len(rows), N // 256, 256).mean((0, 2)).sqrt()
    e_kernel, e_seq = rms(b["out"][orow]), rms(X.sequential_out32(c, rows))
    worst = int((e_kernel / e_seq).argmax())
    with capsys.disabled():
        print(f"\ngaussian [{name} {str(dtype)[6:]} M={M}]: RMS error vs fp64 kernel {float(e_kernel.max()):.3e} / sequential fp32 {float(e_seq.max()):.3e} "
              f"(largest over column tiles); worst ratio {float(e_kernel[worst] / e_seq[worst]):.3f} at column tile {worst}")
    assert bool((e_kernel <= 2 * e_seq).all()), (e_kernel.tolist(), e_seq.tolist())


# ================================================================================================================ attention
ATT_KERNELS = ("fp16", "bf16", "f32_split", "f32_mfma")
GUARD_ELEMS = 64 * X.HIDDEN


def run_attention(env, kernel, qkv, n):
    """qkv through pg_op_attention / pg_op_attention_f32 (either arm) into a buffer with a sentinel guard region behind it."""
    ops, lib, L = env["ops"], env["lib"], env["L"]
    assert qkv.shape == (n * X.TOKENS, 3 * X.HIDDEN) and qkv.is_contiguous()
    out = torch.full((n * X.TOKENS * X.HIDDEN + GUARD_ELEMS,), X.SENTINEL, dtype=qkv.dtype, device=DEV)
    if kernel in ("fp16", "bf16"):
        lib.check(L.pg_op_attention(ops._dt16(qkv), ops._p(qkv), ops._p(out), n, ops._stream()), "pg_op_attention")
    else:
        lib.check(L.pg_tune_exact_attention(1 if kernel == "f32_mfma" else 0), "pg_tune_exact_attention")
        try:
            lib.check(L.pg_op_attention_f32(ops._p(qkv), ops._p(out), n, ops._stream()), "pg_op_attention_f32")
            torch.cuda.synchronize()
        finally:
            L.pg_tune_exact_attention(0)
    torch.cuda.synchronize()
    return out[:n * X.TOKENS * X.HIDDEN].view(n * X.TOKENS, X.HIDDEN), out[n * X.TOKENS * X.HIDDEN:]


def _att_dtype(kernel):
    return {"fp16": F16, "bf16": BF16}.get(kernel, F32)


@pytest.mark.parametrize("n", [1, 2, 3, 33])
@pytest.mark.parametrize("kernel", ATT_KERNELS)
def test_attention_uniform(env, kernel, n):
    """Q = 0: every probability is exactly 1, the row sum exactly 577 -- each of the 577 keys counted once, key 576's single-key step
    included -- and O the exact integer sum of V.  The output is that sum times 1/577 rounded to the output type: one ulp of the 16-bit
    type for the reciprocal, two ulp of fp32 for pg_op_attention_f32, nothing more."""
    dt = _att_dtype(kernel)
    qkv, vs = X.attention_uniform_case(n, dt, device=DEV)
    want = (vs / 577.0).unsqueeze(1).expand(n, X.TOKENS, X.HEADS, X.HDIM).reshape(n * X.TOKENS, X.HIDDEN)
    tol = 2 * X.ulp32(want) if dt == F32 else 2 * X.half_ulp16(want, dt)
    got, guard = run_attention(env, kernel, qkv, n)
    found = X.compare_attention(got, want, tol, guard=guard)
    assert not found, "\n".join(found)


@pytest.mark.parametrize("kind", ["spread", "last"])
@pytest.mark.parametrize("n", [1, 2, 3, 33])
@pytest.mark.parametrize("kernel", ATT_KERNELS)
def test_attention_onehot(env, kernel, n, kind):
    """K rows are +-1 code vectors, Q row i = 16 K[pi(i)] (128 for pg_op_attention_f32, which divides by 8): the target's score is 1024
    and every other at least 160 lower (asserted by the builder on its own fp64 scores), so every other weight is exactly 0 and the
    output row must EQUAL V[pi(i)].  'spread': a permutation that puts the targets of a 16-query block into different key tiles and
    makes every key -- 0, 63, 64, 575, 576 -- a target; 'last': every target is key 576, which raises the maximum after the nine
    matrix-pipe tiles."""
    dt = _att_dtype(kernel)
    qkv, want, gap = X.attention_onehot_case(n, dt, kind, 128.0 if dt == F32 else 16.0, 8.0 if dt == F32 else 1.0, device=DEV)
    assert gap >= 160.0
    got, guard = run_attention(env, kernel, qkv, n)
    found = X.compare_attention(got, want, None, guard=guard)
    assert not found, "\n".join(found)


@pytest.mark.parametrize("step", [7.9, 8.1])
@pytest.mark.parametrize("kernel", ATT_KERNELS)
def test_attention_staircase(env, kernel, step, capsys):
    """Each key tile's maximum exceeds the previous tile's by 7.9 (the lazy softmax keeps its reference until the steps add up to more
    than 8: a rescale every other tile) or 8.1 (a rescale at every tile), key 576 on top; V Gaussian.  Against fp64 on the rounded
    operands, per element:  |out - ref| <= 2 eps_p (softmax . |V|) + u_out |ref| + 577 2^-24 max|V|  with eps_p as derived in
    _exactref.staircase_eps (P's rounding to the operand type, the fp32 score error, the exponential, the rescales)."""
    dt = _att_dtype(kernel)
    n = 3
    f32 = dt == F32
    qkv, q, k, v = X.attention_staircase_case(n, dt, step, 8.0 if f32 else 1.0, device=DEV)
    d = X.staircase_steps(q, k, 8.0 if f32 else 1.0)
    assert bool(((d > 7.8) & (d < 8.0)).all()) if step < 8 else bool(((d > 8.0) & (d < 8.2)).all()), (float(d.min()), float(d.max()))
    want, tol = X.staircase_tol(dt, q, k, v, 8.0 if f32 else 1.0, base2=not f32)
    got, guard = run_attention(env, kernel, qkv, n)
    ratio = ((got.double() - want).abs() / tol).max(1).values
    with capsys.disabled():
        print(f"\nstaircase [{kernel} step {step}]: worst row {int(ratio.argmax())} ({X.attention_where(int(ratio.argmax()), 0).split(' head')[0]}) "
              f"at {float(ratio.max()):.3f} of its bound")
    found = X.compare_attention(got, want, tol, guard=guard)
    assert not found, "\n".join(found)
