"""The exact tier between its GEMM / attention kernels and its end-to-end embedding (run with -m gpu on an MI355X).

tests/test_gpu_exact.py checks the kernels the exact tier shares with the fast path on exact inputs.  What the tier adds on top of them
was seen only through norms at hand-picked sizes; here

  * every streaming kernel of csrc/precise.hip and csrc/rowops.hip runs alone, per element, with sentinel guard rows behind every
    output: a triple written from a KNOWN fp32 value (split, im2col, the one-hot attention) is compared bit for bit -- it is fully
    determined (csrc/x3.h) --, a triple of a value the host cannot reproduce (LayerNorm, QuickGELU, attention) must be a consistent
    triple whose hi + lo lies within the bound derived from the kernel's stated operations (tests/_exactref.py holds the derivations);
  * the encoder runs at every batch size at which pg_vit_precise_plan changes its mind (asked of the library, not restated), one below
    each, and above the 128-image internal pass, against the oracle in fp64: per image, per row, and per image across batch sizes.

tests/test_exactref_cpu.py shows that the comparators reject the mistakes they are meant for.  No input is NaN, Inf or outside a
kernel's contract; the negative control changes arithmetic (two partial products instead of three), nothing else."""
import ctypes as C
import time

import pytest
import torch

import _exactref as X

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
EXACT_TOL = 1e-5          # the exact mode's embeddings against the reference (tests/test_gpu_precise.py)
CROSS_SIZE_TOL = 1e-6     # the same image at two batch sizes (tests/test_gpu_precise.py's figure, here per image)
ROW_TOL = 10 * EXACT_TOL  # a row of the last hidden state (the golden test's figure for lhs_rows)
GUARD = 5                 # sentinel rows behind every output
T0 = time.time()


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops, synthetic
    from oracle import pigeon_oracle as orc
    _lib.require_gpu()                       # fails loudly if the HIP library / GPU is missing -- no fallback
    return dict(lib=_lib, ops=hip_ops, L=_lib.load(), syn=synthetic, orc=orc)


def _guarded(rows, cols, dtype, guard=GUARD):
    return torch.full((rows + guard, cols), X.SENTINEL, dtype=dtype, device=DEV)


def _no(found):
    assert not found, "\n".join(found[:40])


# ================================================================================================================ split_x3
SPLIT_SHAPES = [(r, c) for c in (1024, 4096) for r in (1, 3, 577, 28 * 577)]


@pytest.mark.parametrize("rows,cols", SPLIT_SHAPES)
def test_split_x3_bit_for_bit(env, rows, cols):
    """pg_op_x3_split (no GELU): all three segments equal the triple of the fp32 value bit for bit -- fp16-subnormal halves, ties, +-0 and
    the saturation at +-65504 planted at the first row, the middle and the very end; (28 * 577, 4096) engages the grid-stride loop (the
    grid is capped at 16 384 blocks)."""
    ops, lib, L = env["ops"], env["lib"], env["L"]
    v = X.triple_values(rows, cols, 100 + rows + cols, DEV)
    got = _guarded(rows, 3 * cols, F16)
    lib.check(L.pg_op_x3_split(ops._p(v), ops._p(got), rows, cols, 0, ops._stream()), "pg_op_x3_split")
    torch.cuda.synchronize()
    _no(X.compare_triple(got.cpu(), v.cpu(), cols))


@pytest.mark.parametrize("rows,cols", SPLIT_SHAPES)
def test_split_x3_gelu(env, rows, cols, capsys):
    """pg_op_x3_split through QuickGELU: a consistent triple whose hi + lo lies within gelu_ieee_bound (the accurate expf, the IEEE
    division) + the triple's reconstruction error of x * sigmoid(1.702 x) in fp64; inputs in +-12 and +-40 (the sigmoid saturated)."""
    ops, lib, L = env["ops"], env["lib"], env["L"]
    g = torch.Generator(device=DEV).manual_seed(200 + rows + cols)
    v = (torch.randn((rows, cols), generator=g, device=DEV) * 4.0).clamp(-12.0, 12.0)
    v[0, :4] = torch.tensor([40.0, -40.0, 0.0, -0.0], device=DEV)
    v[rows - 1, cols - 4:] = torch.tensor([-40.0, 40.0, 12.0, -12.0], device=DEV)
    got = _guarded(rows, 3 * cols, F16)
    lib.check(L.pg_op_x3_split(ops._p(v), ops._p(got), rows, cols, 1, ops._stream()), "pg_op_x3_split")
    torch.cuda.synchronize()
    gc = got.cpu()
    found, val = X.triple_consistent(gc, cols, rows)
    vd = v.cpu().double()
    y, e = X.quick_gelu64(vd), X.gelu_ieee_bound(vd)
    tol = e + X.triple_recon_bound(y.abs() + e)
    found += X.compare_values("gelu triple hi+lo", val, y, tol)
    assert bool((gc[rows:].float() == X.SENTINEL).all()), "guard rows written"
    with capsys.disabled():
        print(f"\nsplit_x3 gelu ({rows}, {cols}): worst |err| / bound {float(((val - y).abs() / tol).max()):.3f}")
    _no(found)


# ================================================================================================================ LayerNorm family
LN_ROWS = (1, 2, 3, 5, 577, 28 * 577)


def _run_ln(env, kernel, x, gam, bet):
    """One LayerNorm-type kernel on the rows x -> (buffer with guard rows, out kind for compare_layernorm)."""
    ops, lib, L = env["ops"], env["lib"], env["L"]
    rows = x.shape[0]
    if kernel == "x3":
        got = _guarded(rows, 3 * X.HIDDEN, F16)
        lib.check(L.pg_op_x3_layernorm(ops._p(x), ops._p(gam), ops._p(bet), ops._p(got), rows, 1e-5, ops._stream()), "pg_op_x3_layernorm")
        return got, "x3"
    dt = {"f32": F32, "f16": F16, "bf16": BF16}[kernel]
    got = _guarded(rows, X.HIDDEN, dt)
    pg = {F32: lib.PG_DTYPE_F32, F16: lib.PG_DTYPE_F16, BF16: lib.PG_DTYPE_BF16}[dt]
    lib.check(L.pg_op_layernorm(ops._p(x), ops._p(gam), ops._p(bet), ops._p(got), pg, rows, 1e-5, ops._stream()), "pg_op_layernorm")
    return got, dt


@pytest.mark.parametrize("kernel,rows", [(k, r) for k in ("x3", "f32", "f16", "bf16") for r in LN_ROWS] + [("f16", 512 * 577)])
def test_layernorm_per_element(env, kernel, rows, capsys):
    """pg_op_x3_layernorm and pg_op_layernorm (fp32 / fp16 / bf16 out): every element within layernorm_bound of the fp64 LayerNorm -- on
    Gaussian rows, rows with |mean| >> std (mean 50, std 0.1: where a one-pass variance fails), constant rows (variance 0), rows with
    one 3e3 outlier and small rows, with jittered gamma / beta; the triple also consistent.  512 * 577 rows once (fp16 out)."""
    x = X.ln_rows(rows, 300 + rows % 1000, DEV, kind0=rows)
    gam, bet = X.ln_affine(301, DEV)
    got, out = _run_ln(env, kernel, x, gam, bet)
    torch.cuda.synchronize()
    worst = []
    if out == "x3":                                            # (fp16 conversions of the consistency check: on the CPU)
        found = X.compare_layernorm(got.cpu(), x.cpu(), gam.cpu(), bet.cpu(), 1e-5, out, kind0=rows, worst=worst)
    else:
        found = X.compare_layernorm(got, x, gam, bet, 1e-5, out, kind0=rows, worst=worst)
    with capsys.disabled():
        print(f"\nlayernorm [{kernel}] {rows} rows: worst |err| / bound {max(worst):.3f}")
    _no(found)


@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("stat", [None, F16, BF16], ids=["plain", "stat_f16", "stat_bf16"])
def test_preln_per_element(env, stat, rows):
    """pg_op_preln: a row with row % 577 == 0 becomes LN(cls + pos[0]) whatever X held there (a sentinel is planted), every other row is
    normalised in place; nothing past the last row is written.  With x16 / rowstat: x16 == the 16-bit value of the NEW row bit for bit and
    (rstd, mean rstd) of the NEW row within rowstat_bound."""
    ops = env["ops"]
    x = X.ln_rows(rows, 400 + rows % 1000, DEV, kind0=rows + 1)
    x[::X.TOKENS] = 1234.5
    gam, bet = X.ln_affine(401, DEV)
    g = torch.Generator(device=DEV).manual_seed(402)
    cls, pos0 = torch.randn(X.HIDDEN, generator=g, device=DEV) * 0.03, torch.randn(X.HIDDEN, generator=g, device=DEV) * 0.02
    want_in = x.clone()
    want_in[::X.TOKENS] = cls + pos0                            # one fp32 addition, as the kernel forms the class row
    buf = _guarded(rows, X.HIDDEN, F32)
    buf[:rows] = x
    x16 = rs = None
    if stat is not None:
        x16, rs = _guarded(rows, X.HIDDEN, stat), _guarded(rows, 2, F32)
    ops.preln(buf, cls, pos0, gam, bet, rows=rows, x16=x16, rowstat=rs)
    torch.cuda.synchronize()
    found = X.compare_layernorm(buf, want_in, gam, bet, 1e-5, F32, kind0=rows + 1, name="preln")
    if stat is not None:
        new = buf[:rows].cpu()
        want16 = (new.clamp(-X.F16_MAX, X.F16_MAX) if stat == F16 else new).to(stat)
        h = x16.cpu()
        bad = h[:rows].view(torch.int16) != want16.view(torch.int16)
        found += [f"preln x16: got {float(h[i, j])!r} want {float(want16[i, j])!r} at row {i} col {j}" for (i, j) in X._first(bad)]
        if not bool((h[rows:].float() == X.SENTINEL).all()) or not bool((rs[rows:] == X.SENTINEL).all()):
            found.append("preln: guard rows of x16 / rowstat written")
        ref, bound = X.rowstat_bound(buf[:rows])
        found += X.compare_rowstat("preln rowstat", rs[:rows], ref, bound, kind0=rows + 1)
    _no(found)


@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("dtype", [F16, BF16], ids=["f16", "bf16"])
def test_rowstat_cast_per_element(env, dtype, rows):
    """pg_op_rowstat_cast: the 16-bit copy bit for bit, (rstd, mean rstd) within the two-pass bound, on every row kind."""
    ops, lib, L = env["ops"], env["lib"], env["L"]
    x = X.ln_rows(rows, 500 + rows % 1000, DEV, kind0=rows + 2)
    x16, rs = _guarded(rows, X.HIDDEN, dtype), _guarded(rows, 2, F32)
    lib.check(L.pg_op_rowstat_cast(ops._p(x), ops._p(x16), ops._dt16(x16), ops._p(rs), rows, 1e-5, ops._stream()), "pg_op_rowstat_cast")
    torch.cuda.synchronize()
    xc, h = x.cpu(), x16.cpu()
    want16 = (xc.clamp(-X.F16_MAX, X.F16_MAX) if dtype == F16 else xc).to(dtype)
    bad = h[:rows].view(torch.int16) != want16.view(torch.int16)
    found = [f"rowstat_cast x16: got {float(h[i, j])!r} want {float(want16[i, j])!r} at row {i} col {j}" for (i, j) in X._first(bad)]
    if not bool((h[rows:].float() == X.SENTINEL).all()) or not bool((rs[rows:] == X.SENTINEL).all()):
        found.append("rowstat_cast: guard rows written")
    ref, bound = X.rowstat_bound(x)
    found += X.compare_rowstat("rowstat_cast", rs[:rows], ref, bound, kind0=rows + 2)
    _no(found)


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 28 * 577])
@pytest.mark.parametrize("inputs", ["row_kinds", "integers"])
def test_rowstat_finalize_per_element(env, inputs, rows, capsys):
    """pg_op_rowstat_finalize on 16 slots: (rstd, mean rstd) within rowstat_finalize_bound -- the bound of the ONE-pass form it computes,
    cancellation term included -- of fp64 on the same partials; on the row kinds (partials formed in fp64, rounded once) and on integer
    rows, whose partials and their sums are exact in fp32."""
    ops, lib, L = env["ops"], env["lib"], env["L"]
    if inputs == "integers":
        g = torch.Generator(device=DEV).manual_seed(600 + rows)
        x = torch.randint(-8, 9, (rows, X.HIDDEN), generator=g, device=DEV).float() + (torch.arange(rows, device=DEV) % 7).float()[:, None]
    else:
        x = X.ln_rows(rows, 601 + rows % 1000, DEV, kind0=rows + 3)
    part = X.statparts_of(x)
    if inputs == "integers":
        assert bool((part.double() == X.statparts_of(x.double()).double()).all()) and float(part[:, :, 1].sum(0).max()) < 2.0 ** 24
    rs = _guarded(rows, 2, F32)
    lib.check(L.pg_op_rowstat_finalize(ops._p(part), 16, ops._p(rs), rows, 1e-5, ops._stream()), "pg_op_rowstat_finalize")
    torch.cuda.synchronize()
    ref, bound = X.rowstat_finalize_bound(part)
    found = X.compare_rowstat("rowstat_finalize", rs[:rows], ref, bound, kind0=rows + 3 if inputs == "row_kinds" else None)
    if not bool((rs[rows:] == X.SENTINEL).all()):
        found.append("rowstat_finalize: guard rows written")
    ratio = lambda c: float(((rs[:rows, c].double() - ref[c]).abs() / bound[c].clamp_min(2.0 ** -149)).max())      # (a zero row: 0 of a bound of 0)
    with capsys.disabled():
        print(f"\nrowstat_finalize [{inputs}] {rows} rows: worst |err| / bound rstd {ratio(0):.3f}, mean*rstd {ratio(1):.3f}")
    _no(found)


# ================================================================================================================ im2col
def _pixels(kind, n, pdt):
    if kind == "representable":
        return X.representable_pixels(n, 700 + n, DEV).to(pdt).contiguous()
    g = torch.Generator(device=DEV).manual_seed(701 + n)
    return torch.randn((n, 3, 336, 336), generator=g, device=DEV).to(pdt).contiguous()


@pytest.mark.parametrize("n", [1, 2, 33])
@pytest.mark.parametrize("odt", [F16, BF16], ids=["to_f16", "to_bf16"])
@pytest.mark.parametrize("pdt", [F32, F16, BF16], ids=["px_f32", "px_f16", "px_bf16"])
def test_im2col_all_pairs(env, pdt, odt, n):
    """pg_op_im2col, all six (pixel, operand) type pairs: equal to unfold (k = c 196 + ky 14 + kx) rounded to the operand type, pad columns
    588..639 zero, guard rows untouched -- on pixels exact in every type (one right answer for every pair) and on Gaussian pixels (the
    pairs that round)."""
    ops, lib, L = env["ops"], env["lib"], env["L"]
    for kind in ("representable", "gaussian"):
        px = _pixels(kind, n, pdt)
        got = _guarded(n * X.PATCHES, X.PATCH_KPAD, odt)
        lib.check(L.pg_op_im2col(ops._p(px), ops._PIXDT[pdt], ops._p(got), ops._dt16(got), n, ops._stream()), "pg_op_im2col")
        torch.cuda.synchronize()
        _no([f"[{kind}] {m}" for m in X.compare_im2col(got.cpu(), px.cpu())])


@pytest.mark.parametrize("n", [1, 2, 33])
@pytest.mark.parametrize("pdt", [F32, F16, BF16], ids=["px_f32", "px_f16", "px_bf16"])
def test_x3_im2col_bit_for_bit(env, pdt, n):
    """pg_op_x3_im2col: the three K-segments [0, 588), [640, 1228), [1280, 1868) hold the triple of unfold's value bit for bit, every pad
    column is zero, guard rows untouched."""
    ops = env["ops"]
    for kind in ("representable", "gaussian"):
        px = _pixels(kind, n, pdt)
        got = _guarded(n * X.PATCHES, 3 * X.PATCH_KPAD, F16)
        ops.x3_im2col(px, out=got)
        torch.cuda.synchronize()
        _no([f"[{kind}] {m}" for m in X.compare_triple(got.cpu(), X.im2col_ref(px.cpu()), X.PATCH_K, seg=X.PATCH_KPAD, where=X.im2col_where)])


# ================================================================================================================ sum of the K-parts
@pytest.mark.parametrize("resid", [0, 1])
@pytest.mark.parametrize("S", [2, 3, 4, 6])
def test_sum_parts_bit_for_bit(env, S, resid):
    """pg_op_sum_parts: bit for bit the fp32 additions ((p0 + p1) + p2) ... then dst + that, done in that order with torch on the CPU;
    an element count that fills the capped grid more than once and ends ragged (4 (16384 * 256 + 777)), a small one, a part stride
    larger than the count, parts of very different magnitudes; nothing past element n is written."""
    ops = env["ops"]
    for n in (4 * 1001, 4 * (16384 * 256 + 777)):
        g = torch.Generator(device=DEV).manual_seed(800 + S + n % 100)
        stride = n + 64
        parts = torch.randn((S, stride), generator=g, device=DEV) * torch.tensor([1.0, 300.0, 0.01, 7.0, 1e3, 1e-3][:S], device=DEV)[:, None]
        dst0 = torch.randn(n, generator=g, device=DEV)
        dst = torch.full((n + 1024,), X.SENTINEL, dtype=F32, device=DEV)
        dst[:n] = dst0 if resid else 123.0                      # (without the residual the old content must not matter)
        ops.sum_parts(parts, dst, bool(resid), n=n)
        torch.cuda.synchronize()
        want = X.sum_parts_ref(parts[:, :n], dst0 if resid else None)
        got = dst.cpu()
        bad = got[:n].view(torch.int32) != want.view(torch.int32)
        assert not bool(bad.any()), f"S={S} resid={resid} n={n}: {int(bad.sum())} elements differ, first at {int(bad.nonzero()[0])} " \
                                    f"(block {int(bad.nonzero()[0]) // 1024 % 16384}, pass {int(bad.nonzero()[0]) // (1024 * 16384)})"
        assert bool((got[n:] == X.SENTINEL).all()), "elements past n written"


@pytest.mark.parametrize("S,Kp", [(2, 6144), (4, 2048), (3, 4096), (6, 2048)])
def test_gemm_parts_exact(env, S, Kp):
    """pg_op_gemm16_parts at fc2's shapes (N = 1024, M = 10 * 577): S = 2 with Kp = 6144 and S = 4 with Kp = 2048 (never run before), 3
    and 6 -- on integer operands every part EQUALS the fp64 product of its K slice, the bias rides in part 0 only, and the buffer behind
    the last part is untouched."""
    ops, lib, L = env["ops"], env["lib"], env["L"]
    M, N = 10 * 577, 1024
    c = X.make_exact_gemm_case(X.EPI_F32, M, N, Kp, F16, 900 + S, DEV)            # (checks 9 Kp + ... stays in the exact range)
    g = torch.Generator(device=DEV).manual_seed(901 + S)
    A = torch.randint(-3, 4, (M, S * Kp), generator=g, device=DEV).to(F16)
    W = torch.randint(-3, 4, (N, S * Kp), generator=g, device=DEV).to(F16)
    parts = torch.full((S * M * N + 4096,), X.SENTINEL, dtype=F32, device=DEV)
    lib.check(L.pg_op_gemm16_parts(ops._dt16(A), ops._p(A), A.stride(0), ops._p(W), W.stride(0), ops._p(c.bias), ops._p(parts), M, N, Kp, S,
                                   ops._stream()), "pg_op_gemm16_parts")
    torch.cuda.synchronize()
    found = []
    for p in range(S):
        want = A[:, p * Kp:(p + 1) * Kp].double() @ W[:, p * Kp:(p + 1) * Kp].double().t()
        if p == 0:
            want = want + c.bias.double()[None, :]
        got = parts[p * M * N:(p + 1) * M * N].view(M, N).double()
        bad = got != want
        found += [f"part {p}: got {float(got[i, j])!r} want {float(want[i, j])!r} at row {i} (256-row tile {i // 256} +{i % 256}) col {j}" for (i, j) in X._first(bad)]
        if bad.any():
            found.append(f"part {p}: {int(bad.sum())} wrong elements")
    if not bool((parts[S * M * N:] == X.SENTINEL).all()):
        found.append("elements behind the last part written")
    _no(found)


# ================================================================================================================ attention -> triple
def _attention_x3(env, qkv, n):
    """pg_op_attention_x3 into a guarded buffer, and pg_op_attention_f32 (the split-fp16 arm) on the same input."""
    ops = env["ops"]
    got = _guarded(n * X.TOKENS, 3 * X.HIDDEN, F16)
    ops.attention_x3(qkv, n, out=got)
    f32 = ops.attention_f32(qkv, n)
    torch.cuda.synchronize()
    gc = got.cpu()
    found = [f"vs triple_ref(pg_op_attention_f32): {m}" for m in X.compare_triple(gc, f32.cpu(), X.HIDDEN, where=X.attention_where)]
    return gc, found


@pytest.mark.parametrize("n", [1, 3, 28])
def test_attention_x3_onehot(env, n):
    """The one-hot cases of test_gpu_exact.py through pg_op_attention_x3: the weights are exactly 1 and 0, the fp32 value is V[target]
    itself, so the output triple == triple_ref(V[target]) bit for bit; and == triple_ref of pg_op_attention_f32's output."""
    for kind in ("spread", "last"):
        qkv, want, gap = X.attention_onehot_case(n, F32, kind, 128.0, 8.0, device=DEV)
        assert gap >= 160.0
        gc, found = _attention_x3(env, qkv, n)
        found += X.compare_triple(gc, want.float().cpu(), X.HIDDEN, where=X.attention_where)
        _no([f"[{kind}] {m}" for m in found])


@pytest.mark.parametrize("n", [1, 3, 28])
def test_attention_x3_uniform_and_staircase(env, n, capsys):
    """The uniform and staircase cases: a consistent triple, hi + lo within the tolerance test_gpu_exact.py holds pg_op_attention_f32 to
    (two ulp of fp32 of sum(V) / 577; the staircase bound of _exactref.staircase_eps) + the triple's reconstruction error, and bit-equal to
    triple_ref of pg_op_attention_f32's output."""
    qkv, vs = X.attention_uniform_case(n, F32, device=DEV)
    want = (vs / 577.0).unsqueeze(1).expand(n, X.TOKENS, X.HEADS, X.HDIM).reshape(n * X.TOKENS, X.HIDDEN).cpu()
    gc, found = _attention_x3(env, qkv, n)
    fc, val = X.triple_consistent(gc, X.HIDDEN, n * X.TOKENS)
    found += fc + X.compare_attention(val, want, 2 * X.ulp32(want) + X.triple_recon_bound(want))
    _no(["[uniform] " + m for m in found])
    for step in (7.9, 8.1):
        qkv, q, k, v = X.attention_staircase_case(n, F32, step, 8.0, device=DEV)
        want, tol = X.staircase_tol(F32, q, k, v, 8.0, base2=False)
        want, tol = want.cpu(), tol.cpu()
        gc, found = _attention_x3(env, qkv, n)
        fc, val = X.triple_consistent(gc, X.HIDDEN, n * X.TOKENS)
        tol = tol + X.triple_recon_bound(want.abs() + tol)
        with capsys.disabled():
            print(f"\nattention_x3 staircase step {step} n={n}: worst |err| / bound {float(((val - want).abs() / tol).max()):.3f}")
        found += fc + X.compare_attention(val, want, tol)
        _no([f"[staircase {step}] " + m for m in found])


def test_attention_x3_refused_with_the_fp32_mfma_arm(env):
    ops, lib, L = env["ops"], env["lib"], env["L"]
    qkv = torch.zeros((X.TOKENS, 3 * X.HIDDEN), dtype=F32, device=DEV)
    out = _guarded(X.TOKENS, 3 * X.HIDDEN, F16)
    lib.check(L.pg_tune_exact_attention(1), "pg_tune_exact_attention")
    try:
        assert L.pg_op_attention_x3(ops._p(qkv), ops._p(out), 1, ops._stream()) == -4          # PG_ESTATE
        torch.cuda.synchronize()
        assert bool((out.float() == X.SENTINEL).all()), "a refused call must not launch"
    finally:
        L.pg_tune_exact_attention(0)


# ================================================================================================================ every route of the encoder
LAYERS = 2
FIXED_SIZES = (28, 128, 129, 130, 257)
GEMMS = ("qkv", "out", "fc1", "fc2")


def _sig(p):
    return tuple(p[k] for k in GEMMS) + (p["fc1_fused"], p["attn_x3"])


def change_sizes(ops):
    """Every n in 1 .. 128 at which pg_vit_precise_plan's signature differs from n - 1's (1 included)."""
    out, prev = [], None
    for n in range(1, 129):
        s = _sig(ops.vit_precise_plan(n))
        if s != prev:
            out.append(n)
        prev = s
    return out


def _label(ops, n):
    p = ops.vit_precise_plan(n)
    s = "(" + ",".join(str(p[k]) for k in GEMMS) + ")" + (" fc1-fused" if p["fc1_fused"] else "") + ("" if p["attn_x3"] else " attn-f32")
    return s + (f" x{p['chunks']} passes of <= {p['chunk']}" if p["chunks"] > 1 else "")


@pytest.fixture(scope="module")
def tower(env):
    """The 2-layer tower, a pool of images (batches are prefixes of it) and the oracle's last hidden state of the whole pool in fp64 (torch
    on the GPU: a checker), computed once."""
    ops, syn, orc = env["ops"], env["syn"], env["orc"]
    sd = syn.make_vit_weights(seed=17, layers=LAYERS, affine_jitter=True)
    enc = ops.VitEncoder(sd, layers=LAYERS, precise=True)
    pool = max(FIXED_SIZES)
    px = syn.make_pixels(pool, seed=4321).to(DEV)
    t0 = time.time()
    sd64 = {k: v.to(device=DEV, dtype=torch.float64) for k, v in sd.items()}
    ref_h = torch.cat([orc.vit_last_hidden_state(sd64, px[i:i + 8], dtype=torch.float64) for i in range(0, pool, 8)], dim=0)
    torch.cuda.synchronize()
    t_ref = time.time() - t0
    # for scale: the fp32 oracle's own error against fp64, on the CPU, first four images
    h32 = orc.vit_last_hidden_state(sd, px[:4].cpu()).double()
    r4 = ref_h[:4].cpu()
    e32 = float(((h32.mean(1) - r4.mean(1)).norm(dim=1) / r4.mean(1).norm(dim=1)).max())
    r32 = float(((h32 - r4).norm(dim=2) / r4.norm(dim=2)).max())
    yield dict(enc=enc, px=px, ref_h=ref_h, ref_e=ref_h.mean(1), sd=sd, t_ref=t_ref, e32=e32, r32=r32, lines=[])
    enc.close()


def run_sizes(env, tower, sizes, tag):
    """forward_precise at each size against fp64: per image, per row (first and last image: every row; the others: rows 0, 1, 288, 575,
    576), and per image across the sizes.  Returns (findings, records {n: (label, worst embedding error, worst row error)})."""
    ops, enc, px, ref_h, ref_e = env["ops"], tower["enc"], tower["px"], tower["ref_h"], tower["ref_e"]
    found, rec, embs = [], {}, {}
    some = torch.tensor([0, 1, 288, 575, 576], device=DEV)
    for n in sizes:
        e, h = enc.forward_precise(px[:n], return_hidden=True)
        torch.cuda.synchronize()
        ee = (e.double() - ref_e[:n]).norm(dim=1) / ref_e[:n].norm(dim=1)
        for i in (~(ee <= EXACT_TOL)).nonzero().flatten()[:4].tolist():
            found.append(f"[{tag}] n={n} {_label(ops, n)}: image {i} embedding error {float(ee[i]):.3e} > {EXACT_TOL}")
        worst_row = 0.0
        for imgs, rows in (([0, n - 1] if n > 1 else [0], None), (list(range(1, n - 1)), some)):
            if not imgs:
                continue
            idx = torch.tensor(imgs, device=DEV)
            if rows is None:
                hh, rr = h[idx].double(), ref_h[idx]
            else:
                hh, rr = h[idx[:, None], rows[None, :]].double(), ref_h[idx[:, None], rows[None, :]]
            er = (hh - rr).norm(dim=2) / rr.norm(dim=2)
            worst_row = max(worst_row, float(torch.nan_to_num(er, nan=float("inf")).max()))
            for (a, b) in (~(er <= ROW_TOL)).nonzero()[:4].tolist():
                t = b if rows is None else int(rows[b])
                found.append(f"[{tag}] n={n} {_label(ops, n)}: image {imgs[a]} token {t} (row {imgs[a] * 577 + t}, 256-row tile {(imgs[a] * 577 + t) // 256}) "
                             f"hidden-row error {float(er[a, b]):.3e} > {ROW_TOL}")
        rec[n] = (_label(ops, n), float(torch.nan_to_num(ee, nan=float("inf")).max()), worst_row)
        embs[n] = e.double()
    worst_cross = 0.0
    for a in sizes:
        for b in sizes:
            if b >= a:
                continue
            d = (embs[a][:b] - embs[b]).norm(dim=1) / embs[b].norm(dim=1)
            worst_cross = max(worst_cross, float(torch.nan_to_num(d, nan=float("inf")).max()))
            for i in (~(d <= CROSS_SIZE_TOL)).nonzero().flatten()[:2].tolist():
                found.append(f"[{tag}] image {i}: batch of {a} {_label(ops, a)} against batch of {b} {_label(ops, b)}: {float(d[i]):.3e} > {CROSS_SIZE_TOL}")
    return found, rec, worst_cross


def _table(tower, tag, rec, worst_cross):
    lines = [f"[{tag}] batch -> (QKV, out, fc1, fc2) route: worst image embedding error, worst hidden-row error vs fp64"]
    lines += [f"[{tag}] n={n:4d} {lab:34s} emb {e:.2e}  row {r:.2e}" for n, (lab, e, r) in sorted(rec.items())]
    by = {}
    for n, (lab, e, r) in rec.items():
        k = lab.split(" x")[0]
        by[k] = (max(by.get(k, (0, 0))[0], e), max(by.get(k, (0, 0))[1], r))
    lines += [f"[{tag}] signature {k:28s} worst emb {e:.2e}  worst row {r:.2e}" for k, (e, r) in sorted(by.items())]
    lines.append(f"[{tag}] same image across batch sizes: worst {worst_cross:.2e} (tolerance {CROSS_SIZE_TOL}); fp32 oracle vs fp64: emb {tower['e32']:.2e}, "
                 f"worst row {tower['r32']:.2e}; tolerances {EXACT_TOL} / {ROW_TOL}")
    _keep(tower, lines)
    return lines


def _keep(tower, lines):
    tower["lines"] += lines
    from test_gpu_precise import _report                     # the suite's report writer (the run's output folder)
    _report(tower["lines"], "exact_tier_routes.txt")


def test_every_route_of_the_encoder(env, tower, capsys):
    """The batch sizes are asked of pg_vit_precise_plan: every n in 1 .. 128 at which its signature changes, n - 1 of each, and 28, 128,
    129, 130, 257 (above 128: equal internal passes, output / hidden pointers offset per pass).  Per size: every image's embedding within
    EXACT_TOL of the fp64 oracle, every checked hidden row within 10 EXACT_TOL, and every image's embedding within 1e-6 of its
    embedding at every other size."""
    ops = env["ops"]
    ch = change_sizes(ops)
    sizes = sorted(set(ch) | {n - 1 for n in ch if n > 1} | set(FIXED_SIZES))
    plans = {n: ops.vit_precise_plan(n) for n in sizes}
    routes = {plans[n][k] for n in sizes for k in GEMMS}
    missing = [f"S = {s}" if s else "a gemm_mid route" for s in (0, 1, 2, 3, 6) if s not in routes]
    missing += [w for w, ok in (("fc1 fused", any(p["fc1_fused"] for p in plans.values())), ("fc1 unfused", any(not p["fc1_fused"] for p in plans.values()))) if not ok]
    found, rec, cross = run_sizes(env, tower, sizes, "default")
    with capsys.disabled():
        print("\n" + "\n".join(_table(tower, "default", rec, cross)) + f"\nfp64 reference of {tower['px'].shape[0]} images: {tower['t_ref']:.1f} s")
    assert not missing, f"the cost model no longer produces: {missing} (a dead branch: report it)"
    assert plans[130]["chunks"] == 2 and plans[257]["chunks"] == 3
    _no(found)


@pytest.mark.parametrize("knob", ["gemm_mid_off", "fusion_off"])
def test_every_route_with_a_knob_turned(env, tower, knob, capsys):
    """The same sweep on the signature-change sizes with pg_tune_gemm_mid(0) (small batches forced onto the persistent kernel's parts)
    and with pg_tune_exact_fusion(0) (fp32 buffers + split launches); knobs restored whatever happens."""
    ops, L = env["ops"], env["L"]
    sizes = change_sizes(ops)                                   # of the DEFAULT plan
    try:
        if knob == "gemm_mid_off":
            ops.tune_gemm_mid(False)
            assert all(ops.vit_precise_plan(n)[k] != 0 for n in sizes for k in GEMMS)
        else:
            ops.tune_exact_fusion(False)
            assert all(not ops.vit_precise_plan(n)["fc1_fused"] and not ops.vit_precise_plan(n)["attn_x3"] for n in sizes)
        found, rec, cross = run_sizes(env, tower, sizes, knob)
        lines = _table(tower, knob, rec, cross)
    finally:
        ops.tune_gemm_mid(True)
        ops.tune_exact_fusion(True)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    _no(found)


def test_negative_control_two_products_is_outside_the_tolerance(env, tower, capsys):
    """The tolerances can see ONE missing partial product: with pg_tune_exact_products(2) (the weights at their fp16 value) at least one
    image of a 4-image batch lands outside EXACT_TOL of the fp64 oracle.  Arithmetic only; 3 restored whatever happens."""
    ops, enc, px, ref_e = env["ops"], tower["enc"], tower["px"], tower["ref_e"]
    n = 4
    try:
        ops.tune_exact_products(2)
        e2 = enc.forward_precise(px[:n])
        torch.cuda.synchronize()
    finally:
        ops.tune_exact_products(3)
    e3 = enc.forward_precise(px[:n])
    torch.cuda.synchronize()
    err = lambda e: (e.double() - ref_e[:n]).norm(dim=1) / ref_e[:n].norm(dim=1)
    line = (f"[negative control] {LAYERS} layers, {n} images: two products {[f'{float(v):.2e}' for v in err(e2)]}, three products "
            f"{[f'{float(v):.2e}' for v in err(e3)]} (EXACT_TOL {EXACT_TOL})")
    _keep(tower, [line])
    with capsys.disabled():
        print("\n" + line)
    assert bool((err(e3) <= EXACT_TOL).all())
    assert bool((err(e2) > EXACT_TOL).any()), "two partial products are inside the exact tier's tolerance: the tolerance cannot see a missing product"


def test_empty_batch_and_short_workspace(env, tower):
    """n = 0 stays a no-op; a workspace one byte short of pg_vit_precise_workspace_bytes(n) is PG_ENOMEM for 28 and 130 images (a host
    check: nothing is launched, the outputs keep their sentinel)."""
    ops, lib, L, enc, px = env["ops"], env["lib"], env["L"], tower["enc"], tower["px"]
    emb = torch.full((130, X.HIDDEN), X.SENTINEL, dtype=F32, device=DEV)
    assert L.pg_vit_forward_precise(enc._h, None, lib.PG_DTYPE_F32, 0, None, None, None, 0, ops._stream()) == 0
    e0 = enc.forward_precise(px[:0])
    assert tuple(e0.shape) == (0, X.HIDDEN)
    for n in (28, 130):
        need = C.c_size_t()
        lib.check(L.pg_vit_precise_workspace_bytes(enc._h, n, C.byref(need)), "pg_vit_precise_workspace_bytes")
        ws = torch.empty(need.value + 256, dtype=torch.uint8, device=DEV)
        off = (-ws.data_ptr()) % 256
        rc = L.pg_vit_forward_precise(enc._h, ops._p(px), lib.PG_DTYPE_F32, n, ops._p(emb), None, C.c_void_p(ws.data_ptr() + off), need.value - 1, ops._stream())
        torch.cuda.synchronize()
        assert rc == -2 and bool((emb == X.SENTINEL).all()), (n, rc)                 # PG_ENOMEM
        lib.check(L.pg_vit_forward_precise(enc._h, ops._p(px), lib.PG_DTYPE_F32, n, ops._p(emb), None, C.c_void_p(ws.data_ptr() + off), need.value,
                                           ops._stream()), "pg_vit_forward_precise")
        torch.cuda.synchronize()
        ref = tower["ref_e"][:n]
        assert bool(((emb[:n].double() - ref).norm(dim=1) / ref.norm(dim=1) <= EXACT_TOL).all()) and bool((emb[n:] == X.SENTINEL).all())
        emb.fill_(X.SENTINEL)
        del ws


def test_wall_time_of_this_file(capsys):
    with capsys.disabled():
        print(f"\ntests/test_gpu_exact_tier.py: {time.time() - T0:.0f} s since import")
