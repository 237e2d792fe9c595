"""pg_knn_prepare / pg_knn_search on the GPU (run with -m gpu on an MI355X), through the C ABI.

The result is defined without reference to the path that computes it, so every test compares paths: integer banks against int64
numpy at zero tolerance (mode 0 and mode 1: a wrong A/B fragment map, a dropped K step, a tile at the wrong rows or a lost tie show
up as a location), mode 0 against mode 1 bit for bit on every bank, what mode 2 certifies against mode 1, Gaussian banks against the
float64 truth under tests/_knnref.py's comparators, and the certificate's yield on the banks made to defeat or to please it.  Every
output and the workspace sit between guard regions that must keep their pattern."""
import ctypes as C

import numpy as np
import pytest
import torch

import _georef as G
import _knnref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODES = {"auto": 0, "exact": 1, "filter": 2}


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops
    _lib.require_gpu()
    hip_ops.tune_knn_spans(0)
    yield dict(lib=_lib, ops=hip_ops, L=_lib.load(), banks={})
    hip_ops.tune_knn_spans(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def prepared(env, X):
    """one pg_knn_prepare per bank array (keyed by identity; the array is kept alive by the cache)"""
    key = id(X)
    if key not in env["banks"]:
        env["banks"][key] = (X, env["ops"].knn_prepare(dev(X)))
    return env["banks"][key][1]


def guarded(n, dtype, sentinel):
    buf = torch.full((n + 2 * G.GUARD,), sentinel, dtype=dtype, device=DEV)
    return buf, buf[G.GUARD:G.GUARD + n]


def guards_ok(buf, n, sentinel):
    return bool((buf[:G.GUARD] == sentinel).all()) and bool((buf[G.GUARD + n:] == sentinel).all())


def search(env, X, Q, k, mode="auto", exclude=None, spans=0):
    """-> (idx (B,k) int64, d2 (B,k) fp32, certified (B,) bool) as numpy, through the C ABI, guards and inputs checked"""
    ops, L = env["ops"], env["L"]
    ops.tune_knn_spans(spans)
    try:
        bank = prepared(env, X)
        q = dev(Q)
        keep = q.clone()
        B = q.shape[0]
        ex = None if exclude is None else dev(np.asarray(exclude, np.int64))
        need = ops.knn_workspace_bytes(bank.n, B, k)
        assert need % 256 == 0
        wsb, ws = guarded(need + 4096, torch.uint8, 0x5A)                  # 64 guard bytes each side; the start is aligned below
        off = (-ws.data_ptr()) % 256
        ib, iv = guarded(B * k, torch.int64, -77)
        db, dv = guarded(B * k, torch.float32, G.SENTINEL)
        cb, cv = guarded(B, torch.uint8, 0x5A)
        s = bank.struct()
        env["lib"].check(L.pg_knn_search(C.byref(s), ops._p(q), B, k, ops._p(ex), MODES[mode], ops._p(iv), ops._p(dv),
                                         ops._p(cv), C.c_void_p(ws.data_ptr() + off), need, ops._stream()), "pg_knn_search")
        torch.cuda.synchronize()
        assert guards_ok(ib, B * k, -77) and guards_ok(db, B * k, G.SENTINEL) and guards_ok(cb, B, 0x5A), "an output guard was written"
        assert bool((wsb[:G.GUARD + off] == 0x5A).all()) and bool((wsb[G.GUARD + off + need:] == 0x5A).all()), "a workspace guard was written"
        assert torch.equal(q.view(torch.int32), keep.view(torch.int32)), "the queries changed"       # bits: a NaN query equals itself
        return iv.view(B, k).cpu().numpy(), dv.view(B, k).cpu().numpy(), cv.cpu().numpy().astype(bool)
    finally:
        ops.tune_knn_spans(0)


def same_bits(a, b, what):
    R.compare_exact(a[0], a[1].view(np.int32), b[0], b[1].view(np.int32), what=what)


# ---------------------------------------------------------------------------------------------------------------------- banks, once
@pytest.fixture(scope="module")
def latent(env):
    X, Q = R.latent8(0, 4099, 64)
    return dict(X=X, Q=Q, d64=R.d2_f64(Q, X), exact=search(env, X, Q, 16, "exact"))


@pytest.fixture(scope="module")
def clumped(env):
    X, Q = R.latent8(0, 4099, 64)
    X, Q = R.clump(X, Q)
    return dict(X=X, Q=Q, exact=search(env, X, Q, 16, "exact"))


@pytest.fixture(scope="module")
def int_banks():
    return {N: R.integers(100 + N, N, 33) for N in (1, 63, 64, 65, 127, 129, 257, 1000)}


# ---------------------------------------------------------------------------------------------------------------------- exact integers
@pytest.mark.parametrize("N", [1, 63, 64, 65, 127, 129, 257, 1000])
def test_integers_equal_numpy(env, int_banks, N):
    X, Q33 = int_banks[N]
    d_all = R.d2_int(Q33, X)
    for B in (1, 2, 33):
        Q, d = Q33[:B], d_all[:B]
        for k in (1, 10, 64):
            ref_idx, ref_d2 = R.topk(d.astype(np.float64), k)
            for mode in ("auto", "exact"):
                idx, d2, cert = search(env, X, Q, k, mode)
                R.compare_exact(idx, d2.astype(np.float64), ref_idx, ref_d2, what=f"N {N} B {B} k {k} mode {mode}")
                if N <= R.KP or mode == "exact":
                    assert cert.all(), f"N {N} B {B} k {k} mode {mode}: certified {cert}"


def test_integers_prepare_is_exact(env, int_banks):
    X, _ = int_banks[257]
    bank = prepared(env, X)
    assert torch.equal(bank.x16.float().cpu(), torch.from_numpy(X))
    assert np.array_equal(bank.hn.cpu().numpy(), 0.5 * (X.astype(np.int64) ** 2).sum(1))
    assert bank.bad_values == 0 and bank.max_abs == 4.0
    assert bank.xmax == pytest.approx(float(np.sqrt((X.astype(np.float64) ** 2).sum(1).max())), rel=1e-6)


# ---------------------------------------------------------------------------------------------------------------------- planted rows
def test_planted_row_comes_first(env):
    X0, Q = R.latent8(3, 4099, 4)
    N = X0.shape[0]
    rng = np.random.default_rng(9)
    for spans in (0, 3):
        env["ops"].tune_knn_spans(spans)
        plan = env["ops"].knn_plan(N, 4, 5)
        env["ops"].tune_knn_spans(0)
        rows = {0, 1, 63, 64, N - 1}
        for edge in (plan["rows_per_tile"], plan["exact_rows_per_tile"], 32):
            rows |= {edge - 1, edge, edge + 1, 2 * edge - 1, 2 * edge}
        for s in range(1, plan["spans"]):
            e = s * plan["tiles_per_span"] * plan["rows_per_tile"]
            rows |= {e - 1, e, e + 1}
        rows = sorted(r for r in rows if 0 <= r < N)
        # one search per group of four planted rows: query j's twin goes to rows[i + j]
        for i in range(0, len(rows), 4):
            grp = rows[i:i + 4]
            X = X0.copy()
            for j, r in enumerate(grp):
                X[r] = (Q[j].astype(np.float64) * (1 + 2.0 ** -20 * rng.standard_normal(R.D))).astype(np.float32)
            for mode in ("auto", "exact"):
                idx, d2, _ = search(env, X, Q, 5, mode, spans=spans)
                for j, r in enumerate(grp):
                    assert idx[j, 0] == r, f"spans {spans} mode {mode}: query {j} planted at row {r}, first neighbour {idx[j, 0]} (d2 {d2[j, 0]})"
            env["banks"].pop(id(X), None)


# ---------------------------------------------------------------------------------------------------------------------- truth
@pytest.mark.parametrize("N,B,k", [(4099, 64, 16), (1000, 33, 10)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_against_float64(env, N, B, k, seed):
    X, Q = R.latent8(seed, N, B)
    idx, d2, cert = search(env, X, Q, k, "auto")
    ambiguous, total = R.compare_truth(idx, d2.astype(np.float64), Q, X, k)
    print(f"N {N} B {B} k {k} seed {seed}: {ambiguous} of {total} positions ambiguous, {int(cert.sum())} of {B} certified")
    assert ambiguous <= 0.02 * total
    env["banks"].pop(id(X), None)


# ---------------------------------------------------------------------------------------------------------------------- A == B
def test_auto_equals_exact_on_every_bank(env, latent, clumped, int_banks):
    same_bits(search(env, latent["X"], latent["Q"], 16, "auto"), latent["exact"], "latent")
    same_bits(search(env, clumped["X"], clumped["Q"], 16, "auto"), clumped["exact"], "clump")
    X, Q = R.twins()
    same_bits(search(env, X, Q, 1, "auto"), search(env, X, Q, 1, "exact"), "twins")
    for N, (X, Q) in int_banks.items():
        same_bits(search(env, X, Q, 10, "auto"), search(env, X, Q, 10, "exact"), f"integers N {N}")


def test_a_query_alone_equals_the_query_in_a_batch(env, latent):
    X, Q = latent["X"], latent["Q"]
    alone = search(env, X, Q[5:6], 16, "auto")
    same_bits(alone, (latent["exact"][0][5:6], latent["exact"][1][5:6]), "alone against the batch")
    batch = np.repeat(Q[5:6], 64, axis=0)
    for mode in ("auto", "exact"):
        got = search(env, X, batch, 16, mode)
        same_bits(got, (np.repeat(alone[0], 64, axis=0), np.repeat(alone[1], 64, axis=0)), f"every position of a batch, mode {mode}")


def test_more_than_one_query_tile(env, latent):
    X = latent["X"]
    Q = np.concatenate([latent["Q"], latent["Q"], latent["Q"][:1]])
    assert Q.shape[0] == 129
    want = (np.concatenate([latent["exact"][0]] * 2 + [latent["exact"][0][:1]]), np.concatenate([latent["exact"][1]] * 2 + [latent["exact"][1][:1]]))
    for mode in ("auto", "exact"):
        same_bits(search(env, X, Q, 16, mode), want, f"B 129 mode {mode}")


@pytest.mark.parametrize("spans", [1, 3, 0])
def test_spans_do_not_change_a_bit(env, latent, clumped, spans):
    for mode in ("auto", "exact", "filter"):
        ref = latent["exact"] if mode != "filter" else search(env, latent["X"], latent["Q"], 16, "filter")
        same_bits(search(env, latent["X"], latent["Q"], 16, mode, spans=spans), ref, f"latent spans {spans} mode {mode}")
    same_bits(search(env, clumped["X"], clumped["Q"], 16, "auto", spans=spans), clumped["exact"], f"clump spans {spans}")
    X, Q = R.integers(7, 257, 5)
    d = R.d2_int(Q, X).astype(np.float64)
    for mode in ("auto", "exact"):
        idx, d2, _ = search(env, X, Q, 64, mode, spans=spans)
        R.compare_exact(idx, d2.astype(np.float64), *R.topk(d, 64), what=f"integers spans {spans} mode {mode}")


# ---------------------------------------------------------------------------------------------------------------------- soundness
def test_what_the_filter_certifies_is_exact(env, latent, clumped, int_banks):
    banks = [("latent", latent["X"], latent["Q"], 16, latent["exact"]), ("clump", clumped["X"], clumped["Q"], 16, clumped["exact"])]
    X, Q = R.twins()
    banks.append(("twins", X, Q, 1, search(env, X, Q, 1, "exact")))
    for N, (X, Q) in int_banks.items():
        banks.append((f"integers N {N}", X, Q, 10, search(env, X, Q, 10, "exact")))
    for name, X, Q, k, exact in banks:
        idx, d2, cert = search(env, X, Q, k, "filter")
        if cert.any():
            same_bits((idx[cert], d2[cert]), (exact[0][cert], exact[1][cert]), f"{name}: certified by mode 2")


# ---------------------------------------------------------------------------------------------------------------------- the certificate's yield
def test_certificate_on_the_latent_bank(env, latent):
    _, _, cert = search(env, latent["X"], latent["Q"], 16, "auto")
    print(f"latent8: {int(cert.sum())} of 64 certified")
    assert cert.sum() >= 60


def test_certificate_on_the_clump(env, clumped):
    X, Q, exact = clumped["X"], clumped["Q"], clumped["exact"]
    idx, d2, cert = search(env, X, Q, 16, "auto")
    print(f"clump: queries 0..7 certified {cert[:8].tolist()}, {int(cert[8:].sum())} of the other 56")
    assert not cert[:8].any()
    same_bits((idx, d2), exact, "clump, mode 0")
    fidx, _, fcert = search(env, X, Q, 16, "filter")
    assert not fcert[:8].any()
    for b in range(8):
        assert not set(exact[0][b].tolist()) <= set(fidx[b].tolist()), f"query {b}: the 16-bit pass alone found every true neighbour"
    assert cert[8:].sum() >= 50


def test_certificate_on_the_twins(env):
    X, Q = R.twins()
    idx, d2, cert = search(env, X, Q, 1, "auto")
    assert not cert[0] and idx[0, 0] == 100 and d2[0, 0] == 0.0


# ---------------------------------------------------------------------------------------------------------------------- exclude
def test_exclude(env, latent):
    X = latent["X"]
    Q = X[:64].copy()
    for mode in ("auto", "exact"):
        idx, d2, _ = search(env, X, Q, 16, mode)
        assert np.array_equal(idx[:, 0], np.arange(64)) and np.all(d2[:, 0] == 0) and not np.signbit(d2[:, 0]).any()
        idx17, d17, _ = search(env, X, Q, 17, mode)
        eidx, ed2, _ = search(env, X, Q, 16, mode, exclude=np.arange(64))
        assert not (eidx == np.arange(64)[:, None]).any()
        same_bits((eidx, ed2), (idx17[:, 1:], d17[:, 1:]), f"exclude, mode {mode}")
    none = search(env, X, Q, 16, "auto", exclude=np.full(64, -1))
    same_bits(none, (idx, d2), "exclude = -1")


# ---------------------------------------------------------------------------------------------------------------------- non-finite
def test_non_finite_bank_and_query(env):
    X, Q = R.latent8(4, 1000, 9)
    X = X.copy()
    X[10, 3], X[500, 1000], X[999, 0] = np.nan, np.inf, 70000.0
    bank = prepared(env, X)
    assert bank.bad_values == 3
    Q = Q.copy()
    Q[8, 17] = np.nan
    exact = search(env, X, Q, 10, "exact")
    auto = search(env, X, Q, 10, "auto")
    same_bits(auto[:2], exact[:2], "non-finite bank")
    assert not auto[2].any()                                                # the exact tier answered
    fidx, fd2, fcert = search(env, X, Q, 10, "filter")
    assert (fidx == -1).all() and np.isinf(fd2).all() and not fcert.any()
    # against numpy: the chain's NaN / inf per row, NaN last
    d = R.d2_chain(Q, X)
    assert np.isnan(d[:8, 10]).all() and np.isinf(d[:8, 500]).all()
    big, _, _ = search(env, X, Q[:8], 64, "exact")
    assert not (big == 10).any()                                            # 999 rows rank before the NaN row
    Xs = X[:12].copy()                                                      # 12 rows: the NaN row comes last, the query NaN takes rows in order
    idx, d2, _ = search(env, Xs, Q, 12, "auto")
    assert (idx[:8, 11] == 10).all() and np.isnan(d2[:8, 11]).all() and not np.isnan(d2[:8, :11]).any()
    assert np.array_equal(idx[8], np.arange(12)) and np.isnan(d2[8]).all()
    idx, d2, _ = search(env, X, Q[8:9], 10, "auto")
    assert np.array_equal(idx[0], np.arange(10)) and np.isnan(d2[0]).all()


def test_empty_bank_and_empty_batch(env):
    X = np.zeros((0, R.D), np.float32)
    _, Q = R.latent8(0, 1, 3)
    for mode in ("auto", "exact", "filter"):
        idx, d2, cert = search(env, X, Q, 4, mode)
        assert (idx == -1).all() and np.isinf(d2).all() and cert.all()
    X, _ = R.latent8(0, 10, 1)
    idx, d2, cert = search(env, X, Q[:0], 4, "auto")
    assert idx.shape == (0, 4)
