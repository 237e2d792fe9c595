"""tests/_knnref.py against itself and against exact arithmetic (no GPU): the chain on integers, eps against the 16-bit pass's
observed error (from above and, so that a bound loose enough to certify nothing is rejected too, from below), the conditions the GPU
tests put on their inputs recomputed from the truth alone, and the comparators on planted mistakes."""
import numpy as np
import pytest

import _knnref as R


@pytest.fixture(scope="module")
def small():
    X, Q = R.latent8(0, 1000, 33)
    d64 = R.d2_f64(Q, X)
    idx, d2 = R.topk(R.d2_chain(Q, X), 10)
    return dict(X=X, Q=Q, d64=d64, idx=idx, d2=d2)


# ---------------------------------------------------------------------------------------------------------------------- the chain
def test_chain_equals_integer_arithmetic():
    X, Q = R.integers(3, 257, 5)
    want = R.d2_int(Q, X)
    assert want.max() < 2 ** 24
    got = R.d2_chain(Q, X)
    assert got.dtype == np.float32 and np.array_equal(got.astype(np.int64), want)
    assert np.array_equal(R.d2_f64(Q, X).astype(np.int64), want)


def test_chain_identical_rows_are_zero():
    X, _ = R.latent8(1, 9, 1)
    d = R.d2_chain(X, X)
    assert np.all(np.diag(d) == 0) and d.dtype == np.float32


def test_chain_within_its_bound_of_float64(small):
    d = R.d2_chain(small["Q"], small["X"]).astype(np.float64)
    assert np.all(np.abs(d - small["d64"]) <= 1026 * R.U * small["d64"])


def test_order_rule():
    d = np.array([3.0, np.nan, 1.0, np.inf, 1.0, np.nan, 0.0], np.float32)
    assert R.order(d).tolist() == [6, 2, 4, 0, 3, 1, 5]
    idx, d2 = R.topk(d[None, :], 9)
    assert idx[0].tolist() == [6, 2, 4, 0, 3, 1, 5, -1, -1]
    assert np.isnan(d2[0, 5]) and np.isnan(d2[0, 6]) and d2[0, 7] == np.inf and d2[0, 4] == np.inf
    idx, _ = R.topk(d[None, :], 3, exclude=[2])
    assert idx[0].tolist() == [6, 4, 0]


# ---------------------------------------------------------------------------------------------------------------------- eps
def _norms(Q, X):
    return np.linalg.norm(Q.astype(np.float64), axis=1), np.linalg.norm(X.astype(np.float64), axis=1)


def test_eps_bounds_the_twins_and_is_attained():
    X, Q = R.twins()
    err = R.filter_error(Q, X)[0]
    qn, xn = _norms(Q, X)
    e = float(R.eps(qn[0], R.xmax_of(X)))
    assert err.max() <= e
    assert err[100] >= 0.99 * 2.0 ** -10 * qn[0] * xn[100]              # every element an fp16 tie: the conversion term in full
    assert e <= 4 * 2.0 ** -10 * qn[0] * xn.max()


@pytest.mark.parametrize("scale", [1.0, 1.0 / 32, 40.0])
def test_eps_bounds_gaussian_vectors(scale):
    rng = np.random.default_rng(5)
    X = (scale * rng.standard_normal((300, R.D))).astype(np.float32)
    Q = (scale * rng.standard_normal((7, R.D))).astype(np.float32)
    err = R.filter_error(Q, X)
    qn, xn = _norms(Q, X)
    e = R.eps(qn, R.xmax_of(X))
    assert np.all(err.max(axis=1) <= e)
    assert np.all(e <= 4 * 2.0 ** -10 * qn * xn.max())


def test_eps_covers_fp16_subnormals():
    rng = np.random.default_rng(6)
    X = (2.0 ** -17 * rng.standard_normal((64, R.D))).astype(np.float32)      # most elements fp16 subnormals
    Q = (2.0 ** -17 * rng.standard_normal((3, R.D))).astype(np.float32)
    err = R.filter_error(Q, X)
    qn, _ = _norms(Q, X)
    assert np.all(err.max(axis=1) <= R.eps(qn, R.xmax_of(X)))


# ---------------------------------------------------------------------------------------------------------------------- input conditions
@pytest.mark.parametrize("N,B,k", [(4099, 64, 16), (1000, 33, 10)])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_truth_leaves_few_ambiguous_positions(N, B, k, seed):
    """The truth test's condition, from the float64 distances alone: at most 2 % of the positions may be ambiguous."""
    X, Q = R.latent8(seed, N, B)
    d64 = R.d2_f64(Q, X)
    idx, d2 = R.topk(d64, k)
    ambiguous, total = R.compare_truth(idx, d2.astype(np.float32).astype(np.float64), Q, X, k, d64=d64)
    print(f"latent8 seed {seed} N {N} B {B} k {k}: {ambiguous} of {total} positions ambiguous")
    assert total == B * k and ambiguous <= 0.02 * total


def test_restated_certificate_on_the_latent_bank():
    X, Q = R.latent8(0, 4099, 64)
    d2 = R.d2_chain(Q, X)
    idx, out, cert = R.certify(Q, X, 16, d2=d2)
    print(f"latent8: {int(cert.sum())} of 64 certified in the restatement")
    assert cert.sum() == 64
    R.compare_exact(idx, out, *R.topk(d2, 16), what="restated fast path")


def test_restated_certificate_on_the_clump():
    X, Q = R.latent8(0, 4099, 64)
    X, Q = R.clump(X, Q)
    d2 = R.d2_chain(Q, X)
    idx, out, cert = R.certify(Q, X, 16, d2=d2)
    ref_idx, _ = R.topk(d2, 16)
    cand, _ = R.candidates(Q, X)
    print(f"clump: {int(cert[8:].sum())} of 56 others certified; queries 0..7 certified: {cert[:8].tolist()}")
    assert not cert[:8].any()
    for b in range(8):                                                          # the candidates do not hold the truth
        assert not set(ref_idx[b].tolist()) <= set(cand[b].tolist()), f"query {b}"
    assert cert[8:].sum() == 56
    assert np.array_equal(idx[cert], ref_idx[cert])                             # soundness of the restatement


def test_restated_certificate_on_the_twins():
    X, Q = R.twins()
    a = R.filter_keys(Q, X)[0]
    assert R.order(a).tolist().index(100) >= 199                                # at the very end of the 16-bit pass's order,
    assert R.order(a).tolist().index(100) >= R.KP                               # so no candidate
    d2 = R.d2_chain(Q, X)
    assert d2[0, 100] == 0 and np.delete(d2[0], 100).min() > 0
    assert np.delete(R.d2_f64(Q, X)[0], 100).min() >= 2.4e-7
    idx, out, cert = R.certify(Q, X, 1, d2=d2)
    assert not cert[0] and idx[0, 0] != 100                                    # the fast path alone is wrong, and says so


# ---------------------------------------------------------------------------------------------------------------------- comparators
def _rejects(fn, needle):
    with pytest.raises(AssertionError) as e:
        fn()
    assert needle in str(e.value), str(e.value)


def test_comparators_accept_the_truth(small):
    R.compare_exact(small["idx"], small["d2"], small["idx"].copy(), small["d2"].copy())
    amb, total = R.compare_truth(small["idx"], small["d2"], small["Q"], small["X"], 10, d64=small["d64"])
    assert total == 330 and amb <= 0.02 * total


def test_comparators_reject_a_missing_first_neighbour(small):
    idx, d2 = small["idx"].copy(), small["d2"].copy()
    idx[4, :-1], d2[4, :-1] = idx[4, 1:], d2[4, 1:]
    idx[4, -1], d2[4, -1] = R.topk(R.d2_chain(small["Q"][4:5], small["X"]), 11)[0][0, 10], R.topk(R.d2_chain(small["Q"][4:5], small["X"]), 11)[1][0, 10]
    _rejects(lambda: R.compare_truth(idx, d2, small["Q"], small["X"], 10, d64=small["d64"]), "query 4 position 0")
    _rejects(lambda: R.compare_exact(idx, d2, small["idx"], small["d2"]), "query 4 position 0")


def test_comparators_reject_a_tie_in_the_wrong_order():
    X, Q = R.integers(1, 300, 3)
    r = int(R.topk(R.d2_chain(Q, X), 1)[0][1, 0])
    X[(r + 7) % 300] = X[r]                                                     # query 1's nearest row twice: a tie at the top
    d = R.d2_chain(Q, X)
    idx, d2 = R.topk(d, 10)
    b, p = next((b, p) for b in range(3) for p in range(9) if d2[b, p] == d2[b, p + 1])
    bad = idx.copy()
    bad[b, p], bad[b, p + 1] = idx[b, p + 1], idx[b, p]
    _rejects(lambda: R.compare_exact(bad, d2, idx, d2), f"query {b} position {p}")
    _rejects(lambda: R.compare_truth(bad, d2, Q, X, 10), f"query {b} position {p + 1}")


def test_comparators_reject_a_row_off_by_one(small):
    idx = small["idx"].copy()
    idx[7, 3] += 1
    _rejects(lambda: R.compare_exact(idx, small["d2"], small["idx"], small["d2"]), "query 7 position 3")
    _rejects(lambda: R.compare_truth(idx, small["d2"], small["Q"], small["X"], 10, d64=small["d64"]), "query 7 position 3")


def test_comparators_reject_the_d2_of_another_row(small):
    d2 = small["d2"].copy()
    d2[2, 5] = np.nextafter(d2[2, 6], np.float32(0))                            # still in order, but not this row's distance
    _rejects(lambda: R.compare_exact(small["idx"], d2, small["idx"], small["d2"]), "query 2 position 5")
    _rejects(lambda: R.compare_truth(small["idx"], d2, small["Q"], small["X"], 10, d64=small["d64"]), "query 2 position 5")


def test_comparators_reject_an_excluded_row(small):
    ex = np.full(33, -1, np.int64)
    ex[9] = small["idx"][9, 0]
    _rejects(lambda: R.compare_truth(small["idx"], small["d2"], small["Q"], small["X"], 10, exclude=ex, d64=small["d64"]),
             "query 9 position 0")


def test_comparators_reject_the_neighbouring_querys_list(small):
    idx, d2 = small["idx"].copy(), small["d2"].copy()
    idx[12], d2[12] = small["idx"][13], small["d2"][13]
    _rejects(lambda: R.compare_exact(idx, d2, small["idx"], small["d2"]), "query 12 position 0")
    _rejects(lambda: R.compare_truth(idx, d2, small["Q"], small["X"], 10, d64=small["d64"]), "query 12 position 0")


def test_comparators_reject_an_unsorted_list(small):
    idx, d2 = small["idx"].copy(), small["d2"].copy()
    idx[20, [2, 8]], d2[20, [2, 8]] = idx[20, [8, 2]], d2[20, [8, 2]]
    _rejects(lambda: R.compare_exact(idx, d2, small["idx"], small["d2"]), "query 20 position 2")
    _rejects(lambda: R.compare_truth(idx, d2, small["Q"], small["X"], 10, d64=small["d64"]), "query 20")


def test_banks_are_what_the_issue_describes():
    X, Q = R.latent8(0, 4099, 64)
    assert X.shape == (4099, R.D) and Q.shape == (64, R.D) and X.dtype == Q.dtype == np.float32
    X2, Q2 = R.clump(X, Q)
    assert X2.shape == (4399, R.D) and np.array_equal(X2[:2000], X[:2000]) and np.array_equal(X2[2300:], X[2000:])
    assert np.array_equal(Q2[8:], Q[8:]) and not np.array_equal(Q2[:8], Q[:8])
    Xt, Qt = R.twins()
    assert Xt.shape == (201, R.D) and np.array_equal(Xt[100], Qt[0])
    assert np.array_equal(Xt[np.arange(201) != 100].astype(np.float16).astype(np.float32), Xt[np.arange(201) != 100])
