"""tests/_bootref.py held to itself, without a GPU: Philox4x32-10's known answers, the index rule against Python's big integers, the
bootstrap standard error of a mean against its closed form, and six planted mistakes that the checkers must reject by replicate and
draw."""
import math

import numpy as np
import pytest

import _bootref as B

KNOWN = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
         ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
         ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


@pytest.mark.parametrize("counter, key, want", KNOWN)
def test_philox_known_answers(counter, key, want):
    got = tuple(int(w[0]) for w in B.philox(counter, key))
    assert got == want, [hex(v) for v in got]


def philox_int(counter, key):
    """Philox4x32-10 once more, in Python integers."""
    c, k = list(counter), list(key)
    for _ in range(10):
        p0, p1 = B.M0 * c[0], B.M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xffffffff]
        k = [(k[0] + B.W0) & 0xffffffff, (k[1] + B.W1) & 0xffffffff]
    return c


def idx_int(N, seed, r, j):
    o = philox_int(((j >> 1) & 0xffffffff, (j >> 1) >> 32, r, 0), (seed & 0xffffffff, seed >> 32))
    u = (o[2] | o[3] << 32) if j & 1 else (o[0] | o[1] << 32)
    return (u * N) >> 64


@pytest.mark.parametrize("N", [1, 2, 3, 2 ** 24, 2 ** 31 - 1])
@pytest.mark.parametrize("seed", [0, 5, (0xfeedface << 32) | 0x1234567])
def test_indices_against_big_integers(N, seed):
    for r, j0 in ((0, 0), (1, 7), (0xffffffff, 2 ** 33 - 3), (12345, 2 ** 40 + 1)):
        got = B.indices(N, seed, r, j0, 9)
        want = [idx_int(N, seed, r, j0 + i) for i in range(9)]
        assert got.tolist() == want, (N, seed, r, j0)
        assert got.dtype == np.int64 and 0 <= got.min() and got.max() < N


def test_a_seed_above_2_32_uses_both_key_words():
    lo = B.indices(1000, 7, 0, 0, 64)
    hi = B.indices(1000, 7 + (1 << 32), 0, 0, 64)
    assert not np.array_equal(lo, hi)
    assert hi.tolist() == [idx_int(1000, 7 + (1 << 32), 0, j) for j in range(64)]


def test_mulhi64_edges():
    u = np.array([0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1], dtype=np.uint64)
    for n in (1, 2, 3, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63 + 12345, 2 ** 64 - 1):
        assert B.mulhi64(u, n).tolist() == [(int(v) * n) >> 64 for v in u]


def test_ordered_sum_is_the_stated_order():
    rng = np.random.default_rng(1)
    for n in (1, 2, 255, 256, 257, 1000):
        g = rng.standard_normal(n) * 10.0 ** rng.integers(-8, 8, n)
        acc = [0.0] * 256
        for j in range(n):
            acc[j % 256] = acc[j % 256] + float(g[j])
        v = list(acc)
        for o in (32, 16, 8, 4, 2, 1):
            v = [v[i] + v[i ^ o] for i in range(256)]
        want = (v[0] + v[64]) + (v[128] + v[192])
        assert float(B.ordered_sum(g)) == want
        assert abs(want - math.fsum(g)) <= n * 2.0 ** -53 * float(np.abs(g).sum())


def test_bootstrap_standard_error_of_a_mean():
    N, R = 400, 4000
    x = np.random.default_rng(2024).standard_normal(N)
    reps = B.means(x[None, :], R, seed=11)[:, 0]
    se = float(np.std(reps, ddof=1))
    want = float(np.std(x, ddof=1)) * math.sqrt((N - 1) / N) / math.sqrt(N)
    print(f"bootstrap standard error {se:.6f}, closed form {want:.6f}, relative {se / want - 1:+.4f} (margin {5 / math.sqrt(2 * R):.4f})")
    assert abs(se / want - 1) <= 5 / math.sqrt(2 * R)


def test_quantile_restatement_agrees_with_the_rank_formula():
    rng = np.random.default_rng(5)
    cols = np.stack([rng.standard_normal(37), np.repeat([2.0, -1.0, 2.0], [10, 20, 7]), np.where(np.arange(37) % 3 == 0, -0.0, 0.0),
                     np.concatenate([[5e-324, -5e-324, 0.0, -0.0, 1e-310], rng.standard_normal(32)])])
    rank, srt = B.rank_and_sorted(cols)
    qs = (0, 0.025, 1 / 3, 0.5, 0.975, 1)
    want = B.quantiles(cols, 9, 3, qs)
    for r in range(9):
        idx = B.indices(37, 3, r)
        for m in range(cols.shape[0]):
            for k, q in enumerate(qs):
                got = B.quantile_by_ranks(rank, srt, m, idx, q)[0]
                assert np.float64(got).tobytes() == want[r, m, k].tobytes(), (r, m, q, got, want[r, m, k])


# ------------------------------------------------------------------------------------------------------------ planted mistakes
def _stream(u_of):
    return lambda seed, r, j, N, m: B.mulhi64(u_of(seed, r, j, m), N)


def _u_swapped_halves(seed, r, j, m):
    o = B.words(seed, r, j)
    odd = (j & np.uint64(1)).astype(bool)
    return np.where(odd, o[3] | (o[2] << B.S32), o[1] | (o[0] << B.S32))


def _u_odd_reuses_o0_o1(seed, r, j, m):
    o = B.words(seed, r, j)
    return o[0] | (o[1] << B.S32)


def _u_r_in_the_wrong_word(seed, r, j, m):
    p = j >> np.uint64(1)
    o = B.philox((p & B.MASK32, p >> B.S32, np.uint64(0), np.uint64(r)), (seed & 0xffffffff, seed >> 32))
    odd = (j & np.uint64(1)).astype(bool)
    return np.where(odd, o[2] | (o[3] << B.S32), o[0] | (o[1] << B.S32))


def _idx_rounded(seed, r, j, N, m):
    u = B.draws(seed, r, j)
    return [((int(v) * N + (1 << 63)) >> 64) for v in u]


def _idx_fresh_stream_per_column(seed, r, j, N, m):
    return B.mulhi64(B.draws(seed + m, r, j), N)


@pytest.mark.parametrize("name, fn, columns", [
    ("swapped halves of u", _stream(_u_swapped_halves), 1),
    ("the odd draw reuses o0 | o1", _stream(_u_odd_reuses_o0_o1), 1),
    ("r in the wrong counter word", _stream(_u_r_in_the_wrong_word), 1),
    ("floor replaced by rounding", _idx_rounded, 1),
    ("a fresh index stream per column", _idx_fresh_stream_per_column, 2),
])
def test_planted_index_mistakes_are_rejected(name, fn, columns):
    B.check_index_stream(_stream(lambda seed, r, j, m: B.draws(seed, r, j)), 1000, 9, (0, 1, 64), 512, columns=2)    # the contract passes
    with pytest.raises(AssertionError, match=r"replicate \d+, draw \d+") as e:
        B.check_index_stream(fn, 1000, 9, (1, 64), 512, columns=columns)      # r = 0 would hide the wrong counter word
    print(name, "->", e.value)


def _numpy_rule(s, q, clamp_early=False):
    N = s.shape[0]
    lo, hi, t = B.orders(N, q)
    if clamp_early:
        hi = min(lo + 1, N - 2) if N > 1 else 0
    return B.lerp(s[lo], s[hi], t)


def test_planted_quantile_mistake_is_rejected():
    x = np.random.default_rng(3).standard_normal(37)                 # 0.975 * 36 = 35.1: lo + 1 is the last order statistic
    qs = (0, 0.025, 1 / 3, 0.5, 0.975, 1)
    B.check_quantile_rule(_numpy_rule, x, 4, range(6), qs)
    with pytest.raises(AssertionError, match=r"replicate \d+, draw \d+"):
        B.check_quantile_rule(lambda s, q: _numpy_rule(s, q, clamp_early=True), x, 4, range(6), qs)
