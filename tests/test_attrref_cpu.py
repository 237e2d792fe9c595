"""tests/_attrref.py checked against itself (no GPU): the identity the attribution rests on holds in float64, and the comparators
the GPU tests use reject each planted mistake and name the place.

  1 identity   maps.sum over (view, token) + offset == the logit difference computed the model's way, to 1e-12 relative, for
               P = 1 and P = 4, with and without a bias vector, with and without `against`
  2 mistakes   divisor 576 / a missing P; the class token dropped; the sign of `against`; view and token axes swapped; k taken from
               the neighbouring panorama; the de-bias term left out of the offset; a column permutation inside a row
  3 indices    which columns are NaN for indices outside [0, C)
"""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _attrref as R  # noqa: E402

C, K = 9, 3
PLACE = re.compile(r"row (\d+), view (\d+), token (\d+), k (\d+)")


def _data(P, seed=0, B=3):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((B * P, R.TOKENS, R.HIDDEN)).astype(np.float32)
    W = ((rng.random((C, R.HIDDEN)) * 2 - 1) / 32).astype(np.float32)
    b = ((rng.random(C) * 2 - 1) / 32).astype(np.float32)
    cells = np.stack([rng.permutation(C)[:K] for _ in range(B)]).astype(np.int64)
    against = np.array([[c for c in range(C) if c not in cells[i]][i] for i in range(B)], dtype=np.int64)     # never a listed cell
    against[1] = -1
    beta = (rng.standard_normal(R.HIDDEN) * 1e-4).astype(np.float32)
    return h, W, b, cells, against, beta


@pytest.fixture(scope="module")
def data4():
    d = _data(4, seed=1)
    h, W, b, cells, against, beta = d
    return d, R.maps(h, W, cells, against, 4)


# ------------------------------------------------------------------------------------------------ 1
@pytest.mark.parametrize("P", [1, 4])
@pytest.mark.parametrize("with_beta", [False, True])
@pytest.mark.parametrize("with_against", [False, True])
def test_identity_in_float64(P, with_beta, with_against):
    h, W, b, cells, against, beta = _data(P, seed=10 + P)
    a = against if with_against else None
    bt = beta if with_beta else None
    m = R.maps(h, W, cells, a, P)
    e = R.embeddings(h)
    norms = np.linalg.norm(e, axis=1).reshape(-1, P)
    total = m.sum(axis=(1, 2)) + R.offset(W, b, cells, a, norms if with_beta else None, bt)
    want = R.logit_difference(h, W, b, cells, a, P, bt)
    scale = np.abs(R.dots(h, W, cells, a, P, absolute=True)).sum(axis=(1, 2)) / (R.TOKENS * P) + np.abs(want)
    err = np.abs(total - want) / np.where(scale > 0, scale, 1.0)      # (scale 0: a cell listed against itself, everything exactly 0)
    print(f"\nP={P} beta={with_beta} against={with_against}: largest relative difference {err.max():.2e}")
    assert (err <= 1e-12).all() and (np.abs(total - want) <= 1e-12 * scale).all()
    R.compare_offset(total, want, 1e-12 * scale)
    # the fp32 rounding of g is part of the definition: with the unrounded direction the identity misses 1e-12
    if with_against:
        g64 = W[cells].astype(np.float64) - np.where((a == -1)[:, None, None], 0.0, W[np.clip(a, 0, C - 1)][:, None, :].astype(np.float64))
        assert np.abs(g64 - R.directions(W, cells, a)).max() > 0


# ------------------------------------------------------------------------------------------------ 2
def _rejected(got, want, tol):
    with pytest.raises(AssertionError) as e:
        R.compare_maps(got, want, tol)
    m = PLACE.search(str(e.value))
    assert m, str(e.value)
    return tuple(int(v) for v in m.groups())


def test_comparator_accepts_the_truth_and_its_rounding(data4):
    (h, W, b, cells, against, beta), want = data4
    R.compare_maps(want, want)
    bd = R.bound(h, W, cells, against, 4)
    R.compare_maps(want.astype(np.float32), want, bd)                 # one fp32 rounding of the truth is inside the bound
    assert (bd > 0).all() and bd.shape == want.shape


def test_wrong_divisors_are_rejected(data4):
    (h, W, b, cells, against, beta), want = data4
    bd = R.bound(h, W, cells, against, 4)
    # 1/576 of the value is above the bound wherever the dot product does not cancel to a few per cent of sum |h g|: the first
    # such element is named, in row 0, view 0
    assert _rejected(want * 577.0 / 576.0, want, bd)[:2] == (0, 0)
    assert _rejected(want * 4.0, want, bd)[:3] == (0, 0, 0)           # the views not divided out: 577 instead of 577 P
    missing_p = R.dots(h, W, cells, against, 4) / float(R.TOKENS)
    assert _rejected(missing_p, want, bd)[:3] == (0, 0, 0)


def test_dropped_class_token_is_rejected_at_token_0(data4):
    (h, W, b, cells, against, beta), want = data4
    bd = R.bound(h, W, cells, against, 4)
    got = want.copy()
    got[:, :, 0, :] = 0.0
    assert _rejected(got, want, bd)[1:3] == (0, 0)
    shifted = np.concatenate([want[:, :, 1:, :], want[:, :, :1, :]], axis=2)      # the 576 patches first, the class token last
    assert _rejected(shifted, want, bd)[2] == 0


def test_sign_of_against_is_rejected(data4):
    (h, W, b, cells, against, beta), want = data4
    bd = R.bound(h, W, cells, against, 4)
    plus = R.maps(h, W, cells, None, 4) + (R.maps(h, W, cells, None, 4) - want)   # h . (W[c] + W[a])
    row, view, token, k = _rejected(plus, want, bd)
    assert (row, view, token) == (0, 0, 0)
    R.compare_maps(plus[1:2], want[1:2], bd[1:2])                     # row 1 has no `against`: nothing to get wrong there


def test_swapped_view_and_token_axes_are_rejected(data4):
    (h, W, b, cells, against, beta), want = data4
    bd = R.bound(h, W, cells, against, 4)
    B = want.shape[0]
    got = want.reshape(B, 4 * R.TOKENS, K).reshape(B, R.TOKENS, 4, K).transpose(0, 2, 1, 3)       # rows read as (token, view)
    row, view, token, k = _rejected(got, want, bd)
    assert (row, view, token) == (0, 0, 1)                            # (view 0, token 0) is the same element in both orders


def test_k_from_the_neighbouring_panorama_is_rejected(data4):
    (h, W, b, cells, against, beta), want = data4
    bd = R.bound(h, W, cells, against, 4)
    got = R.maps(h, W, np.roll(cells, 1, axis=0), against, 4)
    assert _rejected(got, want, bd)[:3] == (0, 0, 0)


def test_column_permutation_inside_a_row_is_rejected(data4):
    (h, W, b, cells, against, beta), want = data4
    bd = R.bound(h, W, cells, against, 4)
    perm = np.arange(R.HIDDEN).reshape(4, 64, 4).transpose(1, 0, 2).reshape(-1)  # a lane's 16 columns taken as consecutive
    assert _rejected(R.maps(h[:, :, perm], W, cells, against, 4), want, bd)[:3] == (0, 0, 0)
    got = want.copy()
    got[2, 3, 576, :] = got[2, 3, 576, ::-1]                          # the K outputs of ONE row in another order: the last token
    assert _rejected(got, want, bd)[:3] == (2, 3, 576)


def test_missing_debias_term_is_rejected_in_the_offset(data4):
    (h, W, b, cells, against, beta), want = data4
    norms = np.linalg.norm(R.embeddings(h), axis=1).reshape(-1, 4)
    full = R.offset(W, b, cells, against, norms, beta)
    bare = R.offset(W, b, cells, against)
    tol = 8 * R.U * (np.abs(full) + np.abs(bare))
    R.compare_offset(full.astype(np.float32), full, tol)
    with pytest.raises(AssertionError, match=r"row 0, k 0"):
        R.compare_offset(bare, full, tol)
    with pytest.raises(AssertionError, match=r"shape"):
        R.compare_offset(full[:, :2], full, tol)


# ------------------------------------------------------------------------------------------------ 3
def test_refused_indices_give_nan_columns_only():
    h, W, b, cells, against, beta = _data(1, seed=5)
    cells = cells.copy()
    cells[0, 1], cells[2, 0] = -2, C
    a = against.copy()
    ok = R.valid(cells, a, C)
    assert ok.tolist() == [[True, False, True], [True, True, True], [False, True, True]]
    m = R.maps(h, W, cells, a, 1)
    assert np.isnan(m[0, :, :, 1]).all() and np.isnan(m[2, :, :, 0]).all() and np.isnan(m).sum() == 2 * R.TOKENS
    a[1] = 2 ** 40
    m2 = R.maps(h, W, cells, a, 1)
    assert np.isnan(m2[1]).all() and np.array_equal(np.isnan(m2[[0, 2]]), np.isnan(m[[0, 2]]))
    assert np.isnan(R.offset(W, b, cells, a)[1]).all()
    with pytest.raises(AssertionError, match=r"row 1, view 0, token 0, k 0"):
        R.compare_maps(m, m2)                                         # a NaN on one side only is a difference
