"""tests/_refitref.py, the numpy restatement of the refiner's selection over a grid, held against the oracle's loop
(oracle.pigeon_oracle.proto_refiner_forward) on a small synthetic bank, and shown to tell seven planted mistakes apart at named
(row, g).  No GPU."""
import numpy as np
import pytest
import torch

import _refitref as R
from oracle import pigeon_oracle as O


# ------------------------------------------------------------------------------------------------ against the oracle
@pytest.fixture(scope="module")
def small():
    from pigeon_amd import synthetic
    B, n, cells = 5, 6, 9
    bank = synthetic.make_bank(cells, 3, seed=5, empty_frac=0.3)
    g = torch.Generator().manual_seed(17)
    emb = torch.randn((B, 1024), generator=g)
    cand = torch.stack([torch.randperm(cells, generator=g)[:n] for _ in range(B)])
    probs = torch.sort(torch.softmax(torch.randn((B, n), generator=g), dim=1), dim=1, descending=True).values.float()
    init = torch.stack([torch.rand(B, generator=g, dtype=torch.float64) * 340 - 170, torch.rand(B, generator=g, dtype=torch.float64) * 160 - 80], dim=1)
    # the records: candidate j alone in front (topk = 1 never vetoes anything away) gives its point and its score
    score = np.zeros((B, n), dtype=np.float32)
    lnglat = np.zeros((B, n, 2), dtype=np.float32)
    for j in range(n):
        _, llh, _, _, s = O.proto_refiner_forward(bank, emb, init, cand[:, j:j + 1].contiguous(), None, topk=1, return_debug=True)
        score[:, j], lnglat[:, j] = s[:, 0].numpy(), llh.numpy()
    assert (score == -100000.0).any() and (score > -100000.0).any()           # empty cells and real ones among the candidates
    return dict(bank=bank, emb=emb, cand=cand, probs=probs, init=init, score=score, lnglat=lnglat, B=B, n=n)


def test_restatement_equals_oracle_on_grid(small):
    topks = [1, 2, 3, 4, 5, 6]
    temps = [0.01, 0.3, 0.6, 1.6, 50.0]
    dist = R.veto_distances(small["init"].numpy(), small["lnglat"])
    max_kms = [0.0, float(np.median(dist)), 20000.0, float("inf")]
    choice, tight, _ = R.select_grid(small["score"], small["lnglat"], small["probs"].numpy(), small["init"].numpy(), topks, temps, max_kms)
    assert choice.shape == (6 * 5 * 4, small["B"])
    assert not tight.any()
    seen = set()
    for iK, k in enumerate(topks):
        for iT, T in enumerate(temps):
            for iR, km in enumerate(max_kms):
                _, _, _, want, _ = O.proto_refiner_forward(small["bank"], small["emb"], small["init"], small["cand"], small["probs"], topk=k,
                                                           temperature=T, max_refinement=km, return_debug=True)
                g = R.grid_index(len(temps), len(max_kms), iK, iT, iR)
                got = choice[g]
                assert np.array_equal(got & 63, want.numpy()), (k, T, km, got, want)
                if km == float("inf"):
                    assert not (got & 0x80).any()
                seen.update(int(v) for v in got)
    assert any(v & 0x80 for v in seen) and any(v & 63 for v in seen)         # vetoes and changed choices both occur

    # cand_prob None means [1, 0, 0, ...]
    none_choice, _, _ = R.select_grid(small["score"], small["lnglat"], None, small["init"].numpy(), [3], [0.6], [float("inf")])
    _, _, _, want, _ = O.proto_refiner_forward(small["bank"], small["emb"], small["init"], small["cand"], None, topk=3, temperature=0.6,
                                               max_refinement=float("inf"), return_debug=True)
    assert np.array_equal(none_choice[0] & 63, want.numpy())


# ------------------------------------------------------------------------------------------------ planted mistakes
NEAR, MID, FAR = (10.1, 20.1), (12.0, 21.0), (-170.0, -20.0)               # ~15 km, ~240 km, ~17 000 km from (10, 20)


def planted():
    """five rows of four candidates, each built so that one mistake changes its choice at one grid point"""
    rows = [
        # 0: a candidate beyond topk = 2 whose exp overflows: a sum over all four is inf and every product 0
        dict(score=[-1, 0, 200, -1], cp=[0.4, 0.6, 0, 0], pts=[NEAR] * 4),
        # 1: every exp underflows: 0 / 0 = NaN, the first NaN wins; a max shift would make candidate 1 win
        dict(score=[-500, -400, -600, -700], cp=[0.3, 0.5, 0.1, 0.1], pts=[NEAR] * 4),
        # 2: the refined candidate 1 sits exactly ON a threshold (filled in below): `>` does not veto, `>=` would
        dict(score=[-5, -1, -9, -9], cp=[0.5, 0.45, 0.05, 0], pts=[NEAR, MID, NEAR, NEAR]),
        # 3: the refined candidate 2 is far away: vetoed at 100 km, and the fallback is argmax(cp) = 1, not 0
        dict(score=[-9, -9, -1, -9], cp=[0.2, 0.7, 0.1, 0], pts=[NEAR, NEAR, FAR, NEAR]),
        # 4: probabilities whose prefix sum overflows: renormalising them gives 0 everywhere
        dict(score=[-2, -1, -3, -3], cp=[3e38, 3e38, 0, 0], pts=[NEAR] * 4),
    ]
    score = np.array([r["score"] for r in rows], dtype=np.float32)
    cp = np.array([r["cp"] for r in rows], dtype=np.float32)
    lnglat = np.array([r["pts"] for r in rows], dtype=np.float32)
    init = np.tile(np.array([[10.0, 20.0]]), (len(rows), 1))
    d_exact = float(R.veto_distances(init, lnglat)[2, 1])
    assert 100.0 < d_exact < 1000.0
    return score, lnglat, cp, init, ([1, 2, 3], [0.5, 2.0], [100.0, d_exact, float("inf")])


def g_of(grid, topk, T, km):
    return R.grid_index(len(grid[1]), len(grid[2]), grid[0].index(topk), grid[1].index(T), grid[2].index(km))


def test_planted_inputs_are_what_they_claim():
    score, lnglat, cp, init, grid = planted()
    choice, tight, dist = R.select_grid(score, lnglat, cp, init, *grid)
    inf, d_exact = float("inf"), grid[2][1]
    assert choice[g_of(grid, 2, 0.5, inf), 0] == 1
    assert choice[g_of(grid, 2, 0.5, inf), 1] == 0
    assert choice[g_of(grid, 2, 0.5, d_exact), 2] == 1 and tight[g_of(grid, 2, 0.5, d_exact), 2]     # exactly on the threshold
    assert choice[g_of(grid, 2, 0.5, 100.0), 2] == 0x80 | 0
    assert choice[g_of(grid, 3, 0.5, 100.0), 3] == 0x80 | 1
    assert choice[g_of(grid, 3, 0.5, inf), 3] == 2
    assert choice[g_of(grid, 2, 0.5, inf), 4] == 1
    assert dist[3, 2] > 10000.0
    only = np.zeros_like(tight)
    only[[g_of(grid, k, T, d_exact) for k in (2, 3) for T in grid[1]], 2] = True
    assert np.array_equal(tight, only)


@pytest.mark.parametrize("mistake,row,point", [
    ("sum_all", 0, (2, 0.5, "inf")),
    ("max_shift", 1, (2, 0.5, "inf")),
    ("veto_ge", 2, (2, 0.5, "exact")),
    ("fallback_zero", 3, (3, 0.5, 100.0)),
    ("renorm", 4, (2, 0.5, "inf")),
    ("swap_tr", 3, (3, 0.5, "inf")),
    ("veto_bit_lost", 3, (3, 0.5, 100.0)),
])
def test_planted_mistake_is_rejected(mistake, row, point):
    score, lnglat, cp, init, grid = planted()
    km = {"inf": float("inf"), "exact": grid[2][1]}.get(point[2], point[2])
    g = g_of(grid, point[0], point[1], km)
    good, _, _ = R.select_grid(score, lnglat, cp, init, *grid)
    bad, _, _ = R.select_grid(score, lnglat, cp, init, *grid, mistake=mistake)
    assert good[g, row] != bad[g, row], f"{mistake}: not caught at (row {row}, g {g})"
    first = R.first_difference(good, bad)
    assert first is not None and good[first[1], first[0]] != bad[first[1], first[0]]


# ------------------------------------------------------------------------------------------------ the GPU test's skip cap
def test_tight_share_of_gaussian_batch_is_below_one_percent():
    scratch, cp, init = R.gaussian_batch()
    score, lnglat = R.records(scratch)
    choice, tight, _ = R.select_grid(score, lnglat, cp, init, *R.GAUSSIAN_GRID)
    assert tight.mean() < 0.01, tight.mean()
    assert ((choice & 0x80) != 0).mean() > 0.05 and ((choice & 63) != 0).mean() > 0.05     # the batch exercises both outcomes


def test_totals_restatement():
    rng = np.random.default_rng(3)
    values = rng.integers(0, 9, (7, 3, 2)).astype(np.float64)
    choice = np.array([[0, 1, 2, 0x80, 0x81, 2, 0], [0, 0, 0, 0, 0, 0, 5]], dtype=np.uint8)
    t = R.totals(choice, values, 3)
    assert t[0, 2] == 4 and t[0, 3] == 2
    assert t[0, 0] == sum(values[b, c & 63, 0] for b, c in enumerate(choice[0]))
    assert np.isnan(t[1]).all()
