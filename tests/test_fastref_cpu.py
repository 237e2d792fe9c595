"""tests/_fastref.py is what it claims (CPU, no GPU, no product code): with every rounding switched off both chains ARE the oracle's
network in fp64; with the roundings on they are two different 16-bit chains whose fp16 error lies below the bf16 one on every row; and
compare_hidden, under bounds computed exactly as tests/test_gpu_fast_tier.py computes them, reports each mistake planted into the
restatement's own output -- and nothing on the unmodified output.

One 1-layer tower, 2 images; every forward is computed once (module fixture) and left unchanged."""
import pytest
import torch

import _fastref as R

F16, BF16 = torch.float16, torch.bfloat16
TILE = 2                                                        # the 256-row tile (rows 512 .. 767 of the 1154) whose statistics are shifted


@pytest.fixture(scope="module")
def runs():
    from pigeon_amd import synthetic
    from oracle import pigeon_oracle as orc
    sd = synthetic.make_vit_weights(seed=17, layers=1, affine_jitter=True)
    px = synthetic.make_pixels(2, seed=4321)
    ref = orc.vit_last_hidden_state(sd, px, dtype=torch.float64)
    detail = {}
    out = dict(sd=sd, px=px, ref=ref, detail=detail)
    out["fold_off"] = R.fast_hidden(sd, px, True, None)
    out["sep_off"] = R.fast_hidden(sd, px, False, None)
    out["fold_f16"] = R.fast_hidden(sd, px, True, F16, detail=detail)
    out["sep_f16"] = R.fast_hidden(sd, px, False, F16)
    out["fold_bf16"] = R.fast_hidden(sd, px, True, BF16)

    def shift(layer, name, rstd, mrs):
        """The statistics of row r + 1 applied to row r, for the rows of one 256-row tile of fc1 (flat row = image 577 + token)."""
        if name != "fc1":
            return rstd, mrs
        lo, hi = TILE * 256, (TILE + 1) * 256
        a, b = rstd.reshape(-1).clone(), mrs.reshape(-1).clone()
        a[lo:hi], b[lo:hi] = rstd.reshape(-1)[lo + 1:hi + 1], mrs.reshape(-1)[lo + 1:hi + 1]
        return a.reshape(rstd.shape), b.reshape(mrs.shape)

    out["fold_f16_shifted"] = R.fast_hidden(sd, px, True, F16, rowstat_hook=shift)
    out["bounds"] = R.bounds(*out["fold_f16"], ref)              # the fp16 bounds of the GPU test, computed the same way on these inputs
    return out


def test_without_rounding_both_chains_are_the_oracle(runs):
    """Rounding off: each chain equals oracle.vit_last_hidden_state(dtype=float64) to 1e-12 relative on EVERY row -- the restatement is
    the same network, and the LayerNorm fold (gamma into the weights, rstd acc - mean rstd colsum + (W beta + b)) is the same algebra."""
    for key in ("fold_off", "sep_off"):
        h, e = runs[key]
        assert h.dtype == torch.float64 and tuple(h.shape) == (2, R.TOKENS, R.HIDDEN)
        er = R.row_errors(h, runs["ref"])
        assert float(er.max()) < 1e-12, (key, float(er.max()))
        assert float(R.emb_errors(e, runs["ref"].mean(1)).max()) < 1e-12


def test_with_rounding_the_chains_differ_and_fp16_lies_below_bf16(runs):
    ref = runs["ref"]
    ef, es, eb = [R.row_errors(runs[k][0], ref) for k in ("fold_f16", "sep_f16", "fold_bf16")]
    assert float(ef.min()) > 1e-5 and float(es.min()) > 1e-5, "a 16-bit chain that equals fp64: the roundings are not applied"
    d = R.row_errors(runs["fold_f16"][0], runs["sep_f16"][0])
    assert float(d.min()) > 1e-6, "the folded and the separate chain round at different points: every row must differ"
    assert bool((ef < eb).all()), f"fp16 must lie below bf16 on every row: worst fp16 {float(ef.max()):.3e}, best bf16 {float(eb.min()):.3e}"
    b = runs["bounds"]
    assert float(eb.min()) > b["row_tol"], "the smallest bf16 row error must lie above the fp16 row bound (2 x the largest fp16 one)"
    assert b["row_max"] / b["row_min"] < 2.5, "the rows' errors are no longer tightly distributed: a max-based bound goes blind"
    # the embedding is rounded to fp32 and is the token mean
    h, e = runs["fold_f16"]
    assert torch.equal(e, h.mean(1).float().double())


def _planted(runs):
    h = runs["fold_f16"][0]
    cases = {}
    g = h.clone(); g[0], g[1] = h[1], h[0]
    cases["two images swapped"] = (g, {0, 1}, None)
    g = h.clone(); g[0, 300] = h[1, 300]
    cases["one hidden row replaced by the next image's row at the same token"] = (g, {0}, [(0, 300)])
    g = h.clone(); g[1, 576] = h[1, 575]
    cases["token 576 of one image replaced by token 575"] = (g, {1}, [(1, 576)])
    g = h.clone(); g[1] = runs["detail"]["before_last_fc2"][1]
    cases["one image's last fc2 contribution dropped"] = (g, {1}, None)
    cases["the row statistics of row r + 1 applied to row r in one 256-row tile"] = (runs["fold_f16_shifted"][0], None, "tile")
    g = h.clone(); g[1] = runs["fold_bf16"][0][1]
    cases["one image computed with bf16 operands"] = (g, {1}, None)
    return cases


def test_planted_mistakes_are_reported(runs):
    """Each mistake, applied to a copy of the fp16 restatement's own output, is reported under the fp16 bounds -- in the right image, at
    the right row where the mistake is one row, inside the right 256-row tile where it is the statistics of a tile."""
    b, ref = runs["bounds"], runs["ref"]
    for name, (got, images, rows) in _planted(runs).items():
        found = R.compare_hidden(got, ref, b["row_tol"], b["emb_tol"], label=name, limit=10 ** 6)
        assert found, f"not reported: {name}"
        bad = (~(R.row_errors(got, ref) <= b["row_tol"])).nonzero().tolist()
        if rows == "tile":
            flat = [i * R.TOKENS + t for i, t in bad]
            assert flat and all(TILE * 256 <= r < (TILE + 1) * 256 for r in flat), (name, flat[:5])
            assert len(flat) > 128, f"{name}: only {len(flat)} of the tile's 256 rows reported"
            assert all(f"256-row tile {TILE} " in m for m in found if "hidden-row" in m)
            continue
        if rows is not None:
            assert [tuple(x) for x in bad] == rows, (name, bad[:5])
            i, t = rows[0]
            assert any(f"image {i} token {t} (row {i * R.TOKENS + t}, 256-row tile {(i * R.TOKENS + t) // 256} " in m for m in found), found
        else:
            assert {i for i, _ in bad} == images, (name, sorted({i for i, _ in bad}))
            for i in images:                                    # a whole wrong image: every row, and the embedding
                assert sum(1 for j, _ in bad if j == i) == R.TOKENS, name
                assert any(f"image {i} embedding error" in m for m in found), (name, found[-3:])


def test_the_unmodified_restatement_passes(runs):
    b = runs["bounds"]
    for key in ("fold_f16", "sep_f16"):                         # (the separate chain under the folded chain's bounds: the same roundings, moved)
        h, e = runs[key]
        worst = {}
        assert R.compare_hidden(h, runs["ref"], b["row_tol"], b["emb_tol"], emb=e, worst=worst) == []
        assert 0.0 < worst["row"] <= b["row_tol"] and 0.0 < worst["emb"] <= b["emb_tol"]
    assert b["emb_tol"] <= R.EMB_TOL


def test_comparator_fails_on_nan_and_reports_the_extent(runs):
    h = runs["fold_f16"][0].clone()
    h[1, 5, 7] = float("nan")
    b = runs["bounds"]
    found = R.compare_hidden(h, runs["ref"], b["row_tol"], b["emb_tol"])
    assert any("image 1 token 5 (row 582, 256-row tile 2 +70)" in m for m in found) and any("image 1 embedding" in m for m in found)
    g = runs["fold_f16"][0].clone(); g[0], g[1] = runs["fold_f16"][0][1], runs["fold_f16"][0][0]
    found = R.compare_hidden(g, runs["ref"], b["row_tol"], b["emb_tol"], limit=4)
    assert any("1154 bad rows in all, in 2 images, rows 0 .. 1153 (256-row tiles 0 .. 4)" in m for m in found), found
