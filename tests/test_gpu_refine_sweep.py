"""pg_refine_sweep and pg_refine_sweep_totals on the GPU (run with -m gpu on an MI355X), through the C ABI.

The selection of every grid point is held against pg_refine_forward / pg_refine_forward_ex with that point's settings at zero tolerance
(the bits must be theirs), against tests/_refitref.py on records the test plants itself, and -- on a Gaussian batch -- against the
restatement with the decisions it calls tight skipped (their share is capped at 1 %, tests/test_refitref_cpu.py shows the cap holds by
the restatement alone).  Totals are held against an fp64 host gather-sum.  Every output sits between guard regions.

The veto bit.  Bit 7 says the veto FIRED, which pg_refine_forward's outputs show only when the fallback differs from the refined
candidate.  So it is checked three ways: it equals (veto_km[b, refined] > max_km) with the sweep's own veto_km and pg_refine_forward_ex's
`refined`; wherever pg_refine_forward_ex's refined != choice the bit is set; wherever the bit is clear the choice is the refined one."""
import ctypes as C

import numpy as np
import pytest
import torch

import _refitref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 256
INF = float("inf")
K_CAND = 12


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops, synthetic
    _lib.require_gpu()
    bank = synthetic.make_bank(33, 3, seed=7, empty_frac=0.15)
    assert (np.diff(bank.cell_off) == 0).sum() >= 2                        # a few empty cells
    return dict(lib=_lib, ops=hip_ops, L=_lib.load(), bank=hip_ops.DeviceBank(bank, device=DEV), cells=33)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def guards_intact(buf, n, fill):
    return bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all())


def sweep(env, scratch, cand_prob, init, topks, temps, max_kms, want_veto=True):
    """device tensors in -> (choice (G,B) uint8, veto_km (B,n) f64 or None) through the C ABI, guards and inputs checked"""
    ops = env["ops"]
    B, n, SC = scratch.shape
    G = len(topks) * len(temps) * len(max_kms)
    keep = [t.clone() for t in (scratch, init)] + ([cand_prob.clone()] if cand_prob is not None else [])
    cbuf, cview = guarded(G * B, torch.uint8, 0x55)
    vbuf, vview = guarded(B * n, torch.float64, -7.25)
    ka, ta, ra = (C.c_int32 * len(topks))(*topks), (C.c_float * len(temps))(*temps), (C.c_double * len(max_kms))(*max_kms)
    k = 0 if cand_prob is None else cand_prob.shape[1]
    env["lib"].check(env["L"].pg_refine_sweep(ops._p(scratch), SC, B, n, ops._p(cand_prob), k, ops._p(init), ka, len(topks), ta, len(temps),
                                              ra, len(max_kms), ops._p(cview), ops._p(vview if want_veto else None), ops._stream()),
                     "pg_refine_sweep")
    torch.cuda.synchronize()
    assert guards_intact(cbuf, G * B, 0x55), "pg_refine_sweep wrote outside choice"
    assert guards_intact(vbuf, B * n, -7.25), "pg_refine_sweep wrote outside veto_km"
    if not want_veto:
        assert bool((vview == -7.25).all())
    for a, b in zip(keep, (scratch, init, cand_prob)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8)), "pg_refine_sweep changed an input"
    return cview.reshape(G, B).clone(), (vview.reshape(B, n).clone() if want_veto else None)


def totals(env, choice, values):
    ops = env["ops"]
    G, B = choice.shape
    n, V = values.shape[1], values.shape[2]
    tbuf, tview = guarded(G * (V + 2), torch.float64, -7.25)
    env["lib"].check(env["L"].pg_refine_sweep_totals(ops._p(choice), G, B, n, ops._p(values), V, ops._p(tview), ops._stream()),
                     "pg_refine_sweep_totals")
    torch.cuda.synchronize()
    assert guards_intact(tbuf, G * (V + 2), -7.25), "pg_refine_sweep_totals wrote outside totals"
    return tview.reshape(G, V + 2).clone()


def batch(env, B, seed=0):
    g = torch.Generator().manual_seed(1000 + 7 * B + seed)
    q = torch.randn((B, 1024), generator=g)
    init = torch.stack([torch.rand(B, generator=g, dtype=torch.float64) * 340 - 170, torch.rand(B, generator=g, dtype=torch.float64) * 160 - 80], dim=1)
    cand = torch.stack([torch.randperm(env["cells"], generator=g)[:K_CAND] for _ in range(B)])
    probs = torch.sort(torch.softmax(2 * torch.randn((B, K_CAND), generator=g), dim=1), dim=1, descending=True).values.float()
    return q.to(DEV), init.to(DEV), cand.to(DEV), probs.contiguous().to(DEV)


# ------------------------------------------------------------------------------------------------ A == B: pg_refine_forward's bits
@pytest.mark.parametrize("with_probs", [True, False])
@pytest.mark.parametrize("n_eval", [1, 5, 12])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_every_grid_point_is_refine_forward(env, B, n_eval, with_probs):
    ops = env["ops"]
    q, init, cand, probs = batch(env, B)
    probs = probs if with_probs else None
    topks, temps, max_kms = list(range(1, n_eval + 1)), [0.01, 0.6, 1.6, 50.0], [0.0, 1000.0, INF]
    if with_probs:          # pg_refine_forward's 4-float records, or pg_refine_forward_ex's 12-float ones
        scratch = ops.refine_forward(env["bank"], q, init, cand, probs, n_eval, 1.0, INF, return_scratch=True)[3]
    else:
        scratch = ops.refine_forward_ex(env["bank"], q, init, cand, probs, n_eval, n_eval, 1.0, INF)[4]
    choice, veto_km = sweep(env, scratch, probs, init, topks, temps, max_kms)
    want_choice, want_refined, thresholds = [], [], []
    for topk in topks:
        for T in temps:
            for km in max_kms:
                _, _, ch, ref, _ = ops.refine_forward_ex(env["bank"], q, init, cand, probs, topk, topk, T, km)
                want_choice.append(ch); want_refined.append(ref); thresholds.append(km)
    want_choice, want_refined = torch.stack(want_choice), torch.stack(want_refined).long()
    got, bit = (choice & 63).int(), (choice & 0x80) != 0
    assert torch.equal(got, want_choice), f"{int((got != want_choice).sum())} of {got.numel()} choices differ from pg_refine_forward_ex"
    # (pg_refine_forward itself, at a sample of the points: the same selection kernel behind the other entry point)
    for g in range(0, len(thresholds), 7):
        iK, iT, iR = g // (len(temps) * len(max_kms)), (g // len(max_kms)) % len(temps), g % len(max_kms)
        _, _, ch = ops.refine_forward(env["bank"], q, init, cand, probs, topks[iK], temps[iT], max_kms[iR])
        assert torch.equal(got[g], ch)
    d = torch.gather(veto_km.expand(len(thresholds), B, n_eval), 2, want_refined[:, :, None])[:, :, 0]
    thr = torch.tensor(thresholds, dtype=torch.float64, device=DEV)[:, None]
    assert torch.equal(bit, d > thr)
    assert bool(bit[want_refined != want_choice].all())
    assert torch.equal(got[~bit], want_refined[~bit].int())
    assert not bool(torch.isnan(veto_km).any())
    # the distances themselves against torch's on the host.  The kernel's fp32 cos(lat) is the correctly rounded one, torch's (Sleef) may
    # be one fp32 ulp off: the term it scales is at most a = sin^2(c / 2), so c moves by at most 2^-23 a / sqrt(a (1 - a)) =
    # 2^-23 tan(c / 2); the fp64 rest is granted 1e-9 relative
    want_d = R.veto_distances(init.cpu().numpy(), scratch[:, :, 1:3].cpu().numpy())
    bound = 6378.137 * 2.0 ** -23 * np.tan(want_d / 6378.137 / 2) + 1e-9 * want_d + 1e-9
    assert (np.abs(veto_km.cpu().numpy() - want_d) <= bound).all()


def test_exact_thresholds(env):
    """max_km exactly ON the refined candidate's veto distance does not veto; one ulp below does -- in the sweep and in
    pg_refine_forward alike."""
    ops = env["ops"]
    B, n, T = 64, K_CAND, 0.6
    q, init, cand, probs = batch(env, B, seed=3)
    _, _, free, scratch = ops.refine_forward(env["bank"], q, init, cand, probs, n, T, INF, return_scratch=True)     # never vetoed: the refined candidate
    _, veto_km = sweep(env, scratch, probs, init, [n], [T], [INF])
    dist = torch.gather(veto_km, 1, free.long()[:, None])[:, 0].cpu().numpy()
    rows = [b for b in range(B) if dist[b] > 0][:16]
    assert len(rows) == 16
    max_kms = [v for b in rows for v in (float(dist[b]), float(np.nextafter(dist[b], -np.inf)))]
    choice, _ = sweep(env, scratch, probs, init, [n], [T], max_kms, want_veto=False)
    for i, b in enumerate(rows):
        on, below = choice[2 * i], choice[2 * i + 1]
        assert int(on[b]) == int(free[b]), f"row {b}: vetoed at max_km == its distance"
        assert int(below[b]) & 0x80, f"row {b}: not vetoed one ulp below its distance"
        for g, km in ((on, max_kms[2 * i]), (below, max_kms[2 * i + 1])):
            _, _, ch = ops.refine_forward(env["bank"], q, init, cand, probs, n, T, km)
            assert torch.equal((g & 63).int(), ch), f"row {b}, max_km {km!r}: the sweep and pg_refine_forward disagree"


# ------------------------------------------------------------------------------------------------ planted records, no bank
def planted_records():
    rng = np.random.default_rng(5)
    n = 6
    rows = []
    base_cp = np.array([0.4, 0.25, 0.15, 0.1, 0.06, 0.04], dtype=np.float32)
    rows.append((np.full(n, -100000.0), base_cp))                                        # every exp underflows: 0 / 0
    nan_cp = base_cp.copy(); nan_cp[3] = np.nan
    rows.append((np.array([-3, -1, -2, -9, -0.5, -4.0]), nan_cp))                        # a NaN probability at j = 3: the first NaN wins
    rows.append((np.full(n, -2.0), np.full(n, 0.125, dtype=np.float32)))                 # equal products: the first index wins
    rows.append((np.array([-8, -6, -1, -7, -9, -3.0]), base_cp))                         # a plain row
    score = np.array([r[0] for r in rows], dtype=np.float32)
    cp = np.array([r[1] for r in rows], dtype=np.float32)
    B = len(rows)
    init = np.stack([rng.uniform(-100, 100, B), rng.uniform(-60, 60, B)], axis=1)
    scratch = np.zeros((B, n, 4), dtype=np.float32)
    scratch[:, :, 0] = score
    scratch[:, :, 1] = (init[:, None, 0] + rng.uniform(-30, 30, (B, n))).astype(np.float32)
    scratch[:, :, 2] = (init[:, None, 1] + rng.uniform(-20, 20, (B, n))).astype(np.float32)
    return scratch, cp, init


def against_restatement(env, scratch, cp, init, grid, allow_tight=False):
    choice, _ = sweep(env, dev(scratch), None if cp is None else dev(cp), dev(init), *grid)
    score, lnglat = R.records(scratch)
    want, tight, _ = R.select_grid(score, lnglat, cp, init, *grid)
    got = choice.cpu().numpy()
    if not allow_tight:
        assert not tight.any()
        assert np.array_equal(got, want), R.first_difference(got, want)
    else:
        assert np.array_equal(got[~tight], want[~tight]), R.first_difference(np.where(tight, want, got), want)
    return got, tight


def test_planted_records_equal_the_restatement(env):
    scratch, cp, init = planted_records()
    grid = ([1, 2, 3, 4, 5, 6], [0.6, 1.6], [0.0, 1000.0, INF])
    got, _ = against_restatement(env, scratch, cp, init, grid)
    g = R.grid_index(2, 3, 5, 0, 2)                                  # topk 6, T 0.6, never veto
    assert list(got[g]) == [0, 3, 0, 2]
    against_restatement(env, scratch, None, init, grid)
    # one candidate only
    against_restatement(env, scratch[:, :1].copy(), cp[:, :1].copy(), init, ([1], [0.6, 1.6], [0.0, 1000.0, INF]))
    # topk = 64 of n_eval = 64: scores a quarter apart, so every product is far from the next
    rng = np.random.default_rng(6)
    B = 70
    wide = np.zeros((B, 64, 4), dtype=np.float32)
    perm = np.stack([rng.permutation(64) for _ in range(B)])
    wide[:, :, 0] = -perm.astype(np.float32) / 4
    init64 = np.stack([rng.uniform(-100, 100, B), rng.uniform(-60, 60, B)], axis=1)
    wide[:, :, 1] = (init64[:, None, 0] + rng.uniform(-30, 30, (B, 64))).astype(np.float32)
    wide[:, :, 2] = (init64[:, None, 1] + rng.uniform(-20, 20, (B, 64))).astype(np.float32)
    cp64 = np.full((B, 64), 1 / 64, dtype=np.float32)
    got64, _ = against_restatement(env, wide, cp64, init64, ([64, 1, 33], [0.6], [INF, 1000.0]))
    assert np.array_equal(got64[0], np.argmin(perm, axis=1))
    # SC = 12 records with the same four leading floats: the same bytes out
    wide12 = np.full((B, 64, 12), np.nan, dtype=np.float32)
    wide12[:, :, :4] = wide
    c12, v12 = sweep(env, dev(wide12), dev(cp64), dev(init64), [64, 1, 33], [0.6], [INF, 1000.0])
    c4, v4 = sweep(env, dev(wide), dev(cp64), dev(init64), [64, 1, 33], [0.6], [INF, 1000.0])
    assert torch.equal(c12, c4) and torch.equal(v12.view(torch.int64), v4.view(torch.int64))


def test_gaussian_batch_equals_the_restatement_outside_tight_pairs(env):
    scratch, cp, init = R.gaussian_batch()
    _, tight = against_restatement(env, scratch, cp, init, R.GAUSSIAN_GRID, allow_tight=True)
    assert tight.mean() < 0.01, tight.mean()


# ------------------------------------------------------------------------------------------------ totals
@pytest.fixture(scope="module")
def swept(env):
    """the Gaussian batch: B = 300 rows (no multiple of 64 or 256), its 192-point grid, a values table of 12 columns"""
    scratch, cp, init = R.gaussian_batch()
    B, n = scratch.shape[:2]
    choice, veto_km = sweep(env, dev(scratch), dev(cp), dev(init), *R.GAUSSIAN_GRID)
    assert choice.shape == (192, 300)
    rng = np.random.default_rng(9)
    km = rng.uniform(0, 20000, (B, n))
    cols = [km, np.round(5000 * np.exp(-km / 1492.7))] + [(km < r).astype(np.float64) for r in (1, 5, 10, 25, 50, 100, 200, 750, 1000, 2500)]
    values = np.ascontiguousarray(np.stack(cols, axis=2))
    return dict(scratch=scratch, cp=cp, init=init, choice=choice, values=values, B=B, n=n)


def km_bound(choice, values):
    idx = (choice & 63).astype(np.int64)
    B = choice.shape[1]
    return B * 2.0 ** -52 * np.abs(values[np.arange(B)[None, :], idx, 0]).sum(axis=1)


def test_totals_against_host_sum(env, swept):
    choice = swept["choice"].cpu().numpy()
    got = totals(env, swept["choice"], dev(swept["values"])).cpu().numpy()
    want = R.totals(choice, swept["values"], swept["n"])
    assert np.array_equal(got[:, 1:], want[:, 1:])                              # score, indicators, the two counts: integers, exact
    assert (np.abs(got[:, 0] - want[:, 0]) <= km_bound(choice, swept["values"])).all()
    assert want[:, 12].max() > 0 and want[:, 13].max() > 0


def test_a_grid_point_alone_has_the_same_bits(env, swept):
    values = dev(swept["values"])
    full = totals(env, swept["choice"], values)
    for g in (0, 77, 191):
        alone = totals(env, swept["choice"][g:g + 1].contiguous(), values)
        assert torch.equal(alone.view(torch.int64), full[g:g + 1].view(torch.int64))
    # and from a grid of its own: the point (topk 7, T 1.6, 500 km) swept alone
    g = R.grid_index(4, 4, 6, 2, 1)
    one, _ = sweep(env, dev(swept["scratch"]), dev(swept["cp"]), dev(swept["init"]), [7], [1.6], [500.0])
    assert torch.equal(one[0], swept["choice"][g])
    assert torch.equal(totals(env, one, values).view(torch.int64), full[g:g + 1].view(torch.int64))


def test_chunked_host_path(env, swept):
    ops = env["ops"]
    args = (dev(swept["scratch"]), dev(swept["cp"]), dev(swept["init"]), dev(swept["values"])) + R.GAUSSIAN_GRID
    whole = ops.refine_sweep(*args).cpu().numpy()
    chunked = ops.refine_sweep(*args, max_choice_bytes=192 * 64).cpu().numpy()             # 64 rows a chunk: 5 chunks, the last of 44
    assert np.array_equal(whole[:, 1:], chunked[:, 1:])
    assert (np.abs(whole[:, 0] - chunked[:, 0]) <= km_bound(swept["choice"].cpu().numpy(), swept["values"])).all()
    direct = totals(env, swept["choice"], dev(swept["values"])).cpu().numpy()
    assert np.array_equal(whole.view(np.int64), direct.view(np.int64))


def test_a_bad_choice_byte_forms_no_address(env, swept):
    values = dev(swept["values"])
    choice = swept["choice"][:3].clone()
    choice[1, 17] = 63                                                # index 63 of 12 candidates
    choice[2, 299] = 0x80 | 12
    got = totals(env, choice, values).cpu().numpy()
    clean = totals(env, swept["choice"][:3].contiguous(), values).cpu().numpy()
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all()
    assert np.array_equal(got[0].view(np.int64), clean[0].view(np.int64))


# ------------------------------------------------------------------------------------------------ refusals
def test_einval_by_name_and_nothing_launched(env):
    import _sweep_refusals
    _sweep_refusals.check_refusals(env["L"])
    torch.cuda.synchronize()
