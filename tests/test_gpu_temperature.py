"""pg_temper_stats and pg_temper_logits on the GPU (run with -m gpu on an MI355X), through the C ABI, against tests/_tempref.py: the
longdouble restatement of the contract with derived bounds.  Every finite output lies within its bound and NaNs sit exactly where
the contract puts them; a row is the same bits alone, inside a batch, at another position, with its beta at another index, with
another K and with or without the optional outputs; totals are the stated sum of the kernel's own rows, bit for bit.  Every output
sits between guard regions that must keep their pattern, and no input may change."""
import ctypes as C

import numpy as np
import pytest
import torch

import _tempref as T

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD = 64
# every C of the issue, every N and every K at least once
CASES = [(1, 1, 1), (1, 7, 3), (2, 2, 3), (63, 7, 16), (64, 300, 3), (65, 7, 1), (255, 2, 16), (256, 7, 3), (257, 300, 16),
         (1025, 7, 3), (10007, 7, 16), (10007, 1, 1)]
WORST = {"ratio": 0.0}


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops
    _lib.require_gpu()
    return dict(lib=_lib, ops=hip_ops, L=_lib.load())


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def guarded(n, dtype, fill):
    buf = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + n]


def run(env, logits, labels, betas, stats=True, conf=True, state=True):
    """numpy in -> dict of device tensors (row_stats (N,K,3), conf (N,K), state (N,) where asked for; totals (K,3), counts (2,)),
    through the C ABI; guards and inputs checked"""
    ops = env["ops"]
    N, Cn = logits.shape
    K = len(betas)
    ins = [dev(logits), dev(labels)]
    keep = [t.clone() for t in ins]
    bufs = {"totals": guarded(K * 3, torch.float64, -7.25), "counts": guarded(2, torch.int64, -77)}
    if stats:
        bufs["row_stats"] = guarded(N * K * 3, torch.float64, -7.25)
    if conf:
        bufs["conf"] = guarded(N * K, torch.float64, -7.25)
    if state:
        bufs["state"] = guarded(N, torch.uint8, 201)
    ptr = lambda k: ops._p(bufs[k][1]) if k in bufs else ops._p(None)
    b = (C.c_double * K)(*[float(v) for v in betas])
    env["lib"].check(env["L"].pg_temper_stats(ops._p(ins[0]), N, Cn, ops._p(ins[1]), b, K, ptr("row_stats"), ptr("conf"), ptr("state"),
                                              ptr("totals"), ptr("counts"), ops._stream()), "pg_temper_stats")
    torch.cuda.synchronize()
    for name, (buf, view) in bufs.items():
        n, fill = view.numel(), buf[0].item()
        assert bool((buf[:GUARD] == fill).all()) and bool((buf[GUARD + n:] == fill).all()), f"{name}: wrote outside its output"
    for t, k in zip(ins, keep):
        assert torch.equal(raw(t), raw(k)), "an input changed"
    shapes = {"row_stats": (N, K, 3), "conf": (N, K), "state": (N,), "totals": (K, 3), "counts": (2,)}
    return {k: v[1].clone().reshape(shapes[k]) for k, v in bufs.items()}


def raw(t):
    """the bytes of a tensor (an empty one has none)"""
    return t.contiguous().flatten().view(torch.uint8) if t.numel() else torch.empty(0, dtype=torch.uint8, device=t.device)


def bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def held(env, capsys, logits, labels, betas, what=""):
    got = run(env, logits, labels, betas)
    t = T.truth(logits, labels, betas)
    errors, worst = T.compare(t, got["row_stats"].cpu().numpy(), got["conf"].cpu().numpy(), got["state"].cpu().numpy())
    e2, w2 = T.compare_totals(t, got["totals"].cpu().numpy(), got["counts"].cpu().numpy())
    WORST["ratio"] = max(WORST["ratio"], worst, w2)
    with capsys.disabled():
        print(f"\ntemper_stats {what}: worst |got - truth| / bound {worst:.3g} (rows), {w2:.3g} (totals); worst so far {WORST['ratio']:.3g}")
    assert not errors, errors[:5]
    assert not e2, e2[:5]
    want = T.totals_in_order(got["row_stats"].cpu().numpy(), got["state"].cpu().numpy())
    assert np.array_equal(got["totals"].cpu().numpy().view(np.int64), want.view(np.int64)), "totals are not the stated sum of the rows"
    return got, t


# ================================================================================================================ against the truth
@pytest.mark.parametrize("Cn,N,K", CASES)
def test_rows_and_totals_within_derived_bounds(env, capsys, Cn, N, K):
    """Gaussian rows at scales 1 and 30, ties, constant rows, -inf cells, underflowing weights and (from N = 7 on) a label on a -inf
    cell; at N = 300 also labels outside the range, NaN and +inf cells"""
    logits, labels, kinds = T.make_rows(N, Cn, seed=Cn + N)
    got, t = held(env, capsys, logits, labels, T.betas_of(K), what=f"C = {Cn}, N = {N}, K = {K}")
    rs, cf = got["row_stats"].cpu().numpy(), got["conf"].cpu().numpy()
    for n, kind in enumerate(kinds):
        if kind == "constant":
            assert (rs[n, :, 1] == 0).all() and (rs[n, :, 2] == 0).all(), f"row {n}: derivatives of a constant row"
            assert (cf[n] == 1.0 / Cn).all()                        # Z = C exactly, one rounded division
        if kind == "underflow":
            assert (cf[n] == 1.0).all(), f"row {n}: every other weight underflows"


def test_every_kind_of_row_at_a_small_size(env, capsys):
    logits, labels, kinds = T.make_rows(24, 65, seed=9)
    got, t = held(env, capsys, logits, labels, T.betas_of(3), what="all kinds, C = 65")
    st = got["state"].cpu().numpy()
    for n, kind in enumerate(kinds):
        assert (st[n] == 2) == (kind in T.INVALID_KINDS), (n, kind)
        if kind == "tie":                                            # the first index wins: the label is on it for even n
            assert st[n] == (1 if n % 2 == 0 else 0)
    assert int(got["counts"][0]) == sum(k not in T.INVALID_KINDS for k in kinds)


def test_totals_with_every_third_row_invalid_and_empty(env, capsys):
    logits, labels, _ = T.make_rows(300, 257, seed=11, kinds=("gauss1", "gauss30", "label_negative"))
    got, t = held(env, capsys, logits, labels, T.betas_of(3), what="every third row invalid")
    assert got["counts"].tolist()[0] == 200
    assert bool(torch.isfinite(got["totals"]).all())
    empty = run(env, np.zeros((0, 257), dtype=np.float32), np.zeros((0,), dtype=np.int64), T.betas_of(3))
    assert bool((empty["totals"] == 0).all()) and empty["counts"].tolist() == [0, 0]


# ================================================================================================================ bit identity
@pytest.mark.parametrize("Cn", [65, 1025])
def test_a_row_is_the_same_bits_wherever_it_stands(env, Cn):
    logits, labels, _ = T.make_rows(12, Cn, seed=21)
    betas = T.betas_of(16)
    full = run(env, logits, labels, betas)
    for n in (0, 1, 2, 4, 5):                                        # alone
        one = run(env, logits[n:n + 1], labels[n:n + 1], betas)
        assert bits_equal(one["row_stats"][0], full["row_stats"][n]) and bits_equal(one["conf"][0], full["conf"][n]), f"row {n} alone"
        assert int(one["state"][0]) == int(full["state"][n])
    perm = np.random.default_rng(3).permutation(12)                  # at another position
    moved = run(env, logits[perm], labels[perm], betas)
    assert bits_equal(moved["row_stats"], full["row_stats"][perm]) and bits_equal(moved["conf"], full["conf"][perm])
    assert torch.equal(moved["state"], full["state"][perm])


@pytest.mark.parametrize("Cn", [65, 1025])
def test_a_beta_is_the_same_bits_at_any_index_and_any_K(env, Cn):
    logits, labels, _ = T.make_rows(7, Cn, seed=22)
    betas = T.betas_of(16)
    full = run(env, logits, labels, betas)
    assert bits_equal(full["row_stats"][:, 0], full["row_stats"][:, 3]), "the repeated beta, in two groups of the kernel"
    assert bits_equal(full["row_stats"][:, 4], full["row_stats"][:, 11])
    order = list(reversed(range(16)))
    rev = run(env, logits, labels, [betas[i] for i in order])
    assert bits_equal(rev["row_stats"], full["row_stats"][:, order]) and bits_equal(rev["conf"], full["conf"][:, order])
    for K, pick in ((1, [5]), (3, [9, 2, 14]), (5, [15, 0, 1, 2, 6])):
        sub = run(env, logits, labels, [betas[i] for i in pick])
        assert len(pick) == K and bits_equal(sub["row_stats"], full["row_stats"][:, pick]) and bits_equal(sub["conf"], full["conf"][:, pick])
        assert bits_equal(sub["totals"], full["totals"][pick])


def test_optional_outputs_change_nothing(env):
    logits, labels, _ = T.make_rows(300, 63, seed=23)
    betas = T.betas_of(3)
    full = run(env, logits, labels, betas)
    for stats, conf, state in ((False, False, False), (True, False, False), (False, True, True), (False, False, True)):
        part = run(env, logits, labels, betas, stats=stats, conf=conf, state=state)
        assert bits_equal(part["totals"], full["totals"]) and torch.equal(part["counts"], full["counts"]), (stats, conf, state)
        for k in part:
            assert torch.equal(raw(part[k]), raw(full[k])), (k, stats, conf, state)


# ================================================================================================================ arguments
def test_every_einval_names_its_argument(env):
    ops, L, lib = env["ops"], env["L"], env["lib"]
    lg, lb = dev(np.zeros((2, 5), dtype=np.float32)), dev(np.zeros((2,), dtype=np.int64))
    tot, cnt = torch.zeros((16, 3), dtype=torch.float64, device=DEV), torch.zeros((2,), dtype=torch.int64, device=DEV)
    ok = (C.c_double * 16)(*([1.0] * 16))
    null = ops._p(None)

    def call(logits=lg, N=2, Cn=5, labels=lb, betas=ok, K=1, totals=tot, counts=cnt):
        p = lambda v: v if isinstance(v, C.c_void_p) else ops._p(v)
        return L.pg_temper_stats(p(logits), N, Cn, p(labels), betas, K, null, null, null, p(totals), p(counts), ops._stream())

    def refused(rc, word):
        assert rc == -1, (word, rc)                                 # PG_EINVAL
        assert word in L.pg_last_error().decode(), (word, L.pg_last_error())

    refused(call(N=-1), "N")
    refused(call(Cn=0), "C")
    refused(call(K=0), "K")
    refused(call(K=17), "K")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused(call(betas=(C.c_double * 2)(1.0, bad), K=2), "betas[1]")
    refused(call(logits=null), "logits")
    refused(call(labels=null), "labels")
    refused(call(betas=None), "betas")
    refused(call(totals=null), "totals")
    refused(call(counts=null), "counts")
    out = torch.zeros((2, 5), dtype=torch.float32, device=DEV)
    refused(L.pg_temper_logits(ops._p(lg), -1, 5, 1.0, ops._p(out), ops._stream()), "N")
    refused(L.pg_temper_logits(ops._p(lg), 2, 0, 1.0, ops._p(out), ops._stream()), "C")
    refused(L.pg_temper_logits(ops._p(lg), 2, 5, 0.0, ops._p(out), ops._stream()), "beta")
    refused(L.pg_temper_logits(null, 2, 5, 1.0, ops._p(out), ops._stream()), "logits")
    refused(L.pg_temper_logits(ops._p(lg), 2, 5, 1.0, null, ops._stream()), "out")
    o = (C.c_int32 * 4)()
    refused(L.pg_temper_plan(2, 5, 17, o), "K")
    assert L.pg_temper_plan(300, 257, 16, o) == 0
    assert list(o) == [256, 4, 49, 300 * 16 * 24 + 304]
    with pytest.raises(lib.PigeonHipError, match="labels"):
        ops.temper_stats(lg, lb[:1], [1.0])
    with pytest.raises(lib.PigeonHipError, match="float32"):
        ops.temper_stats(lg.double(), lb, [1.0])
    with pytest.raises(lib.PigeonHipError, match="device"):
        ops.temper_stats(lg.cpu(), lb, [1.0])


def test_wrapper_matches_the_c_abi(env):
    logits, labels, _ = T.make_rows(7, 65, seed=31)
    betas = T.betas_of(3)
    raw_out = run(env, logits, labels, betas)
    got = env["ops"].temper_stats(dev(logits), dev(labels), betas, row_stats=True, conf=True, state=True)
    for k in raw_out:
        assert torch.equal(raw(got[k]), raw(raw_out[k])), k
    assert set(env["ops"].temper_stats(dev(logits), dev(labels), betas)) == {"totals", "counts"}


# ================================================================================================================ the logits
@pytest.mark.parametrize("beta", [1.0 / 64, 0.4, 1.0, 1 / 2.5, 64.0])
def test_temper_logits_is_one_rounded_multiplication(env, beta):
    no_nan = lambda t: torch.where(torch.isnan(t), torch.full_like(t, 1.5), t)      # torch.equal, with NaN equal to NaN
    ops = env["ops"]
    logits, _, _ = T.make_rows(24, 1025, seed=41)
    logits[3] *= 1e30
    logits[4] *= 1e-38                                              # subnormal products
    x = dev(logits)
    keep = x.clone()
    buf, view = guarded(x.numel(), torch.float32, -7.25)
    out = view.view(x.shape)
    ops.temper_logits(x, beta, out=out)
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == -7.25).all()) and bool((buf[GUARD + x.numel():] == -7.25).all())
    want = keep * torch.tensor(beta).float()
    assert torch.equal(no_nan(out), no_nan(want))
    assert torch.equal(torch.isnan(out), torch.isnan(keep)) and torch.equal(out == -np.inf, keep == -np.inf)
    assert torch.equal(x.view(torch.int32), keep.view(torch.int32)), "the input changed"
    ops.temper_logits(x, beta, out=x)                               # in place
    assert torch.equal(no_nan(x), no_nan(want))
    assert ops.temper_logits(x[:0], beta).shape == (0, 1025)


def test_report_worst_ratio(capsys):
    """the figure DESIGN.md records: the worst |got - truth| / bound of this module's comparisons"""
    with capsys.disabled():
        print(f"\ntemper_stats: worst |got - truth| / bound over the module {WORST['ratio']:.3g}")
    assert WORST["ratio"] < 1
