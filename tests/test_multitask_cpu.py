"""SuperGuessr(multi_task=True) and heading=True off the GPU: construction and checkpoint loading against the REAL reference's
state-dict keys and weights (tests/golden/multitask.npz, written by tools/make_multitask_golden.py), the multi-task branch of
compute_geoguessr_metrics, the deferred engine carrying the aux_* columns (scripted stand-in), and the float64 restatement
tests/_auxref.py against deliberate mistakes.  The kernel itself: tests/test_gpu_multitask.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _auxref  # noqa: E402
from _scripted import FAST_THR, ScriptedModel, ScriptedRefiner, make_pixels  # noqa: E402

SETS = {"a": dict(panorama=True, yfcc=False), "b": dict(panorama=False, yfcc=True)}


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "multitask.npz"))


@pytest.fixture()
def geocell_csv(fx, tmp_path):
    from pigeon_amd import synthetic
    path = str(tmp_path / "geocells.csv")
    synthetic.write_geocell_csv(path, fx["geocells"])
    return path


def _model(geocell_csv, **kw):
    from pigeon_amd.super_guessr import SuperGuessr
    return SuperGuessr(None, geocell_path=geocell_csv, **kw)


# ------------------------------------------------------------------------------------------------ 1. construction
@pytest.mark.parametrize("tag", ["a", "b"])
def test_construction_has_the_references_state_and_loads_its_checkpoint(fx, geocell_csv, tmp_path, capsys, tag):
    cfg = SETS[tag]
    m = _model(geocell_csv, multi_task=True, **cfg)
    keys = [str(k) for k in fx[f"{tag}_state_keys"]]
    assert sorted(m.state_dict().keys()) == keys
    assert ("month_layer.weight" in keys) == (not cfg["yfcc"]) and hasattr(m, "month_layer") == (not cfg["yfcc"])
    assert m.input_dim == 1024 and m.multi_task_head.out_features == 6 and m.climate_layer.out_features == 28
    for attr in ("loss_fnc_mt", "loss_fnc_climate") + (() if cfg["yfcc"] else ("loss_fnc_month",)):
        assert hasattr(m, attr)
    sd = {k: torch.from_numpy(fx[f"{tag}_w_{k}"]) for k in keys}
    m.load_state_dict(sd)
    for k in keys:
        assert torch.equal(m.state_dict()[k], sd[k]), k
    # load_state (the reference's name-wise loader): every entry of a multi-task checkpoint finds its place
    ckpt = str(tmp_path / "mt.model")
    torch.save(sd, ckpt)
    m2 = _model(geocell_csv, multi_task=True, **cfg)
    capsys.readouterr()
    m2.load_state(ckpt)
    assert "not in model's state" not in capsys.readouterr().out
    for k in keys:
        assert torch.equal(m2.state_dict()[k], sd[k]), k
    text = str(m)
    assert "multi-task" in text and "= True" in text.split("multi-task")[1].split("\n")[0] and "input_dim" in text
    # the same checkpoint into a model without the heads: the three layers are reported and dropped, as before
    m3 = _model(geocell_csv, **cfg)
    m3.load_state(ckpt)
    assert "Parameter climate_layer.weight not in model's state." in capsys.readouterr().out
    assert not hasattr(m3, "climate_layer")


def test_constants_under_the_references_names():
    from pigeon_amd import super_guessr as sg
    assert (sg.NUM_MULTI_TASK_VARIABLES, sg.NUM_CLIMATES, sg.NUM_MONTHS) == (6, 28, 12)
    assert (sg.REGRESSION_LOSS_SCALING, sg.CLIMATE_LOSS_SCALING, sg.MONTHS_LOSS_SCALING) == (8, 2, 1)
    assert sg.MultiTaskPredictions._fields == ("loss_reg", "preds_mt", "loss_climate", "preds_climate", "loss_month", "preds_month")


# ------------------------------------------------------------------------------------------------ 2. heading
def test_heading_is_accepted_where_the_reference_ignores_it(geocell_csv):
    m = _model(geocell_csv, panorama=True, hierarchical=False, heading=True)
    assert m.heading and m.input_dim == 1024 and m.cell_layer.in_features == 1024
    with pytest.raises(NotImplementedError, match="heading"):
        _model(geocell_csv, panorama=False, heading=True)
    with pytest.raises(NotImplementedError, match="hierarchical"):
        _model(geocell_csv, panorama=True, hierarchical=True)
    with pytest.raises(NotImplementedError, match="hierarchical"):
        _model(geocell_csv, panorama=True, hierarchical=True, heading=True)


# ------------------------------------------------------------------------------------------------ 3. metrics
def _tuple(fx, tag, with_mt=True):
    month = fx[f"{tag}_out_preds_month"] if f"{tag}_out_preds_month" in fx.files else None
    lm = fx[f"{tag}_labels_month"] if f"{tag}_labels_month" in fx.files else None
    mt = (fx[f"{tag}_out_preds_mt"], fx[f"{tag}_out_preds_climate"], month) if with_mt else (None, None, None)
    lab = (fx[f"{tag}_labels_multi_task"], fx[f"{tag}_labels_climate"], lm) if with_mt else (None, None, None)
    return (fx[f"{tag}_out_preds_LLH"], fx[f"{tag}_out_preds_geocell"]) + mt + (fx[f"{tag}_out_top5_indices"], fx[f"{tag}_labels"],
                                                                                 fx[f"{tag}_labels_clf"]) + lab


@pytest.mark.parametrize("tag", ["a", "b"])
def test_metrics_multi_task_entries(fx, tag, capsys):
    from sklearn.preprocessing import StandardScaler
    from pigeon_amd.evaluate import compute_geoguessr_metrics
    base = compute_geoguessr_metrics(_tuple(fx, tag, with_mt=False))
    assert not any("Climate" in k or "Month" in k or k.endswith(("elevation_error", "prec_diff_error")) for k in base)
    assert list(base) == ["Mean_km_error", "Median_km_error"] + [f"Under_{km}_km" for km in (1, 5, 10, 25, 50, 100, 200, 750, 1000, 2500)] + \
        ["Geoguessr_score", "Geocell_accuracy", "Geocell_top5_accuracy"]
    # without a scaler file: the accuracies, one line about the six errors
    capsys.readouterr()
    d = compute_geoguessr_metrics(_tuple(fx, tag))
    assert "Mean_*_error entries are left out" in capsys.readouterr().out
    assert d["Climate_accuracy"] == float(fx[f"{tag}_climate_accuracy"])
    assert ("Month_accuracy" in d) == (tag == "a")
    if tag == "a":
        assert d["Month_accuracy"] == float(fx["a_month_accuracy"])
    assert not any(k.startswith("Mean_") and k != "Mean_km_error" for k in d)
    for k in base:
        assert d[k] == base[k], k
    # class-index climate labels give the same accuracy as the one-hot rows the model's forward takes
    t = list(_tuple(fx, tag))
    t[9] = np.argmax(t[9], axis=-1)
    assert compute_geoguessr_metrics(tuple(t))["Climate_accuracy"] == d["Climate_accuracy"]
    # with a scaler: the six errors on the recovered values (inverse transform, exp on all columns but the third, offsets)
    rng = np.random.RandomState(3)
    scaler = StandardScaler().fit(rng.standard_normal((200, 6)) * np.array([0.4, 0.6, 9.0, 0.5, 0.3, 0.2]) + np.array([6, 3, 12, 2, 4, 3]))
    d2 = compute_geoguessr_metrics(_tuple(fx, tag), scaler=scaler)
    yfcc = tag == "b"

    def recover(v, off):
        v = v.astype(np.float64) * scaler.scale_ + scaler.mean_
        v[:, [0, 1, 3, 4, 5]] = np.exp(v[:, [0, 1, 3, 4, 5]])
        return v - np.array([off, 1, 0, 1, 1, 1])
    p, l = recover(fx[f"{tag}_out_preds_mt"], 416 if yfcc else 408), recover(fx[f"{tag}_labels_multi_task"], 408)
    names = ("elevation", "population", "temperature", "temp_diff", "precipitation", "prec_diff")
    for i, name in enumerate(names):
        want = np.mean(np.abs(l[:, i] - p[:, i]))
        # the function works in the dtype it is handed, as the reference does (fp32 predictions and labels): an inverse transform and
        # an exp of an argument of size <= 16 in fp32 are each good to a few units of 2^-24 of the recovered value -- 64 of them here
        assert abs(d2[f"Mean_{name}_error"] - want) <= 64 * 2.0 ** -24 * max(np.abs(p[:, i]).max(), np.abs(l[:, i]).max(), 408), name
    assert d2["Climate_accuracy"] == d["Climate_accuracy"]


# ------------------------------------------------------------------------------------------------ 4. the engine carries aux_*
class ScriptedAuxModel(ScriptedModel):
    """ScriptedModel whose states carry the auxiliary heads' columns: values that tell the fast pass from the exact one."""

    def _aux(self, st, rows, fast):
        n = rows.shape[0]
        e = st["embedding"].mean(dim=1)
        st["aux_preds"] = torch.cat([e, e[:, :2] * (2.0 if fast else 3.0)], dim=1).contiguous()
        st["aux_cls"] = torch.stack([st["preds_geocell"] % 28, (st["preds_geocell"] + (0 if fast else 1)) % 12], dim=1)
        st["aux_tol"] = rows[:, 4].clone() * (1.0 if fast else 1e-3)
        st["aux_code"] = torch.full((n,), 3 if fast else 104, dtype=torch.int32)
        st["tol"] = torch.minimum(st["tol"], st["aux_tol"])        # row_tol: the row's tolerance over all of its decisions
        return st

    def encode_head(self, pixel_values=None, embedding=None):
        st = super().encode_head(pixel_values, embedding)
        return self._aux(st, pixel_values.reshape(pixel_values.shape[0], 48).float(), fast=True)

    def exact_rows(self, pixel_rows):
        st = super().exact_rows(pixel_rows)
        return self._aux(st, torch.cat([t.reshape(t.shape[0], -1) for t in pixel_rows]).float(), fast=False)


def _run(steps, **kw):
    from oracle import requeue_oracle
    from pigeon_amd.deferred import DeferredExact
    m, r = ScriptedAuxModel(), ScriptedRefiner()
    eng = DeferredExact(m, r, ops=requeue_oracle, **kw)
    out = {}
    for i, px in enumerate(steps):
        for res in eng.submit(px, meta=i):
            out[res["meta"]] = res
    for res in eng.flush():
        out[res["meta"]] = res
    return out, m


def test_deferred_engine_carries_the_aux_columns():
    g = torch.Generator().manual_seed(17)
    steps, aux_only = [], []
    for i in range(12):
        B = 5 if i != 7 else 3
        flags = lambda p: (torch.rand(B, generator=g) > p).float().tolist()        # noqa: E731
        px = make_pixels(flags(0.2), flags(0.1), flags(0.2), flags(0.1), seed=300 + i)
        a = torch.tensor(flags(0.25))
        px.reshape(B, 48)[:, 4] = a                               # the aux tolerance after the fast pass (scripted like px[0])
        flat = px.reshape(B, 48)
        aux_only.append((flat[:, 0] > FAST_THR) & (flat[:, 2] > FAST_THR) & (a <= FAST_THR))
        steps.append(px)
    now, m_now = _run(steps, immediate=True)
    later, m = _run(steps, min_flush=4, max_lag=5)
    keys = ("aux_preds", "aux_cls", "aux_tol", "aux_code")
    n_aux_only = 0
    for i in range(12):
        a, b = now[i]["state"], later[i]["state"]
        for k in a:
            if torch.is_tensor(a[k]):
                assert torch.equal(a[k], b[k]), (i, k)
        for k in keys:
            assert k in b and k not in later[i], (i, k)           # rank-local reports: in the state, not among the gathered tensors
        ex = b["exact"]
        # re-encoded rows carry the exact pass's values, the others the fast pass's
        assert torch.equal(b["aux_code"], torch.where(ex, 104, 3).to(torch.int32)), i
        e = b["embedding"].mean(dim=1)
        assert torch.equal(b["aux_preds"][:, -2:], e[:, :2] * torch.where(ex, 3.0, 2.0)[:, None]), i
        assert torch.equal(b["aux_cls"][:, 1], (b["preds_geocell"] + ex.long()) % 12), i
        # a row that only the aux tolerance flags is re-encoded too
        assert bool(ex[aux_only[i]].all()), i
        n_aux_only += int(aux_only[i].sum())
    assert n_aux_only >= 3 and sum(n for _, n in m.calls) == sum(n for _, n in m_now.calls)
    # a model without the heads: no aux_* anywhere (the plain scripted model)
    from oracle import requeue_oracle
    from pigeon_amd.deferred import DeferredExact
    eng = DeferredExact(ScriptedModel(), None, ops=requeue_oracle, immediate=True)
    st = eng.submit(steps[0])[0]["state"]
    assert not any(k.startswith("aux_") for k in st)


# ------------------------------------------------------------------------------------------------ 5. the restatement itself
def _case(seed=0, B=40, P=4, n=(6, 28, 12)):
    rng = np.random.RandomState(seed)
    A = sum(n)
    return rng.standard_normal((B, P, 1024)), rng.uniform(-1, 1, (A, 1024)) / 32, rng.uniform(-1, 1, A) / 32, n


def test_auxref_layout_and_argmax():
    emb, W, b, n = _case()
    r = _auxref.forward(emb, W, b, *n)
    p = r["preds"]
    assert np.allclose(p, emb.mean(axis=1) @ W.T + b, rtol=0, atol=1e-12)
    assert np.array_equal(r["cls"][:, 0], p[:, 6:34].argmax(-1)) and np.array_equal(r["cls"][:, 1], p[:, 34:].argmax(-1))
    # deliberate mistakes the restatement must tell apart from itself on this data
    swapped = np.stack([p[:, 5:33].argmax(-1), p[:, 33:45].argmax(-1)], axis=1)            # a segment boundary one row off
    month_over_climate = p[:, 6:18].argmax(-1)                                            # month argmax taken over climate columns
    assert (swapped != r["cls"]).any() and (month_over_climate != r["cls"][:, 1]).any()
    # n_month = 0: no month classifier, no month codes
    r0 = _auxref.forward(emb, W[:34], b[:34], 6, 28, 0)
    assert (r0["cls"][:, 1] == -1).all() and (r0["code"] < 101).all() and (r0["code"] >= 1).all()
    # a single class and no other classifier: nothing to decide
    r1 = _auxref.forward(emb, W[:7], b[:7], 6, 1, 0)
    assert np.isinf(r1["tol"]).all() and (r1["code"] == 0).all() and (r1["cls"][:, 0] == 0).all()


def test_auxref_ties_and_nan():
    assert _auxref.first_argmax([1.0, 3.0, 3.0, 2.0]) == 1                                 # ties: the LOWEST index (not 2)
    assert _auxref.first_argmax([1.0, np.nan, 5.0, np.nan]) == 1                           # a NaN ranks above every number
    # exact inputs (integers, eighths): climate class 9 gets class 4's output from a DIFFERENT weight row (two columns swapped on
    # which the embedding agrees), both on top -> an exact tie: the lowest index wins, margin 0 -> tolerance 0, set by class 9
    rng = np.random.RandomState(1)
    n = (6, 28, 12)
    emb = rng.randint(-8, 9, size=(3, 4, 1024)).astype(np.float64) * 4
    emb[:, :, 0] = emb[:, :, 1] = 8.0
    W = rng.randint(-8, 9, size=(46, 1024)).astype(np.float64) / 8
    b = rng.randint(-3, 4, size=46).astype(np.float64)
    W[6 + 4, 0], W[6 + 4, 1] = 0.5, -0.25
    W[6 + 9] = W[6 + 4]
    W[6 + 9, 0], W[6 + 9, 1] = -0.25, 0.5
    b[6 + 4] = b[6 + 9] = 1e6
    r = _auxref.forward(emb, W, b, *n)
    assert (r["preds"][:, 6 + 4] == r["preds"][:, 6 + 9]).all() and (r["cls"][:, 0] == 4).all()          # not 9: ties to the LOWEST index
    assert (r["tol"] == 0).all() and (r["code"] == 1 + 9).all()
    # identical rows are no decision at all: no embedding error can move a margin whose gradient is zero
    W[6 + 9] = W[6 + 4]
    r = _auxref.forward(emb, W, b, *n)
    assert (r["cls"][:, 0] == 4).all() and (r["tol"] > 0).all() and (r["code"] != 1 + 9).all()
    emb[1, 2, 77] = np.nan
    r = _auxref.forward(emb, W, b, *n)
    assert r["cls"][1].tolist() == [0, 0] and r["tol"][1] == 0 and r["code"][1] == 2       # first alternative visited sets it


def test_auxref_tolerance_visits_every_alternative_and_means_what_it_says():
    emb, W, b, n = _case(seed=2, B=160, P=1)
    beta = np.random.RandomState(5).standard_normal(1024) * 2e-4 / 32
    for bt in (None, beta):
        r = _auxref.forward(emb, W, b, *n, beta=bt)
        # a tolerance that skips the LAST alternative of a classifier is larger exactly on the rows where that one sets it
        skipped = []
        for i in range(emb.shape[0]):
            p, e = r["preds"][i], emb[i, 0]
            best = np.inf
            for off, m, c0 in ((6, 28, r["cls"][i, 0]), (34, 12, r["cls"][i, 1])):
                for c in range(m - 1):                                                     # the mistake: range(m - 1)
                    if c != c0:
                        best = min(best, _auxref.tol_of(p[off + c0] - p[off + c], W[off + c0] - W[off + c],
                                                        np.zeros(1024) if bt is None else bt, np.linalg.norm(e)))
            skipped.append(best)
        skipped = np.array(skipped)
        sets_it = np.isin(r["code"], (1 + 27, 101 + 11))
        assert sets_it.sum() >= 2 and np.array_equal(skipped > r["tol"], sets_it) and (skipped >= r["tol"]).all()
    r = _auxref.forward(emb, W, b, *n)
    # without beta: a step of 0.9 x / 1.1 x the tolerance along -g keeps / flips the argmax the code names
    for i in range(20):
        code = int(r["code"][i])
        which, c = (0, code - 1) if code < 101 else (1, code - 101)
        off = 6 if which == 0 else 34
        c0 = int(r["cls"][i, which])
        gvec = W[off + c0] - W[off + c]
        e = emb[i, 0]
        step = r["tol"][i] / 32.0 * np.linalg.norm(e) * gvec / np.linalg.norm(gvec)
        for f, same in ((0.9, True), (1.1, False)):
            e2 = emb[i:i + 1].copy()
            e2[0, 0] = e - f * step
            assert (int(_auxref.forward(e2, W, b, *n)["cls"][0, which]) == c0) == same, (i, f)


def test_auxref_bound_covers_fp32_in_two_orders():
    emb, W, b, n = _case(seed=3, B=16)
    emb, W, b = emb.astype(np.float32), W.astype(np.float32), b.astype(np.float32)
    exact = _auxref.preds(emb, W, b)
    bd = _auxref.bound(emb, W, b)
    mean32 = (emb[:, 0] + emb[:, 1] + emb[:, 2] + emb[:, 3]) * np.float32(0.25)
    fwd = np.zeros((16, 46), dtype=np.float32)
    for k in range(1024):
        fwd += mean32[:, k:k + 1] * W[None, :, k]
    blas = mean32 @ W.T
    for got in (fwd + b, blas + b):
        assert got.dtype == np.float32 and (np.abs(got.astype(np.float64) - exact) <= bd).all()
    assert (bd < 2e-3).all() and (bd > 0).all()
