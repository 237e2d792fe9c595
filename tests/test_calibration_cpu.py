"""The encoder calibration as a FILE keyed by a weight fingerprint (pigeon_amd/certainty.py, csrc/fingerprint.hip), host side: the
numpy restatement of the digest, the save / load round trip, what `load_calibration` refuses (and that a refusal changes nothing), the
precomputed-embedding tolerance, and the command lines.  No GPU: the encoder's fingerprint is scripted (the kernel itself is checked
against the same restatement in tests/test_gpu_calibration.py)."""
import os
import sys

import numpy as np
import pytest
import torch

import _fpref
from pigeon_amd import synthetic
from pigeon_amd.certainty import FORMAT_VERSION, CalibrationError, Certainty
from pigeon_amd.clip_embedder import CLIPEmbedding, HipCLIPVisionModel
from pigeon_amd.super_guessr import SuperGuessr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP_A, FP_B = "0123456789abcdef" * 2, "fedcba9876543210" * 2


# ------------------------------------------------------------------------------------------------ the digest's restatement
def test_fpref_vectorised_equals_chunk_by_chunk():
    rng = np.random.default_rng(0)
    for n in (0, 1, 15, 16, 17, 31, 32, 33, 100, 1000):
        b = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        for seed in (0, 1, 2 ** 63 + 5, 2 ** 64 - 1):
            assert _fpref.fingerprint(b, seed) == _fpref.fingerprint_slow(b, seed), (n, seed)


def test_fpref_reacts_to_what_it_must():
    rng = np.random.default_rng(1)
    a = rng.integers(0, 256, 4096, dtype=np.uint8)
    base = _fpref.fingerprint(a)
    assert base == _fpref.fingerprint(a.copy()) and all(0 <= v < 2 ** 64 for v in base)
    swapped = a.copy()                                            # two chunks change places: the chunk index is in the key
    swapped[16:32], swapped[160:176] = a[160:176], a[16:32]
    assert sorted(swapped.tolist()) == sorted(a.tolist())
    flipped = a.copy()
    flipped[1234] ^= 0x10                                         # one bit
    halves = a.copy()                                             # the two halves of one chunk change places
    halves[0:8], halves[8:16] = a[8:16], a[0:8]
    seen = {base}
    for other in (_fpref.fingerprint(swapped), _fpref.fingerprint(flipped), _fpref.fingerprint(halves), _fpref.fingerprint(a, seed=1),
                  _fpref.fingerprint(a, seed=2 ** 63 + 5)):
        assert other != base                                      # (each word sums one half of every chunk: a change confined to one half moves one word)
        seen.add(other)
    assert len(seen) == 6
    # 15 bytes against the same 15 bytes and a trailing zero: the same padded chunk, another length
    short = bytes(range(1, 16))
    assert _fpref.fingerprint(short) != _fpref.fingerprint(short + b"\0")
    assert _fpref.fingerprint(b"") != _fpref.fingerprint(b"\0") and _fpref.fingerprint(b"", 0) != _fpref.fingerprint(b"", 1)


# ------------------------------------------------------------------------------------------------ Certainty as state
def _measured(n=10, P=4, seed=0, bias_scale=2.5e-4, noise=4e-5):
    """A Certainty calibrated on scripted embeddings with a systematic part (kept) -> (certainty, fast images, exact images)."""
    g = torch.Generator().manual_seed(seed)
    ei = torch.randn((n * P, 1024), generator=g)
    beta = bias_scale * torch.randn((1024,), generator=g) / 32
    fi = ei + ei.norm(dim=1, keepdim=True) * (beta + noise * torch.randn((n * P, 1024), generator=g) / 32)
    c = Certainty()
    c.calibrate(fi.reshape((n, P, -1)).mean(dim=1), ei.reshape((n, P, -1)).mean(dim=1), fast_images=fi, exact_images=ei)
    assert c.bias is not None and c.calibrated and not c.force_exact
    return c, fi, ei


def test_calibrate_records_image_residual_rms():
    c, fi, ei = _measured()
    n, P = 10, 4
    f3, e3 = fi.reshape((n, P, -1)), ei.reshape((n, P, -1))
    b_half = ((f3 - e3) / e3.norm(dim=2, keepdim=True))[0::2].reshape((-1, 1024)).mean(dim=0)
    held_f, held_e = f3[1::2].reshape((-1, 1024)), e3[1::2].reshape((-1, 1024))
    want = float(((Certainty.apply_bias(held_f, b_half) - held_e).norm(dim=1) / held_e.norm(dim=1)).pow(2).mean().sqrt())
    assert c.stats["image_residual_rms"] == pytest.approx(want, rel=1e-6)
    assert 0 < c.stats["image_residual_rms"] < 0.5 * c.stats["image_rel_err"]          # the bias explains most of the raw error here
    # without a bias worth keeping it is the raw per-image RMS error
    g = torch.Generator().manual_seed(3)
    e = torch.randn((32, 1024), generator=g)
    f = e + e.norm(dim=1, keepdim=True) * 1e-4 * torch.randn((32, 1024), generator=g) / 32
    c2 = Certainty()
    st = c2.calibrate(f.reshape((8, 4, -1)).mean(dim=1), e.reshape((8, 4, -1)).mean(dim=1), fast_images=f, exact_images=e)
    assert c2.bias is None
    assert st["image_residual_rms"] == pytest.approx(float(((f - e).norm(dim=1) / e.norm(dim=1)).pow(2).mean().sqrt()), rel=1e-6)


def _assert_same_state(a: Certainty, b: Certainty):
    for k in ("bias", "drift"):
        va, vb = getattr(a, k), getattr(b, k)
        assert (va is None) == (vb is None)
        if va is not None:
            assert vb.dtype == torch.float32 and torch.equal(va.cpu(), vb.cpu())
    for k in ("rel_tol", "rel_tol_exact", "kappa", "debias", "force_exact", "calibrated"):
        assert getattr(a, k) == getattr(b, k) and type(getattr(a, k)) is type(getattr(b, k)), k
    assert a.stats == b.stats
    assert a.threshold() == b.threshold() and a.threshold(True) == b.threshold(True)


def test_certainty_save_load_round_trip(tmp_path):
    c, _, _ = _measured()
    c.kappa = 4.25
    path = str(tmp_path / "sub" / "cal.npz")
    meta = {"layers": 24, "mma_dtype": "f16", "ln_fold": True, "source": "unit test, 10 samples"}
    assert c.save(path, FP_A, 4, meta) == path
    assert os.listdir(os.path.dirname(path)) == ["cal.npz"]                            # the temporary name is gone
    with np.load(path, allow_pickle=False) as z:                                       # no pickled member
        assert all(z[k].dtype != object for k in z.files)
    sd, header = Certainty.load(path)
    assert header == {"format_version": FORMAT_VERSION, "fingerprint": FP_A, "layers": 24, "mma_dtype": "f16", "ln_fold": True, "panels": 4,
                      "samples": 10, "source": "unit test, 10 samples"}
    d = Certainty(kappa=1.0, rel_tol=0.5, debias=False)
    d.load_state_dict(sd)
    _assert_same_state(c, d)
    # the in-memory form round-trips too, and a drift vector / no vectors / force_exact survive
    e = Certainty(debias=False)
    e.drift, e.calibrated, e.force_exact, e.rel_tol, e.stats = torch.arange(1024, dtype=torch.float32) * 1e-7, True, True, 3e-4, {"samples": 9}
    e.save(path, FP_B, 1, {})
    f = Certainty()
    f.load_state_dict(Certainty.load(path)[0])
    _assert_same_state(e, f)
    with pytest.raises(CalibrationError):
        Certainty().save(str(tmp_path / "never.npz"), FP_A, 4, meta)                   # nothing measured: nothing to save
    assert not os.path.exists(str(tmp_path / "never.npz"))


# ------------------------------------------------------------------------------------------------ the objects
class _Tower(HipCLIPVisionModel):
    """A tower whose fingerprint is scripted (the real one is taken on the device)."""

    def __init__(self, fp):
        super().__init__({"encoder.layers.0.layer_norm1.weight": torch.ones(4)})
        self.fp = fp

    def fingerprint(self):
        return self.fp


@pytest.fixture(scope="module")
def geocells(tmp_path_factory):
    p = str(tmp_path_factory.mktemp("cal") / "geocells.csv")
    synthetic.write_geocell_csv(p, synthetic.make_geocells(40, seed=0))
    return p


def _model(geocells, fp=FP_A, panorama=True, **kw):
    return SuperGuessr(_Tower(fp) if fp else None, panorama=panorama, freeze_base=True, geocell_path=geocells, **kw)


def _file(tmp_path, name="cal.npz", fp=FP_A, panels=4, c=None, **meta):
    c = c or _measured()[0]
    m = {"layers": 1, "mma_dtype": "f16", "ln_fold": True, "source": "scripted"}
    m.update(meta)
    return c.save(str(tmp_path / name), fp, panels, m), c


def _snapshot(m):
    return (id(m.certainty), repr(sorted((k, v.tolist() if torch.is_tensor(v) else v) for k, v in m.certainty.state_dict().items())),
            m.calibration_header, m.embedding_rel_tol, len(m._cal_buffer))


def test_super_guessr_loads_and_load_state_drops(geocells, tmp_path):
    path, c = _file(tmp_path)
    m = _model(geocells, margin_kappa=2.0)
    assert not m.certainty.calibrated and m.calibration_header is None
    header = m.load_calibration(path)
    assert header["fingerprint"] == FP_A and m.calibration_header == header
    _assert_same_state(c, m.certainty)
    m2 = _model(geocells, calibration=path)                                            # the constructor keyword
    _assert_same_state(c, m2.certainty)
    # a weight load voids it, loaded or measured: back to the constructor's values
    ck = str(tmp_path / "head.model")
    torch.save({"cell_layer.bias": torch.zeros(m.num_cells)}, ck)
    m.load_state(ck)
    assert not m.certainty.calibrated and m.certainty.bias is None and m.calibration_header is None
    assert m.certainty.rel_tol == 1e-3 and m.certainty.kappa == c.kappa                # (kappa is a parameter, not a measurement)
    m.load_calibration(path)                                                           # ... and the caller loads it again after the weights
    _assert_same_state(c, m.certainty)
    # save_calibration writes what load_calibration reads (fingerprint and panels from the object)
    out = m.save_calibration(str(tmp_path / "again.npz"))
    sd, h2 = Certainty.load(out)
    assert h2["fingerprint"] == FP_A and h2["panels"] == 4 and torch.equal(sd["bias"], c.bias)
    with pytest.raises(CalibrationError):
        _model(geocells).save_calibration(str(tmp_path / "no.npz"))                    # not calibrated


def test_refusals_leave_the_object_unchanged(geocells, tmp_path):
    good, c = _file(tmp_path)
    for loaded_first in (False, True):
        m = _model(geocells)
        if loaded_first:
            m.load_calibration(good)
        before = _snapshot(m)

        def refused(path, *needles):
            with pytest.raises(CalibrationError) as ei:
                m.load_calibration(path)
            for s in needles:
                assert s in str(ei.value), (s, str(ei.value))
            assert _snapshot(m) == before

        # other weights: both fingerprints are named
        refused(_file(tmp_path, "other.npz", fp=FP_B, c=c)[0], FP_A, FP_B)
        # measured on single images, loaded into a panorama model
        refused(_file(tmp_path, "p1.npz", panels=1, c=c)[0], "panels")
        # a later format
        with np.load(good, allow_pickle=False) as z:
            arrays = {k: z[k] for k in z.files}
        arrays["format_version"] = np.int64(FORMAT_VERSION + 1)
        v2 = str(tmp_path / "v2.npz")
        np.savez(v2, **arrays)
        refused(v2, "format_version", str(FORMAT_VERSION + 1))
        # cut short
        raw = open(good, "rb").read()
        for keep in (len(raw) // 2, 10):
            cut = str(tmp_path / f"cut{keep}.npz")
            open(cut, "wb").write(raw[:keep])
            refused(cut, "cannot be read")
        # a member that could only be read by unpickling
        arrays["format_version"] = np.int64(FORMAT_VERSION)
        arrays["stats_json"] = np.array([{"samples": 8}], dtype=object)
        pk = str(tmp_path / "pickled.npz")
        np.savez(pk, **arrays)
        refused(pk, "cannot be read")
        # a member missing
        del arrays["stats_json"]
        ms = str(tmp_path / "missing.npz")
        np.savez(ms, **arrays)
        refused(ms, "cannot be read")
        # a vector of the wrong length
        arrays["stats_json"] = np.str_("{}")
        arrays["bias"] = np.zeros(1000, dtype=np.float32)
        bad = str(tmp_path / "badbias.npz")
        np.savez(bad, **arrays)
        refused(bad, "bias")
        with pytest.raises(FileNotFoundError):
            m.load_calibration(str(tmp_path / "absent.npz"))
        assert _snapshot(m) == before
    with pytest.raises(CalibrationError):
        _model(geocells, calibration=_file(tmp_path, "ctor.npz", fp=FP_B, c=c)[0])     # the constructor keyword refuses the same way


def test_precomputed_embeddings_take_their_tolerance_from_the_file(geocells, tmp_path):
    path, c = _file(tmp_path, fp=FP_B, panels=1)                                       # any fingerprint, any panels: no encoder to compare with
    resid = c.stats["image_residual_rms"]
    m = _model(geocells, fp=None, embedding_rel_tol=5e-6)                              # the caller DECLARES exact embeddings
    assert m.embedding_rel_tol == 5e-6                                                 # ... and is taken at their word: the exact tier's floor
    m.load_calibration(path)
    assert m.embedding_rel_tol == 1.1 * c.stats["image_residual_rms"] and m.embedding_rel_tol > 5e-6
    assert not m.certainty.calibrated and m.certainty.bias is None                     # nothing else moves: there is no fast path here
    c.force_exact = True                                                               # embeddings written by the exact encoder
    fx = c.save(str(tmp_path / "fx.npz"), FP_B, 1, {})
    m2 = _model(geocells, fp=None, calibration=fx)
    assert m2.embedding_rel_tol == m2.certainty.rel_tol_exact == 5e-6
    # ... and a file without the statistic cannot set it
    c.force_exact = False
    del c.stats["image_residual_rms"]
    old = c.save(str(tmp_path / "old.npz"), FP_B, 1, {})
    before = m.embedding_rel_tol
    with pytest.raises(CalibrationError):
        m.load_calibration(old)
    assert m.embedding_rel_tol == before
    # a weight load gives the constructor's tolerance back
    ck = str(tmp_path / "head.model")
    torch.save({"cell_layer.bias": torch.zeros(m.num_cells)}, ck)
    m.load_state(ck)
    assert m.embedding_rel_tol == 5e-6 and m.calibration_header is None
    # without a declaration: the fast path's tolerance at the time of the call (embeddings written by the 16-bit encoder) -- the
    # constructor's uncalibrated one, whatever `certainty.rel_tol` becomes, the file's while one is loaded, and back after a weight load
    d = _model(geocells, fp=None)
    assert d.embedding_rel_tol == d.certainty.rel_tol == 1e-3
    assert _model(geocells, fp=None, margin_rel_tol=4e-4).embedding_rel_tol == 4e-4
    d.certainty.rel_tol = 7e-5
    assert d.embedding_rel_tol == 7e-5
    d.certainty.rel_tol = 1e-3
    d.load_calibration(path)
    assert d.embedding_rel_tol == 1.1 * resid and d.certainty.rel_tol == 1e-3
    d.load_state(ck)
    assert d.embedding_rel_tol == 1e-3 and d.calibration_header is None
    d.certainty.rel_tol = 7e-5
    assert d.embedding_rel_tol == 7e-5                                                 # (restored to "no explicit value", not to a number)
    # an explicit value survives the same round trip, and wins over the fast path's
    x = _model(geocells, fp=None, embedding_rel_tol=2e-4, margin_rel_tol=4e-4)
    assert x.embedding_rel_tol == 2e-4
    x.load_calibration(path)
    x.load_state(ck)
    assert x.embedding_rel_tol == 2e-4
    # with a tower: the calibrated tolerance once there is one
    t = _model(geocells)
    assert t.embedding_rel_tol == 1e-3
    t.load_calibration(_file(tmp_path, "tower.npz", c=c)[0])
    assert t.embedding_rel_tol == t.certainty.rel_tol == c.rel_tol


def test_clip_embedding_takes_the_same_vector(geocells, tmp_path):
    path, c = _file(tmp_path)                                                          # measured on panoramas: accepted, the bias is per image
    e = CLIPEmbedding("unused", device="cpu", clip_model=_Tower(FP_A), calibration=path)
    m = _model(geocells, calibration=path)
    assert torch.equal(e.bias, m.certainty.bias) and torch.equal(e.bias, c.bias)
    assert e.force_exact is False and e.guard_stats is not None and e.guard_stats["from_file"] == path
    assert e.guard_stats["debias"] is True and e.guard_stats["outside"] is False
    # refused before anything changes
    f = CLIPEmbedding("unused", device="cpu", clip_model=_Tower(FP_B))
    with pytest.raises(CalibrationError) as ei:
        f.load_calibration(path)
    assert FP_A in str(ei.value) and FP_B in str(ei.value)
    assert f.bias is None and f.guard_stats is None and f.force_exact is False and f.calibration_header is None
    # force_exact from a file; with contract_guard='raise' it raises as the measurement would
    c.force_exact = True
    fx = c.save(str(tmp_path / "fx.npz"), FP_A, 4, {})
    assert CLIPEmbedding("unused", device="cpu", clip_model=_Tower(FP_A), calibration=fx).force_exact is True
    with pytest.raises(RuntimeError):
        CLIPEmbedding("unused", device="cpu", clip_model=_Tower(FP_A), contract_guard="raise", calibration=fx)
    # what it saves, it loads: panels 1, the same vector
    out = e.save_calibration(str(tmp_path / "emb.npz"))
    sd, h = Certainty.load(out)
    assert h["panels"] == 1 and h["fingerprint"] == FP_A and torch.equal(sd["bias"], c.bias)
    assert sd["stats"]["image_residual_rms"] == c.stats["image_residual_rms"]
    with pytest.raises(CalibrationError):
        CLIPEmbedding("unused", device="cpu", clip_model=_Tower(FP_A)).save_calibration(str(tmp_path / "none.npz"))


# ------------------------------------------------------------------------------------------------ the embedder's judgement
_CASES = ((32, 3e-4), (32, 1e-6), (9, 3e-4), (7, 3e-4), (1, 3e-4))        # (images, scale of the systematic part); a bias is kept in 0 and 2
# What `CLIPEmbedding.save_calibration` wrote for the five cases BEFORE the embedder held a `Certainty` (commit 070f2c5, the same draws
# through `_check_contract` on the CPU with `_to_device_pixels` patched to the identity): sum of the bias in fp64 (None: no vector),
# force_exact, rel_tol, stats['image_residual_rms'].  Cases 1, 3, 4 take both figures from `image_rel_err`, not from `calibrate`.
_PARENT_ROWS = ((-0.0002794648283028778, False, 5.642319847538602e-05, 5.129381679580547e-05),
                (None, False, 5.506579982466065e-05, 5.005981802241877e-05),
                (0.000738847422000255, False, 6.034937759977766e-05, 5.486307054525241e-05),
                (None, False, 0.0003260129655245692, 0.0002963754232041538),
                (None, False, 0.0003382560011232272, 0.00030750545556657016))


@pytest.fixture(scope="module")
def judged():
    """The five scripted (fast, exact) pairs, each through a fresh embedder's judgement -> [(embedder, fast, exact)]."""
    torch.manual_seed(0)
    out = []
    for n, scale in _CASES:
        exact = torch.randn(n, 1024)
        beta = torch.randn(1024) / 32 * scale
        fast = exact + exact.norm(dim=1, keepdim=True) * (beta + torch.randn(n, 1024) / 32 * 5e-5)
        e = CLIPEmbedding("unused", device="cpu", clip_model=_Tower(FP_A), contract_guard="exact")
        assert e.certainty.debias and e.guard_stats is None and e.bias is None and e.force_exact is False
        e._judge(fast, exact)
        out.append((e, fast, exact))
    return out


def _restated(fast, exact):
    """The guard's arithmetic for one image per sample, in independent torch expressions -> (bias or None, expected guard_stats)."""
    n = fast.shape[0]
    err = (fast - exact).norm(dim=1) / exact.norm(dim=1)
    st = {"images": n, "image_rel_err": float((fast - exact).norm() / exact.norm()), "worst_image_rel_err": float(err.max()), "contract": 1e-3}
    bias = None
    if n >= 8:
        rel = (fast - exact) / exact.norm(dim=1, keepdim=True)
        held = fast[1::2] - fast[1::2].norm(dim=1, keepdim=True) * rel[0::2].mean(dim=0)          # what pg_embedding_debias would return
        left = float(((held - exact[1::2]).norm(dim=1) / exact[1::2].norm(dim=1)).pow(2).mean().sqrt())
        st["bias_norm"], st["residual_rms"] = float(rel.mean(dim=0).norm()), left
        if left < 0.9 * float(err.pow(2).mean().sqrt()):
            bias = rel.mean(dim=0)
    st["debias"] = bias is not None
    st["outside"] = st["image_rel_err"] > 0.85e-3 or st["worst_image_rel_err"] > 0.95e-3
    return bias, st


def test_embedder_judgement_is_certainty_calibrate(judged):
    kept = []
    for (e, fast, exact), (n, _) in zip(judged, _CASES):
        bias, want = _restated(fast, exact)
        kept.append(bias is not None)
        assert (e.bias is None) == (bias is None) and (bias is None or torch.equal(e.bias, bias)), n
        assert e.guard_stats == want, n                               # every figure with ==, and exactly these keys
        assert ("bias_norm" in e.guard_stats) == ("residual_rms" in e.guard_stats) == (n >= 8)
        assert e.force_exact is False and e.calibration_header is None
        # the same object is what `Certainty.calibrate` leaves behind
        c = Certainty(debias=True)
        cs = c.calibrate(fast, exact, fast_images=fast, exact_images=exact)
        assert (c.bias is None) == (bias is None) and (bias is None or torch.equal(c.bias, bias)) and c.force_exact is e.force_exact
        assert cs["image_rel_err"] == want["image_rel_err"] and cs["worst_image_rel_err"] == want["worst_image_rel_err"]
        assert e.certainty.bias is e.bias and e.certainty.bias_on(torch.device("cpu")) is e.bias
    assert kept == [True, False, True, False, False]
    # outside the contract: the verdict, and what 'raise' does with it
    exact = judged[0][2]
    fast = exact * (1 + 9e-4)
    out = CLIPEmbedding("unused", device="cpu", clip_model=_Tower(FP_A), contract_guard="exact")
    assert out._judge(fast, exact)["outside"] is True and out.force_exact is True and out.guard_stats["outside"] is True
    strict = CLIPEmbedding("unused", device="cpu", clip_model=_Tower(FP_A), contract_guard="raise")
    with pytest.raises(RuntimeError, match="outside the 1e-3 embedding contract"):
        strict._judge(fast, exact)
    assert strict.guard_stats["outside"] is True and strict.force_exact is False


def test_rank_combination():
    from pigeon_amd.certainty import combine_ranks, outside_contract
    g = torch.Generator().manual_seed(4)
    v = [torch.randn(1024, generator=g) * 1e-5 for _ in range(3)]
    overall, worst, bias = combine_ranks([(3e-4, 9.6e-4, v[0]), (5e-4, 4e-4, v[1]), (2e-4, 3e-4, v[2])])
    assert (overall, worst) == (5e-4, 9.6e-4) and torch.equal(bias, torch.stack(v).mean(dim=0))
    assert outside_contract(overall, worst) and not outside_contract(5e-4, 4e-4) and outside_contract(8.6e-4, 4e-4)
    for missing in range(3):                                          # one rank kept none: none for the job
        every = [(1e-4, 2e-4, None if r == missing else v[r]) for r in range(3)]
        assert combine_ranks(every) == (1e-4, 2e-4, None)
    assert combine_ranks([(1e-4, 2e-4, None)] * 3)[2] is None


def test_embedder_saves_what_it_always_saved(judged, tmp_path):
    for i, ((e, fast, exact), row) in enumerate(zip(judged, _PARENT_ROWS)):
        bias, st = _restated(fast, exact)
        sd, h = Certainty.load(e.save_calibration(str(tmp_path / f"c{i}.npz")))
        assert h["panels"] == 1 and h["samples"] == fast.shape[0] and h["fingerprint"] == FP_A
        assert (sd["bias"] is None) == (bias is None) and (bias is None or torch.equal(sd["bias"], bias)) and sd["drift"] is None
        # the embedder's own rule, with ==: the held-out residual after a kept bias, else the whole batch's raw error
        resid = st["residual_rms"] if bias is not None else st["image_rel_err"]
        assert sd["stats"]["image_residual_rms"] == resid and sd["rel_tol"] == max(1.1 * resid, 1e-5) and sd["force_exact"] is False
        # ... and the recorded rows (approx: a sum over 32k elements may be split differently on another machine; the two rules differ by 2 %)
        got = (None if sd["bias"] is None else float(sd["bias"].double().sum()), sd["force_exact"], sd["rel_tol"], sd["stats"]["image_residual_rms"])
        assert got == pytest.approx(row, rel=1e-6), i
        # every member of the file's statistics: the guard's scalars and the six the file adds
        assert sd["stats"] == dict(st, samples=st["images"], image_residual_rms=resid, rel_tol=sd["rel_tol"], kappa=3.6, force_exact=False)
        assert e.save_calibration(str(tmp_path / "again.npz")) and Certainty.load(str(tmp_path / "again.npz"))[0]["stats"] == sd["stats"]


# ------------------------------------------------------------------------------------------------ command lines
def test_command_lines_accept_calibration(tmp_path, monkeypatch, capsys):
    import importlib
    monkeypatch.setattr(sys, "argv", ["run.py", "embed", "random"])
    sys.path.insert(0, ROOT)
    import run
    importlib.reload(run)
    for fn in ("embed", "evaluate"):
        a = run.argp.parse_args([fn, "random", "--synthetic", "8", "--calibration", "cal.npz"])
        assert a.calibration == "cal.npz"
    assert run.argp.parse_args(["embed", "random"]).calibration is None
    assert "rank 0" in run.argp.format_help()                                          # who writes the file in a multi-rank job
    from pigeon_amd import calibrate, serve
    assert serve._arg_parser().parse_args(["--calibration", "cal.npz"]).calibration == "cal.npz"
    assert serve._arg_parser().parse_args([]).calibration is None
    with pytest.raises(SystemExit) as ei:                                              # load only: the file must exist
        serve.main(["--calibration", str(tmp_path / "absent.npz")])
    assert ei.value.code != 0 and "absent.npz" in capsys.readouterr().err
    a = calibrate._arg_parser().parse_args(["--base", "random", "--layers", "2", "--synthetic", "8", "--seed", "3", "-o", "f.npz"])
    assert (a.base, a.layers, a.synthetic, a.seed, a.panels, a.output) == ("random", 2, 8, 3, 4, "f.npz")
    with pytest.raises(SystemExit):
        calibrate._arg_parser().parse_args(["--base", "random", "--synthetic", "8", "--images", "d", "-o", "f.npz"])
    import inspect
    from pigeon_amd.evaluate import evaluate
    assert inspect.signature(evaluate).parameters["calibration"].default is None
    # precomputed embeddings: the error they carry can be declared on both surfaces (default: the 16-bit path's)
    assert inspect.signature(evaluate).parameters["embedding_rel_tol"].default is None
    assert run.argp.parse_args(["evaluate", "head.model"]).embedding_rel_tol is None
    assert run.argp.parse_args(["evaluate", "head.model", "--embedding-rel-tol", "5e-6"]).embedding_rel_tol == 5e-6
