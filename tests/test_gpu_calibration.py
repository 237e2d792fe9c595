"""The encoder calibration as a file keyed by a weight fingerprint, on the device (run with -m gpu on an MI355X):

  * pg_fingerprint against its numpy restatement (tests/_fpref.py), equal as integers;
  * pg_vit_fingerprint: equal for the same weights (with and without the exact tier's copy), different for any changed weight,
    operand format or LayerNorm fold;
  * with a calibration file, `SuperGuessr` and `CLIPEmbedding` subtract the file's vector -- the same one -- and two objects whose
    first batches differ return the same bits; without one they do not (the contrast that gives the rest its meaning);
  * refusals, the reset by `load_state`, `force_exact` from a file, and `run.py embed|evaluate --calibration`.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _fpref

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIB = 1 << 20


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops, synthetic
    _lib.require_gpu()
    return dict(lib=_lib, ops=hip_ops, syn=synthetic)


# ------------------------------------------------------------------------------------------------ 1. pg_fingerprint
@pytest.fixture(scope="module")
def blob():
    """17 MiB of seeded bytes, on the device and on the host (one reference array for every size below)."""
    g = torch.Generator().manual_seed(7)
    host = torch.randint(0, 256, (17 * MIB,), dtype=torch.uint8, generator=g)
    return host.to(DEV), host.numpy()


# 65 540 and 3 MiB + 20: several blocks and the grid-stride loop; 16 MiB + 52: more full chunks than 1024 blocks x 256 lanes x 4 take
# in a block count that is not capped (the cap on the blocks per buffer)
@pytest.mark.parametrize("nbytes", [0, 1, 15, 16, 17, 4096, 65540, 3 * MIB + 20, 16 * MIB + 52])
def test_fingerprint_equals_restatement(env, blob, nbytes):
    dev, host = blob
    for seed in (0, 2 ** 63 + 5):
        got = env["ops"].fingerprint(dev[:nbytes], seed)
        assert got == _fpref.fingerprint(host[:nbytes], seed), (nbytes, seed)
        assert env["ops"].fingerprint(dev[:nbytes], seed) == got                       # twice: the same value
    # a 16-byte-aligned view into the larger tensor
    off = 48
    n = min(nbytes, host.size - off)
    assert env["ops"].fingerprint(dev[off:off + n], 3) == _fpref.fingerprint(host[off:off + n], 3)


def test_fingerprint_other_dtypes_and_refused_alignment(env, blob):
    dev, host = blob
    ops, lib = env["ops"], env["lib"]
    w = torch.randn((1000, 33), generator=torch.Generator().manual_seed(1)).to(DEV)
    assert ops.fingerprint(w, 5) == _fpref.fingerprint(w.cpu().numpy(), 5)             # the tensor's bytes, whatever its dtype
    h = w.half()
    assert ops.fingerprint(h) == _fpref.fingerprint(h.cpu().numpy()) != ops.fingerprint(w)
    # a pointer 4 bytes off a 16-byte boundary: refused with a named error before any launch, `out` untouched
    view = dev[4:4 + 4096]
    assert view.data_ptr() % 16 == 4
    with pytest.raises(lib.PigeonHipError, match="16-byte aligned"):
        ops.fingerprint(view)
    out = (C.c_uint64 * 2)(0x1111111111111111, 0x2222222222222222)
    rc = lib.load().pg_fingerprint(C.c_void_p(view.data_ptr()), 4096, C.c_uint64(0), out, C.c_void_p(0))
    assert rc == -1 and b"16-byte aligned" in lib.load().pg_last_error()
    assert (out[0], out[1]) == (0x1111111111111111, 0x2222222222222222)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. pg_vit_fingerprint
@pytest.fixture(scope="module")
def sd2(env):
    return env["syn"].make_vit_weights(seed=11, layers=2, affine_jitter=True)


def _vit_fp(env, sd, **kw):
    enc = env["ops"].VitEncoder(sd, layers=2, **kw)
    try:
        return enc.fingerprint()
    finally:
        enc.close()


def test_vit_fingerprint(env, sd2):
    base = _vit_fp(env, sd2)
    assert all(0 <= v < 2 ** 64 for v in base)
    assert _vit_fp(env, {k: v.clone() for k, v in sd2.items()}) == base                # the same weights packed again
    assert _vit_fp(env, sd2, precise=True) == base                                     # the exact tier's copy is not part of it
    seen = {base}

    def changed(edit, **kw):
        sd = {k: v.clone() for k, v in sd2.items()}
        edit(sd)
        fp = _vit_fp(env, sd, **kw)
        assert fp not in seen
        seen.add(fp)

    def one_element(sd):
        sd["encoder.layers.1.mlp.fc2.weight"][123, 456] += 1e-2

    def swap_two(sd):
        w = sd["encoder.layers.0.self_attn.out_proj.weight"]
        a, b = float(w[3, 5]), float(w[700, 900])
        assert a != b
        w[3, 5], w[700, 900] = b, a

    def one_bias(sd):
        sd["encoder.layers.1.mlp.fc1.bias"][77] += 1e-2

    def one_position(sd):
        sd["embeddings.position_embedding.weight"][576, 1023] += 1e-2

    for edit in (one_element, swap_two, one_bias, one_position):
        changed(edit)
    changed(lambda sd: None, mma_dtype="bf16")                                         # the same weights in the other operand format


def test_vit_fingerprint_depends_on_the_layernorm_fold(env, sd2, tmp_path):
    """PIGEON_LN_FOLD is read when the handle is created, once per process for the GEMM planner: a fresh child process each."""
    script = os.path.join(str(tmp_path), "fp.py")
    with open(script, "w") as f:
        f.write("import sys\nsys.path.insert(0, %r)\nfrom pigeon_amd import hip_ops, synthetic\n"
                "enc = hip_ops.VitEncoder(synthetic.make_vit_weights(seed=11, layers=2, affine_jitter=True), layers=2)\n"
                "print('FP %%016x%%016x' %% enc.fingerprint())\nenc.close()\n" % ROOT)
    got = {}
    for fold in ("1", "0"):
        r = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=300, env=dict(os.environ, PIGEON_LN_FOLD=fold))
        assert r.returncode == 0, r.stderr[-2000:]
        got[fold] = [l for l in r.stdout.splitlines() if l.startswith("FP ")][0][3:]
    assert got["1"] == "%016x%016x" % _vit_fp(env, sd2)                                # another process, the same value
    assert got["0"] != got["1"]


# ------------------------------------------------------------------------------------------------ 3. the file's vector is what is subtracted
C_CELLS = 60


@pytest.fixture(scope="module")
def geocells(env, tmp_path_factory):
    p = str(tmp_path_factory.mktemp("gpu_cal") / "geocells.csv")
    env["syn"].write_geocell_csv(p, env["syn"].make_geocells(C_CELLS, seed=0))
    return p


@pytest.fixture(scope="module")
def vit2(sd2):
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    return HipCLIPVisionModel(sd2, layers=2).to(DEV)


def _guessr(env, vit, geocells, **kw):
    from pigeon_amd.super_guessr import SuperGuessr
    m = SuperGuessr(vit, panorama=True, freeze_base=True, num_candidates=5, geocell_path=geocells, **kw)
    W, b = env["syn"].make_head_weights(C_CELLS, seed=1)
    with torch.no_grad():
        m.cell_layer.weight.copy_(W * 64); m.cell_layer.bias.copy_(b)
    return m.to(DEV).eval()


def _scripted_file(path, vit, bias=None, force_exact=False, panels=4, rel_tol=6e-5):
    from pigeon_amd.certainty import Certainty
    c = Certainty()
    c.bias, c.force_exact, c.rel_tol, c.calibrated = bias, force_exact, rel_tol, True
    c.stats = {"samples": 8, "image_residual_rms": 5e-5, "debias": bias is not None}
    return c.save(str(path), vit.fingerprint(), panels, dict(vit.encoder_config(), source="scripted"))


def test_both_paths_subtract_the_files_vector(env, vit2, geocells, tmp_path):
    from pigeon_amd.clip_embedder import CLIPEmbedding
    ops, syn = env["ops"], env["syn"]
    bias = 1e-3 * torch.randn((1024,), generator=torch.Generator().manual_seed(5))
    path = _scripted_file(tmp_path / "known.npz", vit2, bias)
    px = syn.make_pixels(4 * 3, seed=3, panorama=True).to(DEV)                          # 3 panoramas
    flat = px.reshape(-1, 3, 336, 336)
    raw = vit2.embed(flat)
    want = ops.embedding_debias(raw.clone(), bias.to(DEV))
    assert not torch.equal(want, raw)
    m = _guessr(env, vit2, geocells, exact_top1=False)
    m.load_calibration(path)
    out = m(pixel_values=px)
    assert torch.equal(out.embedding, want.reshape(3, 4, 1024))                         # the query path
    e = CLIPEmbedding("unused", device=DEV, clip_model=vit2, calibration=path)
    assert torch.equal(e(flat), want)                                                   # the embed path: the same rows
    assert e.guard_stats["from_file"] == path                                           # ... and its first forward measured nothing
    assert torch.equal(_guessr(env, vit2, geocells, exact_top1=False, calibration=path)(pixel_values=px).embedding, out.embedding)


def test_embedder_guard_is_certainty_calibrate(env, geocells, tmp_path):
    """The guard of `CLIPEmbedding` at its default, on a 2-layer tower and 16 images (the smallest shape with an even / odd split of 8
    images or more and a bias to subtract): what its first forward measures is what `Certainty.calibrate` measures on the same two
    encoders; the file it saves sets a precomputed-embedding model's tolerance; a second embedder given the file measures nothing
    and returns the same bits."""
    from pigeon_amd.certainty import SAFETY, Certainty
    from pigeon_amd.clip_embedder import CLIPEmbedding, HipCLIPVisionModel
    from pigeon_amd.super_guessr import SuperGuessr
    vit = HipCLIPVisionModel(seed=5, layers=2).to(DEV)
    px = env["syn"].make_pixels(16, seed=21).to(DEV)
    e = CLIPEmbedding("unused", device=DEV, clip_model=vit)
    first = e(px)
    st = e.guard_stats
    assert st["images"] == 16 and "bias_norm" in st and "residual_rms" in st and "from_file" not in st
    fast, exact = vit.embed(px), vit.embed_precise(px)
    c = Certainty(debias=True)
    cs = c.calibrate(fast, exact, fast_images=fast, exact_images=exact)
    assert (c.bias is None) == (e.bias is None) and (c.bias is None or torch.equal(c.bias, e.bias))
    assert c.force_exact is e.force_exact and cs["image_rel_err"] == st["image_rel_err"] and st["debias"] == (e.bias is not None)
    print(f"   guard on the 2-layer tower: {st}")
    assert not e.force_exact                                                            # (this tower is inside the contract)
    assert torch.equal(first, fast if e.bias is None else env["ops"].embedding_debias(fast.clone(), e.bias))
    path = e.save_calibration(str(tmp_path / "e.npz"))
    resid = Certainty.load(path)[0]["stats"]["image_residual_rms"]
    m = SuperGuessr(None, panorama=False, freeze_base=True, geocell_path=geocells, calibration=path)
    assert SAFETY == 1.1 and m.embedding_rel_tol == 1.1 * resid and resid > 0
    e2 = CLIPEmbedding("unused", device=DEV, clip_model=vit, calibration=path)
    assert torch.equal(e2(px), first) and e2.guard_stats["from_file"] == path and (e2.bias is None) == (e.bias is None)


# ------------------------------------------------------------------------------------------------ 4. two objects, one file, the same bits
@pytest.fixture(scope="module")
def vit24(env):
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    m = HipCLIPVisionModel(env["syn"].make_vit_weights(seed=0, layers=24), layers=24).to(DEV)
    m.enable_precise(True)
    return m


def test_file_makes_embeddings_reproducible(env, vit24, geocells, tmp_path):
    """The 24-layer default tower keeps a bias (2.5e-4 of 2.6e-4).  Three objects on the same weights: A calibrates on 8 panoramas, B's
    first batch is another 8, C's a single one.  Left to themselves they do not return the same embeddings of one probe batch; with A's
    file they return the same bits, and the same certainty verdicts."""
    syn = env["syn"]
    cal_px = syn.make_pixels(4 * 8, seed=100, panorama=True).to(DEV)
    first_b = syn.make_pixels(4 * 8, seed=200, panorama=True).to(DEV)
    first_c = syn.make_pixels(4 * 1, seed=300, panorama=True).to(DEV)
    probe = syn.make_pixels(4 * 4, seed=400, panorama=True).to(DEV)
    a = _guessr(env, vit24, geocells, exact_top1=True)
    a.calibrate_certainty(cal_px)
    assert a.certainty.bias is not None and not a.certainty.force_exact
    path = a.save_calibration(str(tmp_path / "a.npz"))

    # without a file: the fast pass's embeddings (`encode_head`: before the exact tier replaces rows -- with the same bits everywhere)
    def fast_embedding(m, first):
        if first is not None:
            m(pixel_values=first)
        return m.encode_head(pixel_values=probe)["embedding"].clone()
    b0, c0 = _guessr(env, vit24, geocells, exact_top1=True), _guessr(env, vit24, geocells, exact_top1=True)
    ea, eb, ec = fast_embedding(a, None), fast_embedding(b0, first_b), fast_embedding(c0, first_c)
    assert b0.certainty.calibrated and not c0.certainty.calibrated                      # 8 panoramas calibrate at once, one does not
    assert not (torch.equal(ea, eb) and torch.equal(ea, ec))

    # with A's file
    def loaded(first, exact_top1):
        m = _guessr(env, vit24, geocells, exact_top1=exact_top1)
        m.load_calibration(path)
        o1 = m(pixel_values=first)
        return m, o1, m(pixel_values=probe)
    want = a.encode_head(pixel_values=probe)["embedding"]
    outs = []
    for first in (first_b, first_c):
        m, o1, o = loaded(first, exact_top1=False)
        assert torch.equal(o.embedding, want)
        outs.append(o)
        if first is first_c:                                                            # de-biased on its very first, single-panorama call
            raw = vit24.embed(first_c.reshape(-1, 3, 336, 336))
            deb = env["ops"].embedding_debias(raw.clone(), a.certainty.bias_on(raw.device))
            assert torch.equal(o1.embedding, deb.reshape(1, 4, 1024)) and not torch.equal(deb, raw)
    assert torch.equal(outs[0].embedding, outs[1].embedding) and torch.equal(outs[0].preds_geocell, outs[1].preds_geocell)
    verdicts = []
    for first in (first_b, first_c):
        m, _, o = loaded(first, exact_top1=True)
        assert m.certainty.stats == a.certainty.stats and m.certainty.rel_tol == a.certainty.rel_tol
        verdicts.append((m.last_tol.clone(), m.last_certain.clone(), m.last_reencoded.clone(), o.embedding.clone()))
    for x, y in zip(*verdicts):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 5. refusal and reset
def test_refused_on_other_weights_and_dropped_by_load_state(env, sd2, vit2, geocells, tmp_path):
    """(On the 2-layer tower: what is refused is a fingerprint, whatever the depth.)"""
    from pigeon_amd.certainty import CalibrationError
    from pigeon_amd.clip_embedder import HipCLIPVisionModel
    path = _scripted_file(tmp_path / "a.npz", vit2, 1e-3 * torch.randn((1024,), generator=torch.Generator().manual_seed(5)))
    sd = {k: v.clone() for k, v in sd2.items()}
    sd["encoder.layers.0.self_attn.q_proj.weight"][10, 10] += 1e-2                     # one weight
    other = HipCLIPVisionModel(sd, layers=2).to(DEV)
    m = _guessr(env, other, geocells, exact_top1=True)
    with pytest.raises(CalibrationError) as ei:
        m.load_calibration(path)
    assert vit2.fingerprint() in str(ei.value) and other.fingerprint() in str(ei.value) and vit2.fingerprint() != other.fingerprint()
    assert not m.certainty.calibrated and m.certainty.bias is None and m.calibration_header is None
    # load_state drops a loaded calibration like a measured one
    ok = _guessr(env, vit2, geocells, exact_top1=True)
    ok.load_calibration(path)
    assert ok.certainty.calibrated and ok.certainty.bias is not None
    ck = os.path.join(str(tmp_path), "head.model")
    torch.save({"cell_layer.bias": ok.cell_layer.bias.data.cpu()}, ck)
    ok.load_state(ck)
    assert not ok.certainty.calibrated and ok.certainty.bias is None and ok.calibration_header is None and ok.certainty.rel_tol == 1e-3
    ok.load_calibration(path)                                                          # weights, then calibration
    assert ok.certainty.calibrated


# ------------------------------------------------------------------------------------------------ 6. force_exact from a file
def test_force_exact_from_a_file(env, vit2, geocells, tmp_path):
    path = _scripted_file(tmp_path / "fx.npz", vit2, None, force_exact=True)
    px = env["syn"].make_pixels(4 * 3, seed=3, panorama=True).to(DEV)
    m = _guessr(env, vit2, geocells, exact_top1=True)
    m.load_calibration(path)
    stats = dict(m.certainty.stats)
    out = m(pixel_values=px)
    assert bool(m.last_state["exact"].all()) and m.last_reencoded.tolist() == [0, 1, 2]        # every row on the exact tier
    assert m.encode_head(pixel_values=px)["exact_tier"] is True                                # ... as the fast pass's state says
    assert torch.equal(out.embedding, vit2.embed_precise(px.reshape(-1, 3, 336, 336)).reshape(3, 4, 1024))
    assert m.certainty.stats == stats and m._cal_buffer == []                           # nothing was measured


# ------------------------------------------------------------------------------------------------ 7. run.py
def _run_py(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "run.py")] + args, capture_output=True, text=True, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


def test_run_py_embed_with_calibration_is_reproducible(tmp_path):
    f = os.path.join(str(tmp_path), "F.npz")
    outs = []
    for run in (1, 2):
        out_dir = os.path.join(str(tmp_path), f"emb{run}")
        log = _run_py(["embed", "random", "--synthetic", "64", "--layers", "2", "--yfcc", "--out-dir", out_dir, "--calibration", f])
        if run == 1:
            assert f"Calibration written to {f}" in log and os.path.exists(f)
        else:
            assert f"Loaded calibration {f}" in log and "Calibration written" not in log
        outs.append({n: open(os.path.join(out_dir, n), "rb").read() for n in ("train.npy", "train_indices.npy")})
    assert outs[0] == outs[1]                                                           # byte for byte
    from pigeon_amd.certainty import Certainty
    sd, header = Certainty.load(f)
    assert header["panels"] == 1 and header["layers"] == 2 and len(header["fingerprint"]) == 32 and sd["calibrated"]


def test_run_py_evaluate_with_calibration_is_reproducible(monkeypatch, tmp_path, capsys):
    import importlib
    g = os.path.join(str(tmp_path), "G.npz")
    results = []
    for run in (1, 2):
        monkeypatch.setattr(sys, "argv", ["run.py", "evaluate", "none", "--synthetic", "16", "--layers", "2", "--geocells", "300", "--calibration", g])
        sys.path.insert(0, ROOT)
        import run as run_py
        importlib.reload(run_py)
        torch.manual_seed(0)                                                            # the head is randomly initialised
        results.append(run_py.main())
        log = capsys.readouterr().out
        assert (f"Calibration written to {g}" if run == 1 else f"Loaded calibration {g}") in log
    a, b = results
    assert sorted(a) == sorted(b) and "uncertain_after_exact" in a
    assert a["uncertain_after_exact"] == b["uncertain_after_exact"]
    for k in a:
        if k == "exact_passes":
            assert [p["slots_run"] for p in a[k]] == [p["slots_run"] for p in b[k]]
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), k
        else:
            assert a[k] == b[k] or (a[k] != a[k] and b[k] != b[k]), k
