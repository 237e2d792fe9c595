"""The host side of the encoder's two forward calls (run with -m gpu on an MI355X): the size of each workspace against its closed form,
and the refusals of pg_vit_forward_hidden / pg_vit_forward_precise and of the two counter reads -- code, text, order, nothing launched.

The workspace forms are DESIGN.md section 3's, written out here (never asked of the library): per token row the fast encoder keeps X fp32
4 KB | Xn 16-bit 2 KB | big 16-bit 8 KB, with the LayerNorm fold also Xn2 2 KB | statpart 16 x 8 B | two row-statistics buffers of 8 B; the
exact mode X 4 KB | T3 6 KB | F 16 KB | G3 24 KB | PP 48 KB.  Every buffer is rounded up to 256 bytes, 256 bytes trail.  2-layer synthetic
towers as in test_gpu_fast_tier.py; the environment is read when a handle is created."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
TOKENS, HIDDEN = 577, 1024
SENTINEL = 7.0
PG_OK, PG_EINVAL, PG_ENOMEM, PG_ESTATE = 0, -1, -2, -4


def a(x):
    return (x + 255) // 256 * 256


def fast_form(chunk, fold):
    M = TOKENS * chunk
    b = a(4096 * M) + a(2048 * M) + a(8192 * M) + 256
    if fold:
        b += a(2048 * M) + a(128 * M) + 2 * a(8 * M)
    return b


def fast_bytes(n, fold, max_chunk, streams):
    """pg_vit_workspace_bytes as documented: chunks of at most max_chunk (0: 512) images; with S > 1 streams and n >= 32 S, S parts of
    ceil(n / S) images, each with a workspace of its own."""
    cap = max_chunk if max_chunk > 0 else 512
    if streams > 1 and n >= 32 * streams:
        return streams * a(fast_form(min(-(-n // streams), cap), fold))
    return fast_form(max(min(n, cap), 1), fold)


def precise_form(n):
    M = TOKENS * min(max(n, 1), 128)
    return a(4096 * M) + a(6144 * M) + a(16384 * M) + a(24576 * M) + a(49152 * M) + 256


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops, synthetic
    _lib.require_gpu()                       # fails loudly if the HIP library / GPU is missing -- no fallback
    return dict(lib=_lib, ops=hip_ops, L=_lib.load(), syn=synthetic)


def _setenv(monkeypatch, fold=True, streams=None):
    monkeypatch.setenv("PIGEON_LN_FOLD", "1" if fold else "0")
    for k in ("PIGEON_MMA_DTYPE", "PIGEON_VIT_GRAPH", "PIGEON_GEMM_VARIANT"):
        monkeypatch.delenv(k, raising=False)
    if streams:
        monkeypatch.setenv("PIGEON_VIT_STREAMS", str(streams))
    else:
        monkeypatch.delenv("PIGEON_VIT_STREAMS", raising=False)


def _raw_handle(env, max_chunk=0, precise=0):
    """A created, NOT finalized handle (no weights): what the size queries and the 'not finalized' refusal need."""
    lib, L = env["lib"], env["L"]
    cfg = lib.VitCfg(2, 336, 14, 1024, 16, 4096, 1e-5, max_chunk, 0, precise)
    h = C.c_void_p()
    lib.check(L.pg_vit_create(C.byref(h), 0, C.byref(cfg)), "pg_vit_create")
    return h


def _err(env):
    return (env["L"].pg_last_error() or b"").decode()


# ================================================================================================================ workspace sizes
def _size(env, fn, h, n):
    need = C.c_size_t(12345)
    env["lib"].check(getattr(env["L"], fn)(h, n, C.byref(need)), fn)
    return need.value


FAST_CASES = [(None, (0, 1, 2, 3, 29, 30, 88)), (2, (63, 64, 87)), (3, (97,))]


def test_workspace_sizes_equal_their_closed_forms(env, monkeypatch):
    """pg_vit_workspace_bytes: fold on and off, max_chunk 0 and 29; one stream at n in {0, 1, 2, 3, 29, 30, 88}; PIGEON_VIT_STREAMS=2 at
    63 (below 32 per part: no split), 64 and 87 (two parts of ceil(n / 2)); PIGEON_VIT_STREAMS=3 at 97 (three parts of 33).
    pg_vit_precise_workspace_bytes at n in {0, 1, 28, 128, 129, 130, 1000}: the five-term form at min(max(n, 1), 128) images, although
    equal chunks above 128 are smaller.  A negative n and null arguments are PG_EINVAL."""
    L = env["L"]
    found = []
    for streams, ns in FAST_CASES:
        for fold in (True, False):
            for max_chunk in (0, 29):
                _setenv(monkeypatch, fold, streams)
                h = _raw_handle(env, max_chunk)
                try:
                    for n in ns:
                        got, want = _size(env, "pg_vit_workspace_bytes", h, n), fast_bytes(n, fold, max_chunk, streams or 1)
                        if got != want:
                            found.append(f"fast: streams {streams or 1} fold {fold} max_chunk {max_chunk} n {n}: {got} bytes, closed form {want}")
                finally:
                    L.pg_vit_destroy(h)
    # the forms at the parts the split cases are meant to reach (the test's own arithmetic, stated once)
    assert fast_bytes(63, True, 0, 2) == fast_form(63, True) and fast_bytes(64, True, 0, 2) == 2 * fast_form(32, True)
    assert fast_bytes(87, False, 0, 2) == 2 * fast_form(44, False) and fast_bytes(97, True, 0, 3) == 3 * fast_form(33, True)
    assert fast_bytes(87, True, 29, 2) == 2 * fast_form(29, True) and fast_bytes(88, True, 29, 1) == fast_form(29, True)
    _setenv(monkeypatch)
    h = _raw_handle(env)
    try:
        for n in (0, 1, 28, 128, 129, 130, 1000):
            got, want = _size(env, "pg_vit_precise_workspace_bytes", h, n), precise_form(n)
            if got != want:
                found.append(f"exact: n {n}: {got} bytes, closed form {want}")
        need = C.c_size_t(12345)
        for fn in ("pg_vit_workspace_bytes", "pg_vit_precise_workspace_bytes"):
            for args in ((h, -1, C.byref(need)), (None, 1, C.byref(need)), (h, 1, None)):
                rc = getattr(L, fn)(*args)
                if rc != PG_EINVAL or "bad argument" not in _err(env) or need.value != 12345:
                    found.append(f"{fn}{args[1:2]}: rc {rc}, '{_err(env)}', bytes {need.value}; expected PG_EINVAL, 'bad argument', bytes untouched")
    finally:
        L.pg_vit_destroy(h)
    assert not found, "\n".join(found)


# ================================================================================================================ refusals
@pytest.fixture(scope="module")
def handles(env):
    """One finalized 2-layer encoder with the exact mode's weights, one without, one created but never finalized; a pixel batch of one."""
    syn, ops = env["syn"], env["ops"]
    mp = pytest.MonkeyPatch()
    _setenv(mp)
    sd = syn.make_vit_weights(seed=17, layers=2, affine_jitter=True)
    exact = ops.VitEncoder(sd, layers=2, precise=True)
    plain = ops.VitEncoder(sd, layers=2)
    raw = _raw_handle(env, precise=1)
    mp.undo()
    yield dict(exact=exact, plain=plain, raw=raw, px=syn.make_pixels(1, seed=4321).to(DEV))
    exact.close(); plain.close()
    env["L"].pg_vit_destroy(raw)


CALLS = {"vit_forward": ("pg_vit_forward_hidden", "pg_vit_workspace_bytes"), "vit_forward_precise": ("pg_vit_forward_precise", "pg_vit_precise_workspace_bytes")}


@pytest.mark.parametrize("prefix", list(CALLS))
def test_forward_refusals(env, handles, prefix):
    """Return code and text of every refusal of the two forward calls, in the order the checks run (where two faults are present the
    earlier check answers), each text under the call's own prefix; an empty batch with null buffers is PG_OK.  The sentinel-filled
    embedding buffer is untouched after all of them: a refused call launches nothing."""
    lib, ops, L = env["lib"], env["ops"], env["L"]
    fn, size_fn = CALLS[prefix]
    forward = getattr(L, fn)
    h, px = handles["exact"]._h, handles["px"]
    need = _size(env, size_fn, h, 1)
    ws = torch.empty(need + 512, dtype=torch.uint8, device=DEV)
    wp = ws.data_ptr() + (-ws.data_ptr()) % 256
    emb = torch.full((HIDDEN,), SENTINEL, dtype=torch.float32, device=DEV)
    F32 = lib.PG_DTYPE_F32
    good = dict(h=h, pixels=ops._p(px), dtype=F32, n=1, emb=ops._p(emb), ws=C.c_void_p(wp), bytes=need)
    cases = [  # (what, changed arguments, code, fragments of the text)
        ("null handle", dict(h=None), PG_EINVAL, ["null handle"]),
        ("null handle and n = -1", dict(h=None, n=-1), PG_EINVAL, ["null handle"]),
        ("unfinalized handle", dict(h=handles["raw"]), PG_ESTATE, ["not finalized"]),
        ("unfinalized handle and n = -1", dict(h=handles["raw"], n=-1), PG_ESTATE, ["not finalized"]),
        ("n = -1", dict(n=-1), PG_EINVAL, ["n_images = -1"]),
        ("n = -1 and null pixels", dict(n=-1, pixels=None), PG_EINVAL, ["n_images = -1"]),
        ("n = 0, null buffers", dict(n=0, pixels=None, emb=None, ws=None, bytes=0), PG_OK, None),
        ("null pixels", dict(pixels=None), PG_EINVAL, ["null argument"]),
        ("null embedding", dict(emb=None), PG_EINVAL, ["null argument"]),
        ("null workspace", dict(ws=None), PG_EINVAL, ["null argument"]),
        ("null pixels and dtype 99", dict(pixels=None, dtype=99), PG_EINVAL, ["null argument"]),
        ("pixel dtype 99", dict(dtype=99), PG_EINVAL, ["bad pixel dtype"]),
        ("dtype 99 and a short workspace", dict(dtype=99, bytes=need - 1), PG_EINVAL, ["bad pixel dtype"]),
        ("workspace one byte short", dict(bytes=need - 1), PG_ENOMEM, [f"workspace {need - 1} < required {need} bytes"]),
        ("workspace short and misaligned", dict(bytes=need - 1, ws=C.c_void_p(wp + 128)), PG_ENOMEM, [f"workspace {need - 1} < required {need} bytes"]),
        ("workspace off by 128 bytes", dict(ws=C.c_void_p(wp + 128)), PG_EINVAL, ["256-byte aligned"]),
    ]
    if prefix == "vit_forward_precise":
        plain = handles["plain"]._h
        cases += [("handle without cfg.precise", dict(h=plain), PG_ESTATE, ["without cfg.precise"]),
                  ("handle without cfg.precise and n = -1", dict(h=plain, n=-1), PG_ESTATE, ["without cfg.precise"]),
                  ("handle without cfg.precise, n = 0", dict(h=plain, n=0), PG_ESTATE, ["without cfg.precise"])]
    found = []
    for what, change, code, frags in cases:
        k = dict(good, **change)
        L.pg_vit_forward_hidden(None, None, 0, 0, None, None, None, 0, None)          # a known text in pg_last_error: the case must replace it
        assert _err(env) == "vit_forward: null handle"
        before = _err(env)
        rc = forward(k["h"], k["pixels"], k["dtype"], k["n"], k["emb"], None, k["ws"], k["bytes"], ops._stream())
        msg = _err(env)
        if rc != code:
            found.append(f"{prefix}, {what}: rc {rc}, expected {code} ('{msg}')")
        if frags is None:
            if msg != before:
                found.append(f"{prefix}, {what}: PG_OK, yet the error text changed to '{msg}'")
        elif not msg.startswith(prefix + ": ") or any(f not in msg for f in frags):
            found.append(f"{prefix}, {what}: text '{msg}', expected '{prefix}: ...' with {frags}")
    torch.cuda.synchronize()
    if not bool((emb == SENTINEL).all()):
        found.append(f"{prefix}: the embedding buffer was written by a refused call")
    # ... and the same arguments unchanged are accepted (the refusals above are not an accident of the set-up)
    rc = forward(h, ops._p(px), F32, 1, ops._p(emb), None, C.c_void_p(wp), need, ops._stream())
    torch.cuda.synchronize()
    assert rc == PG_OK, (rc, _err(env))
    assert bool((emb != SENTINEL).any()) and bool(torch.isfinite(emb).all())
    assert not found, "\n".join(found)


def test_counter_reads(env, monkeypatch):
    """pg_vit_range_alarm_read / pg_vit_saturation_read: PG_EINVAL on a null handle or a null result; 0 on a bf16 handle (no alarm
    counter, no scan switched on); on an fp16 handle whose residual rows pass the fp16 range (test_gpu_entrypoints.py's bias) both
    count, a read without `reset` leaves the count, a read with it returns the same count and clears."""
    syn, ops, L = env["syn"], env["ops"], env["L"]
    reads = {"range_alarm_read": L.pg_vit_range_alarm_read, "saturation_read": L.pg_vit_saturation_read}
    _setenv(monkeypatch)
    sd = syn.make_vit_weights(seed=11, layers=2)
    sd["encoder.layers.0.self_attn.out_proj.bias"] = sd["encoder.layers.0.self_attn.out_proj.bias"].clone()
    sd["encoder.layers.0.self_attn.out_proj.bias"][7] = 1.0e5   # channel 7 of every residual row beyond the fp16 range from layer 0 on
    px = syn.make_pixels(1, seed=5).to(DEV)
    bf, fp = ops.VitEncoder(sd, layers=2, mma_dtype="bf16"), ops.VitEncoder(sd, layers=2, mma_dtype="f16")
    try:
        for who, read in reads.items():
            v = C.c_int64(-5)
            for args in ((None, C.byref(v), 0), (fp._h, None, 0), (None, None, 1)):
                assert read(*args) == PG_EINVAL and _err(env) == f"{who}: null argument", (who, _err(env))
            assert v.value == -5
            bf.forward(px)
            assert read(bf._h, C.byref(v), 0) == PG_OK and v.value == 0, (who, v.value)
        fp.saturation_check(True)
        fp.forward(px)
        for who, read in reads.items():
            got = []
            for reset in (0, 0, 1, 0, 1):
                v = C.c_int64(-5)
                assert read(fp._h, C.byref(v), reset) == PG_OK, (who, _err(env))
                got.append(v.value)
            assert got[0] >= 577 and got == [got[0]] * 3 + [0, 0], (who, got)
    finally:
        bf.close(); fp.close()
