"""What pg_vit_load_weight and pg_vit_finalize leave on the device, bit for bit (run with -m gpu on an MI355X).

Every kernel of the encoder has its per-element test; what the kernels multiply WITH had none: the 16-bit conversions, the LayerNorm
fold (W' = cvt(fp32(W gamma)), the column sums of the ROUNDED W', beta . W^T + b in double), q|k|v, the zero padded patch weight, the
exact tier's split-fp16 triples and raw biases.  Here every buffer of a 2-layer tower is read back (pg_vit_param_read) and compared AS
INTEGERS with tests/_weightref.py, a numpy restatement written from the headers, on weights that carry planted ties, subnormals, signed
zeros, values the fold pushes past 65504, values past 65520, +-Inf and one NaN (tests/test_weightref_cpu.py: the restatement is the
network, the planted values convert as derived by hand, and each slip this is meant for shows in a named buffer).  pg_vit_fingerprint
equals the restated value, the table rebuilt from the read-back buffers and -- on the calibration tests' tower -- committed literals;
hip_ops.x3_pack_weight equals the library's triple; the load contract's refusals are refused.  Host code and copies: no kernel but
the fingerprint's is launched, nothing has a tolerance."""
import contextlib
import ctypes as C
import os
import time

import numpy as np
import pytest
import torch

import _weightref as R
from test_weightref_cpu import PINNED

pytestmark = pytest.mark.gpu

T0 = time.time()
LINES = []
CONFIGS = {"fold-f16": ("f16", True), "separate-f16": ("f16", False), "fold-bf16": ("bf16", True), "separate-bf16": ("bf16", False)}
PG_OK, PG_EINVAL, PG_ESTATE = 0, -1, -4


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops, synthetic
    _lib.require_gpu()
    return dict(lib=_lib, ops=hip_ops, L=_lib.load(), syn=synthetic)


@pytest.fixture(scope="module")
def sd2(env):
    return env["syn"].make_vit_weights(seed=11, layers=2, affine_jitter=True)


@pytest.fixture(scope="module")
def planted(sd2):
    return R.plant(sd2)


@contextlib.contextmanager
def _fold_env(fold):
    """PIGEON_LN_FOLD is read when a handle is created (as tests/test_gpu_fast_tier.py sets it); PIGEON_MMA_DTYPE must not decide."""
    old = {k: os.environ.get(k) for k in ("PIGEON_LN_FOLD", "PIGEON_MMA_DTYPE")}
    os.environ["PIGEON_LN_FOLD"] = "1" if fold else "0"
    os.environ.pop("PIGEON_MMA_DTYPE", None)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _slots(layers):
    return [(0, s) for s in range(R.EMBED_SLOTS)] + [(g, s) for g in range(1, layers + 1) for s in range(R.LAYER_SLOTS)]


def _read_all(enc, layers):
    """{(group, slot): uint8 numpy array} of every slot of the numbering (empty where the handle has no such buffer)."""
    return {(g, s): enc.param(g, s).numpy() for g, s in _slots(layers)}


def _compare(tag, got, bufs, found):
    """Every slot of `got` (read back) against the restatement's list, as integers; absent slots must be absent on both sides."""
    want = {(g, s): a for g, s, _, a in bufs}
    for key, raw in got.items():
        if key == (0, 6):
            continue                                            # the normalisation table: against pg_prep_norm_lut, by the caller
        name = R.slot_name(*key)
        if key not in want:
            if raw.size:
                found.append(f"[{tag}] {name}: {raw.size} bytes on the device, none expected")
            continue
        if raw.size != want[key].nbytes:
            found.append(f"[{tag}] {name}: {raw.size} bytes on the device, {want[key].nbytes} expected")
            continue
        d = R.first_difference(raw, want[key])
        if d is not None:
            n = int((raw.view(np.uint16) != want[key].view(np.uint16).reshape(-1)).sum()) if raw.size % 2 == 0 else -1
            found.append(f"[{tag}] {name}: first difference at row {d[0]} column {d[1]}: got 0x{d[2]:x}, restated 0x{d[3]:x} ({n} 16-bit words differ)")
    assert set(want) <= set(got)


def _no(found):
    assert not found, "\n".join(found[:40])


def _keep(lines):
    LINES.extend(lines)
    from test_gpu_precise import _report                     # the suite's report writer (the run's output folder)
    _report(LINES, "weight_buffers.txt")


def _norm_lut(env):
    lut = (C.c_float * 768)()
    env["lib"].check(env["L"].pg_prep_norm_lut(lut), "pg_prep_norm_lut")
    return np.frombuffer(lut, dtype=np.float32).copy()


# ------------------------------------------------------------------------------------------------ 1. every buffer, every bit
@pytest.mark.parametrize("config", list(CONFIGS))
def test_every_buffer_equals_the_restatement(env, planted, config):
    dtype, fold = CONFIGS[config]
    t_start = t0 = time.time()
    ref = R.WeightRef(planted, 2, dtype, fold, precise=True)
    bufs = ref.buffers()
    t_ref = time.time() - t0
    if dtype == "bf16" and fold:                              # the condition under which the restated column sum is order-free (fp16: always)
        for g, s, _, a in bufs:
            if g and s in (0, 5):
                ok = R.rows_sum_exactly_in_double(R.bits_to_f64(dtype, a))
                assert ok.all(), (R.slot_name(g, s), np.flatnonzero(~ok)[:5])
    t0 = time.time()
    with _fold_env(fold):
        enc = env["ops"].VitEncoder(planted, layers=2, mma_dtype=dtype, precise=True)
    try:
        assert enc.mma_dtype == dtype
        t_pack = time.time() - t0
        got = _read_all(enc, 2)
        found = []
        _compare(config, got, bufs, found)
        # the chain asked for is the chain packed: column sums exist exactly with the fold
        assert (got[(1, 2)].size > 0) == fold and (got[(2, 7)].size > 0) == fold
        if not np.array_equal(got[(0, 6)].view(np.float32), _norm_lut(env)):
            found.append(f"[{config}] the handle's normalisation table differs from pg_prep_norm_lut")
        _no(found)
        # the fingerprint: the restated value, and the table rebuilt from what was read back
        fp = enc.fingerprint()
        assert fp == ref.fingerprint(bufs), (config, "%016x%016x" % fp)
        back = [(g, s, (g << 8) | s, got[(g, s)]) for g, s in _slots(2) if got[(g, s)].size]
        assert fp == ref.fingerprint(back)
        assert enc.fingerprint() == fp
        nbytes = sum(a.size for a in got.values())
        _keep([f"[{config}] {len(back)} buffers, {nbytes / 2 ** 20:.0f} MiB read back and bit-equal to the restatement; fingerprint {'%016x%016x' % fp}"
               f"  (restatement {t_ref:.1f} s, create + load + finalize {t_pack:.1f} s, all {time.time() - t_start:.1f} s)"])
    finally:
        enc.close()


def test_without_precise_the_exact_tiers_slots_are_absent(env, planted):
    with _fold_env(True):
        enc = env["ops"].VitEncoder(planted, layers=2, mma_dtype="f16")
    try:
        got = _read_all(enc, 2)
        found = []
        _compare("fold-f16, no precise", got, R.WeightRef(planted, 2, "f16", True, precise=False).buffers(), found)
        _no(found)
        assert all(got[k].size == 0 for k in [(0, 5)] + [(g, s) for g in (1, 2) for s in range(14, 20)])
        assert got[(0, 6)].size == 768 * 4
    finally:
        enc.close()


# ------------------------------------------------------------------------------------------------ 2. the fingerprint's meaning is pinned
@pytest.mark.parametrize("config", list(CONFIGS))
def test_fingerprint_equals_the_committed_literal(env, sd2, config):
    """The calibration tests' tower (tests/test_gpu_calibration.py): the key of a stored calibration cannot drift."""
    dtype, fold = CONFIGS[config]
    for precise in ((False, True) if config == "fold-f16" else (False,)):
        with _fold_env(fold):
            enc = env["ops"].VitEncoder(sd2, layers=2, mma_dtype=dtype, precise=precise)
        try:
            assert "%016x%016x" % enc.fingerprint() == PINNED[(dtype, fold)], (config, precise)
        finally:
            enc.close()


# ------------------------------------------------------------------------------------------------ 3. the mirror of the triple
def test_x3_pack_weight_mirrors_the_library(env, planted):
    """hip_ops.x3_pack_weight, which the building-block tests of the exact tier multiply with, against the library's triples of the
    planted weights (saturation, subnormal low halves, +-Inf, the NaN)."""
    ops = env["ops"]
    with _fold_env(True):
        enc = ops.VitEncoder(planted, layers=2, mma_dtype="f16", precise=True)
    try:
        found = []

        def same(name, lib_bits, mirror):
            m = mirror.view(torch.int16).numpy().view(np.uint16)
            d = R.first_difference(lib_bits, m)
            if d is not None:
                found.append(f"{name}: row {d[0]} column {d[1]}: library 0x{d[2]:x}, x3_pack_weight 0x{d[3]:x}")

        wp = planted["embeddings.patch_embedding.weight"].reshape(R.D, R.PATCH_K)
        lib = enc.param(0, 5, torch.int16).numpy().view(np.uint16).reshape(R.D, 3, R.PATCH_KPAD)
        assert not lib[:, :, R.PATCH_K:].any()
        same("patch triple", np.ascontiguousarray(lib[:, :, :R.PATCH_K]), ops.x3_pack_weight(wp))
        for l in range(2):
            pre = f"encoder.layers.{l}."
            wqkv = torch.cat([planted[pre + f"self_attn.{x}_proj.weight"] for x in "qkv"], dim=0)
            for slot, W in ((14, wqkv), (15, planted[pre + "self_attn.out_proj.weight"]), (16, planted[pre + "mlp.fc1.weight"]),
                            (17, planted[pre + "mlp.fc2.weight"])):
                same(R.slot_name(l + 1, slot), enc.param(l + 1, slot, torch.int16).numpy().view(np.uint16), ops.x3_pack_weight(W))
        _no(found)
    finally:
        enc.close()


# ------------------------------------------------------------------------------------------------ 4. the load contract
class Raw:
    """A pg_vit handle through the C ABI alone: 1 layer, fp16 operands."""

    def __init__(self, env, layers=1, precise=0, fold=True):
        self.lib, self.L = env["lib"], env["L"]
        cfg = self.lib.VitCfg(layers, 336, 14, 1024, 16, 4096, 1e-5, 0, self.lib.PG_DTYPE_F16, precise)
        self.h = C.c_void_p()
        with _fold_env(fold):
            self.lib.check(self.L.pg_vit_create(C.byref(self.h), 0, C.byref(cfg)), "pg_vit_create")

    def load(self, name, t, shape=None, ndim=None, dtype=0):
        """-> (rc, message); t: a CPU fp32 tensor that stays alive over the call; shape / ndim default to the tensor's."""
        a = t.detach().to(torch.float32).contiguous()
        shape = list(a.shape) if shape is None else list(shape)
        arr = (C.c_int64 * max(len(shape), 1))(*(shape or [1]))
        rc = self.L.pg_vit_load_weight(self.h, name.encode(), C.c_void_p(a.data_ptr()), dtype, arr, len(shape) if ndim is None else ndim)
        return rc, (self.L.pg_last_error() or b"").decode()

    def load_all(self, sd, skip=(), prefix=""):
        for k, v in sd.items():
            if k not in skip:
                rc, msg = self.load(prefix + k, v)
                assert rc == PG_OK, (k, msg)

    def finalize(self):
        rc = self.L.pg_vit_finalize(self.h)
        return rc, (self.L.pg_last_error() or b"").decode()

    def fingerprint(self):
        out = (C.c_uint64 * 2)()
        self.lib.check(self.L.pg_vit_fingerprint(self.h, out), "pg_vit_fingerprint")
        return int(out[0]), int(out[1])

    def read(self, g, s, dst=None, dst_bytes=0):
        n = C.c_size_t(12345)
        rc = self.L.pg_vit_param_read(self.h, g, s, dst, dst_bytes, C.byref(n))
        return rc, n.value, (self.L.pg_last_error() or b"").decode()

    def read_all(self, layers=1):
        out = {}
        for g, s in _slots(layers):
            rc, n, msg = self.read(g, s)
            assert rc == PG_OK, (g, s, msg)
            buf = np.zeros(n, dtype=np.uint8)
            if n:
                rc, n2, msg = self.read(g, s, C.c_void_p(buf.ctypes.data), n)
                assert rc == PG_OK and n2 == n, (g, s, msg)
            out[(g, s)] = buf
        return out

    def destroy(self):
        rc = self.L.pg_vit_destroy(self.h) if self.h.value else PG_OK
        self.h = C.c_void_p()
        return rc


@pytest.fixture(scope="module")
def one_layer(env, planted):
    """What a 1-layer handle holds of the planted tower -- loaded from the 2-layer state dict, so layer 1's names are beyond cfg.layers."""
    with _fold_env(True):
        enc = env["ops"].VitEncoder(planted, layers=1, mma_dtype="f16", precise=True)
    try:
        got, fp = _read_all(enc, 1), enc.fingerprint()
    finally:
        enc.close()
    found = []
    _compare("one layer of two", got, R.WeightRef(planted, 1, "f16", True, precise=True).buffers(), found)
    _no(found)
    return got, fp


def _same_buffers(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_key_layouts_duplicates_unknown_names_and_a_second_finalize(env, planted, one_layer):
    want, want_fp = one_layer
    r = Raw(env, precise=1)
    try:
        junk = torch.full((R.F, R.D), 7.0)
        assert r.load("vision_model.encoder.layers.0.mlp.fc1.weight", junk)[0] == PG_OK        # loaded twice: the last value is kept
        assert r.load("encoder.layers.0.layer_norm1.bias", torch.zeros(R.D))[0] == PG_OK        # ... across the two key layouts
        r.load_all(planted, prefix="vision_model.")
        for name, t in (("vision_model.post_layernorm.weight", torch.ones(R.D)), ("embeddings.position_ids", torch.zeros(1, 577)),
                        ("encoder.layers.1.mlp.fc1.weight", torch.zeros(3, 5)), ("encoder.layers.0.mlp.fc3.weight", torch.zeros(2)),
                        ("encoder.layers.00.mlp.fc1.bias", torch.zeros(7))):
            assert r.load(name, t)[0] == PG_OK, name                                           # not read on this path: ignored, any shape
        assert r.finalize()[0] == PG_OK
        assert r.fingerprint() == want_fp
        assert _same_buffers(r.read_all(), want)
        assert r.finalize()[0] == PG_OK and r.fingerprint() == want_fp                          # a second finalize is a no-op
        assert _same_buffers(r.read_all(), want)
        rc, msg = r.load("encoder.layers.0.mlp.fc1.bias", torch.zeros(R.F))
        assert rc == PG_ESTATE and "finalized" in msg                                           # load after finalize
        assert r.fingerprint() == want_fp
    finally:
        assert r.destroy() == PG_OK


def test_a_missing_parameter_is_named_and_can_be_supplied(env, planted, one_layer):
    want, want_fp = one_layer
    missing = "encoder.layers.0.mlp.fc2.bias"
    r = Raw(env, precise=1)
    try:
        r.load_all(planted, skip=(missing,))
        rc, msg = r.finalize()
        assert rc == PG_ESTATE and missing in msg
        rc, n, msg = r.read(0, 0)
        assert rc == PG_ESTATE and n == 0 and "not finalized" in msg                            # nothing to read back yet
        out = (C.c_uint64 * 2)()
        assert r.L.pg_vit_fingerprint(r.h, out) == PG_ESTATE
        assert r.load(missing, planted[missing])[0] == PG_OK
        assert r.finalize()[0] == PG_OK
        assert r.fingerprint() == want_fp and _same_buffers(r.read_all(), want)
    finally:
        assert r.destroy() == PG_OK
    r = Raw(env)
    r.load_all(planted, skip=(missing,))
    assert r.finalize()[0] == PG_ESTATE
    assert r.destroy() == PG_OK                                                                 # a handle that never finalized can be destroyed


SHAPES = {  # name: (the transformers shape, a refused shape of the same element count)
    "encoder.layers.0.mlp.fc1.weight": ((4096, 1024), (1024, 4096)),
    "encoder.layers.0.mlp.fc2.weight": ((1024, 4096), (4096, 1024)),
    "embeddings.position_embedding.weight": ((577, 1024), (1024, 577)),
    "embeddings.patch_embedding.weight": ((1024, 3, 14, 14), (1024, 3, 196)),
}


def test_refused_loads(env, planted):
    """Every refusal is PG_EINVAL with a message, stages nothing (finalize still names the parameter as missing), and reads nothing:
    each refused call is handed a full-size buffer all the same."""
    fmt = lambda s: "(" + ", ".join(str(v) for v in s) + ")"
    r = Raw(env)
    try:
        refused = list(SHAPES) + ["encoder.layers.0.mlp.fc1.bias", "encoder.layers.0.layer_norm2.weight"]
        r.load_all(planted, skip=refused)
        for name, (right, wrong) in SHAPES.items():
            rc, msg = r.load(name, planted[name], shape=wrong)
            assert rc == PG_EINVAL and name in msg and fmt(wrong) in msg and fmt(right) in msg, msg
        # a wrong element count: both numbers
        rc, msg = r.load("encoder.layers.0.mlp.fc1.bias", planted["encoder.layers.0.mlp.fc1.bias"], shape=(4095,))
        assert rc == PG_EINVAL and "4095" in msg and "4096" in msg, msg
        rc, msg = r.load("encoder.layers.0.mlp.fc1.bias", planted["encoder.layers.0.mlp.fc1.bias"], shape=(4096, 1))
        assert rc == PG_EINVAL and "(4096, 1)" in msg and "(4096)" in msg, msg
        # ndim < 1 and extents < 1: refused before anything is read, for a known name and for a name that would be ignored
        ln = "encoder.layers.0.layer_norm2.weight"
        for name in (ln, "post_layernorm.weight"):
            for shape, ndim in (((1024,), 0), ((1024,), -1), ((0,), 1), ((-1024,), 1), ((1024, 0), 2), ((-32, -32), 2), ((1024,), 9)):
                rc, msg = r.load(name, planted[ln], shape=shape, ndim=ndim)
                assert rc == PG_EINVAL and name in msg, (name, shape, ndim, msg)
        # a non-fp32 dtype, null arguments
        L, h, lib = r.L, r.h, r.lib
        t = planted[ln].contiguous()
        one = (C.c_int64 * 1)(1024)
        for dt in (lib.PG_DTYPE_F16, lib.PG_DTYPE_BF16, lib.PG_DTYPE_F64, 99):
            rc, msg = r.load(ln, t, dtype=dt)
            assert rc == PG_EINVAL and "fp32" in msg
        p = C.c_void_p(t.data_ptr())
        for args in ((None, ln.encode(), p, 0, one, 1), (h, None, p, 0, one, 1), (h, ln.encode(), None, 0, one, 1), (h, ln.encode(), p, 0, None, 1)):
            assert L.pg_vit_load_weight(*args) == PG_EINVAL and b"null" in L.pg_last_error()
        assert L.pg_vit_finalize(None) == PG_EINVAL
        # nothing of the above was staged: one after the other is still missing, then the handle finalizes
        left = set(refused)
        while left:
            rc, msg = r.finalize()
            named = [n for n in left if msg.endswith("missing parameter " + n)]
            assert rc == PG_ESTATE and len(named) == 1, (sorted(left), msg)
            assert r.load(named[0], planted[named[0]])[0] == PG_OK
            left.remove(named[0])
        assert r.finalize()[0] == PG_OK
    finally:
        assert r.destroy() == PG_OK


def test_param_read_contract(env, planted, one_layer):
    want, _ = one_layer
    r = Raw(env, precise=0, fold=False)
    try:
        r.load_all(planted)
        assert r.read(0, 0)[0] == PG_ESTATE
        assert r.finalize()[0] == PG_OK
        for g, s in ((0, 7), (0, -1), (-1, 0), (2, 0), (1, 20), (1, -1), (1 << 20, 0)):
            rc, n, msg = r.read(g, s)
            assert rc == PG_EINVAL and n == 0 and "no buffer" in msg, (g, s)
        for g, s in ((0, 5), (1, 2), (1, 7), (1, 14), (1, 19)):                                  # no fold, no precise: not on this handle
            assert r.read(g, s)[:2] == (PG_OK, 0), (g, s)
        rc, n, _ = r.read(1, 4)                                                                  # the out_proj bias: a size query
        assert (rc, n) == (PG_OK, 4 * R.D)
        dst = np.full(n + 16, 0xA5, dtype=np.uint8)
        rc, n2, msg = r.read(1, 4, C.c_void_p(dst.ctypes.data), n - 1)
        assert rc == PG_EINVAL and n2 == n and str(n - 1) in msg and (dst == 0xA5).all()         # too small: nothing is copied
        rc, n2, _ = r.read(1, 4, C.c_void_p(dst.ctypes.data), n + 16)
        assert (rc, n2) == (PG_OK, n) and (dst[n:] == 0xA5).all()                                # ... and a larger one gets the buffer's bytes only
        assert np.array_equal(dst[:n], want[(1, 4)])
        assert r.L.pg_vit_param_read(None, 0, 0, None, 0, C.byref(C.c_size_t())) == PG_EINVAL
        assert r.L.pg_vit_param_read(r.h, 0, 0, None, 0, None) == PG_EINVAL
        assert torch.cuda.current_device() == 0
    finally:
        assert r.destroy() == PG_OK


def test_wall_time_of_this_file(capsys):
    line = f"tests/test_gpu_weights.py: {time.time() - T0:.0f} s since import"
    _keep([line])
    with capsys.disabled():
        print("\n" + line)
