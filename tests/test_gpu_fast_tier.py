"""The fast tier (pg_vit_forward / pg_vit_forward_hidden: 16-bit MFMA operands, LayerNorm folded into the GEMMs) at every route a batch
size takes through it, against fp64 (run with -m gpu on an MI355X).

tests/test_gpu_exact.py checks each GEMM launch and the attention kernel alone; the end-to-end tests meet an independent reference at 2
to 4 images.  What vit_forward_body COMPOSES out of the launches -- the workspace carve-up, the two alternating row-statistics buffers,
the partials' row stride where a RESID_STAT launch is cut, the last layer's EPI_RESID fc2, the per-chunk and per-stream output
offsets, the captured graph per (workspace, n) -- is checked here at every batch size at which pg_gemm_plan changes the form of one of
the chain's launches (asked of the library), one below each, and 88: every hidden row and every embedding against the fp64 oracle,
under bounds that come from tests/_fastref.py (the same 16-bit chain restated in fp64), never from the kernels; bit for bit against the
88-image run; eager against capture against replay; chunks and streams against one launch, with guard regions behind every buffer.

tests/test_fastref_cpu.py shows that the restatement is the network and that the comparator reports the mistakes it is meant for.
No input is NaN, Inf or outside a kernel's contract; the negative control changes the operand type, nothing else."""
import ctypes as C
import time

import pytest
import torch

import _exactref as X
import _fastref as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
F16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32
LAYERS, POOL, VARIANT = 2, 88, 56
GUARD = 4096                                                   # sentinel elements behind every output, pattern bytes behind the workspace
WS_PATTERN = 0x5A
T0 = time.time()
LINES = []                                                     # the file's report: fast_tier_routes.txt in the run's output folder (_report of test_gpu_precise.py)
KIND_NAMES = {(0, -1): "PP6", (1, -1): "PP", (2, -1): "MID", (0, 2): "PP6 + MID cut", (0, 3): "PP6 + TAIL cut", (1, 3): "PP + TAIL cut"}
ROUTES = {"fold-f16": (True, "f16", F16), "separate-f16": (False, "f16", F16), "fold-bf16": (True, "bf16", BF16)}


def _chain(fold):
    """The chain's GEMM launches as csrc/vit.hip makes them: (name, epilogue, N, K, rows per image), shapes from test_gpu_exact.LAUNCHES."""
    from test_gpu_exact import LAUNCHES as LA
    pick = lambda short, name: (short,) + LA[name][:3] + (LA[name][4],)
    if fold:
        return [pick("patch", "patch"), pick("qkv", "qkv_ln"), pick("out", "out"), pick("fc1", "fc1_ln"), pick("fc2", "fc2"), pick("fc2L", "fc2_resid")]
    out = ("out", X.EPI_RESID) + LA["out"][1:3] + (LA["out"][4],)           # the separate chain's out-projection: the same shape, plain EPI_RESID
    return [pick("patch", "patch"), pick("qkv", "qkv"), out, pick("fc1", "fc1"), pick("fc2", "fc2_resid")]


def _sig(env, fold, n):
    """((kernel, rest) of every launch of the chain at n images), from pg_gemm_plan under the current knobs."""
    out = []
    for (_, epi, N, K, rpi) in _chain(fold):
        k, r, s = C.c_int(-9), C.c_int(-9), C.c_int(-9)
        env["lib"].check(env["L"].pg_gemm_plan(VARIANT, epi, n * rpi, N, K, C.byref(k), C.byref(r), C.byref(s)), "pg_gemm_plan")
        out.append((k.value, s.value))
    return tuple(out)


def _label(env, fold, n):
    return " ".join(f"{name}({k},{r})" for (name, *_), (k, r) in zip(_chain(fold), _sig(env, fold, n)))


def route_sizes(env, fold):
    """Every n in 1 .. 88 at which the chain's signature differs from n - 1's (1 included), n - 1 of each, and 88."""
    ch, prev = [], None
    for n in range(1, POOL + 1):
        s = _sig(env, fold, n)
        if s != prev:
            ch.append(n)
        prev = s
    return sorted(set(ch) | {n - 1 for n in ch if n > 1} | {POOL})


@pytest.fixture(scope="module")
def env():
    from pigeon_amd import _lib, hip_ops, synthetic
    from oracle import pigeon_oracle as orc
    _lib.require_gpu()                       # fails loudly if the HIP library / GPU is missing -- no fallback
    return dict(lib=_lib, ops=hip_ops, L=_lib.load(), syn=synthetic, orc=orc)


@pytest.fixture(scope="module")
def tower(env):
    """The 2-layer tower, a pool of 88 images (batches are prefixes of it), the fp64 oracle's hidden state of the pool and the folded
    fp16 restatement's (torch on the GPU: checkers), computed once and left unchanged."""
    syn, orc = env["syn"], env["orc"]
    sd = syn.make_vit_weights(seed=17, layers=LAYERS, affine_jitter=True)
    px = syn.make_pixels(POOL, seed=4321).to(DEV)
    t0 = time.time()
    sd64 = {k: v.to(device=DEV, dtype=torch.float64) for k, v in sd.items()}
    ref_h = torch.cat([orc.vit_last_hidden_state(sd64, px[i:i + 8], dtype=torch.float64) for i in range(0, POOL, 8)], dim=0)
    torch.cuda.synchronize()
    t_ref = time.time() - t0
    tw = dict(sd=sd, px=px, ref_h=ref_h, t_ref=t_ref, rest={}, bounds={}, encs=[], eager={}, enc0=None)
    _bounds(tw, "fold-f16")
    yield tw
    for e in tw["encs"]:
        e.close()


def _bounds(tower, route):
    """row_tol / emb_tol of a route: from ITS restatement's error against the fp64 oracle over the whole pool (_fastref.bounds)."""
    if route not in tower["bounds"]:
        fold, _, dt = ROUTES[route]
        t0 = time.time()
        h, e = R.fast_hidden(tower["sd"], tower["px"], fold, dt)
        torch.cuda.synchronize()
        b = R.bounds(h, e, tower["ref_h"], cap_emb=dt == F16)          # bf16 has its own documented floor: 2 max E_emb only
        tower["rest"][route], tower["bounds"][route] = (h, e), b
        _keep([f"[restatement {route}] vs fp64 over {POOL} images (GPU, torch): row error max {b['row_max']:.3e} median {b['row_median']:.3e} min "
               f"{b['row_min']:.3e}; embedding error {b['emb_min']:.3e} .. {b['emb_max']:.3e}  ->  row_tol {b['row_tol']:.3e}, emb_tol {b['emb_tol']:.3e}"
               f"  ({time.time() - t0:.1f} s; the fp64 oracle of the pool: {tower['t_ref']:.1f} s)"])
    return tower["bounds"][route]


def _keep(lines):
    LINES.extend(lines)
    from test_gpu_precise import _report                     # the suite's report writer (the run's output folder)
    _report(LINES, "fast_tier_routes.txt")


def _no(found):
    assert not found, "\n".join(found[:40])


def _encoder(env, tower, monkeypatch, route="fold-f16", streams=None, graph=False, **kw):
    """A VitEncoder of the tower; PIGEON_LN_FOLD / PIGEON_VIT_STREAMS are read when the handle is created.  Closed with the module."""
    fold, dts, _ = ROUTES[route]
    monkeypatch.setenv("PIGEON_LN_FOLD", "1" if fold else "0")
    for k in ("PIGEON_MMA_DTYPE", "PIGEON_VIT_GRAPH"):
        monkeypatch.delenv(k, raising=False)
    if streams:
        monkeypatch.setenv("PIGEON_VIT_STREAMS", str(streams))
    else:
        monkeypatch.delenv("PIGEON_VIT_STREAMS", raising=False)
    enc = env["ops"].VitEncoder(tower["sd"], layers=LAYERS, mma_dtype=dts, **kw)
    assert enc.mma_dtype == dts
    enc.graph(graph)
    tower["encs"].append(enc)
    # the chain that runs is the chain asked for: only the folded one carves Xn2 | statpart | rsA | rsB out of the workspace
    M = 8 * X.TOKENS
    assert (_ws_bytes(env, enc, 8) > M * (4096 + 2048 + 8192) + 256) == fold
    return enc


def _ws_bytes(env, enc, n):
    need = C.c_size_t()
    env["lib"].check(env["L"].pg_vit_workspace_bytes(enc._h, n, C.byref(need)), "pg_vit_workspace_bytes")
    return need.value


def _eager(env, tower, monkeypatch, n):
    """(embedding, hidden state) of the first n images of the pool from the folded fp16 encoder with the graph off, one launch: computed
    once per n (test_every_route_of_the_fast_encoder[fold-f16] fills it) and left unchanged."""
    if tower["enc0"] is None:
        tower["enc0"] = _encoder(env, tower, monkeypatch, "fold-f16")
    c = tower["eager"]
    if n not in c:
        c[n] = tower["enc0"].forward(tower["px"][:n], return_hidden=True)
        torch.cuda.synchronize()
    return c[n]


# ================================================================================================================ every route against fp64
@pytest.mark.parametrize("route", list(ROUTES))
def test_every_route_of_the_fast_encoder(env, tower, route, monkeypatch, capsys):
    """The batch sizes are asked of pg_gemm_plan (variant 56, the chain's launches): every n in 1 .. 88 at which the signature changes,
    n - 1 of each, and 88.  Per size: EVERY hidden row within row_tol and every embedding within emb_tol of the fp64 oracle (the bounds:
    twice the restatement's own worst error over the pool, the embedding's capped at the contract 1e-3 for fp16), and hidden state and
    embedding bit-equal to the 88-image run's prefix (the five GEMM kernels are bit-identical by design, the attention is per image)."""
    fold, dts, dt = ROUTES[route]
    sizes = route_sizes(env, fold)
    kinds = {s for n in sizes for s in _sig(env, fold, n)}
    want = set(KIND_NAMES) - (set() if fold else {(0, 3)})
    missing = [KIND_NAMES[k] for k in sorted(want - kinds)]
    b = _bounds(tower, route)
    ref_h = tower["ref_h"]
    if route == "fold-f16":
        enc = None
        run = lambda n: _eager(env, tower, monkeypatch, n)
    else:
        enc = _encoder(env, tower, monkeypatch, route)
        run = lambda n: enc.forward(tower["px"][:n], return_hidden=True)
    e88, h88 = run(POOL)
    found, rec = [], {}
    for n in sizes:
        e, h = run(n)
        torch.cuda.synchronize()
        lab, worst = _label(env, fold, n), {}
        found += R.compare_hidden(h, ref_h, b["row_tol"], b["emb_tol"], emb=e, label=f"[{route}] n={n} {lab}", limit=4, worst=worst)
        same_h, same_e = torch.equal(h, h88[:n]), torch.equal(e, e88[:n])
        if not (same_h and same_e):
            rows = (h != h88[:n]).any(dim=2).nonzero()
            where = f"first at image {int(rows[0, 0])} token {int(rows[0, 1])} (row {int(rows[0, 0]) * 577 + int(rows[0, 1])}), {rows.shape[0]} rows" if rows.numel() else "hidden equal"
            found.append(f"[{route}] n={n} {lab}: not bit-equal to the {POOL}-image run's prefix (hidden {same_h}, embedding {same_e}; {where})")
        rec[n] = (lab, worst["emb"], worst["row"])
    rh, re = tower["rest"][route]                              # for the record (printed, not asserted): how closely the restatement tracks the kernels
    track = (f"[{route}] the {POOL}-image run against the RESTATEMENT itself: worst hidden row {float(R.row_errors(h88, rh).max()):.3e}, worst embedding "
             f"{float(R.emb_errors(e88, re).max()):.3e} -- what the restatement does not model")
    lines = _table(route, rec, b, track)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not missing, f"the cost model no longer produces: {missing} (a dead branch: report it)"
    assert any(r != -1 for n in sizes for (_, r) in _sig(env, fold, n)), "no cut launch among the sizes"
    _no(found)


def _table(route, rec, b, track):
    lines = [f"[{route}] batch -> (kernel, rest) of the chain's launches (0 PP6, 1 PP, 2 MID; rest -1 none, 2 MID, 3 TAIL): worst embedding / hidden-row "
             f"error vs fp64 and its ratio to the bound (emb_tol {b['emb_tol']:.3e}, row_tol {b['row_tol']:.3e})"]
    lines += [f"[{route}] n={n:3d} {lab:72s} emb {e:.3e} ({e / b['emb_tol']:.3f})  row {r:.3e} ({r / b['row_tol']:.3f})" for n, (lab, e, r) in sorted(rec.items())]
    by = {}
    for n, (lab, e, r) in sorted(rec.items()):
        o = by.setdefault(lab, [0.0, 0.0, []])
        o[0], o[1] = max(o[0], e), max(o[1], r)
        o[2].append(n)
    lines += [f"[{route}] signature {lab:72s} n = {','.join(map(str, ns)):24s} worst emb {e:.3e} ({e / b['emb_tol']:.3f} of the bound)  worst row {r:.3e} "
              f"({r / b['row_tol']:.3f})" for lab, (e, r, ns) in by.items()]
    lines.append(f"[{route}] worst of all {len(rec)} sizes: emb {max(v[1] for v in rec.values()) / b['emb_tol']:.3f} of the bound, row "
                 f"{max(v[2] for v in rec.values()) / b['row_tol']:.3f} of the bound (restatement itself: 0.500)")
    lines.append(track)
    _keep(lines)
    return lines


def test_negative_control_bf16_is_outside_the_fp16_bounds(env, tower, monkeypatch, capsys):
    """The bounds can see a wrong operand type on the device: the bf16 encoder's output at 4 images fails the fp16 bounds -- every
    embedding, and at least one row of every image.  Arithmetic only."""
    n, b = 4, _bounds(tower, "fold-f16")
    enc = _encoder(env, tower, monkeypatch, "fold-bf16")
    e, h = enc.forward(tower["px"][:n], return_hidden=True)
    torch.cuda.synchronize()
    er, ee = R.row_errors(h, tower["ref_h"][:n]), R.emb_errors(e, tower["ref_h"][:n].mean(1))
    e16, h16 = _eager(env, tower, monkeypatch, n)
    er16, ee16 = R.row_errors(h16, tower["ref_h"][:n]), R.emb_errors(e16, tower["ref_h"][:n].mean(1))
    line = (f"[negative control] bf16 operands, {n} images, against the fp16 bounds: embedding errors {[f'{float(v):.2e}' for v in ee]} (emb_tol "
            f"{b['emb_tol']:.3e}; fp16: {[f'{float(v):.2e}' for v in ee16]}); rows outside row_tol {b['row_tol']:.3e} per image "
            f"{[int(v) for v in (er > b['row_tol']).sum(1)]} of 577, smallest bf16 row error {float(er.min()):.3e} (fp16: largest {float(er16.max()):.3e})")
    _keep([line])
    with capsys.disabled():
        print("\n" + line)
    assert bool((ee > b["emb_tol"]).all()), "a bf16 embedding inside the fp16 bound: the bound cannot see a wrong operand type"
    assert bool((er > b["row_tol"]).any(dim=1).all()), "an image without a single row outside the fp16 row bound"
    assert R.compare_hidden(h, tower["ref_h"], b["row_tol"], b["emb_tol"], emb=e)
    assert bool((ee16 <= b["emb_tol"]).all()) and bool((er16 <= b["row_tol"]).all())


# ================================================================================================================ the captured graph
def test_graph_replay_at_every_route(env, tower, monkeypatch, capsys):
    """Folded fp16, the product's own single-stream capture.  Sizes in descending order (the workspace is allocated once: only n changes
    the key); each size three times -- eager first sight, capture, replay --, all three bit-equal to the graph-off result; one capture per
    key.  After more than 8 keys the first key has left the LRU: eager, capture, replay again, the same bits.  After pg_tune_gemm_mid(0)
    the next forward of a captured key re-captures, with unchanged bits at a size whose plan used gemm_mid."""
    ops, px = env["ops"], tower["px"]
    sizes = sorted(route_sizes(env, True), reverse=True)
    assert sizes[0] == POOL and len(sizes) > 9
    enc = _encoder(env, tower, monkeypatch, "fold-f16", graph=True)
    found = []

    def three(n, tag):
        want_e, want_h = _eager(env, tower, monkeypatch, n)
        r0, c0 = enc.graph()
        steps = []
        for k, what in enumerate(("eager first sight", "capture", "replay")):
            e, h = enc.forward(px[:n], return_hidden=True)
            torch.cuda.synchronize()
            if not (torch.equal(e, want_e) and torch.equal(h, want_h)):
                rows = (h != want_h).any(dim=2).nonzero()
                found.append(f"{tag} n={n} {what}: differs from the graph-off result" + (f", first at image {int(rows[0, 0])} token {int(rows[0, 1])}, "
                             f"{rows.shape[0]} rows" if rows.numel() else " (embedding only)"))
            steps.append(enc.graph())
        want = [(r0, c0), (r0 + 1, c0 + 1), (r0 + 2, c0 + 1)]
        if steps != want:
            found.append(f"{tag} n={n}: (replays, captures) after the three forwards {steps}, expected {want}")

    ws = None
    for n in sizes:
        three(n, "[graph]")
        ws = ws if ws is not None else enc._ws.data_ptr()
        assert enc._ws.data_ptr() == ws, "the workspace moved: the key changed by more than n"
    three(POOL, "[graph, evicted key]")                        # 8-entry LRU: the first key is gone, seen again as new
    # a knob: the epoch invalidates a captured graph; the LRU now holds 88 and the 7 smallest sizes
    held = [POOL] + sizes[-7:]
    mid = [n for n in held if any(2 in s for s in _sig(env, True, n))]
    assert mid, f"none of {held} runs a launch through gemm_mid"
    n = mid[0]
    want_e, want_h = _eager(env, tower, monkeypatch, n)
    before = _sig(env, True, n)
    try:
        ops.tune_gemm_mid(False)
        assert _sig(env, True, n) != before and not any(2 in s for s in _sig(env, True, n))
        r0, c0 = enc.graph()
        e, h = enc.forward(px[:n], return_hidden=True)
        torch.cuda.synchronize()
        if enc.graph() != (r0 + 1, c0 + 1):
            found.append(f"[graph, knob] n={n}: (replays, captures) {enc.graph()} after pg_tune_gemm_mid(0), expected a re-capture {(r0 + 1, c0 + 1)}")
        if not (torch.equal(e, want_e) and torch.equal(h, want_h)):
            found.append(f"[graph, knob] n={n}: the re-captured graph (gemm_mid off) differs from the graph-off result of the default plan")
    finally:
        ops.tune_gemm_mid(True)
    line = f"[graph] {len(sizes)} keys x (eager, capture, replay) + the evicted key + a re-capture at n={n} after pg_tune_gemm_mid(0): (replays, captures) = {enc.graph()}"
    _keep([line])
    with capsys.disabled():
        print("\n" + line)
    _no(found)


# ================================================================================================================ chunks, streams, buffers
def _forward_guarded(env, enc, px, n, short=0):
    """pg_vit_forward_hidden through the C ABI into buffers of the test's own: sentinel guard elements behind the embedding and the
    hidden state, pattern bytes behind the stated workspace size.  -> (rc, embedding, hidden, guards_untouched)."""
    ops, lib, L = env["ops"], env["lib"], env["L"]
    need = _ws_bytes(env, enc, n)
    ws = torch.full((need + 256 + GUARD,), WS_PATTERN, dtype=torch.uint8, device=DEV)
    off = (-ws.data_ptr()) % 256
    emb = torch.full((n * X.HIDDEN + GUARD,), X.SENTINEL, dtype=F32, device=DEV)
    hid = torch.full((n * X.TOKENS * X.HIDDEN + GUARD,), X.SENTINEL, dtype=F32, device=DEV)
    rc = L.pg_vit_forward_hidden(enc._h, ops._p(px), lib.PG_DTYPE_F32, n, ops._p(emb), ops._p(hid), C.c_void_p(ws.data_ptr() + off), need - short,
                                 ops._stream())
    torch.cuda.synchronize()
    guards = dict(emb=bool((emb[n * X.HIDDEN:] == X.SENTINEL).all()), hidden=bool((hid[n * X.TOKENS * X.HIDDEN:] == X.SENTINEL).all()),
                  workspace=bool((ws[off + need:] == WS_PATTERN).all()))
    return rc, emb, hid, guards


def test_chunks_and_streams_place_every_row(env, tower, monkeypatch):
    """max_chunk = 29 on 88 images (29 + 29 + 29 + 1), PIGEON_VIT_STREAMS=2 on 88 (44 + 44) and on 87 (44 + 43): the COMPLETE hidden
    state and every embedding bit-equal to the single-launch run; the guard regions behind both outputs and behind the workspace
    untouched.  A workspace one byte short of pg_vit_workspace_bytes is PG_ENOMEM and launches nothing (88 images, 1 and 2 streams)."""
    px = tower["px"]
    found = []
    cases = [("max_chunk=29", dict(max_chunk=29), (POOL,)), ("2 streams", dict(streams=2), (POOL, POOL - 1)), ("1 stream", dict(), (POOL,))]
    for tag, kw, ns in cases:
        enc = _encoder(env, tower, monkeypatch, "fold-f16", graph=True, **kw)
        for n in ns:
            want_e, want_h = _eager(env, tower, monkeypatch, n)
            rc, emb, hid, guards = _forward_guarded(env, enc, px, n)
            assert rc == 0, (tag, n, rc, env["L"].pg_last_error())
            found += [f"[{tag}] n={n}: the guard region behind the {k} was written" for k, ok in guards.items() if not ok]
            h = hid[:n * X.TOKENS * X.HIDDEN].view(n, X.TOKENS, X.HIDDEN)
            if not torch.equal(h, want_h):
                rows = (h != want_h).any(dim=2).nonzero()
                found.append(f"[{tag}] n={n}: hidden state differs from the single launch in {rows.shape[0]} rows, first at image {int(rows[0, 0])} token "
                             f"{int(rows[0, 1])}, last at image {int(rows[-1, 0])} token {int(rows[-1, 1])}")
            if not torch.equal(emb[:n * X.HIDDEN].view(n, X.HIDDEN), want_e):
                bad = (emb[:n * X.HIDDEN].view(n, X.HIDDEN) != want_e).any(dim=1).nonzero().flatten().tolist()
                found.append(f"[{tag}] n={n}: embeddings of images {bad[:8]} differ from the single launch")
        if tag != "max_chunk=29":
            rc, emb, hid, guards = _forward_guarded(env, enc, px, POOL, short=1)
            if rc != -2:                                                                     # PG_ENOMEM
                found.append(f"[{tag}] a workspace one byte short: rc {rc}, expected PG_ENOMEM (-2)")
            if not (bool((emb == X.SENTINEL).all()) and bool((hid == X.SENTINEL).all()) and guards["workspace"]):
                found.append(f"[{tag}] a workspace one byte short: something was launched (outputs or workspace guard written)")
    _no(found)


def test_wall_time_of_this_file(capsys):
    line = f"tests/test_gpu_fast_tier.py: {time.time() - T0:.0f} s since import"
    _keep([line])
    with capsys.disabled():
        print("\n" + line)
