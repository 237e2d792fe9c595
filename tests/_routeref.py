"""A geocell head with PLANTED top-1 margins, built in float64 from measured embeddings (numpy only; nothing of the code under test).

tests/test_gpu_embedding_route.py measures, on a 2-layer tower, the embeddings the embed path writes (`fast`) and the exact
encoder's (`exact`) for n panoramas, panel means in float64, eps_i = fast_i - exact_i.  `plant_head` builds C = 2 n + 32 cells:

    W[a_i] = A u_i                     u_i: the unit vector along the part of exact_i orthogonal to every other exact_j
                                       (A capped per row where fp32 could not resolve the margin otherwise: RESOLVE below)
    W[b_i] = W[a_i] + D_i              D_i = L o_i - (m_i / (exact_i . u_i)) u_i
    background cells                   small seeded weights
    bias                               0 for the background; for the pair of row i just enough below 0 to stay under every other
                                       row's top logit on its FAST embedding too (on the exact one the pair answers with 0)

o_i is a seeded random unit vector orthogonal to ALL exact_j (drawn without looking at eps_i: the error model's random direction,
not a worst case), its sign chosen so that the fast embedding moves the margin towards b_i.  On exact_i the logits are A (exact_i .
u_i) for a_i, m_i less for b_i, and 0 for the pair of every other row (each plus its bias); with the planted margin

    m_i = f_i |L (o_i . eps_i)|        f_i cycling through F_CYCLE

the top-1 computed from fast_i is b_i exactly where f_i < 1.  The head is stored in fp32: every quantity below (`m`, the logits, the
reference argmax) is computed in float64 FROM THE ROUNDED fp32 weights, i.e. from what the model under test is given; the rounding of
W[b_i] moves the planted margin by up to 1e-9 A |e|, so m_i is corrected until the margin of the rounded weights is the planted one.
"""
import numpy as np

F_CYCLE = (0.25, 0.5, 2.0, 4.0, 16.0, 64.0, 1024.0, 65536.0)
N_BACKGROUND = 32
# One A for every row cannot be had in an fp32 head: the smallest planted margin (f = 0.25) is 2.6e5 times smaller than the largest
# (f = 65536), every other cell has to lie 100 of the LARGEST margins below A (exact_i . u_i), so the smallest margin would be
# 4e-8 of the logits it separates -- a third of an fp32 ulp, for the model under test and for the fp32 reference alike.  A is
# therefore capped per row at RESOLVE planted margins: W[a_i] = min(A, RESOLVE m_i / (exact_i . u_i)) u_i.  Every planted margin
# is then at least 2^-14 of its row's top logit (2^10 ulps), the rows with the largest margins (f = 65536, the larger ones of
# f = 1024) keep the one A, and for a capped row every cell other than b_i is still 2^14 L / A times further away, in units of the
# tolerance, than b_i is (150 times at A = 109, what the 2-layer tower gives).
RESOLVE = 2.0 ** 14


def panel_means(images, n):
    """(4 n, 1024) per-image embeddings -> (n, 1024) float64 panel means."""
    return np.asarray(images, dtype=np.float64).reshape((n, 4, -1)).mean(axis=1)


def _orthogonal_part(v, basis):
    """v minus its projection on the row space of `basis` (least squares, float64)."""
    coef, *_ = np.linalg.lstsq(basis.T, v, rcond=None)
    return v - basis.T @ coef


def plant_head(exact, eps, seed=0, A=None, L=1.0, background=1e-3, f_cycle=F_CYCLE, resolve=RESOLVE):
    """exact, eps: (n, 1024) float64.  Returns a dict: W (C, 1024) float32, bias (C,) float32, a, b (n,) cell indices,
    f, m (n,) the factor and the planted margin of every row, o (n, 1024), r (n,) = exact_i . u_i, A (n,) the scale of every
    W[a_i] (see RESOLVE), L.
    A None: the smallest A that puts every other cell 128 planted margins below (the preconditions ask for 100)."""
    exact, eps = np.asarray(exact, dtype=np.float64), np.asarray(eps, dtype=np.float64)
    n, d = exact.shape
    rng = np.random.default_rng(seed)
    u, r = np.zeros((n, d)), np.zeros(n)
    for i in range(n):
        p = _orthogonal_part(exact[i], np.delete(exact, i, axis=0))
        u[i] = p / np.linalg.norm(p)
        r[i] = exact[i] @ u[i]
    o = np.zeros((n, d))
    for i in range(n):
        p = _orthogonal_part(rng.standard_normal(d), exact)
        o[i] = p / np.linalg.norm(p)
    o *= np.where((o * eps).sum(axis=1) >= 0, 1.0, -1.0)[:, None]          # fast moves (b_i - a_i) up: D_i . eps_i = +L |o_i . eps_i| - ...
    f = np.array([f_cycle[i % len(f_cycle)] for i in range(n)])
    shift = L * np.abs((o * eps).sum(axis=1))                               # what the fast embedding's error moves the margin by
    m = f * shift
    bg = rng.standard_normal((N_BACKGROUND, d)) * (background / np.sqrt(d))
    bg_top = float(np.abs(exact @ bg.T).max())
    if A is None:
        A = float(((128.0 * m + bg_top) / r).max())
    A = np.minimum(A, resolve * m / r)                                       # per row: see RESOLVE
    a, b = np.arange(n), n + np.arange(n)
    W = np.zeros((2 * n + N_BACKGROUND, d), dtype=np.float32)
    W[a] = (A[:, None] * u).astype(np.float32)
    W[2 * n:] = bg.astype(np.float32)
    Wa = W[a].astype(np.float64)
    coef = m / r
    for _ in range(4):                                                      # the margin OF THE ROUNDED WEIGHTS is the planted one
        W[b] = (Wa + L * o - coef[:, None] * u).astype(np.float32)
        got = ((Wa - W[b].astype(np.float64)) * exact).sum(axis=1)
        coef += (m - got) / r
    m_is = ((Wa - W[b].astype(np.float64)) * exact).sum(axis=1)
    # the pair of row j answers exact_i (i != j) with exactly 0 and fast_i with W[a_j] . eps_i, which for a row at the one A is more
    # than a capped row's own top logit: its bias keeps it below 0 on every other row's fast embedding as well
    bias = np.zeros((W.shape[0],), dtype=np.float32)
    cross = np.abs(eps @ W[:2 * n].astype(np.float64).T)
    cross[np.arange(n), a], cross[np.arange(n), b] = 0.0, 0.0
    bias[a] = bias[b] = (-2.0 * np.maximum(cross[:, a].max(axis=0), cross[:, b].max(axis=0))).astype(np.float32)
    return dict(W=W, bias=bias, a=a, b=b, f=f, m=m_is, m_planted=m, shift=shift, o=o, u=u, r=r,
                A=A, L=L)


def logits64(emb, head):
    return np.asarray(emb, dtype=np.float64) @ head['W'].astype(np.float64).T + head['bias'].astype(np.float64)


def reference_top1(exact, head):
    """THE reference: the float64 argmax of exact @ W.T + bias."""
    return np.argmax(logits64(exact, head), axis=1)


def check_preconditions(exact, fast, head):
    """Properties of the INPUTS, in float64: on `exact` the top-1 is a_i, b_i is second, every other cell lies at least 100 planted
    margins below b_i, the logits stay below 1e3; on `fast` the top-1 is b_i exactly where f_i < 1.  Returns a list of complaints
    (empty: all hold)."""
    bad = []
    le, lf = logits64(exact, head), logits64(fast, head)
    a, b, f, m = head['a'], head['b'], head['f'], head['m']
    if not (np.abs(le).max() < 1e3 and np.abs(lf).max() < 1e3):
        bad.append(f'logits reach {max(np.abs(le).max(), np.abs(lf).max()):.4g}')
    order = np.argsort(-le, axis=1, kind='stable')
    for i in range(len(a)):
        if order[i, 0] != a[i] or order[i, 1] != b[i]:
            bad.append(f'row {i} (f {f[i]:g}): exact ranks {order[i, :2].tolist()}, planted {[int(a[i]), int(b[i])]}')
            continue
        if not m[i] > 0:
            bad.append(f'row {i} (f {f[i]:g}): planted margin {m[i]:.3g}')
        gap = le[i, b[i]] - le[i, order[i, 2]]
        if gap < 100.0 * m[i]:
            bad.append(f'row {i} (f {f[i]:g}): third cell {gap / m[i]:.1f} planted margins below the second')
        top_fast = int(np.argmax(lf[i]))
        want = b[i] if f[i] < 1 else a[i]
        if top_fast != want:
            bad.append(f'row {i} (f {f[i]:g}): fast top-1 {top_fast}, expected {int(want)}')
    return bad


def random_direction_score(head, eps):
    """max_i |o_i . eps_i| * 32 / |eps|_rms: how far the planted directions are from a typical draw of the error model (a random
    direction has |o . eps| ~ |eps| / 32 in 1024 dimensions)."""
    eps = np.asarray(eps, dtype=np.float64)
    rms = np.sqrt((eps ** 2).sum(axis=1).mean())
    return float(np.abs((head['o'] * eps).sum(axis=1)).max() * 32.0 / rms)
