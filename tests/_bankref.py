"""Float64 statement of the refiner's certainty for a bank whose rows carry an error (pg_refine_certainty_bank), written from the
error model and not from the kernel.  numpy only.  tests/test_bankref_cpu.py pins it (sigma = 0 is tests/_decisionref.py's
restatement, six planted mistakes are caught, a Monte Carlo over bank perturbations agrees with what it calls certain);
tests/test_gpu_bank_certainty.py holds the kernel to it.

The model.  A decision has a margin m >= 0, a gradient g with respect to the query e, a systematic part |e| g.beta and a random part
N(0, (eps |e| |g| / 32)^2).  Every bank row p is off by |p| r_p, r_p of relative RMS norm eps_b in an unknown direction, independent
from row to row.  A distance |e - p| then moves by -u . delta_p, standard deviation eps_b |p| / 32.  With

    num = m - |e| g.beta      A = |e| |g| / 32      Bk = sigma sqrt(bsum) / 32      sigma = kappa eps_b

and bsum the sum of w^2 |row|^2 over the bank rows that enter the decision, the decision survives a query error eps when
num > kappa sqrt(eps^2 A^2 + eps_b^2 B^2), B = sqrt(bsum) / 32; solved for kappa eps:

    any NaN                       0
    sigma == 0 or bsum == 0       the expression without a bank term, unchanged
    num <= Bk                     0
    g2 == 0                       +inf
    otherwise                     sqrt((num - Bk) (num + Bk)) / A

What enters bsum:
    candidate-score pairs (codes 1000 + j and the pair half of 2000 + j)   the nearest prototype of each of the two candidates,
                                                                           w = 1 / T; an empty cell adds nothing
    nearest prototype (3000 / 3001), farthest member (4000 / 4001)         the picked row and the alternative row, w = 1
    set-boundary margins (the t_in half of 2000 + j, 2999)                 nothing

MISTAKES: keyword switches that each turn on one deliberate error, for the CPU tests to catch."""
import numpy as np

from _decisionref import DIM, F32, candidate_record, q_mean32, record_ints, select

MISTAKES = ("no_inv_t", "winner_only", "boundary_term", "query_norm", "drop_farthest", "empty_norm")


def tol_plain(m, g, beta, en):
    """the expression without a bank term, in _decisionref._tol's order of operations"""
    g2 = float(g @ g)
    if not np.isfinite(m) and m > 0:
        return np.inf
    if g2 == 0:
        return np.inf
    return (m - en * float(g @ beta)) / (en * np.sqrt(g2) / 32.0)


def tol_bank(m, g, beta, en, sigma, bsum):
    if sigma == 0 or bsum == 0:
        return tol_plain(m, g, beta, en)
    g2, gb = float(g @ g), float(g @ beta)
    if np.isnan(m) or np.isnan(g2) or np.isnan(gb) or np.isnan(en) or np.isnan(bsum):
        return 0.0
    num = m - en * gb
    bk = sigma * np.sqrt(bsum) / 32.0
    if num <= bk:
        return 0.0
    if g2 == 0:
        return np.inf
    return np.sqrt((num - bk) * (num + bk)) / (en * np.sqrt(g2) / 32.0)


def decisions(rec, ints, L, cand, topk, n_eval, C, W, bankp, bankt, e, beta, wmax, wbmax, T, r, ch, fin_r, cell_off, member_off,
              member_idx, sigma, mistake=None):
    """-> every decision of one row as (tolerance, code), in the order of the codes' list above; [(inf, 0)] / [(0, -9)] for the rows
    decided before any margin is looked at.  Arguments as _decisionref._refine_tol_restated, plus sigma."""
    assert mistake is None or mistake in MISTAKES
    en = np.linalg.norm(e)
    S = L + rec[:, 0] / T
    if ints[r, 0] < 0 and all(ints[j, 0] < 0 for j in range(topk)):
        return [(np.inf, 0)]
    if not (fin_r >= 1e-30) or ints[r, 0] < 0:
        return [(0.0, -9)]

    def n2(row):
        return en * en if mistake == "query_norm" else float(row @ row)

    def proto_n2(p):
        if p < 0:
            return n2(bankp[0]) if mistake == "empty_norm" else 0.0
        return n2(bankp[p])

    def pair_s(a, j):
        pa, pj = ints[a, 0], ints[j, 0]
        da, dj = -rec[a, 0], -rec[j, 0]
        ia = (1.0 / T) / da if (pa >= 0 and da > 0) else 0.0
        ij = (1.0 / T) / dj if (pj >= 0 and dj > 0) else 0.0
        g = W[cand[a]] - W[cand[j]] + (ia * bankp[pa] if pa >= 0 else 0) - (ij * bankp[pj] if pj >= 0 else 0) + (ij - ia) * e
        w2 = 1.0 if mistake == "no_inv_t" else (1.0 / T) ** 2
        bsum = w2 * (proto_n2(pa) + (0.0 if mistake == "winner_only" else proto_n2(pj)))
        return tol_bank(S[a] - S[j], g, beta, en, sigma, bsum)
    out = []
    for j in range(topk):
        if j != r:
            out.append((pair_s(r, j), 1000 + j))
    for j in range(topk, n_eval):
        bsum = (proto_n2(ints[topk - 1, 0]) + proto_n2(ints[j, 0])) / T ** 2 if mistake == "boundary_term" else 0.0
        t_in = tol_bank(L[topk - 1] - L[j], W[cand[topk - 1]] - W[cand[j]], beta, en, sigma, bsum)
        out.append((t_in if r == topk - 1 else max(t_in, pair_s(r, j)), 2000 + j))
    if n_eval > topk and n_eval < C:
        gmax = np.linalg.norm(W[cand[topk - 1]]) + wmax
        out.append(((L[topk - 1] - L[n_eval - 1] - en * (float(W[cand[topk - 1]] @ beta) + wbmax)) / (en * gmax / 32.0), 2999))
    for which, x in enumerate((r, ch)):
        if which == 1 and ch == r:
            break
        p1, t1 = ints[x, 0], ints[x, 2]
        if p1 >= 0:
            w = e - bankp[p1]
            dw = np.linalg.norm(w)
            for j in range(cell_off[cand[x]], cell_off[cand[x] + 1]):
                if j == p1:
                    continue
                l = e - bankp[j]
                dl = np.linalg.norm(l)
                bsum = n2(bankp[p1]) + (0.0 if mistake == "winner_only" else n2(bankp[j]))
                out.append((tol_bank(dl - dw, l / dl - w / dw, beta, en, sigma, bsum), 3000 + which))
        if t1 >= 0 and p1 >= 0:
            w = e - bankt[t1]
            dw = np.linalg.norm(w)
            for jj in range(member_off[p1], member_off[p1 + 1]):
                j = member_idx[jj]
                if j == t1:
                    continue
                l = e - bankt[j]
                dl = np.linalg.norm(l)
                bsum = 0.0 if mistake == "drop_farthest" else n2(bankt[t1]) + (0.0 if mistake == "winner_only" else n2(bankt[j]))
                out.append((tol_bank(dw - dl, w / dw - l / dl, beta, en, sigma, bsum), 4000 + which))
    return out or [(np.inf, 0)]


def refine_tol_bank(*args, **kw):
    """-> (tol, code, rival): the row's tolerance, the code of the first decision that attains it (0 when nothing can change the row)
    and the smallest tolerance among the decisions of ANOTHER code (inf: none) -- the code is only decided where the two differ."""
    best, code = np.inf, 0
    ds = decisions(*args, **kw)
    for t, c in ds:
        if t < best:
            best, code = t, c
    rival = min([t for t, c in ds if c != code], default=np.inf)
    return best, code, rival


# ================================================================================================================ cases
def make_row(bank, q, cand, prob, topk, n_eval, T, init=(0.0, 0.0), max_km=1e9):
    """One query against `bank` (anything with HostBank's fields), without a GPU: the records refine_candidates_kernel would leave
    (tests/_decisionref.candidate_record), the selection, and the arguments of `decisions` that depend on the row.
    q (P,1024) fp32, cand (k,) cells, prob (k,) fp32 or None."""
    q = np.asarray(q, dtype=F32).reshape(-1, DIM)
    e32 = q_mean32(q[None])[0]
    recs = [candidate_record(bank, e32, int(c))[1] for c in cand[:n_eval]]
    rec = np.stack(recs)
    cp = np.asarray(prob, dtype=F32) if prob is not None else np.array([1.0] + [0.0] * (len(cand) - 1), dtype=F32)
    sel = select(rec[:topk, 0], cp[:topk], T, np.asarray(init, dtype=np.float64), rec[:topk, 1:3], max_km)
    r, ch = sel["refined"], sel["choice"]
    with np.errstate(divide="ignore", under="ignore", invalid="ignore"):
        L = np.log(cp[:n_eval]).astype(np.float64)                 # fp32 log, as the kernel takes it
        ex = np.exp((rec[:topk, 0] / F32(T)).astype(F32)).astype(F32)
        fin_r = float(cp[r]) * float(ex[r] / ex.sum(dtype=F32))
    return dict(rec=rec.astype(np.float64), rec32=rec, ints=record_ints(rec)[:, :4], L=L, cand=np.asarray(cand), e=e32.astype(np.float64),
                r=r, ch=ch, fin_r=fin_r)


def row_args(row, topk, n_eval, C, W, bank, beta, wmax, wbmax, T):
    """the positional arguments of `decisions` / _refine_tol_restated up to fin_r, and the three CSR keywords"""
    pos = (row["rec"], row["ints"], row["L"], row["cand"], topk, n_eval, C, W, bank.proto_emb.astype(np.float64),
           bank.train_emb.astype(np.float64), row["e"], beta, wmax, wbmax, T, row["r"], row["ch"], row["fin_r"])
    return pos, dict(cell_off=bank.cell_off, member_off=bank.member_off, member_idx=bank.member_idx)


# ================================================================================================================ Monte Carlo
def refine64(bankp, bankt, bank, e, cand, logp, topk, T):
    """The refinement in float64 on (possibly perturbed) bank rows: -> (winning candidate, its nearest prototype, the farthest
    member of that prototype's cluster or -1).  No veto (the callers set max_km out of reach)."""
    score, pick = np.full(topk, -np.inf), [-1] * topk
    for j in range(topk):
        lo, hi = int(bank.cell_off[cand[j]]), int(bank.cell_off[cand[j] + 1])
        if hi > lo:
            d = np.linalg.norm(bankp[lo:hi] - e, axis=1)
            pick[j] = lo + int(np.argmin(d))
            score[j] = logp[j] - d.min() / T
        else:
            score[j] = logp[j] - 100000.0 / T
    r = int(np.argmax(score))
    p = pick[r]
    far = -1
    if p >= 0 and bank.proto_count[p] > 1:
        mem = bank.member_idx[int(bank.member_off[p]):int(bank.member_off[p + 1])]
        far = int(mem[int(np.argmax(np.linalg.norm(bankt[mem] - e, axis=1)))])
    return r, p, far


def perturb(rows, eps_b, rng):
    """rows + |row| r, r Gaussian of relative RMS norm eps_b: the model's bank error, independent per row"""
    z = rng.standard_normal(rows.shape)
    return rows + np.linalg.norm(rows, axis=1, keepdims=True) * (eps_b / np.sqrt(rows.shape[1])) * z
