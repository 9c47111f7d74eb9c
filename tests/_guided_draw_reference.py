"""pg_draw v2: the float32 restatement, the float64 reference with its contract, the inputs of
tests/test_guided_draw_cpu.py and tests/test_gpu_guided_draw_kernel.py, and a host replay of what pg_guided_dbg_sample launches.
Test infrastructure only; built on the pieces of tests/_draw_reference.py (pg_draw v1), which it leaves as they are.

v2 adds three things to v1, all optional.  For one draw, with the valid list j = 0 .. nv-1:

    x_j = logits[valid_idx[j]]
    x_j = fl32(x_j + bias_j)            a per-(row, position) bias in valid-list order; -inf = forbidden
    x_j = fl32(x_j / T)                 T = temps[it] with a schedule (the scalar temperature is then not read), else v1's
    stable descending rank; k as v1, then k = min(k, n_allowed), n_allowed = #{x_j > -inf} (the forbidden entries sort last)
    e_r = pg_exp(x_r - x_0), c_j sequential float32 sums, as v1
    top-p (set, < 1, and the iteration's sample flag off): q = fl32(top_p c_{k-1}), k' = min(k, 1 + #{j < k : c_j < q}); else k' = k
    t = fl32(u c_{k'-1}); pick the first j < k' with c_j > t, else k' - 1

The reference.  The bias sum and the quotient are float32 operations by contract (as the quotient is in v1) and are widened after.
With w_r = exp(s_r - s_0), C_j = w_0 + ... + w_j and F_j = C_j / C_{k-1}: the nucleus is the smallest j with
F_j >= float64(float32(top_p)), k' = j + 1, and the pick is the first j < k' with C_j / C_{k'-1} > u.

The bound.  delta(k) = (2 k + 16) 2^-24 is v1's, with the same terms: the float32 draw decides c_j > fl(u c_{k'-1}) over the first k'
terms -- v1's derivation with k' in k's place -- and the nucleus by c_j < fl(p c_{k-1}), which is the same comparison with p = float32
(top_p) in u's place over k terms.  A forbidden entry contributes w = 0 and e = 0 exactly (pg_exp flushes -inf), so it adds no error
term, and k = min(k, n_allowed) drops only such entries.

The contract.  A draw is ambiguous when some F_j, j < k - 1, lies within delta(k) of top_p (then either nucleus size is allowed) or
when, for an allowed nucleus size k', u lies within delta(k') of a boundary C_r / C_{k'-1}, r < k' - 1.  The allowed picks are the
union over the allowed nucleus sizes of v1's interval F_{j-1} - delta <= u < F_j + delta.  The share of ambiguous draws of a case is
capped at SHARE_CAP = 1e-3 as in v1; the nucleus ambiguity of a repeated row is all or nothing, so the share cases are chosen with no
F_j within delta of top_p, which the CPU test asserts.
"""
from collections import namedtuple

import numpy as np

import _draw_reference as ref
from oracle import draw as odraw

SHARE_CAP = ref.SHARE_CAP
NEG_INF = np.float32(-np.inf)


def top_p_on(top_p, sample):
    return top_p is not None and not np.isnan(top_p) and np.float32(top_p) < np.float32(1.0) and not sample


def _scores32(rows, valid_idx, bias, T):
    f32 = np.float32
    s = np.asarray(rows, dtype=f32)[:, np.asarray(valid_idx, dtype=np.int64)]
    if bias is not None:
        s = (s + np.asarray(bias, dtype=f32)).astype(f32)
    if T is not None:
        s = (s / f32(T)).astype(f32)
    return s


def _k_rows(s, top_k, sample):
    k = ref.effective_k(s.shape[1], top_k, sample)
    return k, np.maximum(np.minimum(k, (s > NEG_INF).sum(axis=1)), 1)


def draw32_guided(rows, valid_idx, top_k, sample, temperature, row_id, it, slot, stream, seed, bias=None, top_p=None):
    """v2 in numpy float32.  bias float32 [n][nv] (the table row of every draw) or None; temperature: the T of this iteration
    (temps[it] with a schedule), None = no division; top_p None / NaN = off."""
    f32 = np.float32
    n = np.asarray(rows).shape[0]
    vi = np.asarray(valid_idx, dtype=np.int64)
    s = _scores32(rows, vi, bias, temperature)
    k, k_row = _k_rows(s, top_k, sample)
    order = np.argsort(-s.astype(np.float64), axis=1, kind="stable")[:, :k]
    sv = np.take_along_axis(s, order, axis=1)
    with np.errstate(invalid="ignore"):
        e = ref._pg_exp32((sv - sv[:, :1]).astype(f32), odraw.LOG2E_F32)
    cum = np.add.accumulate(e, axis=1, dtype=f32)
    ar = np.arange(n)
    col = np.arange(k)[None, :]
    kp = k_row
    if top_p_on(top_p, sample):
        q = (f32(top_p) * cum[ar, k_row - 1]).astype(f32)
        kp = np.minimum(k_row, 1 + ((cum < q[:, None]) & (col < k_row[:, None])).sum(axis=1))
    u = ref.uniform_of(row_id, it, slot, stream, seed).astype(f32)
    t = (u * cum[ar, kp - 1]).astype(f32)
    hit = (cum > t[:, None]) & (col < kp[:, None])
    j = np.where(hit.any(axis=1), hit.argmax(axis=1), kp - 1)
    return vi[order[ar, j]].astype(np.int32)


ExactGuided = namedtuple("ExactGuided", "pick ambiguous nucleus_ambiguous ranked allowed u F k_row k_nucleus")


def exact_draw_guided(rows, valid_idx, top_k, sample, temperature, row_id, it, slot, stream, seed, bias=None, top_p=None):
    """pick int32 [n]: the reference's token; ambiguous bool [n] (either kind); nucleus_ambiguous bool [n]; ranked int64 [n][k]: the
    tokens in rank order; allowed bool [n][k]: the ranks a float32 draw may pick; F [n][k]: C_j / C_{k-1} before the nucleus cut."""
    n = np.asarray(rows).shape[0]
    vi = np.asarray(valid_idx, dtype=np.int64)
    s32 = _scores32(rows, vi, bias, temperature)
    k, k_row = _k_rows(s32, top_k, sample)
    s = s32.astype(np.float64)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    ss = np.take_along_axis(s, order, axis=1)
    with np.errstate(invalid="ignore"):
        w = np.exp(ss - ss[:, :1])
    col = np.arange(k)[None, :]
    w = np.where(col < k_row[:, None], w, 0.0)
    C = np.cumsum(w, axis=1)
    ar = np.arange(n)
    F = C / C[ar, k_row - 1][:, None]
    u = ref.uniform_of(row_id, it, slot, stream, seed)
    if top_p_on(top_p, sample):
        p = np.float64(np.float32(top_p))
        d_n = np.array([ref.delta(int(x)) for x in k_row])[:, None]
        inner = col < (k_row[:, None] - 1)      # j < k - 1: F_{k-1} = 1 ends every nucleus
        k_nuc = np.minimum(k_row, 1 + ((F < p) & (col < k_row[:, None])).sum(axis=1))
        nuc_amb = ((np.abs(F - p) <= d_n) & inner).any(axis=1)
        kp_lo = np.minimum(k_row, 1 + ((F < p - d_n) & inner).sum(axis=1))
        kp_hi = np.minimum(k_row, 1 + ((F <= p + d_n) & inner).sum(axis=1))
    else:
        k_nuc, nuc_amb, kp_lo, kp_hi = k_row, np.zeros(n, bool), k_row, k_row
    allowed = np.zeros((n, k), dtype=bool)
    ambiguous = nuc_amb.copy()
    pick_rank = np.zeros(n, dtype=np.int64)
    for kp in range(1, k + 1):
        sel = np.flatnonzero((kp_lo <= kp) & (kp <= kp_hi))
        if not len(sel):
            continue
        d = ref.delta(kp)
        Fp = C[sel, :kp] / C[sel, kp - 1][:, None]
        Fp[:, -1] = 1.0
        us = u[sel][:, None]
        before = np.concatenate([np.full((len(sel), 1), -np.inf), Fp[:, :-1]], axis=1)
        upper = Fp + d
        upper[:, -1] = np.inf
        allowed[sel[:, None], np.arange(kp)[None, :]] |= (before - d <= us) & (us < upper)
        ambiguous[sel] |= (np.abs(Fp[:, :kp - 1] - us) <= d).any(axis=1)
        own = k_nuc[sel] == kp
        pick_rank[sel[own]] = (Fp[own] > us[own]).argmax(axis=1)
    ranked = vi[order]
    return ExactGuided(ranked[ar, pick_rank].astype(np.int32), ambiguous, nuc_amb, ranked, allowed, u, F, k_row, k_nuc)


def contract_guided(ex, got):
    """(indices of the draws that break the contract, share of ambiguous draws)."""
    got = np.asarray(got).astype(np.int64)
    at = ex.ranked == got[:, None]
    ok = (at & ex.allowed).any(axis=1)
    return np.flatnonzero(~ok), float(ex.ambiguous.mean())


def nucleus_margin(ex, top_p):
    """min over rows and j < k - 1 of |F_j - top_p| / delta(k): > 1 everywhere means no nucleus-ambiguous row."""
    p = np.float64(np.float32(top_p))
    col = np.arange(ex.F.shape[1])[None, :]
    inner = col < (ex.k_row[:, None] - 1)
    d = np.array([ref.delta(int(x)) for x in ex.k_row])[:, None]
    r = np.where(inner, np.abs(ex.F - p) / d, np.inf)
    return float(r.min())


# ---- bias tables ------------------------------------------------------------------------------------------------------------------------
def bias_table(bias_rows, width, nv, seed, forbid_counts=(0, 1, -2, -1), scale=2.0):
    """float32 [bias_rows][width][nv]: finite N(0, scale) entries; cell (r, p) forbids forbid_counts[(r * width + p) % len] entries
    (a negative count c means nv + c), never all of them."""
    rng = np.random.default_rng([seed, bias_rows, width, nv])
    t = (rng.standard_normal((bias_rows, width, nv)) * scale).astype(np.float32)
    for r in range(bias_rows):
        for p in range(width):
            c = forbid_counts[(r * width + p) % len(forbid_counts)]
            c = nv + c if c < 0 else c
            c = max(0, min(c, nv - 1))
            t[r, p, rng.permutation(nv)[:c]] = NEG_INF
    return t


# the share cases of the issue: (n_valid, V, top_k, top_p, scalar temperature, schedule, forbidden entries, biased)
GuidedShare = namedtuple("GuidedShare", "nv V top_k top_p temperature schedule n_forbidden biased")
SHARE_CASES_GUIDED = (
    GuidedShare(32, 33, 0, 0.9, None, (1.7, 1.0, 0.6), 0, False),
    GuidedShare(20, 33, 5, 0.5, None, None, 0, True),
    GuidedShare(20, 33, 0, None, 0.7, None, 12, False),
)
SHARE_FAMILIES = ("gauss3", "two_level", "descending", "dominant")


def share_bias(case, seed=5):
    if not case.biased and not case.n_forbidden:
        return None
    rng = np.random.default_rng([seed, case.nv])
    b = (rng.standard_normal(case.nv) * 1.5).astype(np.float32) if case.biased else np.zeros(case.nv, np.float32)
    b[rng.permutation(case.nv)[:case.n_forbidden]] = NEG_INF
    return b


# ---- what pg_guided_dbg_sample launches, replayed on the host -----------------------------------------------------------------------
def replay_entry_guided(tokens, logits, V, compact, idx, row_map, valid, top_k, burnin, temperature, seed, stream, row_id_base,
                        iter_base, first_iter, n_steps, mask_idx=-1, bias=None, temps=None, top_p=None, draw=draw32_guided):
    """replay_entry of _draw_reference with a guide: bias float32 [bias_rows][width][nv] (bias_rows 1 or n_rows; read at the TOKEN row)
    or None, temps [n_temps] or None (step s draws at temps[first_iter + s]; the scalar temperature is then not read), top_p."""
    tokens = np.array(tokens, dtype=np.int32)
    n_rows, width = tokens.shape
    n_tables, n_sel, P = idx.shape
    sampled = np.full((n_steps, n_sel, P), -1, dtype=np.int32)
    masked = np.empty((n_steps, n_rows, width), dtype=np.int32) if mask_idx >= 0 else None
    exact, lives = [], []
    trow = np.arange(n_sel) if row_map is None else np.asarray(row_map)
    for s in range(n_steps):
        it = first_iter + s
        raw = idx[it].reshape(-1).astype(np.int64)
        pos = raw & 0x3FFFFFFF
        live = np.flatnonzero((raw >= 0) & (pos < width))
        sel, slot = live // P, live % P
        if mask_idx >= 0:
            tokens[trow[sel], pos[live]] = mask_idx
            masked[s] = tokens
        rows = np.asarray(logits)[it].reshape(-1, V)[live] if compact else np.asarray(logits)[trow[sel], pos[live]]
        b = None
        if bias is not None:
            b = bias[trow[sel] if bias.shape[0] > 1 else np.zeros(len(live), np.int64), pos[live]]
        T = temperature if temps is None else float(np.float32(temps[it]))
        args = (rows, valid, top_k, it < burnin, T, row_id_base + sel, iter_base + it, slot, stream, seed)
        want = draw(*args, bias=b, top_p=top_p) if len(live) else np.zeros(0, np.int32)
        sampled[s].reshape(-1)[live] = want
        for i, tok in zip(live, want):      # in entry order: the last write to a position wins
            if not raw[i] & ref.BIT30:
                tokens[trow[i // P], pos[i]] = tok
        exact.append(exact_draw_guided(*args, bias=b, top_p=top_p) if len(live) else None)
        lives.append(live)
    return ref.Replay(sampled, masked, tokens, exact, lives)
