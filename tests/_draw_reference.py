"""Float64 reference of the token draw (pg_draw v1), the contract a float32 draw is held to against it, the
input families and parameter sets of tests/test_draw_reference_cpu.py and tests/test_gpu_draw_kernel.py, and a host replay of what
pg_dbg_sample launches.  Test infrastructure only.

The reference.  For one draw with scores s_0 >= s_1 >= ... >= s_{k-1} (the float32 logits at valid_idx, divided in float32 by the
temperature when there is one -- that quotient is generate_step's own float32 operation --, widened to float64 and put in stable
descending order, ties lowest valid-list position first; k = n_valid when sample, top_k <= 0 or top_k > n_valid, else top_k):

    w_r = exp(s_r - s_0)      F_j = (w_0 + ... + w_j) / (w_0 + ... + w_{k-1})      pick = first j with F_j > u

u = (word 0 of Philox4x32-10 with counter (row id, iteration, slot, stream) and key (seed lo, seed hi)) >> 8, times 2^-24: exact in
float32 and float64 alike.  The generator below is this module's own; it shares no code with oracle/draw.py.

The bound.  A float32 draw (oracle/draw.py, csrc/sample.hip) computes e_r, c_j = fl(c_{j-1} + e_r), t = fl(u c_{k-1}) and picks the
first j with c_j > t, else k - 1.  Put F^_j = c_j / t * u; the float32 draw picks the first j with F^_j > u, so it can differ from the
reference only where u lies within max_j |F^_j - F_j| of a boundary F_j, j < k - 1 (at j = k - 1 both pick k - 1 whatever is left).
With v = 2^-24, T = sum_r w_r >= 1, and to first order in v (the second-order terms are below (2 k v)^2 < 2e-11):

  1. x^_r = fl(s_r - s_0) = x_r (1 + d1), |d1| <= v.
  2. z^_r = fl(x^_r L^) with L^ = float32(log2 e) = log2 e (1 - 0.23 v): z^ = z (1 + th), |th| <= 2.23 v, so 2^z^ = w_r exp(x_r th):
     a relative error of 2.23 v |x_r|, an absolute one of 2.23 v |x_r| w_r <= 2.23 v / e = 0.82 v  (|x| e^-|x| <= 1 / e).
     A term with z^ < -126 is flushed to 0: w_r < 2^-126 there, an absolute error below 1.2e-38.
  3. f = fl(z^ - floor(z^)) is off by at most v / 2 (z^ in (-1/2, 0) has a finer grid than f in (1/2, 1)): 2^f off by ln 2 v / 2 =
     0.35 v relative.
  4. the degree-6 polynomial against 2^f on [0, 1], in exact arithmetic with its float32 coefficients: 0.24 v relative
     (test_polynomial_error evaluates it in float64 on 2^20 + 1 points and asserts <= 0.3 v).
  5. Horner in float32, six multiply-add pairs on a value that ends in [1, 2): v (last add) + v / 2 + v / 2 + v / 4 + v / 8 + ... <=
     2.5 v; the exponent is then added exactly.
     So e_r = w_r (1 + eta_r) with |eta_r| <= 2.23 v |x_r| + b v, b = 0.35 + 0.3 + 2.5 = 3.15, and eta_0 = 0 (pg_exp(0) = 1).
  6. the k - 1 ordered additions.  With phi = (exact sum of e_0 .. e_j) / (exact sum of all e_r), c_j = E_j (1 + a_j), |a_j| <= j v, and
     c_{k-1} = c_j (1 + g1) + (E_{k-1} - E_j)(1 + g2), |g1|, |g2| <= (k - 1 - j) v:  c_j / c_{k-1} is off phi by at most
     phi ((1 - phi) j + (k - 1 - j)) v <= (k - 1) v.
  7. t = fl(u c_{k-1}): one more v.
  The e_r enter numerator and denominator: F_j (beta_j - beta_{k-1}) with beta_j = sum_{r <= j} w_r eta_r / C_j is at most
  sum_r w_r |eta_r| / T <= b v + 2.23 v sum_r |x_r| w_r / T <= b v + 0.82 (k - 1) v.

  max_j |F^_j - F_j| <= ((k - 1)(1 + 0.82) + 1 + 3.15) v < (2 k + 16) v = delta(k).

delta is the issue's figure; the derivation above shows it to be an upper bound with room (1.82 k + 2.4 against 2 k + 16), and it is
used as stated, not the tighter sum.  Nothing in it was measured on a kernel.

The contract.  A draw is *ambiguous* when |F_r - u| <= delta for some r < k - 1.  A draw that is not must equal the reference's pick.
An ambiguous one may be any j with F_{j-1} - delta <= u < F_j + delta -- either neighbour of the boundary, or further where several
boundaries coincide within delta (flushed or tied-to-zero terms).  The share of ambiguous draws of a case is capped at 1e-3; its
expectation is at most 2 delta (k - 1), 3.0e-4 at k = 32.
"""
from collections import namedtuple

import numpy as np

from oracle import draw as odraw

V24 = 2.0 ** -24
SHARE_CAP = 1e-3


def delta(k):
    return (2 * k + 16) * V24


def effective_k(n_valid, top_k, sample):
    return n_valid if (sample or top_k <= 0 or top_k > n_valid) else top_k


# ---- Philox4x32-10, this module's own ---------------------------------------------------------------------------------------------
_MUL_A, _MUL_B = 0xD2511F53, 0xCD9E8D57
_WEYL_A, _WEYL_B = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)


def _mulhilo(m, x):
    p = np.uint64(m) * x          # 32 x 32 bits: fits in 64
    return p >> np.uint64(32), p & _LOW


def philox4x32_10(counter, key):
    """counter: four broadcastable integer arrays (words 0 .. 3); key: two ints.  Returns the four output words as uint32 arrays."""
    x = [np.asarray(c).astype(np.int64).astype(np.uint64) & _LOW for c in np.broadcast_arrays(*[np.asarray(c) for c in counter])]
    ka, kb = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        hi_a, lo_a = _mulhilo(_MUL_A, x[0])
        hi_b, lo_b = _mulhilo(_MUL_B, x[2])
        x = [hi_b ^ x[1] ^ np.uint64(ka), lo_b, hi_a ^ x[3] ^ np.uint64(kb), lo_a]
        ka, kb = (ka + _WEYL_A) & 0xFFFFFFFF, (kb + _WEYL_B) & 0xFFFFFFFF
    return [w.astype(np.uint32) for w in x]


def uniform_of(row_id, it, slot, stream, seed, word=0, counter_order=(0, 1, 2, 3)):
    """u of DESIGN.md section 5 as float64; word / counter_order exist for the mutated draws of the CPU test."""
    n = len(np.asarray(row_id))
    c = [np.asarray(row_id), np.full(n, int(it)), np.asarray(slot), np.full(n, int(stream))]
    w = philox4x32_10([c[i] for i in counter_order], (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[word]
    return (w >> np.uint32(8)).astype(np.float64) * V24


Exact = namedtuple("Exact", "pick ambiguous ranked lo hi u F k")


def exact_draw(rows, valid_idx, top_k, sample, temperature, row_id, it, slot, stream, seed):
    """rows float32 [n][V].  pick int32 [n]: the reference's token; ambiguous bool [n]; ranked int64 [n][k]: the tokens in rank order;
    lo, hi [n]: the ranks a float32 draw may pick (lo == hi == the reference's rank where the draw is not ambiguous)."""
    rows = np.asarray(rows, dtype=np.float32)
    n = rows.shape[0]
    vi = np.asarray(valid_idx, dtype=np.int64)
    k = effective_k(len(vi), top_k, sample)
    s32 = rows[:, vi]
    if temperature is not None:
        s32 = s32 / np.float32(temperature)
        assert s32.dtype == np.float32
    s = s32.astype(np.float64)
    order = np.argsort(-s, axis=1, kind="stable")[:, :k]
    ss = np.take_along_axis(s, order, axis=1)
    F = np.cumsum(np.exp(ss - ss[:, :1]), axis=1)
    F /= F[:, -1:].copy()
    F[:, -1] = 1.0
    u = uniform_of(row_id, it, slot, stream, seed)[:, None]
    d = delta(k)
    rank = (F > u).argmax(axis=1)
    ambiguous = (np.abs(F[:, :k - 1] - u) <= d).any(axis=1)
    lo = (F + d > u).argmax(axis=1)
    before = np.concatenate([np.full((n, 1), -np.inf), F[:, :-1]], axis=1)
    hi = k - 1 - (before - d <= u)[:, ::-1].argmax(axis=1)
    lo, hi = np.where(ambiguous, lo, rank), np.where(ambiguous, hi, rank)
    ranked = vi[order]
    return Exact(ranked[np.arange(n), rank].astype(np.int32), ambiguous, ranked, lo, hi, u[:, 0], F, k)


def contract(ex, got):
    """(indices of the draws that break the contract, share of ambiguous draws)."""
    got = np.asarray(got).astype(np.int64)
    at = ex.ranked == got[:, None]
    rank = np.where(at.any(axis=1), at.argmax(axis=1), -1)
    return np.flatnonzero((rank < ex.lo) | (rank > ex.hi)), float(ex.ambiguous.mean())


# ---- the float32 draw restated with one switch per mutation (mutate None: oracle/draw.py bit for bit) -------------------------------
MUTATIONS = ("ties_highest_index_first", "k_one_too_small", "k_one_too_large", "cumulative_sum_in_lane_order", "philox_word_1",
             "iteration_and_slot_swapped", "temperature_after_the_cut", "exp2_without_log2e")
# A change of rounding alone -- the same terms summed in rank order from the other end -- is not one of them: it moves a pick only
# where u sits within a few 2^-24 of a boundary, which the contract allows by construction and which 1.08 million draws of the share
# cases did not show once against the oracle's bits.  The CPU test holds it to the contract and asserts nothing more of it.
ROUNDING_ONLY = "cumulative_sum_reversed"


def _pg_exp32(x, scale):
    f32 = np.float32
    z = (x * f32(scale)).astype(f32)
    flush = z < f32(-126.0)
    z = np.where(flush, f32(0.0), z).astype(f32)
    n = np.floor(z).astype(f32)
    f = (z - n).astype(f32)
    p = np.full_like(f, odraw.EXP2_COEF[6])
    for c in odraw.EXP2_COEF[5::-1]:
        p = ((p * f).astype(f32) + c).astype(f32)
    out = (p.view(np.int32) + (n.astype(np.int32) << 23)).view(f32)
    return np.where(flush, f32(0.0), out).astype(f32)


def draw32(rows, valid_idx, top_k, sample, temperature, row_id, it, slot, stream, seed, mutate=None):
    assert mutate is None or mutate in MUTATIONS or mutate == ROUNDING_ONLY
    f32 = np.float32
    rows = np.asarray(rows, dtype=f32)
    n = rows.shape[0]
    vi = np.asarray(valid_idx, dtype=np.int64)
    nv = len(vi)
    k = effective_k(nv, top_k, sample)
    if mutate == "k_one_too_small":
        k = max(k - 1, 1)
    if mutate == "k_one_too_large":
        k = min(k + 1, nv)
    s = rows[:, vi]
    late = mutate == "temperature_after_the_cut"
    if temperature is not None and not late:
        s = (s / f32(temperature)).astype(f32)
    if mutate == "ties_highest_index_first":
        order = nv - 1 - np.argsort(-s[:, ::-1].astype(np.float64), axis=1, kind="stable")
    else:
        order = np.argsort(-s.astype(np.float64), axis=1, kind="stable")
    top = np.take_along_axis(s, order[:, :1], axis=1)      # s_0, the largest score
    order = order[:, :k]
    if mutate == "cumulative_sum_in_lane_order":      # the top k, summed and picked in valid-list order
        order = np.sort(order, axis=1)
    sv = np.take_along_axis(s, order, axis=1)
    if temperature is not None and late:
        sv, top = (sv / f32(temperature)).astype(f32), (top / f32(temperature)).astype(f32)
    e = _pg_exp32((sv - top).astype(f32), 1.0 if mutate == "exp2_without_log2e" else odraw.LOG2E_F32)
    if mutate == "cumulative_sum_reversed":      # c_j = e_j + e_{j-1} + ... + e_0, each a sequential float32 sum
        cum = np.stack([np.add.accumulate(e[:, j::-1], axis=1, dtype=f32)[:, -1] for j in range(k)], axis=1)
    else:
        cum = np.add.accumulate(e, axis=1, dtype=f32)
    u = uniform_of(row_id, it, slot, stream, seed, word=1 if mutate == "philox_word_1" else 0,
                   counter_order=(0, 2, 1, 3) if mutate == "iteration_and_slot_swapped" else (0, 1, 2, 3)).astype(f32)
    t = (u * cum[:, -1]).astype(f32)
    hit = cum > t[:, None]
    j = np.where(hit.any(axis=1), hit.argmax(axis=1), k - 1)
    return vi[order[np.arange(n), j]].astype(np.int32)


# ---- input families: values in valid-list order, [n][nv] float32 ----------------------------------------------------------------------
FAMILIES = ("gauss3", "equal", "two_level", "two_level_merge", "descending", "ascending", "steep40", "flush_edge", "dominant")


def flush_edge_pair():
    """(x_flushed, x_kept): the adjacent float32 values either side of pg_exp's flush, fl(x float32(log2 e)) < -126 and >= -126."""
    x = np.float32(-126.0 / 1.4426950408889634)
    flushed = lambda v: np.float32(v * odraw.LOG2E_F32) < np.float32(-126.0)
    while not flushed(x):
        x = np.nextafter(x, np.float32(-np.inf))
    while flushed(np.nextafter(x, np.float32(0.0))):
        x = np.nextafter(x, np.float32(0.0))
    return x, np.nextafter(x, np.float32(0.0))


def merge_levels(temperature=7.5):
    """Two adjacent float32 values whose float32 quotients by the temperature are equal."""
    a = np.float32(7.75)
    while True:
        b = np.nextafter(a, np.float32(np.inf))
        if a / np.float32(temperature) == b / np.float32(temperature):
            return a, b
        a = b


def family_values(name, n, nv, seed):
    rng = np.random.default_rng([seed, FAMILIES.index(name), nv])
    g = rng.standard_normal((n, nv))
    if name == "gauss3":
        v = g * 3
    elif name == "equal":
        v = np.repeat(0.75 * (np.arange(n) % 3 - 1.0)[:, None], nv, axis=1)
    elif name == "two_level":
        v = np.where(rng.random((n, nv)) < 0.5, 1.5, -0.25)
    elif name == "two_level_merge":      # the lower level first, so that ranking before and after the division differ
        a, b = merge_levels()
        v = np.where(rng.random((n, nv)) < 0.5, a, b)
        v[:, 0] = a
        if nv > 1:
            v[:, -1] = b
    elif name == "descending":
        v = -np.sort(-g * 3, axis=1)
    elif name == "ascending":
        v = np.sort(g * 3, axis=1)
    elif name == "steep40":
        v = g * 40
    elif name == "flush_edge":      # the top score is 0, so s_r - s_0 is s_r itself
        v = -np.abs(g) - 0.1
        x_flushed, x_kept = flush_edge_pair()
        for r in range(n):
            p = rng.permutation(nv)
            v[r, p[0]] = 0.0
            if nv > 1:
                v[r, p[1]] = x_flushed if (r % 2 == 0 or nv == 2) else x_kept
            if nv > 2:
                v[r, p[2]] = x_kept if r % 2 == 0 else x_flushed
    elif name == "dominant":
        v = g.copy()
        v[np.arange(n), rng.integers(0, nv, n)] += 30.0
    else:
        raise KeyError(name)
    return v.astype(np.float32)


UNSELECTED = np.float32(60.0)      # what every column outside valid_idx holds: it would win every draw if it were read


def embed_rows(values, valid_idx, V):
    rows = np.full((values.shape[0], V), UNSELECTED, dtype=np.float32)
    rows[:, np.asarray(valid_idx)] = values
    return rows


def valid_list(nv, V, order, seed=0):
    """nv distinct columns of 0 .. V-1 that hold V-1 and (nv >= 2) 0, ascending, descending or shuffled."""
    rng = np.random.default_rng([seed, nv, V])
    keep = {V - 1} if nv == 1 else {0, V - 1}
    rest = [c for c in rng.permutation(V) if c not in keep]
    cols = sorted(keep | set(int(c) for c in rest[:nv - len(keep)]))
    assert len(cols) == nv
    if order == "descending":
        cols = cols[::-1]
    elif order == "shuffled":
        cols = [cols[i] for i in rng.permutation(nv)]
    return cols


N_VALID = (1, 2, 3, 19, 20, 31, 32)
ORDERS = ("ascending", "descending", "shuffled")
TEMPERATURES = (None, 0.05, 0.7, 7.5)


def vocab_sizes(nv):
    return sorted({nv, 33, 64} - {v for v in (33, 64) if v < nv})


def top_ks(nv):
    return sorted({0, 1, 2, nv - 1, nv, nv + 1} - {-1})


def lane_cases(nv):
    """Every (V, order, top_k, temperature) of the lane-count test for one n_valid; each runs with sample on and off."""
    return [(V, order, top_k, temp) for V in vocab_sizes(nv) for order in ORDERS for top_k in top_ks(nv) for temp in TEMPERATURES]


ROWS_PER_FAMILY = 2


def stacked_rows(nv, valid, V, seed):
    """ROWS_PER_FAMILY rows of every family, stacked: float32 [len(FAMILIES) * ROWS_PER_FAMILY][V]."""
    return np.concatenate([embed_rows(family_values(f, ROWS_PER_FAMILY, nv, seed), valid, V) for f in FAMILIES])


# the share-cap cases: (n_valid, V, top_k, temperature), 20 000 draws of one repeated row per family each
SHARE_DRAWS = 20000
SHARE_CASES = ((32, 33, 0, None), (32, 64, 31, 7.5), (20, 33, 5, 0.7), (20, 33, 40, 0.05), (5, 33, 0, 1.3), (2, 33, 0, None))


def share_rows(family, nv, V, seed=3):
    valid = valid_list(nv, V, "shuffled", seed)
    row = embed_rows(family_values(family, 2, nv, seed)[1:], valid, V)
    return valid, row


# ---- what pg_dbg_sample launches, replayed on the host -----------------------------------------------------------------------------
BIT30 = 1 << 30
Replay = namedtuple("Replay", "sampled masked tokens exact live")


def replay_entry(tokens, logits, V, compact, idx, row_map, valid, top_k, burnin, temperature, seed, stream, row_id_base, iter_base,
                 first_iter, n_steps, mask_idx=-1, draw=odraw.draw_rows):
    """tokens [n_rows][width]; idx [n_tables][n_sel][P]; logits compact [n_tables][n_sel*P][V] or full [n_rows][width][V].
    sampled [n_steps][n_sel][P] by `draw` (-1 for padding and positions >= width); masked [n_steps][n_rows][width] (None without a
    mask step); tokens after the run: writes in entry order, a shadowed entry (bit 30) drawn but not written; exact[s]: the float64
    reference of step s's live draws, live[s] their flat indices."""
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
        args = (rows, valid, top_k, it < burnin, temperature, row_id_base + sel, iter_base + it, slot, stream, seed)
        want = draw(*args) if len(live) else np.zeros(0, np.int32)
        sampled[s].reshape(-1)[live] = want
        for i, tok in zip(live, want):      # in entry order: the last write to a position wins
            if not raw[i] & BIT30:
                tokens[trow[i // P], pos[i]] = tok
        exact.append(exact_draw(*args) if len(live) else None)
        lives.append(live)
    return Replay(sampled, masked, tokens, exact, lives)
