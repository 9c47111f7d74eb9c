"""sample_writeback_kernel<true> (pg_draw v2, csrc/sample.hip) launched through pg_guided_dbg_sample in the forms the engine launches it,
asserted per case as tests/test_gpu_draw_kernel.py asserts v1: the draws equal the float32 restatement of
tests/_guided_draw_reference.py bit for bit, the tokens equal a host replay of the writes, and the draws meet the float64 contract.
Every shape is tiny; the largest launch is 20 000 waves."""
import ctypes

import numpy as np
import pytest

import _draw_reference as dr
import _guided_draw_reference as gr
from protein_gibbs_sampler_amd import _lib

pytestmark = pytest.mark.gpu

SEED, STREAM, ROW_BASE, ITER_BASE = 0x5EED0123456789, 3, 1000, 10
PATTERN = -7
WRONG_T = 123.0      # the scalar temperature handed in next to a schedule: never read


def run_entry(tokens, logits, V, compact, idx, row_map, valid, top_k, burnin, temp, first_iter, n_steps, bias=None, temps=None, top_p=None,
              device_iter=0, mask_idx=-1, permit=0, guided=True):
    """-> (tokens after, sampled [n_steps][n_sel][P], masked or None); guided False: pg_dbg_sample itself"""
    n_tables, n_sel, P = idx.shape
    tok = np.ascontiguousarray(tokens, dtype=np.int32).copy()
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    row_map = None if row_map is None else np.ascontiguousarray(row_map, dtype=np.int32)
    params = _lib.make_sample_params(mask_idx >= 0, max(mask_idx, 0), top_k, burnin, temp, valid, SEED, STREAM, ROW_BASE, ITER_BASE)
    sampled = np.full((n_steps, n_sel, P), PATTERN, dtype=np.int32)
    masked = np.full((n_steps,) + tok.shape, PATTERN, dtype=np.int32) if mask_idx >= 0 else None
    opt = lambda a: None if a is None else _lib.ptr(a)
    args = (0, _lib.ptr(tok), tok.shape[0], tok.shape[1], _lib.ptr(logits), V, compact, _lib.ptr(idx), n_tables, opt(row_map), n_sel, P,
            ctypes.byref(params), first_iter, n_steps, device_iter, mask_idx, permit, _lib.ptr(sampled), opt(masked), None)
    if guided:
        g, keep = _lib.make_draw_guide(bias, temps, top_p)
        _lib.check(_lib.lib().pg_guided_dbg_sample(*args, ctypes.byref(g)))
    else:
        _lib.check(_lib.lib().pg_dbg_sample(*args))
    return tok, sampled, masked


def check(tokens, logits, V, compact, idx, row_map, valid, top_k, burnin, temp, first_iter, n_steps, bias=None, temps=None, top_p=None, **kw):
    """The three assertions of every case; the scalar temperature is WRONG_T whenever a schedule is there.  Returns the replay and
    the largest ambiguous share of a step."""
    mask_idx = kw.get("mask_idx", -1)
    want = gr.replay_entry_guided(tokens, logits, V, compact, idx, row_map, valid, top_k, burnin, temp, SEED, STREAM, ROW_BASE, ITER_BASE,
                                  first_iter, n_steps, mask_idx, bias=bias, temps=temps, top_p=top_p)
    tok, sampled, masked = run_entry(tokens, logits, V, compact, idx, row_map, valid, top_k, burnin, WRONG_T if temps is not None else temp,
                                     first_iter, n_steps, bias, temps, top_p, **kw)
    assert (sampled == want.sampled).all(), "draws differ from the restatement at %s" % (np.argwhere(sampled != want.sampled)[:5].tolist(),)
    assert (tok == want.tokens).all(), "tokens differ from the host replay at %s" % (np.argwhere(tok != want.tokens)[:5].tolist(),)
    if mask_idx >= 0:
        assert (masked == want.masked).all(), "masked tokens differ at %s" % (np.argwhere(masked != want.masked)[:5].tolist(),)
    share = 0.0
    for s in range(n_steps):
        if want.exact[s] is not None:
            wrong, sh = gr.contract_guided(want.exact[s], sampled[s].reshape(-1)[want.live[s]])
            assert len(wrong) == 0, "step %d: draws %s leave the float64 contract" % (s, want.live[s][wrong][:5].tolist())
            share = max(share, sh)
    return want, share


FORMS = ("bias", "schedule", "top_p", "all")
TOP_PS = (0.1, 0.5, 0.9, 1.0)


def guide_of(form, top_p, bias, temps):
    return dict(bias=bias if form in ("bias", "all") else None, temps=temps if form in ("schedule", "all") else None,
                top_p=top_p if form in ("top_p", "all") else None)


@pytest.mark.parametrize("nv", (1, 2, 3, 20, 32))
def test_lane_and_parameter_cases(nv):
    """n_valid x V x guide form x top_k x top_p, every family stacked, two steps with burn-in between them (sample on, then off), the
    bias table cycling through 0, 1, nv - 2 and nv - 1 forbidden entries per position"""
    tokens = np.full((9, 4), 150, np.int32)
    idx = np.tile(np.array([[1, 3]], np.int32), (2, 9, 1))
    temps = [1.6, 0.6]
    for V in dr.vocab_sizes(nv):
        valid = dr.valid_list(nv, V, "shuffled")
        rows = dr.stacked_rows(nv, valid, V, seed=1)
        logits = np.stack([rows, rows])
        for n_bias_rows in (1, 9):
            bias = gr.bias_table(n_bias_rows, 4, nv, seed=V)
            for top_k in sorted({0, 1, nv - 1, nv + 1}):
                for form in FORMS:
                    for top_p in (TOP_PS if form in ("top_p", "all") else (None,)):
                        if n_bias_rows == 9 and form not in ("bias", "all"):
                            continue
                        check(tokens, logits, V, 1, idx, None, valid, top_k, 1, 0.7, 0, 2, **guide_of(form, top_p, bias, temps))


def shape_case(seed, compact, V, valid, n_tables):
    """n_sel = 5 selected rows of 6 token rows through a row_map that permutes them, P = 3, width = 7; per table one padding entry, one
    shadowed entry and one duplicate whose earlier copy is shadowed"""
    rng = np.random.default_rng([seed, compact])
    n_sel, P, width, n_rows = 5, 3, 7, 6
    row_map = rng.permutation(n_rows)[:n_sel].astype(np.int32)
    assert (row_map != np.arange(n_sel)).any()
    tokens = rng.integers(100, 200, (n_rows, width)).astype(np.int32)
    idx = np.stack([np.stack([1 + rng.permutation(width - 1)[:P] for _ in range(n_sel)]) for _ in range(n_tables)]).astype(np.int32)
    for t in range(n_tables):
        idx[t, t % n_sel, P - 1] = idx[t, t % n_sel, 0]
        idx[t, t % n_sel, 0] |= dr.BIT30
        idx[t, (t + 1) % n_sel, 1] = -1
        idx[t, (t + 2) % n_sel, 2] |= dr.BIT30
    nv = len(valid)
    if compact:
        logits = np.stack([dr.embed_rows(dr.family_values("gauss3", n_sel * P, nv, seed + t), valid, V) for t in range(n_tables)])
    else:
        logits = dr.embed_rows(dr.family_values("gauss3", n_rows * width, nv, seed), valid, V).reshape(n_rows, width, V)
    return tokens, logits, V, compact, idx, row_map


@pytest.mark.parametrize("compact", [1, 0])
@pytest.mark.parametrize("first_iter", [0, 2])
def test_rows_schedule_and_device_iteration(compact, first_iter):
    """three steps, a different temperature each, the schedule indexed by the call-local iteration (first_iter 2 starts at its third
    entry); a shared and a per-token-row bias table under a row_map that permutes the rows (a table read at the selected row instead of
    the token row shows); the iteration and the guide's pointers on the host (device_iter 0) and in the state block (1); the scalar
    temperature set to a wrong value throughout"""
    valid = dr.valid_list(20, 33, "shuffled")
    case = shape_case(21, compact, 33, valid, first_iter + 3)
    temps = [2.5, 1.7, 1.0, 0.6, 0.3][:first_iter + 3]
    rows_differ = False
    for n_bias_rows in (1, 6):
        bias = gr.bias_table(n_bias_rows, 7, 20, seed=3)
        for device_iter in (0, 1):
            for top_k, top_p, mask_idx in ((0, 0.9, 32), (5, None, -1)):
                a = case + (valid, top_k, first_iter + 1, 0.7, first_iter, 3)
                want, _ = check(*a, bias=bias, temps=temps, top_p=top_p, device_iter=device_iter, mask_idx=mask_idx)
                check(*a, temps=temps, device_iter=device_iter, mask_idx=mask_idx)
        if n_bias_rows == 6:      # the case can tell the token row from the selected row: the replay read at s gives other draws
            wrong_rows = gr.replay_entry_guided(*case[:5], None, valid, 0, first_iter + 1, 0.7, SEED, STREAM, ROW_BASE, ITER_BASE, first_iter, 3,
                                                -1, bias=bias, temps=temps, top_p=0.9)
            right = gr.replay_entry_guided(*case, valid, 0, first_iter + 1, 0.7, SEED, STREAM, ROW_BASE, ITER_BASE, first_iter, 3, -1, bias=bias,
                                           temps=temps, top_p=0.9)
            rows_differ = compact == 0 or (wrong_rows.sampled != right.sampled).any()
    assert rows_differ
    # the schedule matters: the scalar temperature in its place gives other draws on this case
    flat = gr.replay_entry_guided(*case, valid, 0, first_iter + 1, WRONG_T, SEED, STREAM, ROW_BASE, ITER_BASE, first_iter, 3, -1)
    sched = gr.replay_entry_guided(*case, valid, 0, first_iter + 1, WRONG_T, SEED, STREAM, ROW_BASE, ITER_BASE, first_iter, 3, -1, temps=temps)
    assert (flat.sampled != sched.sampled).any()


def test_bias_contents():
    """positions with 0, 1, nv - 2 and nv - 1 forbidden entries; a forbidden entry that holds the largest logit; top_k above the allowed
    count; a finite bias that reorders the ranks; a bias that merges two levels into a tie (lowest valid-list position first)"""
    nv, V, width, P = 20, 33, 6, 5
    valid = dr.valid_list(nv, V, "shuffled")
    n_sel = 100
    n = n_sel * P
    values = dr.family_values("gauss3", n, nv, 8)
    a, b = np.float32(1.5), np.float32(1.25)
    values[0::P] -= np.float32(8.0)                                        # slot 0 (position 1): the two levels are the row's top
    values[0::P, 3], values[0::P, 11] = a, b
    bias = np.zeros((1, width, nv), np.float32)
    bias[0, 1, 11] = a - b                                                 # merged into a tie; nothing forbidden here
    assert np.float32(b + bias[0, 1, 11]) == a
    dead2 = np.argsort(-values.mean(axis=0))[:nv - 2]
    bias[0, 2, dead2] = -np.inf                                            # nv - 2 forbidden
    values[1::P, dead2[0]] = 30.0                                          # ... one of which holds the row's largest logit
    bias[0, 3, :] = np.linspace(6, -6, nv, dtype=np.float32)               # reorders the ranks
    bias[0, 4, 1:] = -np.inf                                               # nv - 1 forbidden: one residue left
    bias[0, 5, 7] = -np.inf                                                # one forbidden
    tokens = np.full((n_sel, width), 150, np.int32)
    idx = np.tile(np.arange(1, P + 1, dtype=np.int32), (1, n_sel, 1))
    logits = dr.embed_rows(values, valid, V)[None]
    for top_k, top_p, temp in ((0, None, None), (5, None, 0.7), (5, 0.5, None), (nv - 1, 0.9, 7.5), (1, None, None)):
        want, _ = check(tokens, logits, V, 1, idx, None, valid, top_k, 0, temp, 0, 1, bias=bias, top_p=top_p)
        s = want.sampled[0]
        k_row = want.exact[0].k_row.reshape(n_sel, P)
        assert (s[:, 3] == valid[0]).all()                                 # the one residue left
        assert set(s[:, 1].tolist()) <= {valid[j] for j in np.flatnonzero(bias[0, 2] > -np.inf)}
        assert valid[7] not in set(s[:, 4].tolist())
        k = dr.effective_k(nv, top_k, False)
        assert (k_row[:, 0] == k).all() and (k_row[:, 1] == min(k, 2)).all() and (k_row[:, 3] == 1).all() and (k_row[:, 4] == min(k, nv - 1)).all()
    # the tie: with top_k 1 position 1 picks entry 3, the lower valid-list position of the merged level
    want, _ = check(tokens, logits, V, 1, idx, None, valid, 1, 0, None, 0, 1, bias=bias)
    top_is_level = values[0::P].max(axis=1) == a
    assert top_is_level.sum() > n_sel // 2 and (want.sampled[0][top_is_level, 0] == valid[3]).all()
    # the reorder: without the bias position 3 draws other tokens
    plain = gr.replay_entry_guided(tokens, logits, V, 1, idx, None, valid, 1, 0, None, SEED, STREAM, ROW_BASE, ITER_BASE, 0, 1)
    assert (plain.sampled[0][:, 2] != want.sampled[0][:, 2]).any()


def test_padding_shadow_and_guards_as_v1():
    width, V = 6, 33
    valid = list(range(4, 24))
    tokens = np.arange(100, 100 + 4 * width, dtype=np.int32).reshape(4, width)
    idx = np.array([[[1, 2, -1, 4],
                     [3 | dr.BIT30, 5, 3, -1],
                     [width, 1, (width + 2) | dr.BIT30, 2],
                     [0x3FFFFFFF, 5 | dr.BIT30, 0, 4]]], np.int32)
    bias = gr.bias_table(4, width, 20, seed=1)
    for compact in (1, 0):
        rng = np.random.default_rng(compact)
        logits = (rng.standard_normal((1, 16, V) if compact else (4, width, V)) * 3).astype(np.float32)
        for row_map in (None, np.array([2, 0, 3, 1], np.int32)):
            for mask_idx in (-1, 32):
                want, _ = check(tokens, logits, V, compact, idx, row_map, valid, 0, 0, None, 0, 1, bias=bias, temps=[0.8], top_p=0.9,
                                mask_idx=mask_idx, permit=1)
                assert (want.sampled[0] >= 0).sum() == 11 and want.sampled[0, 2, 0] == want.sampled[0, 2, 2] == want.sampled[0, 3, 0] == -1
    with pytest.raises(_lib.PgError, match="target position 6 is out of range"):
        run_entry(tokens, logits, V, 0, idx, None, valid, 0, 0, None, 0, 1, bias=bias)


@pytest.mark.parametrize("device_iter", [0, 1])
def test_empty_guide_gives_pg_dbg_sample_bits(device_iter):
    valid = dr.valid_list(20, 33, "shuffled")
    for compact in (1, 0):
        case = shape_case(31, compact, 33, valid, 3)
        a = case + (valid, 5, 1, 0.7, 0, 3)
        v1 = run_entry(*a, device_iter=device_iter, mask_idx=32, guided=False)
        for kw in (dict(), dict(top_p=1.0), dict(top_p=float("nan"))):
            v2 = run_entry(*a, device_iter=device_iter, mask_idx=32, **kw)
            assert all((x == y).all() for x, y in zip(v1, v2))
        # and a zero bias, a schedule of the scalar temperature and top_p just below 1 on a nucleus that is the whole list anyway
        # take the v2 kernel to the same bits
        v2 = run_entry(*a, device_iter=device_iter, mask_idx=32, bias=np.zeros((1, 7, 20), np.float32), temps=[0.7, 0.7, 0.7])
        assert all((x == y).all() for x, y in zip(v1, v2))


def test_public_guided_device_entry_gives_the_same_bits():
    """pg_sample_writeback_guided_device (full logits, device tables, the iteration a host argument) against the debug entry"""
    import torch
    valid = list(range(4, 24))
    for use_map in (False, True):
        rng = np.random.default_rng(17 + use_map)
        n_sel, P, width = 37, 6, 9
        n_rows = n_sel if use_map else n_sel + 1
        row_map = rng.permutation(n_rows)[:n_sel].astype(np.int32) if use_map else None
        tokens = rng.integers(100, 200, (n_rows, width)).astype(np.int32)
        idx = np.stack([1 + rng.permutation(width - 1)[:P] for _ in range(n_sel)])[None].astype(np.int32)
        logits = dr.embed_rows(dr.family_values("gauss3", n_rows * width, 20, 3), valid, 33).reshape(n_rows, width, 33)
        temps = np.array([1.5, 0.9, 0.4], np.float32)
        for bias_rows, top_k, burnin, top_p, it in ((1, 0, 0, 0.9, 2), (n_rows, 3, 0, None, 1), (n_rows, 0, 5, 0.5, 0)):
            bias = gr.bias_table(bias_rows, width, 20, seed=9)
            # the debug entry at first_iter = it reads table `it`: hand it the same table under every index
            idx_t = np.repeat(idx, it + 1, axis=0)
            tok, sampled, _ = run_entry(tokens, logits, 33, 0, idx_t, row_map, valid, top_k, burnin, WRONG_T, it, 1, bias=bias, temps=temps,
                                        top_p=top_p)
            d = {k: torch.from_numpy(v).to("cuda:0") for k, v in (("tok", tokens), ("log", logits), ("idx", idx[0]), ("bias", bias),
                                                                   ("temps", temps))}
            d_map = torch.from_numpy(row_map).to("cuda:0") if use_map else None
            d_out = torch.full(idx[0].shape, PATTERN, dtype=torch.int32, device="cuda:0")
            params = _lib.make_sample_params(False, 0, top_k, burnin, WRONG_T, valid, SEED, STREAM, ROW_BASE, ITER_BASE)
            p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
            _lib.check(_lib.lib().pg_sample_writeback_guided_device(
                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(d["tok"]), n_rows, width, p(d["log"]), 33, p(d["idx"]), p(d_map),
                n_sel, P, ctypes.byref(params), it, p(d_out), p(d["bias"]), bias_rows, p(d["temps"]), len(temps),
                float("nan") if top_p is None else top_p))
            torch.cuda.synchronize()
            assert (d_out.cpu().numpy() == sampled[0]).all() and (d["tok"].cpu().numpy() == tok).all()
    # what the entry can check without reading the tables
    L = _lib.lib()
    args = (None, p(d["tok"]), n_rows, width, p(d["log"]), 33, p(d["idx"]), None, n_sel, P, ctypes.byref(params))
    for tail, text in (((3, None, p(d["bias"]), n_rows, p(d["temps"]), 3, float("nan")), "3 entries, the call 4 iterations"),
                       ((0, None, p(d["bias"]), 2, None, 0, float("nan")), "neither 1 nor the call's"),
                       ((0, None, None, 0, None, 0, 1.5), "top_p must be in (0, 1]")):
        assert L.pg_sample_writeback_guided_device(*args, *tail) == _lib.PG_ERR_INVALID
        assert text in L.pg_last_error().decode()


@pytest.mark.parametrize("family", gr.SHARE_FAMILIES)
@pytest.mark.parametrize("case", gr.SHARE_CASES_GUIDED, ids=lambda c: "nv%d_k%d_p%s" % (c.nv, c.top_k, c.top_p))
def test_share_of_ambiguous_draws(case, family):
    """20 000 draws of one repeated row per case and step: bit for bit the restatement's, no unambiguous draw off the float64 pick,
    ambiguous share <= 1e-3 (tests/test_guided_draw_cpu.py asserts that no row of these cases is nucleus-ambiguous)"""
    n_sel, P = dr.SHARE_DRAWS // 5, 5
    n_steps = len(case.schedule) if case.schedule else 1
    tokens = np.full((n_sel, P + 1), 150, np.int32)
    idx = np.tile(np.arange(1, P + 1, dtype=np.int32), (n_steps, n_sel, 1))
    valid, row = dr.share_rows(family, case.nv, case.V)
    logits = np.repeat(np.repeat(row, dr.SHARE_DRAWS, axis=0)[None], n_steps, axis=0)
    b = gr.share_bias(case)
    bias = None if b is None else np.repeat(b[None, None, :], P + 1, axis=1)
    want, share = check(tokens, logits, case.V, 1, idx, None, valid, case.top_k, 0, case.temperature, 0, n_steps, bias=bias,
                        temps=case.schedule, top_p=case.top_p)
    print("%s %s: ambiguous share %.2e" % (family, case, share))
    assert share <= gr.SHARE_CAP
    assert not any(ex.nucleus_ambiguous.any() for ex in want.exact)
