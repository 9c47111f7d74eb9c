"""sample_writeback_kernel and mask_scatter_kernel (csrc/sample.hip) launched through pg_dbg_sample in every form the engine launches
them -- compact and full logits, with and without a row_map, the iteration on the host and in device memory -- and asserted three ways
per case: the draws equal oracle/draw.py bit for bit, the tokens equal a host replay of the writes, and the draws meet the float64
contract of tests/_draw_reference.py.  Every shape is tiny; the largest launch is 20 000 waves."""
import ctypes

import numpy as np
import pytest

import _draw_reference as dr
from protein_gibbs_sampler_amd import _lib

pytestmark = pytest.mark.gpu

SEED, STREAM, ROW_BASE, ITER_BASE = 0x5EED0123456789, 3, 1000, 10
PATTERN = -7


def run_entry(tokens, logits, V, compact, idx, row_map, valid, top_k, burnin, temp, first_iter, n_steps, device_iter=0, mask_idx=-1,
              permit=0, nonfinite=False):
    """-> (tokens after, sampled [n_steps][n_sel][P], masked [n_steps][n_rows][width] or None, nonfinite word or None)"""
    n_tables, n_sel, P = idx.shape
    tok = np.ascontiguousarray(tokens, dtype=np.int32).copy()
    logits = np.ascontiguousarray(logits, dtype=np.float32)
    idx = np.ascontiguousarray(idx, dtype=np.int32)
    row_map = None if row_map is None else np.ascontiguousarray(row_map, dtype=np.int32)
    params = _lib.make_sample_params(mask_idx >= 0, max(mask_idx, 0), top_k, burnin, temp, valid, SEED, STREAM, ROW_BASE, ITER_BASE)
    sampled = np.full((n_steps, n_sel, P), PATTERN, dtype=np.int32)
    masked = np.full((n_steps,) + tok.shape, PATTERN, dtype=np.int32) if mask_idx >= 0 else None
    nf = np.full(1, 77, dtype=np.uint32) if nonfinite else None
    opt = lambda a: None if a is None else _lib.ptr(a)
    _lib.check(_lib.lib().pg_dbg_sample(0, _lib.ptr(tok), tok.shape[0], tok.shape[1], _lib.ptr(logits), V, compact, _lib.ptr(idx), n_tables,
                                        opt(row_map), n_sel, P, ctypes.byref(params), first_iter, n_steps, device_iter, mask_idx, permit,
                                        _lib.ptr(sampled), opt(masked), opt(nf)))
    return tok, sampled, masked, None if nf is None else int(nf[0])


def check(tokens, logits, V, compact, idx, row_map, valid, top_k, burnin, temp, first_iter, n_steps, **kw):
    """The three assertions of every case; returns the replay and the largest ambiguous share of a step."""
    mask_idx = kw.get("mask_idx", -1)
    want = dr.replay_entry(tokens, logits, V, compact, idx, row_map, valid, top_k, burnin, temp, SEED, STREAM, ROW_BASE, ITER_BASE,
                           first_iter, n_steps, mask_idx)
    tok, sampled, masked, _ = run_entry(tokens, logits, V, compact, idx, row_map, valid, top_k, burnin, temp, first_iter, n_steps, **kw)
    assert (sampled == want.sampled).all(), "draws differ from the oracle at %s" % (np.argwhere(sampled != want.sampled)[:5].tolist(),)
    assert (tok == want.tokens).all(), "tokens differ from the host replay at %s" % (np.argwhere(tok != want.tokens)[:5].tolist(),)
    if mask_idx >= 0:
        assert (masked == want.masked).all(), "masked tokens differ at %s" % (np.argwhere(masked != want.masked)[:5].tolist(),)
    share = 0.0
    for s in range(n_steps):
        if want.exact[s] is not None:
            wrong, sh = dr.contract(want.exact[s], sampled[s].reshape(-1)[want.live[s]])
            assert len(wrong) == 0, "step %d: draws %s leave the float64 contract" % (s, want.live[s][wrong][:5].tolist())
            share = max(share, sh)
    return want, share


def make_case(seed, n_sel, P, n_tables, V, valid, compact, use_map, special=True):
    """Token rows of width P + 3, idx tables of distinct positions 1 .. width - 1 per row, logits whose every fifth row is one of the
    stacked families, and (special) one padding entry, one shadowed entry and one duplicate whose earlier copy is shadowed per table."""
    rng = np.random.default_rng([seed, n_sel, P])
    width = P + 3
    n_rows = n_sel if use_map else n_sel + 1
    row_map = rng.permutation(n_rows)[:n_sel].astype(np.int32) if use_map else None
    tokens = rng.integers(100, 200, (n_rows, width)).astype(np.int32)
    idx = np.stack([np.stack([1 + rng.permutation(width - 1)[:P] for _ in range(n_sel)]) for _ in range(n_tables)]).astype(np.int32)
    if special:
        for t in range(n_tables):
            flat = idx[t].reshape(-1)
            dup = int(rng.integers(0, n_sel)) if P > 1 else -1
            if P > 1:
                idx[t, dup, P - 1] = idx[t, dup, 0]
                idx[t, dup, 0] |= dr.BIT30
            picks = [i for i in rng.permutation(n_sel * P) if i // P != dup]
            if len(picks) > 1:
                flat[picks[0]] = -1
            if len(picks) > 2:
                flat[picks[1]] |= dr.BIT30
    nv = len(valid)
    pool = dr.stacked_rows(nv, valid, V, seed)

    def rows(n, salt):
        r = dr.embed_rows(dr.family_values("gauss3", n, nv, seed + salt), valid, V)
        r[::5] = pool[np.arange(len(r[::5])) % len(pool)]
        return r
    if compact:
        logits = np.stack([rows(n_sel * P, 10 + t) for t in range(n_tables)])
    else:
        logits = rows(n_rows * width, 10).reshape(n_rows, width, V)
    return tokens, logits, V, compact, idx, row_map


VALID20 = list(range(4, 24))


@pytest.mark.parametrize("nv", dr.N_VALID)
def test_lane_counts_k_and_temperature(nv):
    """n_valid x V x valid-list order x top_k x temperature, all families stacked, two steps with burnin between them (sample on, off)"""
    tokens = np.full((9, 4), 150, np.int32)
    idx = np.tile(np.array([[1, 3]], np.int32), (2, 9, 1))
    for V, order, top_k, temp in dr.lane_cases(nv):
        valid = dr.valid_list(nv, V, order)
        rows = dr.stacked_rows(nv, valid, V, seed=1)
        check(tokens, np.stack([rows, rows]), V, 1, idx, None, valid, top_k, 1, temp, 0, 2)


SHAPES = [(1, 1), (3, 1), (1, 3), (4, 1), (5, 1), (1, 5), (256, 1), (257, 1), (85, 3), (87, 3), (51, 5), (77, 5)]


@pytest.mark.parametrize("n_sel,P", SHAPES)
def test_entry_shapes_in_all_four_addressing_forms(n_sel, P):
    """draw counts 1, 3, 4, 5, 255 ... 261, 385: the early exit of the last workgroup's idle waves; compact / full x row_map or none"""
    for compact in (1, 0):
        for use_map in (False, True):
            case = make_case(5, n_sel, P, 1, 33, VALID20, compact, use_map)
            check(*case, VALID20, 3, 0, 0.7, 0, 1)
            check(*case, VALID20, 0, 1, None, 0, 1, mask_idx=32)


@pytest.mark.parametrize("compact", [1, 0])
@pytest.mark.parametrize("first_iter", [0, 2])
def test_iteration_in_device_memory(compact, first_iter):
    """four steps over four index tables: the form a captured graph replays (table offset, iteration, sample = it < burnin and the
    parameter block all read from device memory) gives the bits of the host form, and both the oracle's with iter_base + it"""
    valid = dr.valid_list(20, 33, "shuffled")
    for use_map in (False, True):
        case = make_case(9, 7, 3, first_iter + 4, 33, valid, compact, use_map)
        for top_k, temp, mask_idx in ((5, 0.7, 32), (0, None, -1)):
            a = case + (valid, top_k, first_iter + 2, temp, first_iter, 4)
            check(*a, device_iter=0, mask_idx=mask_idx)      # both forms hold the oracle's bits, so each holds the other's
            check(*a, device_iter=1, mask_idx=mask_idx)


def test_padding_shadow_duplicates_and_the_kernels_own_guards():
    """-1 entries and (under the permit) positions == width and shadowed positions > width: -1, nothing written, nothing masked; a
    shadowed entry is drawn but not written; of a duplicate position the later entry's draw stays"""
    width, V = 6, 33
    tokens = np.arange(100, 100 + 4 * width, dtype=np.int32).reshape(4, width)
    idx = np.array([[[1, 2, -1, 4],
                     [3 | dr.BIT30, 5, 3, -1],                      # duplicate 3: the earlier copy shadowed
                     [width, 1, (width + 2) | dr.BIT30, 2],          # the guards
                     [0x3FFFFFFF, 5 | dr.BIT30, 0, 4]]], np.int32)   # the largest position there is; position 0
    for compact in (1, 0):
        rng = np.random.default_rng(compact)
        logits = (rng.standard_normal((1, 16, V) if compact else (4, width, V)) * 3).astype(np.float32)
        for row_map in (None, np.array([2, 0, 3, 1], np.int32)):
            for mask_idx in (-1, 32):
                want, _ = check(tokens, logits, V, compact, idx, row_map, VALID20, 0, 0, None, 0, 1, mask_idx=mask_idx, permit=1)
                assert (want.sampled[0] >= 0).sum() == 11 and want.sampled[0, 2, 0] == want.sampled[0, 2, 2] == want.sampled[0, 3, 0] == -1
    with pytest.raises(_lib.PgError, match="target position 6 is out of range"):
        run_entry(tokens, logits, V, 0, idx, None, VALID20, 0, 0, None, 0, 1)


@pytest.mark.parametrize("compact", [1, 0])
def test_nonfinite_word(compact):
    """0 on finite rows; 1 for a NaN or an inf in a selected column of a selected row; 0 when it sits in an unselected column or row;
    the draws of the launch's finite rows are the oracle's all the same"""
    valid = dr.valid_list(20, 33, "shuffled")
    free = [c for c in range(33) if c not in valid][0]
    base = make_case(11, 6, 2, 1, 33, valid, compact, False)
    tokens, logits, V, _, idx, row_map = base
    dead = np.flatnonzero(idx[0].reshape(-1) < 0)[0]      # make_case's padding entry: its row is read by no draw
    flat = idx[0].reshape(-1)      # a written entry whose position no other entry of its row shares
    live = [i for i in range(12) if flat[i] >= 0 and not flat[i] & dr.BIT30 and (idx[0, i // 2] & 0x3FFFFFFF == flat[i]).sum() == 1][2]

    def row_of(lg, i):      # the logits row draw i reads (compact) / the row at token row s, position 0, which no entry selects (full)
        s, p = divmod(i, 2)
        return lg[0, i] if compact else lg[s, idx[0, s, p] & 0x3FFFFFFF]

    assert run_entry(*base, valid, 3, 0, 0.7, 0, 1, nonfinite=True)[3] == 0
    want = dr.replay_entry(*base, valid, 3, 0, 0.7, SEED, STREAM, ROW_BASE, ITER_BASE, 0, 1)
    for bad in (np.nan, np.inf, -np.inf):
        lg = logits.copy()
        row_of(lg, live)[valid[7]] = bad
        tok, sampled, _, word = run_entry(tokens, lg, V, compact, idx, row_map, valid, 3, 0, 0.7, 0, 1, nonfinite=True)
        assert word == 1
        others = np.arange(12) != live
        assert (sampled.reshape(-1)[others] == want.sampled.reshape(-1)[others]).all()
        s, p = divmod(live, 2)
        differs = np.argwhere(tok != want.tokens)
        assert all(tuple(d) == (s, idx[0, s, p] & 0x3FFFFFFF) for d in differs.tolist())
        lg = logits.copy()
        row_of(lg, live)[free] = bad                       # an unselected column of a selected row
        if compact:
            lg[0, dead, :] = bad                           # the row of a padding entry
        else:
            lg[:, 0, :] = bad                              # position 0 of every token row: selected by no entry
        tok, sampled, _, word = run_entry(tokens, lg, V, compact, idx, row_map, valid, 3, 0, 0.7, 0, 1, nonfinite=True)
        assert word == 0 and (sampled == want.sampled).all() and (tok == want.tokens).all()


@pytest.mark.parametrize("family", dr.FAMILIES)
def test_share_of_ambiguous_draws(family):
    """20 000 draws of one repeated row per case: bit for bit the oracle's, no unambiguous draw off the float64 pick, ambiguous share
    <= 1e-3"""
    n_sel, P = dr.SHARE_DRAWS // 5, 5
    tokens = np.full((n_sel, P + 1), 150, np.int32)
    idx = np.tile(np.arange(1, P + 1, dtype=np.int32), (1, n_sel, 1))
    for nv, V, top_k, temp in dr.SHARE_CASES:
        valid, row = dr.share_rows(family, nv, V)
        logits = np.repeat(row, dr.SHARE_DRAWS, axis=0)[None]
        _, share = check(tokens, logits, V, 1, idx, None, valid, top_k, 0, temp, 0, 1)
        print("%s n_valid %d top_k %d temperature %s: ambiguous share %.2e" % (family, nv, top_k, temp, share))
        assert share <= dr.SHARE_CAP


@pytest.mark.parametrize("n_sel,P", [(85, 3), (256, 1), (64, 4), (257, 1)])
def test_mask_scatter_alone(n_sel, P):
    """255 / 256 / 257 entries (the 256-thread block edge), with a row_map, through the device-side iteration at iteration 2, with
    skipped entries (-1, and positions >= width under the permit): the tokens after the scatter against a host loop, every other
    token untouched"""
    for use_map in (False, True):
        case = make_case(13, n_sel, P, 3, 33, VALID20, 1, use_map)
        idx = case[4]
        idx[2, n_sel // 2, 0] = P + 3                      # == width
        idx[2, n_sel - 1, P - 1] = (P + 9) | dr.BIT30
        for device_iter in (0, 1):
            _, _, masked, _ = run_entry(*case, VALID20, 0, 0, None, 2, 1, device_iter=device_iter, mask_idx=32, permit=1)
            exp = case[0].copy()
            for s in range(n_sel):
                for p in range(P):
                    raw = int(idx[2, s, p])
                    if raw >= 0 and (raw & 0x3FFFFFFF) < P + 3:
                        exp[case[5][s] if use_map else s, raw & 0x3FFFFFFF] = 32
            assert (masked[0] == exp).all() and (exp != case[0]).sum() >= n_sel * P - 5
            check(*case, VALID20, 0, 0, None, 2, 1, device_iter=device_iter, mask_idx=32, permit=1)


def test_public_device_entry_gives_the_same_bits():
    """pg_sample_writeback_device (full logits, the iteration a host argument) against pg_dbg_sample on the same case"""
    import torch
    for use_map in (False, True):
        tokens, logits, V, _, idx, row_map = make_case(17, 37, 6, 1, 33, VALID20, 0, use_map)
        for top_k, burnin, temp, it in ((0, 5, None, 0), (3, 0, 0.7, 0)):
            tok, sampled, _, _ = run_entry(tokens, logits, V, 0, idx, row_map, VALID20, top_k, burnin, temp, it, 1)
            d = {k: torch.from_numpy(v).to("cuda:0") for k, v in (("tok", tokens), ("log", logits), ("idx", idx[0])) }
            d_map = torch.from_numpy(row_map).to("cuda:0") if use_map else None
            d_out = torch.full(idx[0].shape, PATTERN, dtype=torch.int32, device="cuda:0")
            params = _lib.make_sample_params(False, 0, top_k, burnin, temp, VALID20, SEED, STREAM, ROW_BASE, ITER_BASE)
            p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())
            _lib.check(_lib.lib().pg_sample_writeback_device(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), p(d["tok"]),
                                                             tokens.shape[0], tokens.shape[1], p(d["log"]), V, p(d["idx"]), p(d_map),
                                                             idx.shape[1], idx.shape[2], ctypes.byref(params), it, p(d_out)))
            torch.cuda.synchronize()
            assert (d_out.cpu().numpy() == sampled[0]).all() and (d["tok"].cpu().numpy() == tok).all()
