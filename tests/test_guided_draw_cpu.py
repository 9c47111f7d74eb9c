"""pg_draw v2 without a GPU: the float32 restatement of tests/_guided_draw_reference.py against oracle/draw.py (empty guide) and against
its own float64 contract, forbidden entries under forced uniforms, the DrawGuide compiler, annealing schedules, the ctypes mirror of
pg_draw_guide, and the host refusals of pg_guided_dbg_sample / pg_engine_set_draw_guide, which precede any device lookup."""
import ctypes

import numpy as np
import pytest

import _draw_reference as dr
import _guided_draw_reference as gr
from oracle import draw as odraw
from protein_gibbs_sampler_amd import _lib, guides

SEED, STREAM = 0x5EED0123456789, 3


# ---- empty guide == pg_draw v1 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", dr.N_VALID)
def test_empty_guide_is_v1_bit_for_bit(nv):
    n = len(dr.FAMILIES) * dr.ROWS_PER_FAMILY
    row_id, slot = 1000 + np.arange(n), np.arange(n) % 3
    for V, order, top_k, temp in dr.lane_cases(nv):
        valid = dr.valid_list(nv, V, order)
        rows = dr.stacked_rows(nv, valid, V, seed=1)
        for sample in (True, False):
            args = (rows, valid, top_k, sample, temp, row_id, 12, slot, STREAM, SEED)
            want = odraw.draw_rows(*args)
            assert (gr.draw32_guided(*args) == want).all()
            assert (gr.draw32_guided(*args, bias=None, top_p=1.0) == want).all()      # top_p 1 is off
            assert (gr.draw32_guided(*args, bias=np.zeros((n, nv), np.float32), top_p=float("nan")) == want).all()
            ex = gr.exact_draw_guided(*args)
            v1 = dr.exact_draw(*args)
            assert (ex.pick == v1.pick).all() and (ex.ambiguous == v1.ambiguous).all()


# ---- the restatement inside its own contract ----------------------------------------------------------------------------------------
def share_case_args(case, family, step=0):
    valid, row = dr.share_rows(family, case.nv, case.V)
    n = dr.SHARE_DRAWS
    rows = np.repeat(row, n, axis=0)
    b = gr.share_bias(case)
    bias = None if b is None else np.repeat(b[None], n, axis=0)
    T = case.temperature if case.schedule is None else case.schedule[step]
    return (rows, valid, case.top_k, False, T, 1000 + np.arange(n) // 5, 10 + step, np.arange(n) % 5, STREAM, SEED), bias


@pytest.mark.parametrize("family", gr.SHARE_FAMILIES)
@pytest.mark.parametrize("case", gr.SHARE_CASES_GUIDED, ids=lambda c: "nv%d_k%d_p%s" % (c.nv, c.top_k, c.top_p))
def test_restatement_meets_the_float64_contract(case, family):
    for step in range(len(case.schedule) if case.schedule else 1):
        args, bias = share_case_args(case, family, step)
        got = gr.draw32_guided(*args, bias=bias, top_p=case.top_p)
        ex = gr.exact_draw_guided(*args, bias=bias, top_p=case.top_p)
        wrong, share = gr.contract_guided(ex, got)
        assert len(wrong) == 0
        assert share <= gr.SHARE_CAP
        assert not ex.nucleus_ambiguous.any()
        if case.top_p is not None:
            assert gr.nucleus_margin(ex, case.top_p) > 1.0      # no F_j within delta of top_p: the inputs were chosen so
        if case.n_forbidden:
            assert (ex.k_row == case.nv - case.n_forbidden).all()
        off = np.flatnonzero(~ex.ambiguous)
        assert (got[off] == ex.pick[off]).all()


def test_nucleus_rule_on_a_hand_case():
    """weights 1/2, 1/4, 1/8, 1/8, so F = 0.5, 0.75, 0.875, 1: the nucleus is the shortest prefix that reaches top_p"""
    valid = [0, 1, 2, 3]
    row = np.log(np.array([[0.5, 0.25, 0.125, 0.125]], np.float32))
    args = (np.repeat(row, 4000, axis=0), valid, 0, False, None, np.arange(4000), 0, np.zeros(4000, int), 0, 7)
    for top_p, keep in ((0.4, 1), (0.6, 2), (0.8, 3), (0.9, 4), (1.0, 4)):
        got = gr.draw32_guided(*args, top_p=top_p)
        assert set(got.tolist()) == set(range(keep)), (top_p, sorted(set(got.tolist())))
        ex = gr.exact_draw_guided(*args, top_p=top_p)
        assert (ex.k_nucleus == keep).all()
    burn = list(args)
    burn[3] = True      # sample on: top_p is ignored, as top_k is
    assert set(gr.draw32_guided(*burn, top_p=0.4).tolist()) == {0, 1, 2, 3}


# ---- forbidden entries are never drawn ------------------------------------------------------------------------------------------------
_INV_A, _INV_B = pow(dr._MUL_A, -1, 2 ** 32), pow(dr._MUL_B, -1, 2 ** 32)


def philox_counter_for(words, key):
    """The counter whose Philox4x32-10 output is `words`: the rounds run backwards (each is a bijection of the counter)."""
    ka, kb = key
    ks = []
    for _ in range(10):
        ks.append((ka, kb))
        ka, kb = (ka + dr._WEYL_A) & 0xFFFFFFFF, (kb + dr._WEYL_B) & 0xFFFFFFFF
    x = list(words)
    for ka, kb in reversed(ks):
        c2 = (x[1] * _INV_B) & 0xFFFFFFFF
        c0 = (x[3] * _INV_A) & 0xFFFFFFFF
        c1 = x[0] ^ ((dr._MUL_B * c2) >> 32) ^ ka
        c3 = x[2] ^ ((dr._MUL_A * c0) >> 32) ^ kb
        x = [c0, c1, c2, c3]
    return x


def test_philox_inverse():
    key = (SEED & 0xFFFFFFFF, SEED >> 32)
    for words in ([0, 1, 2, 3], [0xFFFFFFFF, 0x12345678, 0, 0x9ABCDEF0]):
        c = philox_counter_for(words, key)
        out = dr.philox4x32_10([np.array([c[0]]), np.array([c[1]]), np.array([c[2]]), np.array([c[3]])], key)
        assert [int(w[0]) for w in out] == words


@pytest.mark.parametrize("nv,n_forbidden,top_k,top_p,temp", [(20, 1, 0, None, None), (20, 18, 0, 0.9, 0.7), (20, 19, 5, 0.5, None),
                                                             (32, 12, 31, None, 7.5), (3, 2, 0, 0.1, 0.05), (2, 1, 1, None, None)])
def test_forbidden_entries_are_never_drawn(nv, n_forbidden, top_k, top_p, temp):
    """20 000 draws per case over every family, the forbidden entries holding the row's LARGEST logits, plus u = 0 and the largest u
    (Philox word 0 = 0 and 0xFFFFFFFF, by running the generator backwards to the counter)"""
    V = 33
    valid = dr.valid_list(nv, V, "shuffled", 2)
    rng = np.random.default_rng([nv, n_forbidden])
    per = 20000 // len(dr.FAMILIES) + 1
    key = (SEED & 0xFFFFFFFF, SEED >> 32)
    for family in dr.FAMILIES:
        values = dr.family_values(family, per, nv, 4)
        bias = np.zeros((per, nv), np.float32)
        dead = np.argsort(-values, axis=1, kind="stable")[:, :n_forbidden]      # the largest logits are the forbidden ones
        np.put_along_axis(bias, dead, -np.inf, axis=1)
        rows = dr.embed_rows(values, valid, V)
        for sample in (False, True):
            got = gr.draw32_guided(rows, valid, top_k, sample, temp, np.arange(per), 3, rng.integers(0, 5, per), STREAM, SEED, bias=bias,
                                   top_p=top_p)
            col = np.array([valid.index(int(t)) for t in got])
            assert np.isfinite(bias[np.arange(per), col]).all()
            ex = gr.exact_draw_guided(rows, valid, top_k, sample, temp, np.arange(per), 3, np.zeros(per, int), STREAM, SEED, bias=bias,
                                      top_p=top_p)
            assert (ex.k_row <= nv - n_forbidden).all()
            for word in (0, 0xFFFFFFFF):
                c = philox_counter_for([word, 11, 22, 33], key)
                assert dr.uniform_of([c[0]], c[1], [c[2]], c[3], SEED)[0] == (word >> 8) * dr.V24
                for r in range(0, per, per // 7):
                    tok = gr.draw32_guided(rows[r:r + 1], valid, top_k, sample, temp, [c[0]], c[1], [c[2]], c[3], SEED, bias=bias[r:r + 1],
                                           top_p=top_p)
                    assert np.isfinite(bias[r, valid.index(int(tok[0]))])


# ---- DrawGuide ----------------------------------------------------------------------------------------------------------------------
RES = list("LAGVSERTIDPKQNFYMHWC")      # some sampler order: not alphabetical


def test_drawguide_residue_order_and_position_convention():
    g = guides.DrawGuide(position_bias={2: {"A": 1.5, "c": -2.0}}, allowed_residues={1: "DE"}, forbidden_residues="C")
    c = g.compile(RES, 5, 10)
    assert c.bias.shape == (1, 5, 20) and c.bias.dtype == np.float32 and c.temperatures is None and c.top_p is None
    allowed_at_1 = [RES[j] for j in np.flatnonzero(c.bias[0, 1] > -np.inf)]
    assert sorted(allowed_at_1) == ["D", "E"]                     # token position 1 = residue 0 behind <cls>
    assert c.bias[0, 2, RES.index("A")] == np.float32(1.5)
    assert c.bias[0, 2, RES.index("C")] == -np.inf                # forbidden everywhere wins over a finite bias
    for pos in (0, 3, 4):
        assert (c.bias[0, pos, :-1] == 0).all() and c.bias[0, pos, RES.index("C")] == -np.inf
    per_pos = guides.DrawGuide(forbidden_residues={3: "LA"}).compile(RES, 5)
    assert np.flatnonzero(per_pos.bias[0, 3] == -np.inf).tolist() == [0, 1] and np.isfinite(per_pos.bias[0, [0, 1, 2, 4]]).all()
    arr = np.arange(100, dtype=np.float32).reshape(5, 20)
    assert (guides.DrawGuide(position_bias=arr).compile(RES, 5).bias[0] == arr).all()


def test_drawguide_top_p_and_schedule():
    c = guides.DrawGuide(top_p=0.9, temperature_schedule=[2.0, 1.0, 0.5]).compile(RES, 4, 3)
    assert c.bias is None and c.top_p == 0.9 and c.temperatures.dtype == np.float32 and c.temperatures.tolist() == [2.0, 1.0, 0.5]
    c = guides.DrawGuide(temperature_schedule="geometric:4:1").compile(RES, 4, 3)
    assert c.temperatures.tolist() == [4.0, 2.0, 1.0]
    assert guides.from_arguments() is None and guides.DrawGuide().compile(RES, 4).empty


def test_drawguide_refusals():
    with pytest.raises(IndexError, match="position 5 is out of range"):
        guides.DrawGuide(allowed_residues={5: "D"}).compile(RES, 5)
    with pytest.raises(IndexError, match="position -1 is out of range"):
        guides.DrawGuide(forbidden_residues={-1: "D"}).compile(RES, 5)
    with pytest.raises(Exception, match="Invalid input character: B"):
        guides.DrawGuide(forbidden_residues="B").compile(RES, 5)
    with pytest.raises(Exception, match="Invalid input character: X"):
        guides.DrawGuide(position_bias={1: {"X": 1.0}}).compile(RES, 5)
    with pytest.raises(ValueError, match="forbids every residue at position 2"):
        guides.DrawGuide(allowed_residues={2: "C"}, forbidden_residues="C").compile(RES, 5)
    with pytest.raises(ValueError, match="shape"):
        guides.DrawGuide(position_bias=np.zeros((4, 20))).compile(RES, 5)
    with pytest.raises(ValueError, match="finite"):
        guides.DrawGuide(position_bias={1: {"A": float("nan")}}).compile(RES, 5)
    for bad in (0.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match="top_p"):
            guides.DrawGuide(top_p=bad).compile(RES, 5)
    for bad in ([1.0, 0.0], [1.0, float("inf")], [-1.0], []):
        with pytest.raises(ValueError, match="finite and > 0"):
            guides.DrawGuide(temperature_schedule=bad).compile(RES, 5, 1)
    with pytest.raises(ValueError, match="3 entries.*7 iterations"):
        guides.DrawGuide(temperature_schedule=[1.0, 1.0, 1.0]).compile(RES, 5, 7)


def test_drawguide_uses_the_samplers_own_message():
    from protein_gibbs_sampler_amd.esm_sampler import ESM_sampler
    with pytest.raises(Exception, match="Invalid input character: "):
        guides.DrawGuide(forbidden_residues="AZ#").compile(RES, 5, clean=ESM_sampler.clean_seed_seq)


def test_annealing_schedule():
    for kind in guides.SCHEDULE_KINDS:
        s = guides.annealing_schedule(kind, 2.0, 0.25, 7)
        assert len(s) == 7 and s[0] == 2.0 and s[-1] == 0.25 and all(a > b for a, b in zip(s, s[1:]))
        assert guides.annealing_schedule(kind, 1.3, 0.2, 1) == [1.3]
        up = guides.annealing_schedule(kind, 0.5, 1.5, 4)
        assert up[0] == 0.5 and up[-1] == 1.5 and all(a < b for a, b in zip(up, up[1:]))
    assert guides.annealing_schedule("linear", 2.0, 1.0, 3) == [2.0, 1.5, 1.0]
    assert guides.annealing_schedule("geometric", 4.0, 1.0, 3) == [4.0, 2.0, 1.0]
    for bad in (("cosine", 1.0, 0.5, 3), ("linear", 0.0, 0.5, 3), ("linear", 1.0, float("inf"), 3), ("geometric", 1.0, 0.5, 0)):
        with pytest.raises(ValueError):
            guides.annealing_schedule(*bad)
    assert guides.parse_schedule("linear:2:1", 3) == [2.0, 1.5, 1.0]
    with pytest.raises(ValueError, match="kind:t_start:t_end"):
        guides.parse_schedule("linear:2", 3)


# ---- the C side that needs no device ----------------------------------------------------------------------------------------------------
def test_ctypes_struct_matches_the_header():
    assert ctypes.sizeof(_lib.DrawGuideStruct) == _lib.lib().pg_guided_sizeof_draw_guide()


VALID20 = list(range(4, 24))


def dbg_guided(guide, width=4, n_rows=3, first_iter=0, n_steps=2, nv=20):
    tok = np.full((n_rows, width), 5, np.int32)
    idx = np.ones((first_iter + n_steps, n_rows, 1), np.int32)
    logits = np.zeros((first_iter + n_steps, n_rows, 33), np.float32)
    out = np.zeros((n_steps, n_rows, 1), np.int32)
    params = _lib.make_sample_params(False, 0, 0, 0, None, VALID20[:nv], 1)
    g, keep = guide
    return _lib.lib().pg_guided_dbg_sample(99, _lib.ptr(tok), n_rows, width, _lib.ptr(logits), 33, 1, _lib.ptr(idx), idx.shape[0], None, n_rows,
                                           1, ctypes.byref(params), first_iter, n_steps, 0, -1, 0, _lib.ptr(out), None, None, ctypes.byref(g))


def refused(rc, text):
    assert rc == _lib.PG_ERR_INVALID
    assert text in _lib.lib().pg_last_error().decode(), _lib.lib().pg_last_error().decode()


def bad_tables():
    ok = np.zeros((1, 4, 20), np.float32)
    nan, pinf, dead = ok.copy(), ok.copy(), ok.copy()
    nan[0, 2, 7] = np.nan
    pinf[0, 1, 3] = np.inf
    dead[0, 3, :] = -np.inf
    return [(dict(bias=nan), "NaN at row 0, position 2, entry 7"), (dict(bias=pinf), "+inf at row 0, position 1, entry 3"),
            (dict(bias=dead), "forbids every residue at row 0, position 3"),
            (dict(temperatures=[1.0, 0.0]), "temperature 1 is not finite and > 0"),
            (dict(temperatures=[float("inf")]), "temperature 0 is not finite and > 0"),
            (dict(temperatures=[float("nan"), 1.0]), "temperature 0 is not finite and > 0"),
            (dict(top_p=0.0), "top_p must be in (0, 1]"), (dict(top_p=1.25), "top_p must be in (0, 1]"),
            (dict(bias=np.zeros((1, 4, 33), np.float32)), "n_valid must be in 1..32")]


def test_set_time_refusals_need_no_device():
    """each with its own message, from both entries; device 99 / a null engine would be the next refusal"""
    L = _lib.lib()
    for kw, text in bad_tables():
        g, keep = _lib.make_draw_guide(**kw)
        refused(L.pg_engine_set_draw_guide(None, ctypes.byref(g)), text)
        refused(dbg_guided((g, keep)), text)
    g, keep = _lib.make_draw_guide(top_p=0.5)
    refused(L.pg_engine_set_draw_guide(None, ctypes.byref(g)), "null engine")


def test_debug_entry_keeps_pg_dbg_samples_host_refusals():
    tok, idx, logits, out = np.full((3, 4), 5, np.int32), np.ones((2, 3, 1), np.int32), np.zeros((2, 3, 33), np.float32), np.zeros((2, 3, 1), np.int32)
    params = _lib.make_sample_params(False, 0, 0, 0, None, VALID20, 1)
    g, keep = _lib.make_draw_guide(top_p=0.5)
    args = [0, _lib.ptr(tok), 3, 4, _lib.ptr(logits), 33, 1, _lib.ptr(idx), 2, None, 3, 1, ctypes.byref(params), 0, 2, 0, -1, 0, _lib.ptr(out), None,
            None, ctypes.byref(g)]
    for index in (1, 4, 7, 12, 18):      # a null required pointer
        refused(_lib.lib().pg_guided_dbg_sample(*(args[:index] + [None] + args[index + 1:])), "pg_dbg_sample: bad argument")
    refused(_lib.lib().pg_guided_dbg_sample(*(args[:8] + [1] + args[9:])), "n_tables must be at least first_iter + n_steps")


def test_run_time_refusals_need_no_device():
    ok = lambda *shape: np.zeros(shape, np.float32)
    refused(dbg_guided(_lib.make_draw_guide(bias=ok(1, 5, 20))), "5 positions wide, the token rows 4")
    refused(dbg_guided(_lib.make_draw_guide(bias=ok(1, 4, 19))), "19 entries per position, the valid list 20")
    refused(dbg_guided(_lib.make_draw_guide(bias=ok(2, 4, 20))), "2 rows, which is neither 1 nor the call's 3 token rows")
    refused(dbg_guided(_lib.make_draw_guide(temperatures=[1.0, 1.0, 1.0]), first_iter=2, n_steps=2), "3 entries, the call 4 iterations")
    # a guide that fits reaches the device lookup: no device here, or ordinal 99 on a machine that has some
    for g in (_lib.make_draw_guide(bias=ok(3, 4, 20), temperatures=[1.0, 2.0], top_p=1.0), _lib.make_draw_guide()):
        assert dbg_guided(g) in (_lib.PG_ERR_NO_DEVICE, _lib.PG_ERR_INVALID)
        assert _lib.lib().pg_last_error().decode() in ("no HIP device visible", "bad device ordinal")


def test_command_line_flags_reach_the_sampler_arguments():
    from protein_gibbs_sampler_amd import _cli, pgen_esm_from_fasta, pgen_msa_revised
    for mod, base in ((pgen_esm_from_fasta, ["-i", "x.tsv"]), (pgen_msa_revised, ["--templates", "t", "--references", "r", "-o", "o"])):
        args = mod.build_parser().parse_args(base)
        assert _cli.guide_kwargs(args) == {}                      # nothing given: generate() is called as before
        args = mod.build_parser().parse_args(base + ["--top_p", "0.9", "--temperature_schedule", "geometric:2:0.5", "--forbid", "CM"])
        assert _cli.guide_kwargs(args) == dict(top_p=0.9, temperature_schedule="geometric:2:0.5", forbidden_residues="CM")
