"""Guided draws (pg_draw v2) through the samplers and the engine's Gibbs entries: every recorded draw replayed through the float32
restatement of tests/_guided_draw_reference.py, constraints visible in the outputs, the guide cleared after a call, one captured graph
for guided calls with different tables, the plug-in path, a sharded batch, and the run-time refusals.  The engines are the smallest
synthetic ones of tests/test_gpu_engine.py / test_gpu_msa.py: 2 layers, T <= 12 / R = 3, C = 9."""
import json
import os
import random
import subprocess
import sys
import warnings

import numpy as np
import pytest

import _guided_draw_reference as gr
from _standin import make_standin_torch_module, standin_logits_np
from oracle.esm_forward import EsmConfig, synthetic_esm_weights
from oracle.msa_forward import MsaConfig, synthetic_msa_weights
from protein_gibbs_sampler_amd import _lib, esm_msa_sampler, esm_sampler, guides, models, weights
from protein_gibbs_sampler_amd.alphabet import Alphabet

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ESM_CK = dict(d_model=128, n_layers=2, n_heads=2, d_ffn=256, max_pos=80)
MSA_CK = dict(d_model=128, n_layers=2, n_heads=2, d_ffn=256, max_pos=80, max_rows=16)
SEED_SEQ = "MEPAATGQEA"      # T = 12 with <cls> and <eos>
MSA = ["ACDEFGHI", "ACDEFGHI", "AC-EFGHV"]      # R = 3, C = 9

GUIDE_FORMS = {
    "bias": dict(position_bias={2: {"A": 2.5, "W": -1.0}, 7: {"K": 4.0}}, allowed_residues={3: "DE"}, forbidden_residues="C"),
    "schedule": dict(temperature_schedule=[2.0, 1.4, 0.9, 0.5]),
    "top_p": dict(top_p=0.6),
    "all": dict(position_bias={2: {"A": 2.5}}, forbidden_residues={4: "LAGV"}, top_p=0.8, temperature_schedule="geometric:2.0:0.5"),
}


def esm_sampler_on_gpu(seed=31):
    sd = synthetic_esm_weights(EsmConfig(**ESM_CK), seed=seed, std=0.08, embed_std=0.5, ln_jitter=0.1)
    cfg = weights.make_config(weights.ESM1B_CONFIG, d_model=128, n_layers=2, d_ffn=256, max_positions=80)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return esm_sampler.ESM_sampler(models.ESM1b(state_dict=sd, config=cfg, precision="bf16"), device="cuda:0")


def msa_sampler_on_gpu(seed=8):
    sd = synthetic_msa_weights(MsaConfig(**MSA_CK), seed=seed, std=0.08, embed_std=0.5, ln_jitter=0.1)
    cfg = weights.make_config(weights.MSA1B_CONFIG, d_model=128, n_layers=2, d_ffn=256, max_positions=80, max_msa_rows=16)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return esm_msa_sampler.ESM_MSA_sampler(models.ESM_MSA1(state_dict=sd, config=cfg, precision="bf16"), device="cuda:0")


def tables_of(sampler, form, width, n_iters):
    return guides.compile_for(sampler, guides.DrawGuide(**GUIDE_FORMS[form]), width, n_iters)


def replay_step(c, rows, positions, valid, top_k, sample, temperature, row_id, it, slot, seed):
    """one iteration's draws by the restatement: the guide's tables c (CompiledGuide) read at `positions`"""
    bias = None if c.bias is None else c.bias[0, positions]
    T = temperature if c.temperatures is None else float(c.temperatures[it])
    return gr.draw32_guided(rows, valid, top_k, sample, T, row_id, it, slot, 0, seed, bias=bias, top_p=c.top_p)


@pytest.fixture(scope="module")
def esm():
    return esm_sampler_on_gpu()


@pytest.fixture(scope="module")
def msa():
    return msa_sampler_on_gpu()


@pytest.mark.parametrize("form", sorted(GUIDE_FORMS))
def test_esm_generate_replays_draw_for_draw(esm, form):
    s = esm
    s.draw_seed, s.record = 99, True
    B, P, iters = 3, 3, 4
    random.seed(5)
    out = s.generate(2 * B, SEED_SEQ, batch_size=B, num_iters=iters, num_positions=P, top_k=4, burnin=1, temperature=1.1,
                     show_progress_bar=False, **GUIDE_FORMS[form])
    assert len(out) == 2 * B and len(s.last_run) == 2
    c = tables_of(s, form, 12, iters)
    for batch_n, run in enumerate(s.last_run):
        tok = s.get_init_seq(SEED_SEQ, len(SEED_SEQ), B).numpy().astype(np.int32)
        for it in range(iters):
            pos = run["table"][it].reshape(-1)
            rows = run["sampled_logits"][it].reshape(-1, 33)
            args = (rows, s.valid_aa_idx, 4, it < 1, 1.1, batch_n * B + np.repeat(np.arange(B), P), it, np.tile(np.arange(P), B), 0, 99)
            want = replay_step(c, rows, pos, *args[1:5], *args[5:8], 99).reshape(B, P)
            assert (want == run["sampled_tokens"][it]).all()
            for b in range(B):
                tok[b, run["table"][it, b]] = want[b]
        assert (tok == run["tokens"]).all()
    s.record = False


def test_constraints_show_in_the_outputs(esm, msa):
    only_w = {r: float("-inf") for r in "ACDEFGHIKLMNPQRSTVY"}      # a bias that allows exactly one residue at position 5
    kw = dict(forbidden_residues="C", allowed_residues={3: "DE"}, position_bias={5: only_w})
    msa_kw = dict(kw, position_bias={5: dict(only_w, **{"-": float("-inf")})})
    esm.draw_seed, esm.record = 4, False
    random.seed(1)
    out = esm.generate(8, SEED_SEQ, batch_size=4, num_iters=3, show_progress_bar=False, **kw)      # every position, every iteration
    assert len(out) == 8
    for seq in out:
        assert "C" not in seq and seq[2] in "DE" and seq[4] == "W"      # token position p is residue p - 1
    msa.draw_seed = 4
    random.seed(1)
    out = msa.generate(6, MSA, batch_size=2, num_iters=3, show_progress_bar=False, **msa_kw)
    assert len(out) == 6
    for seq in out:
        assert "C" not in seq and seq[2] in "DE" and seq[4] == "W"
    random.seed(1)
    row = msa.generate_single(MSA, steps=2, passes=2, burn_in=1, target_index=1, k=3, **msa_kw)
    assert "C" not in row and row[2] in "DE" and row[4] == "W"


def test_guide_is_cleared_after_the_call_and_after_an_exception(esm):
    kw = dict(batch_size=2, num_iters=3, num_positions=4, top_k=3, burnin=1, show_progress_bar=False)

    def plain(s):
        s.draw_seed, s.record = 11, False
        random.seed(2)
        return s.generate(4, SEED_SEQ, **kw)

    fresh = plain(esm_sampler_on_gpu())
    esm.draw_seed = 11
    random.seed(2)
    guided = esm.generate(4, SEED_SEQ, **kw, **GUIDE_FORMS["bias"])
    assert guided != fresh and plain(esm) == fresh
    lm = esm.model.model
    with pytest.raises(RuntimeError, match="inside"):
        with lm.draw_guide(tables_of(esm, "all", 12, 3)):
            raise RuntimeError("inside the call")
    assert lm._guide is None and plain(esm) == fresh
    # a native refusal inside a guided call (a schedule shorter than the loop, set past the Python check) leaves no guide behind either
    short = guides.CompiledGuide(None, np.array([1.0, 0.5], np.float32), None)
    tok = esm.get_init_seq(SEED_SEQ, len(SEED_SEQ), 2).numpy().astype(np.int32)
    table = np.tile(np.array([1, 2], np.int32), (3, 2, 1))
    params = _lib.make_sample_params(True, 32, 0, 0, None, esm.valid_aa_idx, 1)
    with pytest.raises(_lib.PgError, match="2 entries, the call 3 iterations"):
        with lm.draw_guide(short):
            lm.gibbs_run(tok, table, params)
    assert plain(esm) == fresh


_GRAPH_CHILD = r"""
import json, random, sys
sys.path[:0] = [%r, %r]
import test_gpu_guided_sampling as t
print(json.dumps(t.two_guided_calls(t.esm_sampler_on_gpu())[0]))
"""


def two_guided_calls(s):
    lm = s.model.model
    c0, r0 = lm.get_stat("graph_captures"), lm.get_stat("graph_replays")
    outs = []
    for i, sched in enumerate(("linear:2.0:0.5", [1.5] * 10 + [0.4] * 10)):
        s.draw_seed, s.record = 100 + i, False
        random.seed(i)
        outs.append(s.generate(1, SEED_SEQ, batch_size=1, num_iters=20, num_positions=2, top_k=3, burnin=5, show_progress_bar=False,
                               temperature_schedule=sched, forbidden_residues="C", top_p=0.9))
    return outs, lm.get_stat("graph_captures") - c0, lm.get_stat("graph_replays") - r0


def test_one_graph_serves_guided_calls_with_different_schedules():
    outs, caps, reps = two_guided_calls(esm_sampler_on_gpu())
    assert caps == 1, caps
    assert reps == 2 * 20 - 1, reps
    env = dict(os.environ, PGIBBS_GRAPH="0")
    p = subprocess.run([sys.executable, "-c", _GRAPH_CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, env=env,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    assert json.loads(p.stdout.strip().splitlines()[-1]) == outs
    assert "C" not in "".join(o[0] for o in outs)


def test_generate_single_indexes_the_schedule_by_step(msa):
    s = msa
    s.draw_seed, s.record = 3, True
    temps = [2.2, 1.8, 1.4, 1.0, 0.7, 0.4]
    kw = dict(temperature_schedule=temps, forbidden_residues="C-", position_bias={2: {"W": 3.0}}, top_p=0.9)
    random.seed(2)
    out = s.generate_single(MSA, steps=3, passes=2, burn_in=1, target_index=1, k=2, **kw)
    run = s.last_run[0]
    c = guides.compile_for(s, guides.DrawGuide(**kw), 9, 6)
    tok = s.get_init_msa(MSA, 8, 1).numpy().astype(np.int32)
    for i in range(6):
        st = [int(p) for p in run["table"][i, 0] if p >= 0]
        rows = run["sampled_logits"][i][:len(st)]
        want = replay_step(c, rows, st, s.valid_aa_idx, 2, i < 3, None, [1] * len(st), i, np.arange(len(st)), 3)
        assert (want == run["sampled_tokens"][i][:len(st)]).all()
        tok[0, 2, st] = 32
        tok[0, 1, st] = want
    assert (tok == run["tokens"]).all()
    assert out == s.untokenize_batch(tok)[1]
    with pytest.raises(ValueError, match="5 entries.*6 iterations"):
        s.generate_single(MSA, steps=3, passes=2, temperature_schedule=temps[:5])
    s.record = False


def test_msa_generate_replays_draw_for_draw(msa):
    s = msa
    s.draw_seed, s.record = 7, True
    B, R, P, iters = 2, 3, 3, 4
    random.seed(11)
    out = s.generate(R * B, MSA, batch_size=B, num_iters=iters, num_positions=P, top_k=3, burnin=1, temperature=0.8,
                     show_progress_bar=False, **GUIDE_FORMS["all"])
    assert len(out) == R * B
    c = tables_of(s, "all", 9, iters)
    run = s.last_run[0]
    tok = s.get_init_msa(MSA, 8, B).numpy().astype(np.int32)
    for it in range(iters):
        pos = run["table"][it].reshape(-1)
        rows = run["sampled_logits"][it].reshape(-1, 33)
        want = replay_step(c, rows, pos, s.valid_aa_idx, 3, it < 1, 0.8, np.repeat(np.arange(B * R), P), it, np.tile(np.arange(P), B * R),
                           7).reshape(B, R, P)
        assert (want == run["sampled_tokens"][it]).all()
        for b in range(B):
            for r in range(R):
                tok[b, r, run["table"][it, b, r]] = want[b, r]
    assert (tok == run["tokens"]).all()
    with pytest.raises(ValueError, match="3 entries.*4 iterations"):
        s.generate(R, MSA, num_iters=4, temperature_schedule=[1.0, 1.0, 1.0], show_progress_bar=False)
    s.record = False


class _Plugin:
    def __init__(self):
        self.alphabet = Alphabet(True, True)
        self.batch_converter = self.alphabet.get_batch_converter(msa=False)
        self.model = make_standin_torch_module()


@pytest.mark.parametrize("form", ["all", "bias"])
def test_plugin_model_path(form):
    s = esm_sampler.ESM_sampler(_Plugin(), device="cuda:0")
    s.draw_seed, s.record = 21, True
    B, P, iters = 3, 4, 4
    random.seed(3)
    s.generate(B, SEED_SEQ, batch_size=B, num_iters=iters, num_positions=P, top_k=5, burnin=2, temperature=0.9, show_progress_bar=False,
               **GUIDE_FORMS[form])
    run = s.last_run[0]
    c = tables_of(s, form, 12, iters)
    tok = s.get_init_seq(SEED_SEQ, len(SEED_SEQ), B).numpy().astype(np.int32)
    for it in range(iters):
        table = run["table"][it]
        for b in range(B):
            tok[b, table[b]] = s.model.alphabet.mask_idx
        logits = standin_logits_np(tok)
        rows = np.stack([logits[b, table[b]] for b in range(B)]).reshape(-1, 33)
        want = replay_step(c, rows, table.reshape(-1), s.valid_aa_idx, 5, it < 2, 0.9, np.repeat(np.arange(B), P), it, np.tile(np.arange(P), B),
                           21).reshape(B, P)
        for b in range(B):
            tok[b, table[b]] = want[b]
    assert (tok == run["tokens"]).all()


def test_two_way_shard_equals_the_whole_batch(esm):
    """176 chains of 12 tokens = 2112 token rows, just past the 2048 above which a shard that knows the job's size computes the whole
    job's bits (pg_engine_set_job_items): whole, and as two halves with their row_id_base, under one shared guide"""
    lm = esm.model.model
    c = tables_of(esm, "all", 12, 4)
    B = 176
    rng = np.random.default_rng(2)
    table = np.stack([np.stack([1 + rng.permutation(10)[:3] for _ in range(B)]) for _ in range(4)]).astype(np.int32)
    start = esm.get_init_seq(SEED_SEQ, 10, B).numpy().astype(np.int32)
    start[:, 1:11] = rng.integers(4, 24, (B, 10))

    def params(base):
        return _lib.make_sample_params(True, 32, 4, 1, 1.1, esm.valid_aa_idx, 77, row_id_base=base)

    whole = start.copy()
    with lm.draw_guide(c):
        lg_whole, _ = lm.gibbs_run(whole, table, params(0), want_logits=True)
        halves = [start[:B // 2].copy(), start[B // 2:].copy()]
        lgs = []
        lm.set_job_items(B)
        try:
            for h, base in zip(halves, (0, B // 2)):
                lgs.append(lm.gibbs_run(h, np.ascontiguousarray(table[:, base:base + B // 2]), params(base), want_logits=True)[0])
        finally:
            lm.set_job_items(0)
    assert (np.concatenate(lgs, axis=1) == lg_whole).all()
    assert (np.concatenate(halves) == whole).all() and (whole != start).any()
    plain = start.copy()
    lm.gibbs_run(plain, table, params(0))
    assert (plain != whole).any()


def test_run_time_refusals(esm, msa):
    lm = esm.model.model
    tok = esm.get_init_seq(SEED_SEQ, len(SEED_SEQ), 2).numpy().astype(np.int32)
    table = np.tile(np.array([1, 2], np.int32), (3, 2, 1))
    params = _lib.make_sample_params(True, 32, 0, 0, None, esm.valid_aa_idx, 1)
    zeros = lambda *shape: np.zeros(shape, np.float32)
    for c, text in ((guides.CompiledGuide(zeros(1, 11, 20), None, None), "11 positions wide, the token rows 12"),
                    (guides.CompiledGuide(None, zeros(2) + 1, None), "2 entries, the call 3 iterations"),
                    (guides.CompiledGuide(zeros(3, 12, 20), None, None), "3 rows, which is neither 1 nor the call's 2 token rows"),
                    (guides.CompiledGuide(zeros(1, 12, 19), None, None), "19 entries per position, the valid list 20")):
        before = tok.copy()
        with pytest.raises(_lib.PgError, match=text) as e:
            with lm.draw_guide(c):
                lm.gibbs_run(tok, table, params)
        assert e.value.code == _lib.PG_ERR_INVALID and (tok == before).all()
    # a per-row table of the call's own row count is taken
    with lm.draw_guide(guides.CompiledGuide(zeros(2, 12, 20), None, None)):
        lm.gibbs_run(tok, table, params)
    mlm = msa.model.model
    mtok = msa.get_init_msa(MSA, 8, 1).numpy().astype(np.int32)
    mparams = [_lib.make_sample_params(True, 32, 0, 0, None, msa.valid_aa_idx, 1)]
    steps = np.array([[[1, 2]], [[3, 4]]], np.int32)
    for c, text in ((guides.CompiledGuide(zeros(1, 8, len(msa.valid_aa_idx)), None, None), "8 positions wide, the token rows 9"),
                    (guides.CompiledGuide(None, zeros(1) + 1, None), "1 entries, the call 2 iterations"),
                    (guides.CompiledGuide(zeros(2, 9, len(msa.valid_aa_idx)), None, None), "2 rows, which is neither 1 nor the call's 3 token rows")):
        with pytest.raises(_lib.PgError, match=text):
            with mlm.draw_guide(c):
                mlm.gibbs_single_batch_run(mtok, 2, 1, steps, [0, 0], mparams)
        with pytest.raises(_lib.PgError, match=text):
            with mlm.draw_guide(c):
                mlm.gibbs_run(mtok, np.tile(np.array([1, 2], np.int32), (2, 1, 3, 1)), mparams[0])
