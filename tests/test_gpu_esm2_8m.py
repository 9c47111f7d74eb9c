"""ESM-2 8M (esm2_t6_8M_UR50D: 20 heads of 16, d_model 320; models.ESM2_8M) on the HIP engine: the head-16 attention kernels alone
(pg_dbg_attention_hd: the whole-sequence ladder, the long-sequence kernel, <pad> keys, three precisions) and the head-16 rotation
(pg_dbg_rope_hd) against numpy, the row kernels at d = 320, the engine forward against the numpy reference and a HuggingFace fixture
(the 6 x 320 model IS the full-size model), which GEMM kernels a forward takes, the sampler (positions, draws, likelihoods,
substitution tables, hipGraph replay, shards), and the refusals of heads of 16 elsewhere."""
import json
import os
import random
import warnings

import numpy as np
import pytest

import _esm2_gpu_common as common
import _esm2_reference_hd as ref
import _row_reference as rr
import test_gpu_row_kernels as rk
from _esm2_gpu_common import PREC, SEED25, replay_draws as _replay_draws, round_bf16 as _round_bf16, round_f16 as _round_f16, tokens as _tokens
from _ln_host import PLAIN, _ln_inplace_host
from protein_gibbs_sampler_amd import _lib, esm_sampler, models, weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HD = 16
F32 = np.float32


def _case(n_layers=6, d=320, seed=7, **over):
    cfg = weights.make_config(weights.ESM2_T6_CONFIG, n_layers=n_layers, d_model=d, d_ffn=4 * d, **over)
    assert cfg["n_heads"] * HD == d
    sd = weights.synthetic_state_dict(cfg, seed=seed, std=0.03, embed_std=0.15, ln_jitter=0.1)
    return cfg, sd, ref.Esm2Config.of(cfg)


def _model(cfg, sd, precision):
    return common.model(models.ESM2_8M, cfg, sd, precision)


# ---- the attention kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("H", [2, 20])
@pytest.mark.parametrize("T", [16, 27, 258, 300, 576, 577, 1026])
def test_attention_hd16_against_numpy(T, H, precision):
    """16, 258 / 300, 576: the first, a mid and the last rung of the whole-sequence ladder; 577 and 1026: the long-sequence kernel (two
    and four 288-key tiles).  Each shape without and with <pad> keys (the PADMASK forms); row 1's tail is padding.  q is drawn at 0.5
    so that the score's spread is the head-32 test's (0.35 sqrt(32) = 0.5 sqrt(16)); the bounds are that test's, unchanged."""
    B = 2
    rng = np.random.default_rng(T * 7 + H)
    qkv = rng.standard_normal((B, T, 3, H, HD)).astype(np.float32)
    qkv[:, :, 0] *= np.float32(0.5)
    rnd = {"fp32": lambda a: a, "bf16": _round_bf16, "fp16": _round_f16}[precision]
    x = np.ascontiguousarray(rnd(qkv).reshape(B, T, 3 * H * HD))
    tok = np.full((B, T), 5, dtype=np.int32)
    tok[1, max(1, T - 1 - T // 3):] = 1
    L = _lib.lib()
    for key_tok in (None, tok):
        got = np.zeros((B, T, H * HD), np.float32)
        _lib.check(L.pg_dbg_attention_hd(0, PREC[precision], _lib.ptr(x), _lib.ptr(got), B, T, H, HD,
                                         _lib.ptr(key_tok) if key_tok is not None else None, 1))
        want = ref.softmax_attention(x, B, T, H, HD, None if key_tok is None else key_tok == 1)
        err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        print("\n[attention hd16 T=%d H=%d %s pad=%d] relative error %.3e" % (T, H, precision, key_tok is not None, err))
        tol = {"fp32": 6e-5, "bf16": 2.5e-2, "fp16": 4e-3}[precision]
        assert np.isfinite(got).all() and err < tol, (T, H, precision, key_tok is not None, err)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_attention_hd16_every_head_lands_in_its_own_columns(precision):
    """Two heads of 16 share one 32-column group of the strict mode's context row and one 64-byte line of the 16-bit one: with v of head
    h set to the constant h + 1 the context of head h is h + 1 in all of its 16 columns, whatever q and k are."""
    B, T, H = 1, 70, 5 if precision == "bf16" else 6
    rng = np.random.default_rng(11)
    qkv = rng.standard_normal((B, T, 3, H, HD)).astype(np.float32)
    qkv[:, :, 2] = np.arange(1, H + 1, dtype=np.float32)[None, None, :, None]
    x = np.ascontiguousarray(qkv.reshape(B, T, 3 * H * HD))
    got = np.zeros((B, T, H * HD), np.float32)
    _lib.check(_lib.lib().pg_dbg_attention_hd(0, PREC[precision], _lib.ptr(x), _lib.ptr(got), B, T, H, HD, None, 1))
    want = np.broadcast_to(np.repeat(np.arange(1, H + 1, dtype=np.float32), HD), got.shape)
    assert np.abs(got - want).max() < (1e-4 if precision == "fp32" else 0.05)


def test_attention_hd_at_64_is_pg_dbg_attention():
    B, T, H = 2, 70, 3
    x = np.random.default_rng(3).standard_normal((B, T, 3 * H * 64)).astype(np.float32) * np.float32(0.5)
    L = _lib.lib()
    for prec in PREC.values():
        a, b = np.zeros((B, T, H * 64), np.float32), np.zeros((B, T, H * 64), np.float32)
        _lib.check(L.pg_dbg_attention(0, prec, _lib.ptr(x), _lib.ptr(a), B, T, H))
        _lib.check(L.pg_dbg_attention_hd(0, prec, _lib.ptr(x), _lib.ptr(b), B, T, H, 64, None, -1))
        assert np.array_equal(a, b)
    assert L.pg_dbg_attention_hd(0, _lib.PG_PREC_BF16, _lib.ptr(x), _lib.ptr(a), B, T, H, 48, None, -1) != 0


# ---- the rotation kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [4, 20, 32])
@pytest.mark.parametrize("T", [1, 27, 258, 1026])
def test_rope_hd16_against_numpy(T, H):
    B = 2 if T < 600 else 1
    rng = np.random.default_rng(T * 31 + H)
    x = (rng.standard_normal((B * T, 3 * H * HD)) * 2.0).astype(np.float32)
    L = _lib.lib()
    d2 = 2 * H * HD
    got = x.copy()
    _lib.check(L.pg_dbg_rope_hd(0, _lib.PG_PREC_FP32, _lib.ptr(got), B, T, H, HD))
    want = ref.rotate_qkv_rows(x, B, T, H, HD)
    assert np.array_equal(got, want)                                            # strict mode: the host fp32 loop, bit for bit (v included)
    assert np.array_equal(got[:, d2:], x[:, d2:]) and np.array_equal(got[0, :d2], x[0, :d2])
    if T > 1:
        assert not np.array_equal(got[1, :d2], x[1, :d2])
    for prec, rnd, mant in ((_lib.PG_PREC_BF16, _round_bf16, 7), (_lib.PG_PREC_F16, _round_f16, 10)):
        got = x.copy()
        _lib.check(L.pg_dbg_rope_hd(0, prec, _lib.ptr(got), B, T, H, HD))
        x16 = rnd(x)
        want = rnd(ref.rotate_qkv_rows(x16, B, T, H, HD))
        assert np.array_equal(got[:, d2:], x16[:, d2:])
        ulp16 = np.spacing(np.maximum(np.abs(want[:, :d2]), np.float32(2.0 ** -14))) * np.float32(2.0 ** (23 - mant))
        assert (np.abs(got[:, :d2] - want[:, :d2]) <= ulp16).all()


def test_rope_hd16_refuses_more_than_32_heads():
    x = np.zeros((2, 3 * 33 * HD), np.float32)
    assert _lib.lib().pg_dbg_rope_hd(0, _lib.PG_PREC_BF16, _lib.ptr(x), 1, 2, 33, HD) != 0


# ---- the row kernels at d = 320 (two chunks of the 8-chunk form, the second a quarter full) ------------------------------------------
D = 320


@pytest.mark.parametrize("M", [1, 37, 4099])
def test_layernorm_rows_at_320(M):
    x = rk._rows(M, D, M * 7 + D)
    g, b = rk._affine(D, D)
    L = _lib.lib()
    y = np.full_like(x, np.nan)
    _lib.check(L.pg_dbg_layernorm(0, _lib.ptr(x), _lib.ptr(g), _lib.ptr(b), _lib.ptr(y), M, D, rk.EPS))
    x64 = x.astype(np.float64)
    want = (x64 - x64.mean(-1, keepdims=True)) / np.sqrt(x64.var(-1, keepdims=True) + rk.EPS) * g + b
    assert np.abs(y - want).max() < 2e-5 * max(1.0, np.abs(want).max())          # the bound test_gpu_kernels.py::test_layernorm uses
    y0 = _ln_inplace_host(x, g, b, rk.EPS)
    for name, prec, form in rk.FORMS:                                             # the operand stores: bf16, fp16, split with / without dup
        h, kernel = rk.ln_rows(x, g, b, form, prec)
        assert kernel == "plain", (name, kernel)
        rk._check_against_host_loop(h, x, g, b, form, prec, y0)
    for prec, rnd in ((_lib.PG_PREC_BF16, _round_bf16), (_lib.PG_PREC_F16, _round_f16), (_lib.PG_PREC_FP32, None)):
        h = np.full_like(x, np.nan)
        _lib.check(L.pg_dbg_layernorm_operand(0, prec, _lib.ptr(x), _lib.ptr(g), _lib.ptr(b), _lib.ptr(h), M, D, rk.EPS))
        hi = _round_bf16(y)
        assert np.array_equal(h, rnd(y) if rnd else hi + _round_bf16(y - hi))


def test_embedding_at_320():
    has_pos, ln_before, dropout, scaled, rows_per_msa = rk.EMBED_MODELS["esm2"]
    rng = np.random.default_rng(D)
    e = (rng.standard_normal((rk.V, D), dtype=F32) * F32(0.3)).astype(F32)
    e[:, 0] += np.arange(rk.V, dtype=F32)
    gb2 = rk._affine(D, D + 6)
    for i, (n_seq, T) in enumerate([(1, 1), (3, 27), (5, 258)]):
        for j, pattern in enumerate(rr.PATTERNS):
            tok = rr.make_tokens(pattern, n_seq, T, seed=T * 10 + j)
            prec = (rk.BF16, rk.F16)[(i + j) % 2]
            x, h2 = rk.embed(tok, e, None, None, 0, None, gb2, dropout, 1.0, prec)
            want, mag = rr.embed_reference(tok, e, None, None, 0, None, None, token_dropout=dropout, eps=rk.EPS, embed_scale=F32(1.0))
            want, mag = want.reshape(-1, D), mag.reshape(-1, D)
            pad = (tok == rr.PAD).ravel()
            case = (n_seq, T, pattern)
            assert (x[pad] == 0).all() and not np.signbit(x[pad]).any(), case
            assert (np.abs(x - want) - 8 * rk.U * mag <= 0).all(), case
            h, kernel = rk.ln_rows(x, gb2[0], gb2[1], PLAIN, prec, extra=0)
            assert kernel == "plain" and np.array_equal(h2, h), case


@pytest.mark.parametrize("n", [2, 800, 1025])
def test_lm_tail_at_320(n):
    """the bound of test_gpu_row_kernels.py::test_lm_tail_small_and_large_kernels (at most 10 chunk terms per lane: here 2)"""
    for vocab in (33, 5):
        g, e, bias, gb = rk._tail_input(n, D, vocab)
        for with_ln in (0, 1):
            logits, small = rk.lm_tail(g, e, bias, gb if with_ln else None)
            assert small == (1 if n <= 1024 else 0) and logits.shape == (n, vocab) and np.isfinite(logits).all()
            want, mag, vmax, esum = rr.lm_tail_reference(g, e, bias, gb[0] if with_ln else None, gb[1] if with_ln else None, rk.EPS)
            bound = 24 * rk.U * mag + (2e-5 * max(1.0, vmax) * esum[None, :] if with_ln else 0.0)
            assert (np.abs(logits - want) <= bound).all(), (n, vocab, with_ln, float((np.abs(logits - want) / bound).max()))


# ---- forward ------------------------------------------------------------------------------------------------------------------------
# max |engine - reference| per unit of logit std: the 650M / 150M tests' bounds
FWD_TOL = {"fp32": None, "bf16": 0.05, "fp16": 0.008}
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_esm2_8m_forward_against_the_reference(precision):
    """esm2_t6_8M_UR50D's own shape: 6 layers x 320, 20 heads of 16."""
    cfg, sd, rcfg = _case()
    assert (cfg["n_layers"], cfg["d_model"], cfg["n_heads"], cfg["d_ffn"]) == (6, 320, 20, 1280)
    lm = _model(cfg, sd, precision).model.to("cuda:0")
    rng = np.random.default_rng(5)
    worst, std = 0.0, 1.0
    for T in (16, 27, 64, 160, 258, 288, 600):
        B = 3 if T < 300 else 1
        tok = _tokens(rng, B, T)
        want = ref.esm2_forward(sd, rcfg, tok)
        got = lm.forward_logits(tok)
        assert got.shape == want.shape == (B, T, 33)
        std = float(want.std())
        err = np.abs(got - want).max()
        worst = max(worst, err / (1.0 if precision == "fp32" else std))
        assert err < (1e-3 if precision == "fp32" else FWD_TOL[precision] * std), (T, err, std)
    # a right-padded batch: <pad> keys masked, positions are token indices
    tok = np.full((3, 40), 1, dtype=np.int64)
    lens = (40, 23, 9)
    for b, n in enumerate(lens):
        tok[b, :n] = _tokens(rng, 1, n, mask_every=5)[0]
    got = lm.forward_logits(tok)
    want = ref.esm2_forward(sd, rcfg, tok)
    for b, n in enumerate(lens):
        err = np.abs(got[b, :n] - want[b, :n]).max()
        assert err < (1e-3 if precision == "fp32" else FWD_TOL[precision] * float(want.std())), (b, err)
        alone = lm.forward_logits(tok[b:b + 1, :n])
        assert np.abs(alone[0] - got[b, :n]).max() < (2e-4 if precision == "fp32" else 0.08)
    print("\n[ESM-2 6 x 320, 20 heads of 16, %s] max|engine - reference| = %.3e %s (logit std %.2f)"
          % (precision, worst, "absolute" if precision == "fp32" else "per unit of logit std", std))


def test_esm2_8m_forward_against_huggingface_logits():
    z = np.load(os.path.join(HERE, "golden", "esm2_hf_hd16.npz"))
    cfg = weights.make_config(weights.ESM2_T6_CONFIG, **json.loads(str(z["cfg"])))
    sd = weights.synthetic_state_dict(cfg, seed=int(z["seed"]), std=float(z["std"]), embed_std=float(z["embed_std"]),
                                      ln_jitter=float(z["ln_jitter"]))
    for precision, tol in (("fp32", 1e-3), ("fp16", 0.04)):
        got = _model(cfg, sd, precision).model.to("cuda:0").forward_logits(z["tokens"])
        assert np.abs(got - z["logits"]).max() < tol, precision


def test_esm2_8m_auto_precision_and_synthetic_default():
    cfg, sd, rcfg = _case(n_layers=2, d=128)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = models.ESM2_8M(state_dict=sd, config=cfg)                            # precision="auto"
    lm = m.model.to("cuda:0")
    tok = _tokens(np.random.default_rng(1), 2, 30)
    want = ref.esm2_forward(sd, rcfg, tok)
    assert np.abs(lm.forward_logits(tok) - want).max() < 0.05 * max(1.0, float(want.std()))


# ---- dispatch -----------------------------------------------------------------------------------------------------------------------
def _kernels_of(lm, run):
    lm.prof_enable(True)
    lm.prof_reset()
    run()
    lm.synchronize()
    out = {c: lm.prof_get_kernels(c) for c in ("gemm_qkv", "gemm_out", "gemm_fc1", "gemm_fc2", "attention")}
    lm.prof_enable(False)
    return out


def test_esm2_8m_dispatch_at_config_2_and_for_a_single_chain():
    """N = 320 / 960 run on 64 x 64 tiles, fc1 (N = 1280, K = 320) on the 256 x 256 kernel; a single chain takes the per-layer launches
    with the weight-streaming GEMMs and separate LayerNorms (the LayerNorm-folding GEMM needs K a multiple of 256)."""
    cfg, sd, _ = _case(n_layers=2)
    lm = _model(cfg, sd, "bf16").model.to("cuda:0")
    tok = _tokens(np.random.default_rng(9), 256, 258)
    k = _kernels_of(lm, lambda: lm.forward_logits(tok))
    assert k["gemm_qkv"].startswith("tile64x64") and k["gemm_out"].startswith("tile64x64") and k["gemm_fc2"].startswith("tile64x64"), k
    assert k["gemm_fc1"].startswith("w16-256x256"), k
    assert k["attention"] == "whole kb18 hd16 5120wg", k
    one = _tokens(np.random.default_rng(10), 1, 27)
    k = _kernels_of(lm, lambda: lm.forward_logits(one))
    assert all(k[c].startswith("skinny") for c in ("gemm_qkv", "gemm_out", "gemm_fc1", "gemm_fc2")), k
    assert "ln" not in k["gemm_qkv"] and "ln" not in k["gemm_fc1"], k
    assert k["attention"] == "whole kb2 hd16 20wg", k


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base, name, cls", [("ESM1B_CONFIG", "ESM-1b", "ESM1b"), ("MSA1B_CONFIG", "ESM-MSA-1b", "ESM_MSA1"),
                                             ("ESM1_T6_CONFIG", "ESM-1", "ESM6")])
def test_engine_refuses_heads_of_16_for_the_other_architectures(base, name, cls):
    cfg = weights.make_config(getattr(weights, base), n_layers=1, d_model=128, n_heads=8, d_ffn=512, max_positions=40)
    sd = weights.synthetic_state_dict(cfg, seed=1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = getattr(models, cls)(state_dict=sd, config=cfg, precision="bf16")
    with pytest.raises(Exception, match=r"%s with heads of 16.*64" % name):
        m.model.to("cuda:0")


def test_engine_refuses_33_heads_of_16_and_heads_of_24():
    cfg = weights.make_config(weights.ESM2_T6_CONFIG, n_layers=1, d_model=576, n_heads=36, d_ffn=512, max_positions=40)
    sd = weights.synthetic_state_dict(cfg, seed=1)
    with pytest.raises(Exception, match="heads of 16.*at most 32"):
        _model(cfg, sd, "bf16").model.to("cuda:0")
    cfg = weights.make_config(weights.ESM2_T6_CONFIG, n_layers=1, d_model=384, n_heads=16, d_ffn=512, max_positions=40)      # heads of 24
    sd = weights.synthetic_state_dict(cfg, seed=1)
    with pytest.raises(Exception, match=r"head dim must be 64 .* or 32"):
        _model(cfg, sd, "bf16").model.to("cuda:0")


# ---- the sampler --------------------------------------------------------------------------------------------------------------------
def test_esm2_8m_sampler_positions_draws_and_likelihoods():
    cfg, sd, rcfg = _case(n_layers=4)
    s = esm_sampler.ESM_sampler(_model(cfg, sd, "fp32"), device="cuda:0")
    s.draw_seed, s.record = 11, True
    random.seed(2)
    out = s.generate(4, SEED25, batch_size=4, num_iters=3, num_positions=5, top_k=3, burnin=2, temperature=0.9, show_progress_bar=False)
    assert len(out) == 4 and all(len(x) == 25 for x in out)
    run = s.last_run[0]
    random.seed(2)
    table = np.asarray([[random.sample(range(1, 26), 5) for _ in range(4)] for _ in range(3)])
    assert (run["table"] == table).all(), "position selection is not bit-exact with random.sample"
    _replay_draws(s, run, 4, 5, 3, 3, 2, 0.9, 11)
    tok = s.get_init_seq(SEED25, 25, 4).numpy()
    for b in range(4):
        tok[b, table[0, b]] = 32
    want = ref.esm2_forward(sd, rcfg, tok)
    for b in range(4):
        assert np.abs(run["sampled_logits"][0][b] - want[b, table[0, b]]).max() < 1e-3
    seq = "MRHGDISSSNDTVGVAVVNYKMPRLHTAAEVLDNAR"
    ll, per = s.log_likelihood(seq)
    tok = s.get_init_seq(seq, len(seq), 1).numpy()
    masked = []
    for i in range(1, len(seq) + 1):
        t = tok.copy()
        t[0, i] = 32
        masked.append(ref.log_softmax(ref.esm2_forward(sd, rcfg, t)[0, i])[tok[0, i]])
    assert np.abs(np.asarray(per) - np.asarray(masked)).max() < 2e-3 and abs(ll - np.mean(masked)) < 1e-3
    # the substitution table read at the sequence's own residues is the likelihood's list, bit for bit
    seqs = [seq, seq[:20], SEED25]
    lls = list(s.log_likelihood_batch(seqs))
    for sq, (ll_b, per_b), (logp, entropy, toks) in zip(seqs, lls, s.masked_marginals_batch(seqs)):
        own = np.asarray([logp[i, toks.index(c)] for i, c in enumerate(sq)], dtype=np.float32)
        assert np.array_equal(own, np.asarray(per_b, dtype=np.float32)) and np.isfinite(entropy).all()
    assert np.array_equal(np.asarray(lls[0][1], dtype=np.float32), np.asarray(per, dtype=np.float32))


def _single_chain_run():
    cfg, sd, _ = _case(n_layers=3, seed=13)
    return common.single_chain_run(_model(cfg, sd, "bf16"))


def _single_chain_child():
    common.single_chain_child(_single_chain_run)


def _child(call, **env):
    return common.child("test_gpu_esm2_8m", call, **env)


def test_esm2_8m_single_chain_replays_a_graph_and_equals_the_eager_loop():
    common.check_single_chain(_single_chain_run, "test_gpu_esm2_8m")


def _shard_job(worlds):
    """A 64-chain job of config 2's chain length, whole and as contiguous shards that know the job's size: a digest of (tokens,
    logits) of the whole job, after checking every world against it bit for bit."""
    cfg, sd, _ = _case(n_layers=3)
    return common.shard_job(_model(cfg, sd, "bf16"), worlds)


def _shard_child():
    print("CHILD_DIGEST " + _shard_job((2,)))


def test_esm2_8m_shards_reproduce_the_whole_job():
    """64 chains x 20 heads at 18 key blocks (four workgroups per CU: 1024 slots): the whole job is 1280 pairs, a full round and a
    quarter that the attention launch splits; the 32- and 8-chain shards are partial rounds -- and with PGIBBS_ATTN_SPLIT=0 (read once
    per process: a child) the same bits come out."""
    digest = _shard_job((2, 8))
    line = [l for l in _child("_shard_child", PGIBBS_ATTN_SPLIT="0") if l.startswith("CHILD_DIGEST ")][-1]
    assert line.split()[1] == digest


def test_strict_valu_switch_refuses_heads_of_16_by_name():
    """PGIBBS_ATTN_F32=valu selects the all-VALU cross-check kernel, built for heads of 64 only: it must refuse, not run wrong."""
    out = _child("_refuse_valu_child", PGIBBS_ATTN_F32="valu")
    assert any(l.startswith("CHILD_REFUSED ") and "PGIBBS_ATTN_F32" in l and "heads of 16" in l for l in out), out


def _refuse_valu_child():
    common.refuse_valu_child(HD)
