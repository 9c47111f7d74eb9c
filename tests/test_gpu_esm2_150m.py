"""ESM-2 150M (esm2_t30_150M_UR50D: heads of 32; models.ESM2_150M) on the HIP engine: the head-32 attention kernels alone
(pg_dbg_attention_hd: the whole-sequence ladder, the long-sequence kernel, <pad> keys, three precisions) and the head-32 rotation
(pg_dbg_rope_hd) against numpy, the engine forward against the numpy reference and a HuggingFace fixture, the full-size model in
strict mode, the sampler (positions, draws, likelihoods, hipGraph replay, shards), and the refusals of heads of 32 elsewhere."""
import json
import os
import random
import warnings

import numpy as np
import pytest

import _esm2_gpu_common as common
import _esm2_reference_hd as ref
from _esm2_gpu_common import PREC, SEED25, replay_draws as _replay_draws, round_bf16 as _round_bf16, round_f16 as _round_f16, tokens as _tokens
from protein_gibbs_sampler_amd import _lib, esm_sampler, models, weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _case(n_layers=6, d=640, seed=7, **over):
    cfg = weights.make_config(weights.ESM2_T30_CONFIG, n_layers=n_layers, d_model=d, d_ffn=4 * d, **over)
    assert cfg["n_heads"] * 32 == d
    sd = weights.synthetic_state_dict(cfg, seed=seed, std=0.03, embed_std=0.15, ln_jitter=0.1)
    return cfg, sd, ref.Esm2Config.of(cfg)


def _model(cfg, sd, precision):
    return common.model(models.ESM2_150M, cfg, sd, precision)


# ---- the attention kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("H", [2, 20])
@pytest.mark.parametrize("T", [16, 27, 258, 300, 576, 577, 1026])
def test_attention_hd32_against_numpy(T, H, precision):
    """16 ... 576: rungs of the whole-sequence ladder (576 = the last one), 577 and 1026: the long-sequence kernel (two and four
    288-key tiles).  Each shape without and with <pad> keys (the PADMASK forms); row 1's tail is padding."""
    B = 2
    rng = np.random.default_rng(T * 7 + H)
    qkv = rng.standard_normal((B, T, 3, H, 32)).astype(np.float32)
    qkv[:, :, 0] *= np.float32(0.35)                                            # q as the engine hands it over: scaled, |score| of a few units
    rnd = {"fp32": lambda a: a, "bf16": _round_bf16, "fp16": _round_f16}[precision]
    x = np.ascontiguousarray(rnd(qkv).reshape(B, T, 3 * H * 32))
    tok = np.full((B, T), 5, dtype=np.int32)
    tok[1, max(1, T - 1 - T // 3):] = 1
    L = _lib.lib()
    for key_tok in (None, tok):
        got = np.zeros((B, T, H * 32), np.float32)
        _lib.check(L.pg_dbg_attention_hd(0, PREC[precision], _lib.ptr(x), _lib.ptr(got), B, T, H, 32,
                                         _lib.ptr(key_tok) if key_tok is not None else None, 1))
        want = ref.softmax_attention(x, B, T, H, 32, None if key_tok is None else key_tok == 1)
        err = np.abs(got - want).max() / max(1.0, np.abs(want).max())
        # strict: split-bf16 products and a context returned as a (hi, lo) bf16 pair, 16-17 mantissa bits: the bound of the head-64
        # strict kernel's test (first measured value here: 1.3e-5 at T = 16); 16-bit modes: P and the context are rounded to the
        # operand type (bf16: the bound the head-64 kernel is held to on inputs drawn the same way; fp16 has three more mantissa bits)
        tol = {"fp32": 6e-5, "bf16": 2.5e-2, "fp16": 4e-3}[precision]
        assert np.isfinite(got).all() and err < tol, (T, H, precision, key_tok is not None, err)


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
def test_rope_hd32_against_numpy(T, H):
    B = 2 if T < 600 else 1
    rng = np.random.default_rng(T * 31 + H)
    x = (rng.standard_normal((B * T, 3 * H * 32)) * 2.0).astype(np.float32)
    L = _lib.lib()
    d2 = 2 * H * 32
    got = x.copy()
    _lib.check(L.pg_dbg_rope_hd(0, _lib.PG_PREC_FP32, _lib.ptr(got), B, T, H, 32))
    want = ref.rotate_qkv_rows(x, B, T, H, 32)
    assert np.array_equal(got, want)                                            # strict mode: the host fp32 loop, bit for bit (v included)
    assert np.array_equal(got[:, d2:], x[:, d2:]) and np.array_equal(got[0, :d2], x[0, :d2])
    if T > 1:
        assert not np.array_equal(got[1, :d2], x[1, :d2])
    for prec, rnd, mant in ((_lib.PG_PREC_BF16, _round_bf16, 7), (_lib.PG_PREC_F16, _round_f16, 10)):
        got = x.copy()
        _lib.check(L.pg_dbg_rope_hd(0, prec, _lib.ptr(got), B, T, H, 32))
        x16 = rnd(x)
        want = rnd(ref.rotate_qkv_rows(x16, B, T, H, 32))
        assert np.array_equal(got[:, d2:], x16[:, d2:])
        ulp16 = np.spacing(np.maximum(np.abs(want[:, :d2]), np.float32(2.0 ** -14))) * np.float32(2.0 ** (23 - mant))
        assert (np.abs(got[:, :d2] - want[:, :d2]) <= ulp16).all()


def test_rope_hd32_refuses_more_than_32_heads():
    x = np.zeros((2, 3 * 33 * 32), np.float32)
    assert _lib.lib().pg_dbg_rope_hd(0, _lib.PG_PREC_BF16, _lib.ptr(x), 1, 2, 33, 32) != 0


# ---- forward ------------------------------------------------------------------------------------------------------------------------
# max |engine - reference| per unit of logit std: the 650M tests' bounds (0.25 and 0.04 at logit std 5)
FWD_TOL = {"fp32": None, "bf16": 0.05, "fp16": 0.008}
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_esm2_150m_forward_against_the_reference(precision):
    cfg, sd, rcfg = _case()
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
    print("\n[ESM-2 6 x 640, 20 heads of 32, %s] max|engine - reference| = %.3e %s (logit std %.2f)"
          % (precision, worst, "absolute" if precision == "fp32" else "per unit of logit std", std))


def test_esm2_150m_forward_against_huggingface_logits():
    z = np.load(os.path.join(HERE, "golden", "esm2_hf_hd32.npz"))
    cfg = weights.make_config(weights.ESM2_T30_CONFIG, **json.loads(str(z["cfg"])))
    sd = weights.synthetic_state_dict(cfg, seed=int(z["seed"]), std=float(z["std"]), embed_std=float(z["embed_std"]),
                                      ln_jitter=float(z["ln_jitter"]))
    for precision, tol in (("fp32", 1e-3), ("fp16", 0.04)):
        got = _model(cfg, sd, precision).model.to("cuda:0").forward_logits(z["tokens"])
        assert np.abs(got - z["logits"]).max() < tol, precision


def test_esm2_150m_full_size_strict_logits():
    """esm2_t30_150M's shape (30 layers x 640, 20 heads of 32), two chains of config 2's length, strict mode."""
    cfg = dict(weights.ESM2_T30_CONFIG)
    sd = weights.synthetic_state_dict(cfg, seed=0, std=0.035, embed_std=0.3, ln_jitter=0.1)
    lm = _model(cfg, sd, "fp32").model.to("cuda:0")
    tok = _tokens(np.random.default_rng(3), 2, 258, mask_every=9)
    got = lm.forward_logits(tok)
    want = ref.esm2_forward(sd, ref.Esm2Config.of(cfg), tok)
    err = np.abs(got - want).max()
    print("\n[ESM-2 30 x 640, fp32] max|engine - reference| = %.3e (logit std %.2f)" % (err, want.std()))
    assert err < 1e-3


def test_esm2_150m_auto_precision_and_synthetic_default():
    """precision="auto" (fp16 behind the range guard) resolves and runs; synthetic=True builds the full 150M configuration."""
    cfg, sd, rcfg = _case(n_layers=2, d=128)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = models.ESM2_150M(state_dict=sd, config=cfg)                          # precision="auto"
    lm = m.model.to("cuda:0")
    tok = _tokens(np.random.default_rng(1), 2, 30)
    want = ref.esm2_forward(sd, rcfg, tok)
    assert np.abs(lm.forward_logits(tok) - want).max() < 0.05 * max(1.0, float(want.std()))


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base, name", [("ESM1B_CONFIG", "ESM-1b"), ("MSA1B_CONFIG", "ESM-MSA-1b")])
def test_engine_refuses_heads_of_32_for_the_other_architectures(base, name):
    cfg = weights.make_config(getattr(weights, base), n_layers=1, d_model=128, n_heads=4, d_ffn=512, max_positions=40)
    sd = weights.synthetic_state_dict(cfg, seed=1)
    cls = models.ESM_MSA1 if base == "MSA1B_CONFIG" else models.ESM1b
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = cls(state_dict=sd, config=cfg, precision="bf16")
    with pytest.raises(Exception, match=r"%s with heads of 32.*64" % name):
        m.model.to("cuda:0")


def test_engine_names_the_widths_that_run():
    cfg = weights.make_config(weights.ESM2_T30_CONFIG, n_layers=1, d_model=384, n_heads=16, d_ffn=512, max_positions=40)      # heads of 24
    sd = weights.synthetic_state_dict(cfg, seed=1)
    with pytest.raises(Exception, match=r"head dim must be 64 .* or 32"):
        _model(cfg, sd, "bf16").model.to("cuda:0")


# ---- the sampler --------------------------------------------------------------------------------------------------------------------
def test_esm2_150m_sampler_positions_draws_and_likelihoods():
    cfg, sd, rcfg = _case(n_layers=4, d=256)
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
    ll0, per0 = s.log_likelihood(seq, with_masking=False)
    lp = ref.log_softmax(ref.esm2_forward(sd, rcfg, tok)[0])
    plain = [lp[i, tok[0, i]] for i in range(1, len(seq) + 1)]
    assert np.abs(np.asarray(per0) - np.asarray(plain)).max() < 2e-3 and abs(ll0 - np.mean(plain)) < 1e-3


def _single_chain_run():
    cfg, sd, _ = _case(n_layers=3, d=256, seed=13)
    return common.single_chain_run(_model(cfg, sd, "bf16"))


def _single_chain_child():
    common.single_chain_child(_single_chain_run)


def _child(call, **env):
    return common.child("test_gpu_esm2_150m", call, **env)


def test_esm2_150m_single_chain_replays_a_graph_and_equals_the_eager_loop():
    common.check_single_chain(_single_chain_run, "test_gpu_esm2_150m")


def _shard_job(worlds):
    """A 64-chain job of config 2's chain length, whole and as contiguous shards that know the job's size: (tokens, logits) of the
    whole job, after checking every world against it bit for bit."""
    cfg, sd, _ = _case(n_layers=3)
    return common.shard_job(_model(cfg, sd, "bf16"), worlds)


def _shard_child():
    print("CHILD_DIGEST " + _shard_job((2,)))


def test_esm2_150m_shards_reproduce_the_whole_job():
    """64 chains x 20 heads at 18 key blocks: the whole job and the 32- and 8-chain shards each end in a partial round that the
    attention launch splits -- and with PGIBBS_ATTN_SPLIT=0 (read once per process: a child) the same bits come out."""
    digest = _shard_job((2, 8))
    line = [l for l in _child("_shard_child", PGIBBS_ATTN_SPLIT="0") if l.startswith("CHILD_DIGEST ")][-1]
    assert line.split()[1] == digest


def test_strict_valu_switch_refuses_heads_of_32_by_name():
    """PGIBBS_ATTN_F32=valu selects the all-VALU cross-check kernel, built for heads of 64 only: it must refuse, not run wrong."""
    code = ("_refuse_valu_child")
    out = _child(code, PGIBBS_ATTN_F32="valu")
    assert any(l.startswith("CHILD_REFUSED ") and "PGIBBS_ATTN_F32" in l for l in out), out


def _refuse_valu_child():
    common.refuse_valu_child(32)
