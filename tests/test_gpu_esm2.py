"""ESM-2 (PG_ARCH_ESM2: models.ESM2) on the HIP engine: the rotary-embedding kernel alone (pg_dbg_rope) against numpy in the three
precision modes; the forward against the fp32 reference (tests/_esm2_reference.py) over the sequence lengths that cross every
attention-kernel boundary, against the stored HuggingFace logits, with right-padded batches, and once at full size (33 x 1280);
the sampler on the models.ESM2 holder in its three regimes (one chain: weight-streaming GEMMs + hipGraph replay; a few chains:
64-row tiles; 64 chains x 258 tokens: big tiles, pruned last layer); shards of a job against the whole job, bit for bit."""
import json
import os
import random

import numpy as np
import pytest

import _esm2_gpu_common as common
import _esm2_reference as ref
from _esm2_gpu_common import SEED25, replay_draws as _replay_draws, round_bf16 as _round_bf16, round_f16 as _round_f16, tokens as _tokens
from protein_gibbs_sampler_amd import _lib, esm_sampler, models, weights

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _case(n_layers=6, d=768, seed=7, **over):
    cfg = weights.make_config(weights.ESM2_T33_CONFIG, n_layers=n_layers, d_model=d, d_ffn=4 * d, **over)
    sd = weights.synthetic_state_dict(cfg, seed=seed, std=0.03, embed_std=0.15, ln_jitter=0.1)      # logit std ~5 at d = 768
    return cfg, sd, ref.Esm2Config.of(cfg)


def _model(cfg, sd, precision):
    return common.model(models.ESM2, cfg, sd, precision)


# ---- the rotation kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H", [4, 20])
@pytest.mark.parametrize("T", [1, 16, 27, 258, 600, 1024])
def test_rope_kernel_against_numpy(T, H):
    B = 2 if T < 600 else 1
    rng = np.random.default_rng(T * 31 + H)
    x = (rng.standard_normal((B * T, 3 * H * 64)) * 2.0).astype(np.float32)
    L = _lib.lib()
    d2 = 2 * H * 64

    # strict mode: <= 2 fp32 ulp of the larger member of the (i, i + 32) pair
    got = x.copy()
    _lib.check(L.pg_dbg_rope(0, _lib.PG_PREC_FP32, _lib.ptr(got), B, T, H))
    want = ref.rotate_qkv_rows(x, B, T, H)
    assert np.array_equal(got[:, d2:], x[:, d2:])                                # v: bit-identical
    pair = np.abs(x[:, :d2].reshape(B * T, 2 * H, 2, 32)).max(axis=2, keepdims=True)
    ulp = np.broadcast_to(np.spacing(pair), (B * T, 2 * H, 2, 32)).reshape(B * T, d2)
    assert (np.abs(got[:, :d2] - want[:, :d2]) <= 2 * ulp).all()
    if T > 1:
        assert not np.array_equal(got[1, :d2], x[1, :d2])
    assert np.array_equal(got[0, :d2], x[0, :d2])                               # position 0 is the identity

    # 16-bit modes: round16(rotate_fp32(round16(x))) within one ulp of the 16-bit type
    for prec, rnd, mant in ((_lib.PG_PREC_BF16, _round_bf16, 7), (_lib.PG_PREC_F16, _round_f16, 10)):
        got = x.copy()
        _lib.check(L.pg_dbg_rope(0, prec, _lib.ptr(got), B, T, H))
        x16 = rnd(x)
        want = rnd(ref.rotate_qkv_rows(x16, B, T, H))
        assert np.array_equal(got[:, d2:], x16[:, d2:])                          # v: the input's 16-bit value, untouched
        ulp16 = np.spacing(np.maximum(np.abs(want[:, :d2]), np.float32(2.0 ** -14))) * np.float32(2.0 ** (23 - mant))
        assert (np.abs(got[:, :d2] - want[:, :d2]) <= ulp16).all()


# ---- forward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_esm2_forward_against_the_reference(precision):
    cfg, sd, rcfg = _case()
    lm = _model(cfg, sd, precision).model.to("cuda:0")
    rng = np.random.default_rng(5)
    worst = 0.0
    tol = {"fp32": 1e-3, "bf16": 0.25, "fp16": 0.04}[precision]
    # 16 / 27: one 16- / 32-row tile (weight-streaming GEMMs), 64 ... 288: the attention kernels' key-count boundaries, 600: the
    # long-sequence kernel
    for T in (16, 27, 64, 160, 258, 288, 600):
        B = 3 if T < 300 else 1
        tok = _tokens(rng, B, T)
        want = ref.esm2_forward(sd, rcfg, tok)
        got = lm.forward_logits(tok)
        assert got.shape == want.shape == (B, T, 33)
        err = np.abs(got - want).max()
        worst = max(worst, err)
        assert err < tol, (T, err)
    print("\n[ESM-2 6 x 768, %s] max|engine - reference| over 7 sequence lengths = %.3e (logit std %.2f)" % (precision, worst, want.std()))


@pytest.mark.parametrize("name", ["small", "mid"])
def test_esm2_forward_against_huggingface_logits(name):
    z = np.load(os.path.join(HERE, "golden", "esm2_hf_%s.npz" % name))
    cfg = weights.make_config(weights.ESM2_T33_CONFIG, **json.loads(str(z["cfg"])))
    sd = weights.synthetic_state_dict(cfg, seed=int(z["seed"]), std=float(z["std"]), embed_std=float(z["embed_std"]),
                                      ln_jitter=float(z["ln_jitter"]))
    for precision, tol in (("fp32", 1e-3), ("fp16", 0.04)):
        got = _model(cfg, sd, precision).model.to("cuda:0").forward_logits(z["tokens"])
        assert np.abs(got - z["logits"]).max() < tol, precision


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_esm2_right_padded_batch(precision):
    """<pad> keys are masked and positions are token indices: they do not shift under right padding, so a padded row equals the row
    run alone (and the reference, which takes t from the token axis)."""
    cfg, sd, rcfg = _case(n_layers=3)
    lm = _model(cfg, sd, precision).model.to("cuda:0")
    rng = np.random.default_rng(9)
    tok = np.full((3, 40), 1, dtype=np.int64)
    lens = (40, 23, 9)
    for b, n in enumerate(lens):
        tok[b, :n] = _tokens(rng, 1, n, mask_every=5)[0]
    got = lm.forward_logits(tok)
    want = ref.esm2_forward(sd, rcfg, tok)
    tol = 1e-3 if precision == "fp32" else 0.2
    for b, n in enumerate(lens):
        assert np.abs(got[b, :n] - want[b, :n]).max() < tol
        alone = lm.forward_logits(tok[b:b + 1, :n])
        assert np.abs(alone[0] - got[b, :n]).max() < (2e-4 if precision == "fp32" else 0.08)


def test_esm2_full_size_strict_logits():
    """esm2_t33_650M's shape (33 layers x 1280, 20 heads), two chains of config 2's length, strict mode against the fp32 reference."""
    cfg = dict(weights.ESM2_T33_CONFIG)
    sd = weights.synthetic_state_dict(cfg, seed=0, std=0.025, embed_std=0.3, ln_jitter=0.1)      # logit std ~10
    lm = _model(cfg, sd, "fp32").model.to("cuda:0")
    tok = _tokens(np.random.default_rng(3), 2, 258, mask_every=9)
    got = lm.forward_logits(tok)
    want = ref.esm2_forward(sd, ref.Esm2Config.of(cfg), tok)
    err = np.abs(got - want).max()
    print("\n[ESM-2 33 x 1280, fp32] max|engine - reference| = %.3e (logit std %.2f)" % (err, want.std()))
    assert err < 1e-3


def test_msa_entry_points_reject_an_esm2_engine():
    cfg, sd, _ = _case(n_layers=1, d=128)
    lm = _model(cfg, sd, "bf16").model.to("cuda:0")
    tok = np.zeros((1, 2, 8), dtype=np.int32)
    out = np.empty((1, 2, 8, 33), dtype=np.float32)
    assert _lib.lib().pg_msa_forward_logits(lm.handle, _lib.ptr(tok), 1, 2, 8, _lib.ptr(out)) == _lib.PG_ERR_INVALID


# ---- the sampler --------------------------------------------------------------------------------------------------------------------


def test_esm2_sampler_positions_draws_and_likelihoods():
    cfg, sd, rcfg = _case(n_layers=4, d=256)
    s = esm_sampler.ESM_sampler(_model(cfg, sd, "fp32"), device="cuda:0")
    assert s.get_init_seq("AA", 5, 1).tolist() == [[0, 5, 5, 32, 32, 32, 2]]
    s.draw_seed, s.record = 11, True
    random.seed(2)
    out = s.generate(4, SEED25, batch_size=4, num_iters=3, num_positions=5, top_k=3, burnin=2, temperature=0.9, show_progress_bar=False)
    assert len(out) == 4 and all(len(x) == 25 for x in out)
    run = s.last_run[0]
    random.seed(2)
    table = np.asarray([[random.sample(range(1, 26), 5) for _ in range(4)] for _ in range(3)])
    assert (run["table"] == table).all(), "position selection is not bit-exact with random.sample"
    _replay_draws(s, run, 4, 5, 3, 3, 2, 0.9, 11)
    # iteration 0's logits are those of the seed masked at the chosen positions
    tok = s.get_init_seq(SEED25, 25, 4).numpy()
    for b in range(4):
        tok[b, table[0, b]] = 32
    want = ref.esm2_forward(sd, rcfg, tok)
    for b in range(4):
        assert np.abs(run["sampled_logits"][0][b] - want[b, table[0, b]]).max() < 1e-3
    # log-likelihoods: one position masked at a time, and unmasked, against the reference's log-softmax
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


def test_esm2_single_chain_replays_a_graph_and_equals_the_eager_loop():
    common.check_single_chain(_single_chain_run, "test_gpu_esm2")


@pytest.mark.parametrize("B,L,P", [(8, 25, 4), (64, 256, 25)])
def test_esm2_sampler_batch_regimes(B, L, P):
    """8 chains of 25 residues: 216 token rows on 64-row tiles; 64 chains of 256: 16 512 rows on the big tiles, the last layer
    pruned to the 1600 sampled rows.  fp16 operands: logits of iteration 0 against the reference, every draw from its logits."""
    cfg, sd, rcfg = _case(n_layers=3, d=256, seed=17, max_positions=512)
    s = esm_sampler.ESM_sampler(_model(cfg, sd, "fp16"), device="cuda:0")
    rng = np.random.default_rng(L)
    seq = "".join(np.asarray(list("ACDEFGHIKLMNPQRSTVWY"))[rng.integers(0, 20, L)])
    s.draw_seed, s.record = 5, True
    random.seed(8)
    out = s.generate(B, seq, batch_size=B, num_iters=2, num_positions=P, top_k=0, temperature=1.0, burnin=float("inf"), show_progress_bar=False)
    assert len(out) == B and all(len(x) == L for x in out)
    run = s.last_run[0]
    random.seed(8)
    table = np.asarray([[random.sample(range(1, L + 1), P) for _ in range(B)] for _ in range(2)])
    assert (run["table"] == table).all()
    _replay_draws(s, run, B, P, 2, 0, float("inf"), 1.0, 5)
    tok = s.get_init_seq(seq, L, B).numpy()
    for b in range(B):
        tok[b, table[0, b]] = 32
    want = ref.esm2_forward(sd, rcfg, tok[:4])
    for b in range(4):
        assert np.abs(run["sampled_logits"][0][b] - want[b, table[0, b]]).max() < 0.04


def test_esm2_shards_reproduce_the_whole_job():
    """A 64-chain job of config 2's chain length run whole and as 2 and 8 contiguous shards that know the job's size
    (pg_engine_set_job_items): tokens and the logits of every draw, bit for bit."""
    cfg, sd, _ = _case()
    common.shard_job(_model(cfg, sd, "bf16"), (2, 8))
