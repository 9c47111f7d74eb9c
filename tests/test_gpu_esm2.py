"""ESM-2 (PG_ARCH_ESM2: models.ESM2) on the HIP engine, what is peculiar to the 650M size: the rotary-embedding kernel alone
(pg_dbg_rope) against numpy in the three precision modes, right-padded batches against the fp32 reference (tests/_esm2_reference.py),
the MSA entry points' refusal, and the sampler's batch regimes (a few chains: 64-row tiles; 64 chains x 258 tokens: big tiles, pruned
last layer); and the shared bodies of tests/_esm2_gpu_common.py at this size: the forward over the sequence lengths that cross every
attention-kernel boundary and against the stored HuggingFace logits.  The full size, the sampler, the single chain and the shards are
the esm2 rows of tests/test_gpu_esm2_sizes.py."""
import random

import numpy as np
import pytest

import _esm2_gpu_common as common
import _esm2_reference as ref
from _esm2_gpu_common import replay_draws as _replay_draws, round_bf16 as _round_bf16, round_f16 as _round_f16, tokens as _tokens
from protein_gibbs_sampler_amd import _lib, esm_sampler, models

pytestmark = pytest.mark.gpu


def _case(**kw):
    return common.case("esm2", **kw)


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
    common.check_forward("esm2", "", precision)


@pytest.mark.parametrize("name", ["small", "mid"])
def test_esm2_forward_against_huggingface_logits(name):
    common.check_huggingface_logits(name)


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


def test_msa_entry_points_reject_an_esm2_engine():
    cfg, sd, _ = _case(n_layers=1, d=128)
    lm = _model(cfg, sd, "bf16").model.to("cuda:0")
    tok = np.zeros((1, 2, 8), dtype=np.int32)
    out = np.empty((1, 2, 8, 33), dtype=np.float32)
    assert _lib.lib().pg_msa_forward_logits(lm.handle, _lib.ptr(tok), 1, 2, 8, _lib.ptr(out)) == _lib.PG_ERR_INVALID


# ---- the sampler --------------------------------------------------------------------------------------------------------------------
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


