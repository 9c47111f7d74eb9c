"""ESM-2 8M (esm2_t6_8M_UR50D: 20 heads of 16, d_model 320; models.ESM2_8M) on the HIP engine, what is peculiar to the size: every head
of 16 in its own columns of the context row, the row kernels at d = 320, which GEMM and attention kernels a forward takes, and the
refusal of a 33rd head; then the shared bodies of tests/_esm2_gpu_common.py at this size: the head-16 attention and rotation kernels
against numpy, the forward (the 6 x 320 model IS the full-size model) and the refusals of heads of 16 elsewhere.  precision="auto" and
the sampler are the esm2_8m rows of tests/test_gpu_esm2_sizes.py."""
import numpy as np
import pytest

import _esm2_gpu_common as common
import _row_reference as rr
import test_gpu_row_kernels as rk
from _esm2_gpu_common import PREC, round_bf16 as _round_bf16, round_f16 as _round_f16, tokens as _tokens
from _esm2_sizes import ATTENTION_H, ATTENTION_T, PRECISIONS, ROPE_H, ROPE_T
from _ln_host import PLAIN, _ln_inplace_host
from protein_gibbs_sampler_amd import _lib, models, weights

pytestmark = pytest.mark.gpu

SIZE = "esm2_8m"
HD = 16
F32 = np.float32


def _case(**kw):
    return common.case(SIZE, **kw)


def _model(cfg, sd, precision):
    return common.model(models.ESM2_8M, cfg, sd, precision)


# ---- the attention kernels ----------------------------------------------------------------------------------------------------------
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
def test_engine_refuses_33_heads_of_16_and_heads_of_24():
    cfg = weights.make_config(weights.ESM2_T6_CONFIG, n_layers=1, d_model=576, n_heads=36, d_ffn=512, max_positions=40)
    sd = weights.synthetic_state_dict(cfg, seed=1)
    with pytest.raises(Exception, match="heads of 16.*at most 32"):
        _model(cfg, sd, "bf16").model.to("cuda:0")
    cfg = weights.make_config(weights.ESM2_T6_CONFIG, n_layers=1, d_model=384, n_heads=16, d_ffn=512, max_positions=40)      # heads of 24
    sd = weights.synthetic_state_dict(cfg, seed=1)
    with pytest.raises(Exception, match=r"head dim must be 64 .* or 32"):
        _model(cfg, sd, "bf16").model.to("cuda:0")

# ---- the shared bodies (tests/_esm2_gpu_common.py) at this size: the head-16 kernels alone, the forward, the refusals elsewhere -------
@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("H", ATTENTION_H)
@pytest.mark.parametrize("T", ATTENTION_T)
def test_attention_hd16_against_numpy(T, H, precision):
    common.check_attention_hd(SIZE, T, H, precision)


@pytest.mark.parametrize("H", ROPE_H)
@pytest.mark.parametrize("T", ROPE_T)
def test_rope_hd16_against_numpy(T, H):
    common.check_rope_hd(SIZE, T, H)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_esm2_8m_forward_against_the_reference(precision):
    common.check_forward(SIZE, "", precision)


def test_esm2_8m_forward_against_huggingface_logits():
    common.check_huggingface_logits("hd16")


@pytest.mark.parametrize("base, name, cls", [("ESM1B_CONFIG", "ESM-1b", "ESM1b"), ("MSA1B_CONFIG", "ESM-MSA-1b", "ESM_MSA1"),
                                             ("ESM1_T6_CONFIG", "ESM-1", "ESM6")])
def test_engine_refuses_heads_of_16_for_the_other_architectures(base, name, cls):
    assert common.OTHER_ARCHS[name] == (base, cls)
    common.check_other_architectures_refuse_the_width(SIZE, name)
