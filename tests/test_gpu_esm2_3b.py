"""ESM-2 3B (esm2_t36_3B_UR50D: d_model 2560, 40 heads -- models.ESM2_3B) on the HIP engine: the wide-row kernels alone (LayerNorm in
its four forms at d = 2560 and 2304, the rotation at H = 40) against numpy, the 8-chunk LayerNorm at d = 1280 bit for bit against a
host loop in the kernel's operation order (up to the hardware square root), the GEMM dispatcher at the 3B shapes, the forward of a
3-layer cut against the fp32 reference (tests/_esm2_reference.py), fc2's split-K form and the models.ESM2_3B synthetic holder.  The full
size, the sampler, the single chain and the shards are the esm2_3b rows of tests/test_gpu_esm2_sizes.py."""
import random
import warnings

import numpy as np
import pytest

import _esm2_gpu_common as common
import _esm2_reference as ref
from _esm2_gpu_common import SEED25, round_bf16 as _round_bf16, round_f16 as _round_f16, tokens as _tokens
from _ln_host import _fma32, _ln_inplace_host, _wave_sum  # noqa: F401  (the host restatement of csrc/ln_row.h)
from protein_gibbs_sampler_amd import _lib, esm_sampler, models, weights

pytestmark = pytest.mark.gpu

F32 = np.float32


# ---- LayerNorm: the 10-chunk row kernels ------------------------------------------------------------------------------------------
def _ln_inputs(M, d):
    rng = np.random.default_rng(M * 7 + d)
    x = (rng.standard_normal((M, d), dtype=np.float32) * 3 + 1).astype(np.float32)
    x[:, -1] += 40.0                                           # the last chunk's last lane matters to the mean and the variance
    g = rng.standard_normal(d, dtype=np.float32)
    b = rng.standard_normal(d, dtype=np.float32)
    x64 = x.astype(np.float64)
    want = (x64 - x64.mean(-1, keepdims=True)) / np.sqrt(x64.var(-1, keepdims=True) + 1e-5) * g + b
    return x, g, b, want


@pytest.mark.parametrize("d", [2560, 2304])      # 2304: lanes 0 .. 63 hold 9 chunks, the tenth is empty
@pytest.mark.parametrize("M", [1, 17, 4099])
def test_layernorm_wide_rows(M, d):
    x, g, b, want = _ln_inputs(M, d)
    L = _lib.lib()
    big = max(1.0, np.abs(want).max())
    y = np.full_like(x, np.nan)
    _lib.check(L.pg_dbg_layernorm(0, _lib.ptr(x), _lib.ptr(g), _lib.ptr(b), _lib.ptr(y), M, d, 1e-5))
    assert np.abs(y - want).max() < 2e-5 * big                  # the bound test_gpu_kernels.py::test_layernorm uses
    # operand rows: one rounding to the 16-bit type on top (bf16 2^-9, fp16 2^-12 relative), the split rows hi + lo 2^-17
    for prec, rel in ((_lib.PG_PREC_BF16, 2.0 ** -8), (_lib.PG_PREC_F16, 2.0 ** -11), (_lib.PG_PREC_FP32, 2.0 ** -16)):
        h = np.full_like(x, np.nan)
        _lib.check(L.pg_dbg_layernorm_operand(0, prec, _lib.ptr(x), _lib.ptr(g), _lib.ptr(b), _lib.ptr(h), M, d, 1e-5))
        assert (np.abs(h - want) <= 2e-5 * big + np.abs(want) * rel).all(), prec
        if prec == _lib.PG_PREC_BF16:
            assert np.array_equal(h, _round_bf16(y))            # the same arithmetic as the fp32 form, rounded once
        elif prec == _lib.PG_PREC_F16:
            assert np.array_equal(h, _round_f16(y))
        else:
            hi = _round_bf16(y)
            assert np.array_equal(h, hi + _round_bf16(y - hi))    # the split store: hi = bf16(v), lo = bf16(v - hi)


def test_layernorm_refuses_rows_wider_than_2560():
    x, g, b, _ = _ln_inputs(2, 2816)
    y = np.empty_like(x)
    L = _lib.lib()
    assert L.pg_dbg_layernorm(0, _lib.ptr(x), _lib.ptr(g), _lib.ptr(b), _lib.ptr(y), 2, 2816, 1e-5) != 0
    assert b"2560" in L.pg_last_error()
    assert L.pg_dbg_layernorm_operand(0, _lib.PG_PREC_BF16, _lib.ptr(x), _lib.ptr(g), _lib.ptr(b), _lib.ptr(y), 2, 2816, 1e-5) != 0


@pytest.mark.parametrize("d", [1280, 768, 2560, 2304])
def test_layernorm_bits_equal_the_host_loop(d):
    """d = 1280 / 768: the 8-chunk instantiation every model up to d_model 2048 runs -- its bits are pinned through the change of
    ln_row.h to a template.  d = 2560 / 2304: the 10-chunk instantiation obeys the same definition."""
    M = 37
    x, g, b, _ = _ln_inputs(M, d)
    y = np.empty_like(x)
    _lib.check(_lib.lib().pg_dbg_layernorm(0, _lib.ptr(x), _lib.ptr(g), _lib.ptr(b), _lib.ptr(y), M, d, 1e-5))
    # every row equals the host loop bit for bit, with the root of its variance at most one ulp from the correctly rounded one
    wants = [_ln_inplace_host(x, g, b, 1e-5, u).view(np.uint32) for u in (0, -1, 1)]
    rows_equal = np.stack([(y.view(np.uint32) == w).all(axis=1) for w in wants])
    assert rows_equal.any(axis=0).all(), (rows_equal.sum(axis=1), np.abs(y - wants[0].view(F32)).max())


# ---- the rotation at 40 heads -----------------------------------------------------------------------------------------------------
def _rotate_rows_strict(x, B, T, H):
    """The rotation with every product and the add / subtract rounded to float32 separately (what -ffp-contract=off compiles)."""
    cos, sin = ref.cos_sin(T)
    u = np.array(x, dtype=F32).reshape(B, T, 3, H, 64)
    for part in (0, 1):
        lo, hi = u[:, :, part, :, :32].copy(), u[:, :, part, :, 32:].copy()
        c, s = cos[None, :, None, :], sin[None, :, None, :]
        u[:, :, part, :, :32] = ((lo * c).astype(F32) - (hi * s).astype(F32)).astype(F32)
        u[:, :, part, :, 32:] = ((hi * c).astype(F32) + (lo * s).astype(F32)).astype(F32)
    return u.reshape(B * T, 3 * H * 64)


@pytest.mark.parametrize("H", [40, 36, 33])       # 36 / 33: the last pass is partly empty
@pytest.mark.parametrize("T", [1, 27, 258, 600])
def test_rope_kernel_at_40_heads(T, H):
    B = 2 if T < 600 else 1
    rng = np.random.default_rng(T * 31 + H)
    x = (rng.standard_normal((B * T, 3 * H * 64)) * 2.0).astype(np.float32)
    L = _lib.lib()
    d2 = 2 * H * 64
    got = x.copy()
    _lib.check(L.pg_dbg_rope(0, _lib.PG_PREC_FP32, _lib.ptr(got), B, T, H))
    want = _rotate_rows_strict(x, B, T, H)
    assert np.array_equal(want, ref.rotate_qkv_rows(x, B, T, H))
    # strict mode: the numpy loop's bits (the engine's table takes cos / sin from libm, numpy from its own routines: an entry may
    # differ in its last bit, hence the bound of test_rope_kernel_against_numpy on the few values that are not identical)
    assert np.array_equal(got[:, d2:], x[:, d2:])                                # v: bit-identical
    assert (got == want).mean() > 0.999
    pair = np.abs(x[:, :d2].reshape(B * T, 2 * H, 2, 32)).max(axis=2, keepdims=True)
    ulp = np.broadcast_to(np.spacing(pair), (B * T, 2 * H, 2, 32)).reshape(B * T, d2)
    assert (np.abs(got[:, :d2] - want[:, :d2]) <= 2 * ulp).all()
    assert np.array_equal(got[0, :d2], x[0, :d2])                                # position 0 is the identity
    for prec, rnd, mant in ((_lib.PG_PREC_BF16, _round_bf16, 7), (_lib.PG_PREC_F16, _round_f16, 10)):
        got = x.copy()
        _lib.check(L.pg_dbg_rope(0, prec, _lib.ptr(got), B, T, H))
        x16 = rnd(x)
        want = rnd(_rotate_rows_strict(x16, B, T, H))
        assert np.array_equal(got[:, d2:], x16[:, d2:])                          # v: the input's 16-bit value, untouched
        ulp16 = np.spacing(np.maximum(np.abs(want[:, :d2]), np.float32(2.0 ** -14))) * np.float32(2.0 ** (23 - mant))
        assert (np.abs(got[:, :d2] - want[:, :d2]) <= ulp16).all()


def test_rope_refuses_more_than_40_heads():
    x = np.zeros((2, 3 * 41 * 64), dtype=np.float32)
    assert _lib.lib().pg_dbg_rope(0, _lib.PG_PREC_BF16, _lib.ptr(x), 1, 2, 41) != 0


# ---- the GEMM dispatcher at the 3B shapes -----------------------------------------------------------------------------------------
def _gelu(x):
    from scipy.special import erf
    return 0.5 * x * (1.0 + erf(x * 0.7071067811865476))


_OPERANDS = {}


def _operands(M, N, K):
    """Seeded operands, generated once per width (the 8256-row activations are 340 MB at K = 10240)."""
    if ("x", K) not in _OPERANDS:
        rng = np.random.default_rng(K)
        x = rng.standard_normal((8256, K), dtype=np.float32)
        x[:, 0] += np.arange(8256, dtype=np.float32) * 0.01       # break any row symmetry
        _OPERANDS[("x", K)] = x
    if ("w", N, K) not in _OPERANDS:
        rng = np.random.default_rng(N * 3 + K)
        _OPERANDS[("w", N, K)] = (rng.standard_normal((N, K), dtype=np.float32) * np.float32(1.0 / np.sqrt(K)),
                                  rng.standard_normal(N, dtype=np.float32))
    w, b = _OPERANDS[("w", N, K)]
    return np.ascontiguousarray(_OPERANDS[("x", K)][:M]), w, b


# (N, K, bf16 / fp16 epilogues, strict epilogues): QKV, out-projection (+ the LM head's dense: fp32 + GELU / plain), fc1, fc2
GEMMS_3B = [(7680, 2560, (3,), (0,)), (2560, 2560, (2, 1), (2, 0)), (10240, 2560, (4,), (5,)), (2560, 10240, (2,), (2,))]


@pytest.mark.parametrize("M", [32, 258, 8256])    # one chain (weight streaming), a few (64-row tiles), a 32-chain shard (big tiles)
@pytest.mark.parametrize("N,K,epis16,epis32", GEMMS_3B)
def test_gemm_at_3b_shapes(M, N, K, epis16, epis32):
    x, w, b = _operands(M, N, K)
    rows = np.unique(np.concatenate([np.arange(0, M, 37), np.arange(max(0, M - 70), M)]))      # every 64-row block, the whole tail
    rng = np.random.default_rng(M + N)
    res = rng.standard_normal((M, N), dtype=np.float32) * 3
    L = _lib.lib()
    for prec, rnd, epis in ((_lib.PG_PREC_BF16, _round_bf16, epis16), (_lib.PG_PREC_F16, _round_f16, epis16), (_lib.PG_PREC_FP32, None, epis32)):
        if rnd is None:
            plain = x[rows].astype(np.float64) @ w.astype(np.float64).T + b
        else:
            plain = (rnd(x[rows]) @ rnd(w).T).astype(np.float64) + b             # fp32 matmul of the rounded operands
        for epi in epis:
            out = res.copy()
            _lib.check(L.pg_dbg_gemm(0, prec, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(out), M, N, K, epi))
            want = plain
            if epi in (1, 4, 5):
                want = _gelu(want)
            if epi == 2:
                want = want + res[rows].astype(np.float64)
            big = max(1.0, np.abs(want).max())
            got = out[rows]
            if rnd is None:       # strict: 2^-17 relative per product (the dropped lo.lo term), 2^-16 for rows that leave as hi + lo
                tol = 6e-5 * big + (np.abs(want) * 2.0 ** -15 if epi == 5 else 0)       # 6e-5: test_gpu_strict_kernels.py's REL
                # the fused fc1 epilogue evaluates GELU with a fit of abs error 3.2e-6
                assert (np.abs(got - want) <= tol + (1e-5 if epi == 5 else 0)).all(), (prec, epi, float(np.abs(got - want).max()))
            elif epi >= 3:        # 16-bit outputs: the output rounding on top (bf16 2^-9, fp16 2^-12; GELU fit of the bf16 epilogue)
                assert (np.abs(got - want) <= 3e-3 * big + np.abs(want) * 2.0 ** -8).all(), (prec, epi, float(np.abs(got - want).max()))
                assert np.array_equal(got, rnd(got))
            else:                 # fp32 outputs: accumulation-order noise against the fp32 matmul
                assert np.abs(got - want).max() < 3e-3 * big, (prec, epi, float(np.abs(got - want).max()))
            if epi == 2 and M > 1:
                assert not np.array_equal(out[rows], res[rows])


# ---- forward ------------------------------------------------------------------------------------------------------------------------
def _cached_case():
    """the 3-layer cut of the shared suite (236 M weights on the host), drawn once while the tests that use it follow each other"""
    return common.case("esm2_3b")


def _model(cfg, sd, precision):
    return common.model(models.ESM2_3B, cfg, sd, precision)


def test_engine_refuses_wider_models_by_name():
    cfg = weights.make_config(weights.ESM2_T36_CONFIG, n_layers=1, d_model=2688, n_heads=42, d_ffn=256)
    sd = weights.synthetic_state_dict(cfg, seed=1)
    with pytest.raises(Exception, match="2560"):
        _model(cfg, sd, "bf16").model.to("cuda:0")


# max |engine - reference| over the lengths and the padded batch, per unit of logit std (5.30 for this model).  First measured run on
# an MI355X: fp32 5.6e-5 (the bound is 1e-3 absolute), bf16 3.12e-2, fp16 3.21e-3; the bounds are 2.5 x those, the ratio the 650M
# tests keep (0.25 and 0.04 at logit std 5).
FWD_TOL = {"fp32": None, "bf16": 0.08, "fp16": 0.008}


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_esm2_3b_forward_against_the_reference(precision):
    cfg, sd, rcfg = _cached_case()
    lm = _model(cfg, sd, precision).model.to("cuda:0")
    rng = np.random.default_rng(5)
    worst, std = 0.0, 1.0
    # 16: one 16-row tile (weight-streaming GEMMs, LayerNorm in launches of its own), 258: whole-sequence attention, 600: the
    # long-sequence kernel; then a right-padded batch
    for T in (16, 258, 600):
        B = 2 if T < 300 else 1
        tok = _tokens(rng, B, T)
        want = ref.esm2_forward(sd, rcfg, tok)
        got = lm.forward_logits(tok)
        assert got.shape == want.shape == (B, T, 33)
        std = float(want.std())
        err = float(np.abs(got - want).max())
        worst = max(worst, err / std)
        assert err < (1e-3 if precision == "fp32" else FWD_TOL[precision] * std), (T, err, std)
    tok = np.full((3, 40), 1, dtype=np.int64)
    lens = (40, 23, 9)
    for b, n in enumerate(lens):
        tok[b, :n] = _tokens(rng, 1, n, mask_every=5)[0]
    got = lm.forward_logits(tok)
    want = ref.esm2_forward(sd, rcfg, tok)
    for b, n in enumerate(lens):
        err = float(np.abs(got[b, :n] - want[b, :n]).max())
        worst = max(worst, err / std)
        assert err < (1e-3 if precision == "fp32" else FWD_TOL[precision] * std), (b, err)
    print("\n[ESM-2 3 x 2560, %s] max|engine - reference| / logit std = %.3e (logit std %.2f)" % (precision, worst, std))


def test_esm2_3b_small_job_does_not_depend_on_earlier_calls():
    """fc2 at K = 10240 runs as 8 K-splits when the job is small (<= 2048 token rows).  The engine's split-K scratch only grows, so the
    choice must come from the shape alone: ~200 token rows on a fresh engine (the scratch sized by this very call), the same rows
    again after a ~600-row call has enlarged it, and on a second engine that saw the 600 rows first -- identical logits, and the
    split form every time."""
    cfg, sd, rcfg = _cached_case()
    rng = np.random.default_rng(77)
    small, large = _tokens(rng, 4, 50), _tokens(rng, 3, 200)

    def fc2_kernels(lm, tok):
        lm.prof_enable(True)
        lm.prof_reset()
        out = lm.forward_logits(tok)
        kernels = lm.prof_get_kernels("gemm_fc2")
        lm.prof_enable(False)
        return out, kernels

    lm = _model(cfg, sd, "bf16").model.to("cuda:0")
    first, k_first = fc2_kernels(lm, small)
    lm.forward_logits(large)
    again, k_again = fc2_kernels(lm, small)
    assert "x8k" in k_first and k_first == k_again, (k_first, k_again)
    assert np.array_equal(first, again)
    other = _model(cfg, sd, "bf16").model.to("cuda:0")
    other.forward_logits(large)
    assert np.array_equal(other.forward_logits(small), first)
    assert np.abs(first - ref.esm2_forward(sd, rcfg, small)).max() < FWD_TOL["bf16"] * 5.3


@pytest.mark.parametrize("M", [64, 192, 256])
def test_fc2_split_k_at_3b_depth(M):
    """(N, K) = (2560, 10240) with the residual epilogue at the heights that take the K-split tile kernels (64-row tiles at 64 and 192
    rows, 128-row tiles at 256; beyond 256 rows this shape has tiles enough unsplit) and the 8-way fixed-order reduction; every row
    against the fp32 matmul of the rounded operands."""
    x, w, b = _operands(M, 2560, 10240)
    res = np.random.default_rng(M).standard_normal((M, 2560), dtype=np.float32) * 3
    for prec, rnd in ((_lib.PG_PREC_BF16, _round_bf16), (_lib.PG_PREC_F16, _round_f16)):
        want = (rnd(x) @ rnd(w).T).astype(np.float64) + b + res
        out = res.copy()
        _lib.check(_lib.lib().pg_dbg_gemm(0, prec, _lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(out), M, 2560, 10240, 2))
        assert np.abs(out - want).max() < 3e-3 * max(1.0, np.abs(want).max()), prec


def test_esm2_3b_one_chain_of_27_tokens():
    """27 token rows: the weight-streaming GEMMs, where d_model 2560 takes the separate LayerNorm launch (the LayerNorm-folding GEMM
    holds K <= 1280)."""
    cfg, sd, rcfg = _cached_case()
    tok = _tokens(np.random.default_rng(27), 1, 27)
    want = ref.esm2_forward(sd, rcfg, tok)
    for precision in ("fp32", "bf16", "fp16"):
        got = _model(cfg, sd, precision).model.to("cuda:0").forward_logits(tok)
        err = float(np.abs(got - want).max())
        assert err < (1e-3 if precision == "fp32" else FWD_TOL[precision] * want.std()), (precision, err)


# ---- the sampler --------------------------------------------------------------------------------------------------------------------
def test_models_esm2_3b_synthetic_holder():
    cfg = weights.make_config(weights.ESM2_T36_CONFIG, n_layers=3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        s = esm_sampler.ESM_sampler(models.ESM2_3B(config=cfg, synthetic=True), device="cuda:0")
    assert s.model.cfg["d_model"] == 2560 and s.model.cfg["n_heads"] == 40
    random.seed(1)
    out = s.generate(2, SEED25, batch_size=2, num_iters=2, num_positions=3, top_k=0, temperature=1.0, burnin=float("inf"), show_progress_bar=False)
    assert len(out) == 2 and all(len(x) == 25 and set(x) <= set("ACDEFGHIKLMNPQRSTVWY") for x in out)
