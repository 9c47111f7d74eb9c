"""ESM-2 15B (esm2_t48_15B_UR50D: 40 heads of 128, d_model 5120; models.ESM2_15B) on the HIP engine: the head-128 attention kernels
alone (pg_dbg_attention_kv: the whole-sequence ladder up to 288 keys, 128-key tiles beyond, <pad> keys, three precisions) element by
element under the bounds of tests/_attention_reference.py, the head-128 rotation (pg_dbg_rope_hd) against the separately rounded
numpy loop, the 20-chunk row kernels (LayerNorm, embedding, gather, LM tail) at d = 3072 .. 5120, the GEMMs at the 15B shapes, the engine
forward of one full-width layer and of a HuggingFace fixture, a call whose buffers pass 2 GiB, and the refusals of wider models and of
heads of 128 elsewhere.  The sampler on a small deep model, the single chain and the shards are the esm2_15b rows of
tests/test_gpu_esm2_sizes.py."""
import warnings

import numpy as np
import pytest

import _attention_reference as ar
import _esm2_gpu_common as common
import _esm2_reference as ref
import _row_reference as rr
import test_gpu_attention_kernels as ak
import test_gpu_gemm_kernels as gm
import test_gpu_row_kernels as rk
from _esm2_gpu_common import PREC, round_bf16 as _round_bf16, round_f16 as _round_f16, tokens as _tokens
from _ln_host import PLAIN, SPLIT_DUP, _ln_inplace_host
from protein_gibbs_sampler_amd import _lib, esm_sampler, models, weights

pytestmark = pytest.mark.gpu

F32 = np.float32
HD = 128


# ---- the attention kernels ----------------------------------------------------------------------------------------------------------
def _expected_form(T, strict):
    """what plan_attention / plan_attention_f32 must say at head 128: whole sequences up to 288 keys (the fine ladder), 128-key tiles
    beyond; strict: 64-key tiles, at most three query blocks per wave"""
    if strict:
        blocks = (T + 15) // 16
        return "split-f32 kb4 nqb%d hd128" % (1 if blocks <= 4 else 2 if blocks <= 8 else 3)
    return "whole kb%d hd128" % ((((T + 15) // 16) + 1) & ~1) if T <= 288 else "long t128 hd128"


@pytest.mark.parametrize("fmt", ["f32", "bf16", "f16"])
@pytest.mark.parametrize("H", [2, 40])
@pytest.mark.parametrize("T", [16, 27, 258, 288, 289, 300, 577, 1026])
def test_attention_hd128_under_the_derived_bound(T, H, fmt):
    """16 .. 288: rungs of the whole-sequence ladder (288 = the last one at this width), 289 .. 1026: three to nine 128-key tiles of the
    online-softmax kernel.  late_last / late_tile put the row maximum in the last tile, so every earlier tile's sum is rescaled.
    Without and with a ragged <pad> batch; 40 heads: one sequence and the families whose error would show a wrong head or tile."""
    strict = fmt == "f32"
    families = ar.FAMILIES if H == 2 else ("late_last", "late_tile", "intcode")
    for pad in (False, True):
        tok = (ar.pad_tokens(T) if H == 2 else ar.pad_tokens(T)[:1]) if pad else None
        n_seq = tok.shape[0] if pad else (2 if H == 2 else 1)
        want = ak._plan(0, ak.PREC[fmt], n_seq, T, 0, H, HD, pad, False)
        assert want.startswith(_expected_form(T, strict) + (" pad" if pad else "")), want
        live = np.ones((n_seq, T), bool) if tok is None else tok != ar.PAD
        for family in families:
            if family == "late_tile" and T <= 288:
                continue                                    # the same key as every family's first
            peak = ar.last_real_key(tok) if pad and family == "late_last" else None
            qkv = ar.family_qkv(family, T, n_seq, T, H, HD, peak=peak)
            if pad:
                ar.poison_pad(qkv, tok, H, HD)
            qkv = ar.round_to(fmt, qkv)
            ctx, ran = ak._run_chain(fmt, qkv, H, HD, tok, None, None)
            assert ran == want, (ran, want)
            assert np.isfinite(ctx).all(), (family, "non-finite context (rows of <pad> queries included)")
            res = ar.chain_attention(qkv, H, HD, tok)
            err = np.abs(ctx - res.ref)[live]
            if strict and family == "gaussian":
                b = np.full(err.shape, ak.REL * max(1.0, np.abs(res.ref[live]).max()))
            else:
                b = (ar.bound_strict(res) if strict else ar.bound(res, fmt))[live]
            frac = float((err / np.maximum(b, 1e-300)).max())
            print("hd128 %s %s T=%d H=%d %s: %.3f of the bound" % (ran.split(" hd128")[0], "pad" if pad else "plain", T, H, family, frac))
            assert (err <= b).all(), (family, fmt, T, H, pad, frac)
            if family == "unity":
                assert (ctx[live] == 1.0).all() if not strict else np.abs(ctx[live] - 1.0).max() <= 2.0 ** -23, (fmt, T, pad)


@pytest.mark.parametrize("fmt,n_seq,T", [("bf16", 9, 258), ("f16", 13, 130)])
def test_attention_hd128_split_form(fmt, n_seq, T):
    """more pairs than resident workgroups at 40 heads: the last round's pairs run as several workgroups each (one workgroup per CU at
    18 key blocks, two at 10)"""
    want = ak._plan(0, ak.PREC[fmt], n_seq, T, 0, 40, HD, False, False)
    assert " split" in want and want.startswith(_expected_form(T, False)), want
    for family in ("negative", "intcode", "unity"):
        qkv = ar.round_to(fmt, ar.family_qkv(family, T, n_seq, T, 40, HD))
        ctx, ran = ak._run_chain(fmt, qkv, 40, HD, None, None, None)
        assert ran == want
        res = ar.chain_attention(qkv, 40, HD, None)
        assert (np.abs(ctx - res.ref) <= ar.bound(res, fmt)).all(), (family, fmt)


def test_attention_hd_at_64_and_32_is_what_it_was():
    B, T, H = 2, 70, 3
    L = _lib.lib()
    x = np.random.default_rng(3).standard_normal((B, T, 3 * H * 64)).astype(np.float32) * np.float32(0.5)
    for prec in PREC.values():
        a, b = np.zeros((B, T, H * 64), np.float32), np.zeros((B, T, H * 64), np.float32)
        _lib.check(L.pg_dbg_attention(0, prec, _lib.ptr(x), _lib.ptr(a), B, T, H))
        _lib.check(L.pg_dbg_attention_hd(0, prec, _lib.ptr(x), _lib.ptr(b), B, T, H, 64, None, -1))
        assert np.array_equal(a, b)
    assert L.pg_dbg_attention_hd(0, _lib.PG_PREC_BF16, _lib.ptr(x), _lib.ptr(a), B, T, H, 48, None, -1) != 0
    for hd, fmt in ((64, "bf16"), (32, "f16"), (32, "f32")):
        qkv = ar.round_to(fmt, ar.family_qkv("gaussian", 5, B, 300, H, hd))
        ctx, ran = ak._run_chain(fmt, qkv, H, hd, None, None, None)
        res = ar.chain_attention(qkv, H, hd, None)
        assert " hd%d" % hd in ran and "t128" not in ran
        b = ak.REL * max(1.0, np.abs(res.ref).max()) if fmt == "f32" else ar.bound(res, fmt)
        assert (np.abs(ctx - res.ref) <= b).all(), (hd, fmt)


# ---- the rotation kernel ------------------------------------------------------------------------------------------------------------
def _rotate_rows_strict(x, B, T, H):
    """The rotation with every product and the add / subtract rounded to float32 separately (what -ffp-contract=off compiles)."""
    cos, sin = ref.cos_sin(T, HD)
    u = np.array(x, dtype=F32).reshape(B, T, 3, H, HD)
    for part in (0, 1):
        lo, hi = u[:, :, part, :, :64].copy(), u[:, :, part, :, 64:].copy()
        c, s = cos[None, :, None, :], sin[None, :, None, :]
        u[:, :, part, :, :64] = ((lo * c).astype(F32) - (hi * s).astype(F32)).astype(F32)
        u[:, :, part, :, 64:] = ((hi * c).astype(F32) + (lo * s).astype(F32)).astype(F32)
    return u.reshape(B * T, 3 * H * HD)


@pytest.mark.parametrize("H", [40, 36, 33, 2])       # 36 / 33: the last pass is partly empty; 2: the narrow instantiation (H <= 20)
@pytest.mark.parametrize("T", [1, 27, 258, 600])
def test_rope_kernel_at_heads_of_128(T, H):
    B = 2 if T < 600 else 1
    rng = np.random.default_rng(T * 31 + H)
    x = (rng.standard_normal((B * T, 3 * H * HD)) * 2.0).astype(np.float32)
    L = _lib.lib()
    d2 = 2 * H * HD
    got = x.copy()
    _lib.check(L.pg_dbg_rope_hd(0, _lib.PG_PREC_FP32, _lib.ptr(got), B, T, H, HD))
    want = _rotate_rows_strict(x, B, T, H)
    assert np.array_equal(want, ref.rotate_qkv_rows(x, B, T, H, HD))
    # strict mode: the numpy loop's bits (the engine's table takes cos / sin from libm, numpy from its own routines: an entry may
    # differ in its last bit, hence the two-ulp bound on the few values that are not identical)
    assert np.array_equal(got[:, d2:], x[:, d2:])                                # v: bit-identical
    assert (got == want).mean() > 0.999
    pair = np.abs(x[:, :d2].reshape(B * T, 2 * H, 2, 64)).max(axis=2, keepdims=True)
    ulp = np.broadcast_to(np.spacing(pair), (B * T, 2 * H, 2, 64)).reshape(B * T, d2)
    assert (np.abs(got[:, :d2] - want[:, :d2]) <= 2 * ulp).all()
    assert np.array_equal(got[0, :d2], x[0, :d2])                                # position 0 is the identity
    if T > 1:
        assert not np.array_equal(got[1, :d2], x[1, :d2])
    for prec, rnd, mant in ((_lib.PG_PREC_BF16, _round_bf16, 7), (_lib.PG_PREC_F16, _round_f16, 10)):
        got = x.copy()
        _lib.check(L.pg_dbg_rope_hd(0, prec, _lib.ptr(got), B, T, H, HD))
        x16 = rnd(x)
        want = rnd(_rotate_rows_strict(x16, B, T, H))
        assert np.array_equal(got[:, d2:], x16[:, d2:])                          # v: the input's 16-bit value, untouched
        ulp16 = np.spacing(np.maximum(np.abs(want[:, :d2]), np.float32(2.0 ** -14))) * np.float32(2.0 ** (23 - mant))
        assert (np.abs(got[:, :d2] - want[:, :d2]) <= ulp16).all()


@pytest.mark.parametrize("hd, H", [(64, 32), (64, 33), (128, 20), (128, 21)])
def test_rope_at_the_narrow_wide_boundary(hd, H):
    """The rotary launcher's two instantiations per width (csrc/head_width.h: rope_narrow heads, then max_heads) on both sides of the
    threshold: the last head count the narrow kernel takes and the first one of the wide kernel -- a threshold one too high would
    leave the last heads of the row unrotated."""
    B, T = 2, 27
    rng = np.random.default_rng(hd * 31 + H)
    x = (rng.standard_normal((B * T, 3 * H * hd)) * 2.0).astype(np.float32)
    L = _lib.lib()
    d2 = 2 * H * hd
    got = x.copy()
    _lib.check(L.pg_dbg_rope_hd(0, _lib.PG_PREC_FP32, _lib.ptr(got), B, T, H, hd))
    want = ref.rotate_qkv_rows(x, B, T, H, hd)
    print("\n[rope %d heads of %d, fp32] %d of %d values differ from the numpy loop" % (H, hd, int((got != want).sum()), got.size))
    assert np.array_equal(got, want)                                            # strict mode: the host fp32 loop, bit for bit (v included)
    assert np.array_equal(got[:, d2:], x[:, d2:]) and np.array_equal(got[0, :d2], x[0, :d2])
    assert not np.array_equal(got[1, d2 - hd:d2], x[1, d2 - hd:d2])             # the last head of k is rotated
    for prec, rnd, mant in ((_lib.PG_PREC_BF16, _round_bf16, 7), (_lib.PG_PREC_F16, _round_f16, 10)):
        got = x.copy()
        _lib.check(L.pg_dbg_rope_hd(0, prec, _lib.ptr(got), B, T, H, hd))
        x16 = rnd(x)
        want = rnd(ref.rotate_qkv_rows(x16, B, T, H, hd))
        assert np.array_equal(got[:, d2:], x16[:, d2:])
        ulp16 = np.spacing(np.maximum(np.abs(want[:, :d2]), np.float32(2.0 ** -14))) * np.float32(2.0 ** (23 - mant))
        assert (np.abs(got[:, :d2] - want[:, :d2]) <= ulp16).all()


def test_rope_refuses_41_heads_of_128():
    x = np.zeros((2, 3 * 41 * HD), np.float32)
    assert _lib.lib().pg_dbg_rope_hd(0, _lib.PG_PREC_BF16, _lib.ptr(x), 1, 2, 41, HD) != 0
    assert _lib.lib().pg_dbg_rope(0, _lib.PG_PREC_BF16, _lib.ptr(x), 1, 2, 41) != 0


# ---- rows of 3072 .. 5120 features: the 20-chunk row kernels ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5120, 4096, 3072])      # 4096 / 3072: lanes hold 16 / 12 chunks, the rest of the 20 are empty
@pytest.mark.parametrize("M", [1, 17, 4099])
def test_layernorm_rows_up_to_5120(M, d):
    x = rk._rows(M, d, M * 7 + d)
    g, b = rk._affine(d, d)
    L = _lib.lib()
    y = np.full_like(x, np.nan)
    _lib.check(L.pg_dbg_layernorm(0, _lib.ptr(x), _lib.ptr(g), _lib.ptr(b), _lib.ptr(y), M, d, rk.EPS))
    # every row equals the host loop bit for bit, with the root of its variance at most one ulp from the correctly rounded one
    wants = [_ln_inplace_host(x, g, b, rk.EPS, u).view(np.uint32) for u in (0, -1, 1)]
    rows_equal = np.stack([(y.view(np.uint32) == w).all(axis=1) for w in wants])
    assert rows_equal.any(axis=0).all(), (rows_equal.sum(axis=1), np.abs(y - wants[0].view(F32)).max())
    x64 = x.astype(np.float64)
    want = (x64 - x64.mean(-1, keepdims=True)) / np.sqrt(x64.var(-1, keepdims=True) + rk.EPS) * g + b
    assert np.abs(y - want).max() < 2e-5 * max(1.0, np.abs(want).max())          # the bound test_gpu_kernels.py::test_layernorm uses
    # the operand stores (bf16, fp16, split with and without the duplicate block) on the same rows
    y0 = wants[0].view(F32)
    for name, prec, form in rk.FORMS:
        h, kernel = rk.ln_rows(x, g, b, form, prec)
        assert kernel == "plain", (name, kernel)
        rk._check_against_host_loop(h, x, g, b, form, prec, y0)
    for prec, rnd in ((_lib.PG_PREC_BF16, _round_bf16), (_lib.PG_PREC_F16, _round_f16), (_lib.PG_PREC_FP32, None)):
        h = np.full_like(x, np.nan)
        _lib.check(L.pg_dbg_layernorm_operand(0, prec, _lib.ptr(x), _lib.ptr(g), _lib.ptr(b), _lib.ptr(h), M, d, rk.EPS))
        hi = _round_bf16(y)
        assert np.array_equal(h, rnd(y) if rnd else hi + _round_bf16(y - hi))


def test_rows_above_2560_come_in_whole_units_only():
    L = _lib.lib()
    for d in (2816, 5632, 2564):
        x, g = np.zeros((2, d), F32), np.zeros(d, F32)
        assert L.pg_dbg_layernorm(0, _lib.ptr(x), _lib.ptr(g), _lib.ptr(g), _lib.ptr(x.copy()), 2, d, 1e-5) != 0
        assert b"2560" in L.pg_last_error()
    h = np.full((24, 3072), rk.FILL, dtype=np.uint16)                             # column-major output stays d <= 2048
    x, g = np.zeros((8, 3072), F32), np.zeros(3072, F32)
    assert L.pg_dbg_layernorm_rows(0, rk.BF16, rk._p(x), rk._p(g), rk._p(g), rk._p(h), 24, 8, 3072, rk.EPS, PLAIN, 2, 4, None) == _lib.PG_ERR_INVALID
    assert b"column-major" in L.pg_last_error() and (h == rk.FILL).all()


def test_embedding_at_5120():
    """ESM-2's form (no positions, token dropout) and ESM-1b's (positions, LayerNorm before) through the 20-chunk kernel"""
    d = 5120
    for model in ("esm2", "esm1b"):
        has_pos, ln_before, dropout, scaled, rows_per_msa = rk.EMBED_MODELS[model]
        rng = np.random.default_rng(d + len(model))
        e = (rng.standard_normal((rk.V, d), dtype=F32) * F32(0.3)).astype(F32)
        e[:, 0] += np.arange(rk.V, dtype=F32)
        pos = (rng.standard_normal((258 + rr.PAD + 1, d), dtype=F32) * F32(0.2)).astype(F32) if has_pos else None
        gb = rk._affine(d, d + 5) if ln_before else None
        gb2 = rk._affine(d, d + 6)
        for i, (n_seq, T) in enumerate([(1, 1), (3, 27), (5, 258)]):
            for j, pattern in enumerate(rr.PATTERNS):
                tok = rr.make_tokens(pattern, n_seq, T, seed=T * 10 + j)
                prec = (rk.BF16, rk.F16)[(i + j) % 2]
                x, h2 = rk.embed(tok, e, pos, None, 0, gb, gb2, dropout, 1.0, prec)
                want, mag = rr.embed_reference(tok, e, pos, None, 0, gb[0] if gb else None, gb[1] if gb else None, token_dropout=dropout,
                                               eps=rk.EPS, embed_scale=F32(1.0))
                want, mag = want.reshape(-1, d), mag.reshape(-1, d)
                pad = (tok == rr.PAD).ravel()
                case = (model, n_seq, T, pattern)
                assert (x[pad] == 0).all() and not np.signbit(x[pad]).any(), case
                if ln_before:
                    assert np.abs(x - want).max() < 2e-5 * max(1.0, np.abs(want).max()), case
                else:
                    assert (np.abs(x - want) - 8 * rk.U * mag <= 0).all(), case
                h, kernel = rk.ln_rows(x, gb2[0], gb2[1], PLAIN, prec, extra=0)
                assert kernel == "plain" and np.array_equal(h2, h), case


@pytest.mark.parametrize("P", [1, 5])
def test_gather_layernorm_at_5120(P):
    d, width = 5120, 9
    g, b = rk._affine(d, d + P)
    rng = np.random.default_rng(d * 10 + P)
    for n_sel in (1, 7, 801):
        S = (n_sel + P - 1) // P
        n_seq = S + 3
        x = rk._rows(n_seq * width, d, n_sel + d)
        for split, prec in ((0, rk.BF16), (1, rk.BF16), (0, rk.F16)):
            want_all, kernel = rk.ln_rows(x, g, b, SPLIT_DUP if split else PLAIN, prec, extra=0)
            assert kernel == "plain"
            for maps in ("none", "repeats"):
                idx, row_map = rk._index_case(rng, n_sel, P, width, n_seq, maps)
                h = rk.gather_ln(x, idx, row_map, P, width, g, b, n_sel, split, prec)
                pos = idx & 0x3fffffff
                zero = (idx < 0) | (pos >= width)
                s = np.arange(n_sel) // P
                src = (s if row_map is None else row_map[s]) * width + pos
                assert (h[:n_sel][zero] == 0).all() and np.array_equal(h[:n_sel][~zero], want_all[src[~zero]]), (P, n_sel, split, maps)
                assert (h[n_sel:] == rk.FILL).all()
    head = np.ascontiguousarray(x[:64])
    rk._check_against_host_loop(rk.ln_rows(head, g, b, PLAIN, rk.BF16, extra=0)[0], head, g, b, PLAIN, rk.BF16)


@pytest.mark.parametrize("n", [2, 800, 1025])
def test_lm_tail_at_5120(n):
    """Rows wider than 2560 always take the row-per-wave kernel (the workgroup-per-row form is not built with 20 chunks).  Per logit
    a lane adds at most 20 chunk terms of 3 adds each, the butterfly 6 more, the bias 1: with the products' own roundings
    |err| <= 34 u (sum |v_i e_i| + |bias|) -- the 24 u of the 10-chunk kernels with ten more additions in the lane's chain; with the
    LayerNorm in front, its tolerance (2e-5 max(1, |ln|max) per value) carried through the dot product on top."""
    d = 5120
    for vocab in (33, 5):
        g, e, bias, gb = rk._tail_input(n, d, vocab)
        for with_ln in (0, 1):
            logits, small = rk.lm_tail(g, e, bias, gb if with_ln else None)
            assert small == 0 and logits.shape == (n, vocab) and np.isfinite(logits).all()
            want, mag, vmax, esum = rr.lm_tail_reference(g, e, bias, gb[0] if with_ln else None, gb[1] if with_ln else None, rk.EPS)
            bound = 34 * rk.U * mag + (2e-5 * max(1.0, vmax) * esum[None, :] if with_ln else 0.0)
            assert (np.abs(logits - want) <= bound).all(), (n, vocab, with_ln, float((np.abs(logits - want) / bound).max()))


# ---- the GEMM dispatcher at the 15B shapes: exact integers ---------------------------------------------------------------------------
# (N, K, epilogues of pg_dbg_gemm_v with an exact result): QKV (16-bit rows), out-projection / LM-head dense (residual, plain fp32),
# fc1 (its GEMM body through the 16-bit store; its GELU epilogues, which have no exact result, are held per element below: test_gemm_
# gelu_epilogues_at_15b_shapes), fc2 (residual).  Operands are the small integers of tests/_gemm_reference.py: |sum| <= 64 K + 2^21 < 2^24 at K = 20480, so
# every partial sum is exact in fp32 whatever the order, and equality is bit for bit.
GEMMS_15B = [(15360, 5120, (3,)), (5120, 5120, (2, 0)), (20480, 5120, (3,)), (5120, 20480, (2,))]
_INTS = {}


def _int_operands(M, N, K):
    """seeded once per width; rows / columns are prefixes, so a height shares its operands with the others"""
    if ("x", K) not in _INTS:
        for key in [k for k in _INTS if k[0] == "x"]:
            del _INTS[key]
        _INTS[("x", K)] = gm.gr._small_ints(np.random.default_rng([15, K]), 8256, 1, K)[0]
    if ("w", N, K) not in _INTS:
        for key in [k for k in _INTS if k[0] == "w"]:
            del _INTS[key]
        rng = np.random.default_rng([15, N, K])
        _INTS[("w", N, K)] = (gm.gr._small_ints(rng, 1, N, K)[1], rng.integers(-2 ** 20, 2 ** 20 + 1, N).astype(F32),
                              (rng.integers(3000, 40001, N) * rng.choice([-1, 1], N)).astype(F32))
    w, bias32, bias16 = _INTS[("w", N, K)]
    return np.ascontiguousarray(_INTS[("x", K)][:M]), w, bias32, bias16


def _check_exact_sample(out, x, w, bias, res, fmt16):
    """a sample of rows (all columns) and of columns (all rows) that touches every 64-row and every 64-column band and both tails"""
    M, N = out.shape
    rows = np.unique(np.concatenate([np.arange(0, M, 37), np.arange(max(0, M - 70), M)]))
    cols = np.unique(np.concatenate([np.arange(0, N, 53), np.arange(N - 70, N)]))
    for sel, got, want in ((rows, out[rows], np.rint(x[rows].astype(np.float64) @ w.astype(np.float64).T)),
                           (cols, out[:, cols], np.rint(x.astype(np.float64) @ w[cols].astype(np.float64).T))):
        by_rows = want.shape[1] == N
        want = want + (bias if by_rows else bias[cols]).astype(np.float64)
        if res is not None:
            want = want + (res[rows] if by_rows else res[:, cols]).astype(np.float64)
        want = gm.gr.round_to(fmt16, want) if fmt16 else want.astype(F32)
        gm._assert_bits(got, want, "%d x %d, sampled %s" % (M, N, "rows" if by_rows else "columns"))


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("M", [32, 258, 8256])    # one chain (weight streaming), a few (64-row tiles), a 32-chain shard (big tiles)
@pytest.mark.parametrize("N,K,epis", GEMMS_15B)
def test_gemm_at_15b_shapes_exact(M, N, K, epis, fmt):
    x, w, bias32, bias16 = _int_operands(M, N, K)
    for epi in epis:
        res = np.random.default_rng([M, N]).integers(-2 ** 20, 2 ** 20 + 1, (M, N)).astype(F32) if epi == 2 else None
        bias = bias16 if epi == 3 else bias32
        out, ran = gm._run(fmt, x, w, bias, res, epi)
        assert ran and not ran.startswith("error"), ran
        _check_exact_sample(out, x, w, bias, res, fmt if epi == 3 else None)


# The GELU epilogues the engine runs at these shapes -- fc1 (20480, 5120): the 16-bit store with the polynomial GELU (dbg epi 4) and, in
# the strict mode, the fused three-product form that writes split rows (epi 5); the LM head's dense (5120, 5120): fp32 with the erf
# GELU (epi 1) -- on the sparse exact pre-activations of tests/_gemm_reference.py (z = x . w + bias is exact in every order), per
# element under that file's documented epilogue bound (gelu_bound), on the same sample of rows and columns.
_GELU_OPS = {}


def _gelu_operands(M, N, K):
    """gr.gelu_inputs' recipe without its full M x N reference: sparse -1 / 0 / 1 operands, P(non-zero) = sqrt(3.5 / K)"""
    key = (N, K)
    if key not in _GELU_OPS:
        _GELU_OPS.clear()
        rng = np.random.default_rng([3, N, K, 7])
        p = min(1.0, np.sqrt(3.5 / K))
        x = (rng.integers(-1, 2, (8256, K)) * (rng.random((8256, K)) < p * 1.5)).astype(F32)
        w = (rng.integers(-1, 2, (N, K)) * (rng.random((N, K)) < p * 1.5)).astype(F32)
        x[:, 0] = (np.arange(8256) % 3) - 1
        w[:, 1] = (np.arange(N) % 3) - 1
        _GELU_OPS[key] = (x, w, (rng.integers(-8, 9, N) / 8.0).astype(F32))
    x, w, bias = _GELU_OPS[key]
    return np.ascontiguousarray(x[:M]), w, bias


def _sample(M, N):
    rows = np.unique(np.concatenate([np.arange(0, M, 37), np.arange(max(0, M - 70), M)]))
    cols = np.unique(np.concatenate([np.arange(0, N, 53), np.arange(N - 70, N)]))
    return rows, cols
@pytest.mark.parametrize("M", [32, 258, 8256])
@pytest.mark.parametrize("N,K,epi,fmts", [(20480, 5120, 4, ("bf16", "f16")), (20480, 5120, 5, ("f32",)), (5120, 5120, 1, ("bf16", "f16"))])
def test_gemm_gelu_epilogues_at_15b_shapes(M, N, K, epi, fmts):
    from scipy.special import erf
    x, w, bias = _gelu_operands(M, N, K)
    rows, cols = _sample(M, N)
    for fmt in fmts:
        out, ran = gm._run(fmt, x, w, bias, None, epi)
        assert ran and not ran.startswith("error") and np.isfinite(out).all(), ran
        for got, xs, ws, bs in ((out[rows], x[rows], w, bias), (out[:, cols], x, w[cols], bias[cols])):
            z = xs.astype(np.float64) @ ws.astype(np.float64).T + bs.astype(np.float64)
            g = gm.gr.Gelu(xs, ws, bs, z, 0.5 * z * (1.0 + erf(z / np.sqrt(2.0))))
            bound = gm.gr.gelu_bound(g, epi, {1: "f32", 4: fmt, 5: "pair"}[epi])
            err = np.abs(got.astype(np.float64) - g.ref)
            assert (err <= bound).all(), (M, N, K, epi, fmt, float((err / bound).max()))


# The strict mode's three-product GEMMs at the same four shapes, on gr.strict_integers' recipe (small integers with three 9-bit values
# per row, so hi and lo are both used; x = xh + xl and w = wh + wl exactly): bit for bit against xh.wh + xl.wh + xh.wl in int64.
@pytest.mark.parametrize("M", [32, 258, 8256])
@pytest.mark.parametrize("N,K,epis", [(15360, 5120, (0,)), (5120, 5120, (2, 0)), (5120, 20480, (2,))])
def test_strict_gemm_at_15b_shapes_exact(M, N, K, epis):
    x, w, bias, _ = _int_operands(M, N, K)
    x, w = x.copy(), w.copy()
    for t, v in enumerate(gm.gr.NINE_BIT[:3]):
        x[np.arange(M), (3 * np.arange(M) + 11 * t) % K] = v
        w[np.arange(N), (5 * np.arange(N) + 11 * t + 1) % K] = gm.gr.NINE_BIT[t + 1]
    (xh, xl), (wh, wl) = gm.gr.split_pair(x), gm.gr.split_pair(w)
    assert (xh + xl == x).all() and (wh + wl == w).all()
    rows, cols = _sample(M, N)
    mm = lambda a, b: np.rint(a.astype(np.float64) @ b.astype(np.float64).T)
    for epi in epis:
        res = np.random.default_rng([M, N, 3]).integers(-2 ** 20, 2 ** 20 + 1, (M, N)).astype(F32) if epi == 2 else None
        out, ran = gm._run("f32", x, w, bias, res, epi)
        assert ran and not ran.startswith("error"), ran
        for got, r, c in ((out[rows], rows, slice(None)), (out[:, cols], slice(None), cols)):
            want = mm(xh[r], wh[c]) + mm(xl[r], wh[c]) + mm(xh[r], wl[c]) + bias[c].astype(np.float64)
            if res is not None:
                want = want + res[r][:, c].astype(np.float64)
            gm._assert_bits(got, want.astype(F32), "strict %d x %d x %d epi %d" % (M, N, K, epi))


@pytest.mark.parametrize("M", [64, 192, 256])
def test_fc2_split_k_at_15b_depth(M):
    """(N, K) = (5120, 20480) with the residual epilogue, scratch on offer and withheld: 16 K-splits at 64 rows, one pass at 192 and
    256 and whenever the scratch is withheld -- the same exact integers every time"""
    x, w, bias32, _ = _int_operands(M, 5120, 20480)
    res = np.random.default_rng([M, 7]).integers(-2 ** 20, 2 ** 20 + 1, (M, 5120)).astype(F32)
    want = (np.rint(x.astype(np.float64) @ w.astype(np.float64).T) + bias32 + res).astype(F32)
    for fmt in ("bf16", "f16"):
        split, ran_split = gm._run(fmt, x, w, bias32, res, 2, have_ws=1)
        whole, ran_whole = gm._run(fmt, x, w, bias32, res, 2, have_ws=0)
        # the launcher splits while (64 x 64 tiles) x splits <= 1280: 80 tiles x 16 at 64 rows; 240 and 320 tiles run unsplit
        assert ("x16k" in ran_split) == (M == 64) and "x16k" not in ran_whole, (ran_split, ran_whole)
        gm._assert_bits(split, want, "split-K %s" % fmt)
        gm._assert_bits(whole, want, "unsplit %s" % fmt)


# ---- forward: one layer at the full width ------------------------------------------------------------------------------------------------
def _model(cfg, sd, precision):
    return common.model(models.ESM2_15B, cfg, sd, precision)


_WIDE = {}


def _wide_case():
    """one layer x 5120 x 40 heads of 128 with d_ffn 512: 131 M weights, built once per module"""
    if not _WIDE:
        cfg = weights.make_config(weights.ESM2_T48_CONFIG, n_layers=1, d_ffn=512)
        assert (cfg["d_model"], cfg["n_heads"]) == (5120, 40)
        sd = weights.synthetic_state_dict(cfg, seed=7, std=0.012, embed_std=0.1, ln_jitter=0.1)
        _WIDE["case"] = (cfg, sd, ref.Esm2Config.of(cfg))
    return _WIDE["case"]


# max |engine - reference| over the three cases (one chain of 27 tokens, 2 x 258, a right-padded batch), per unit of logit std (7.4 -
# 8.0).  First run on an MI355X that measured all three: fp32 2.9e-4 absolute (the bound is 1e-3 absolute); bf16 1.790e-1 / 1.498e-1 /
# 1.932e-1, worst 2.596e-2 of the logit std; fp16 1.773e-2 / 2.136e-2 / 1.968e-2, worst 2.893e-3.  The bounds are 2.5 x the worst,
# the ratio the 650M / 3B / 150M files keep.
FWD_MEASURED = {"bf16": 2.596e-2, "fp16": 2.893e-3}
FWD_TOL = {k: 2.5 * v for k, v in FWD_MEASURED.items()}


@pytest.mark.parametrize("precision", ["fp32", "bf16", "fp16"])
def test_esm2_15b_width_forward_against_the_reference(precision):
    cfg, sd, rcfg = _wide_case()
    lm = _model(cfg, sd, precision).model.to("cuda:0")
    rng = np.random.default_rng(5)
    worst, std = 0.0, 1.0
    cases = [_tokens(rng, 1, 27), _tokens(rng, 2, 258)]
    tok = np.full((3, 40), 1, dtype=np.int64)                                    # a right-padded batch
    lens = (40, 23, 9)
    for b, n in enumerate(lens):
        tok[b, :n] = _tokens(rng, 1, n, mask_every=5)[0]
    cases.append(tok)
    for tok in cases:
        want = ref.esm2_forward(sd, rcfg, tok)
        got = lm.forward_logits(tok)
        assert got.shape == want.shape
        std = float(want[tok != 1].std())
        err = float(np.abs(got - want)[tok != 1].max())
        worst = max(worst, err / (1.0 if precision == "fp32" else std))
        print("\n[ESM-2 1 x 5120, 40 heads of 128, %s] %s: max|engine - reference| = %.3e (logit std %.2f)" % (precision, tok.shape, err, std))
        if precision == "fp32":
            assert err < 1e-3, (tok.shape, err)
        else:
            assert err < FWD_TOL[precision] * std, (tok.shape, err, std)
    print("[ESM-2 1 x 5120, %s] worst %.3e %s" % (precision, worst, "absolute" if precision == "fp32" else "per unit of logit std"))


def test_esm2_hd128_forward_against_huggingface_logits():
    common.check_huggingface_logits("hd128")


# ---- a deeper small model: two heads of 128 ----------------------------------------------------------------------------------------------
def test_esm2_hd128_auto_precision_and_small_job_independence():
    """precision="auto" resolves and runs; a small job's logits do not depend on what the engine ran before (grow-only buffers)"""
    cfg, sd, rcfg = common.case("esm2_15b", n_layers=2)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lm = models.ESM2_15B(state_dict=sd, config=cfg).model.to("cuda:0")        # precision="auto"
    rng = np.random.default_rng(1)
    small, large = _tokens(rng, 4, 50), _tokens(rng, 3, 300)
    want = ref.esm2_forward(sd, rcfg, small)
    first = lm.forward_logits(small)
    assert np.abs(first - want).max() < 0.05 * max(1.0, float(want.std()))
    lm.forward_logits(large)
    assert np.array_equal(lm.forward_logits(small), first)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        other = models.ESM2_15B(state_dict=sd, config=cfg).model.to("cuda:0")
    other.forward_logits(large)
    assert np.array_equal(other.forward_logits(small), first)


# ---- activation buffers past 2^31 bytes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_config2_call_with_buffers_over_2_gib_equals_its_shards(precision):
    """256 chains x 258 tokens on two full-width layers (d_model 5120, d_ffn 20480): the first layer's fc1 output is 66048 x 20480 x
    2 B = 2.7 GB (strict: split rows of 8.1 GB, fp32 qkv of 4.1 GB) -- the first buffers of the project past 2^31 bytes, the size at which
    a 32-bit row offset in any kernel would show.  Each 32-chain shard keeps every buffer under 2^31 bytes (0.34 GB; strict 1.0 GB), the
    sizes every other test runs, and under set_job_items the kernels are row-invariant: the whole job must give the shards' tokens
    and sampled logits bit for bit.  (Two layers: the last one is pruned to the sampled rows and would never fill the buffer.)"""
    from protein_gibbs_sampler_amd import sharding
    cfg = weights.make_config(weights.ESM2_T48_CONFIG, n_layers=2)
    assert (cfg["d_model"], cfg["d_ffn"], cfg["n_heads"]) == (5120, 20480, 40)
    if "sd" not in _BIG:
        _BIG["sd"] = weights.synthetic_state_dict(cfg, seed=3, std=0.012, embed_std=0.1, ln_jitter=0.1)
    s = esm_sampler.ESM_sampler(_model(cfg, _BIG["sd"], precision), device="cuda:0")
    B, L, P, iters = 256, 256, 5, 1
    assert B * (L + 2) * cfg["d_ffn"] * 2 > 2 ** 31
    tok_all = common.shard_tokens(B, L, seed=4321)
    run = common.shard_runner(s, tok_all, P, iters)

    parts = [run(*sharding.shard_range(B, 8, g)) for g in range(8)]           # the shards first: the sizes that are known ground
    whole, whole_lg = run(0, B)
    assert np.isfinite(whole_lg).all() and (whole != tok_all).any()
    assert (np.concatenate([p[1] for p in parts], axis=1) == whole_lg).all(), "sampled-position logits differ from the shards'"
    assert (np.concatenate([p[0] for p in parts]) == whole).all()


_BIG = {}


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base, name", [("ESM1B_CONFIG", "ESM-1b"), ("MSA1B_CONFIG", "ESM-MSA-1b"), ("ESM1_T6_CONFIG", "ESM-1")])
def test_engine_refuses_heads_of_128_for_the_other_architectures(base, name):
    assert common.OTHER_ARCHS[name][0] == base
    common.check_other_architectures_refuse_the_width("esm2_15b", name)


@pytest.mark.parametrize("d_model, n_heads, words", [(6144, 48, "at most 40"), (5632, 44, "at most 40"), (2688, 21, "multiples of 512")])
def test_engine_refuses_models_wider_than_40_heads_of_128(d_model, n_heads, words):
    cfg = weights.make_config(weights.ESM2_T48_CONFIG, n_layers=1, d_model=d_model, n_heads=n_heads, d_ffn=256, max_positions=40)
    sd = weights.synthetic_state_dict(cfg, seed=1)
    with pytest.raises(Exception, match=words):
        _model(cfg, sd, "bf16").model.to("cuda:0")
