"""Without a GPU: (1) the float64 attention reference that tests/test_gpu_attention_kernels.py trusts (tests/_attention_reference.py)
reproduces the attention inside the three oracles -- ESM-1b's with <pad>, ESM-1's with the bias key, the MSA Transformer's tied rows and
padded columns; (2) a numpy model of the 16-bit kernels' arithmetic stays inside the derived bound for every input family and every
kind of shape the GPU test runs, so the reference and the bound are consistent with each other before any kernel is asked; (3) three
wrong models -- one dead key, a <pad> flag shifted by one key, a bias key that reads bias_k as its value -- leave the bound on the
negative family at every rung edge; (4) the attention debug entries refuse bad arguments on the host, before they look for a device."""
import ctypes

import numpy as np
import pytest

import _attention_reference as ar
from oracle import esm1_forward, esm_forward, msa_forward
from protein_gibbs_sampler_amd import _lib

F32 = np.float32


def _proj(w, p, h):
    return [esm_forward.linear(h, w[p + n + "_proj.weight"], w[p + n + "_proj.bias"]) for n in "qkv"]


def _close(got, want):
    return np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max())


# ---- (1) the reference against the oracles ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,pad", [(2, 7, False), (3, 27, True), (2, 65, True)])
def test_reference_reproduces_the_esm1b_attention(B, T, pad):
    cfg = esm_forward.EsmConfig(d_model=128, n_layers=1, n_heads=2, d_ffn=256, max_pos=100)
    w = esm_forward.synthetic_esm_weights(cfg, seed=3, std=0.08, embed_std=0.3, ln_jitter=0.1)
    rng = np.random.default_rng(T)
    h = rng.standard_normal((B, T, 128)).astype(F32)
    tok = np.full((B, T), 5)
    if pad:
        tok[0, T - 3:] = tok[1, 1:] = ar.PAD
    p = "layers.0.self_attn."
    q, k, v = _proj(w, p, h)
    res = ar.chain_attention(np.concatenate([q * F32(64 ** -0.5), k, v], -1), 2, 64, tok if pad else None)
    want = esm_forward.mha(w, p, cfg, h, tok == ar.PAD)
    assert _close(esm_forward.linear(res.ref.astype(F32), w[p + "out_proj.weight"], w[p + "out_proj.bias"]), want)
    assert (res.pabs >= np.abs(res.ref) - 1e-12).all()


@pytest.mark.parametrize("B,T,pad", [(2, 7, False), (3, 40, True)])
def test_reference_reproduces_the_esm1_attention_with_its_bias_key(B, T, pad):
    cfg = esm1_forward.Esm1Config(d_model=128, n_layers=1, n_heads=2, d_ffn=256, max_pos=100)
    w = esm1_forward.synthetic_esm1_weights(cfg, seed=4, std=0.08, embed_std=0.3, ln_jitter=0.1)
    rng = np.random.default_rng(T)
    h = rng.standard_normal((B, T, 128)).astype(F32)
    tok = np.full((B, T), 5)
    if pad:
        tok[0, T - 3:] = tok[1, 1:] = ar.PAD
    p = "layers.0.self_attn."
    q, k, v = _proj(w, p, h)
    res = ar.chain_attention(np.concatenate([q * F32(64 ** -0.5), k, v], -1), 2, 64, tok if pad else None,
                             bias_k=w[p + "bias_k"].reshape(2, 64), bias_v=w[p + "bias_v"].reshape(2, 64))
    want = esm1_forward.mha_bias_kv(w, p, cfg, h, tok == ar.PAD)
    assert res.n_keys == T + 1
    assert _close(esm_forward.linear(res.ref.astype(F32), w[p + "out_proj.weight"], w[p + "out_proj.bias"]), want)


@pytest.mark.parametrize("B,R,C,pad", [(2, 3, 20, False), (2, 5, 33, True)])
def test_reference_reproduces_the_msa_row_and_column_attention(B, R, C, pad):
    cfg = msa_forward.MsaConfig(d_model=128, n_layers=1, n_heads=2, d_ffn=256, max_pos=100, max_rows=16)
    w = msa_forward.synthetic_msa_weights(cfg, seed=5, std=0.08, embed_std=0.3, ln_jitter=0.1)
    rng = np.random.default_rng(C)
    h = rng.standard_normal((B, R, C, 128)).astype(F32)
    tok = np.full((B, R, C), 5)
    if pad:
        tok[0, :, C - 4:] = ar.PAD           # a shorter alignment: <pad> key columns in row 0
        tok[1, R - 2:] = ar.PAD              # a shallower one: <pad> rows
        tok[1, :, 3] = ar.PAD                # and a column that is all <pad>
    mask = (tok == ar.PAD) if pad else None
    for name, oracle in (("row_self_attention.layer.", msa_forward.row_attention), ("column_self_attention.layer.", msa_forward.column_attention)):
        p = "layers.0." + name
        q, k, v = _proj(w, p, h)
        if oracle is msa_forward.row_attention:
            res = ar.tied_row_attention(np.concatenate([q, k, v], -1), 2, F32(64 ** -0.5) / F32(np.sqrt(R)), tok if pad else None)
        else:
            res = ar.column_attention(np.concatenate([q * F32(64 ** -0.5), k, v], -1), 2, tok if pad else None)
        assert np.isfinite(res.ref).all()
        got = esm_forward.linear(res.ref.astype(F32), w[p + "out_proj.weight"], w[p + "out_proj.bias"])
        assert _close(got, oracle(w, p, cfg, h, mask)), name


# ---- (2) the kernel model stays inside the bound ------------------------------------------------------------------------------------------
def _case(family, fmt, T, hd, pad, bias, seed=0):
    """the rounded inputs of one chain case as the GPU test builds them, split per head, and its reference"""
    H = 2 if hd == 64 else 1
    tok = ar.pad_tokens(T) if pad else None
    n_seq = 3 if pad else 2
    peak = ar.last_real_key(tok) if pad and family == "late_last" else None
    qkv = ar.family_qkv(family, seed, n_seq, T, H, hd, peak=peak)
    if pad:
        ar.poison_pad(qkv, tok, H, hd)
    qkv = ar.round_to(fmt, qkv)
    bk, bv = (ar.round_to(fmt, x) for x in ar.family_bias(family, seed, H, hd)) if bias else (None, None)
    res = ar.chain_attention(qkv, H, hd, tok, bias_k=bk, bias_v=bv)
    d = H * hd
    q, k, v = (qkv[..., i * d:(i + 1) * d].reshape(n_seq, T, H, hd).transpose(0, 2, 1, 3) for i in range(3))
    return q, k, v, tok, bk, bv, res, H, d


def _model_ctx(q, k, v, fmt, tok, bk, bv, **kw):
    N, H, T, hd = q.shape
    return ar.kernel_model(q, k, v, fmt, None if tok is None else tok == ar.PAD, -3.0e38, bk, bv, **kw).transpose(0, 2, 1, 3).reshape(N, T, H * hd)


def _fraction(ctx, res, fmt, tok):
    b = ar.bound(res, fmt)
    live = np.ones(ctx.shape[:2], bool) if tok is None else tok != ar.PAD      # rows whose query is <pad> are not compared
    err = np.abs(ctx - res.ref)[live]
    return float((err / np.maximum(b[live], 1e-300)).max()), bool((err <= b[live]).all())


MODEL_LENGTHS = [1, 17, 31, 32, 258, 513, 576, 577, 865]


@pytest.mark.parametrize("fmt", ["bf16", "f16"])
@pytest.mark.parametrize("family", ar.FAMILIES)
def test_kernel_model_stays_inside_the_bound(family, fmt):
    worst = 0.0
    for hd, pad, bias in [(64, False, False), (64, True, False), (64, False, True), (64, True, True), (32, False, False), (32, True, False)]:
        for T in MODEL_LENGTHS:
            q, k, v, tok, bk, bv, res, H, d = _case(family, fmt, T, hd, pad, bias)
            frac, ok = _fraction(_model_ctx(q, k, v, fmt, tok, bk, bv), res, fmt, tok)
            assert ok, (family, fmt, hd, pad, bias, T, frac)
            worst = max(worst, frac)
    print("\nkernel model, %-9s %-4s: at most %.2f of the bound" % (family, fmt, worst))
    assert worst > 0 or family == "unity"


def test_unity_is_exact_in_the_model():
    for fmt in ("bf16", "f16"):
        for T in (31, 258, 577):
            q, k, v, tok, bk, bv, res, H, d = _case("unity", fmt, T, 64, True, True)
            ctx = _model_ctx(q, k, v, fmt, tok, bk, bv)
            assert (ctx[tok != ar.PAD] == 1.0).all() and np.abs(res.ref[tok != ar.PAD] - 1.0).max() < 1e-12


# ---- (3) wrong models leave the bound on the negative family, at every rung edge ------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16", "f16"])
def test_mutated_models_break_the_bound_at_every_rung_edge(fmt):
    for T in ar.rung_edge_lengths():
        # one dead key: zero-filled, unmasked, score 0
        for bias in (False, True):
            q, k, v, tok, bk, bv, res, H, d = _case("negative", fmt, T, 64, False, bias)
            assert _fraction(_model_ctx(q, k, v, fmt, tok, bk, bv), res, fmt, tok)[1]
            assert not _fraction(_model_ctx(q, k, v, fmt, tok, bk, bv, dead_key=True), res, fmt, tok)[1], ("dead key", T, bias)
        # the <pad> flags shifted by one key: the first <pad> key of every run is let through
        q, k, v, tok, bk, bv, res, H, d = _case("negative", fmt, T, 64, True, False)
        if (tok == ar.PAD).any():
            late = np.zeros_like(tok)
            late[:, 1:] = tok[:, :-1]
            late[late != ar.PAD] = 5
            live = tok != ar.PAD
            err = np.abs(_model_ctx(q, k, v, fmt, late, bk, bv) - res.ref)
            assert not (err <= ar.bound(res, fmt))[live].all(), ("pad flag one key late", T)
        # the bias key's value read from bias_k
        q, k, v, tok, bk, bv, res, H, d = _case("negative", fmt, T, 64, False, True)
        assert not _fraction(_model_ctx(q, k, v, fmt, tok, bk, bk), res, fmt, tok)[1], ("bias_v from bias_k", T)


def test_rung_edges_cover_both_ladders():
    edges = ar.rung_edge_lengths()
    assert {ar.expected_rung(T, False) for T in edges} == set(range(2, 37, 2)) | {0}
    assert {ar.expected_rung(T, True) for T in edges} == {2, 4, 8, 12, 18, 24, 30, 36, 0}
    for r in (2, 4, 8, 12, 18, 24, 30):      # the bias key alone in the next rung's block
        assert 16 * r in edges and ar.expected_rung(16 * r, True) > r
    assert {288, 576, 864} <= set(edges)
    for T in edges:                          # the reference's restatement of the ladder is the library's
        for bias in (0, 1):
            buf = ctypes.create_string_buffer(256)
            _lib.check(_lib.lib().pg_dbg_attention_plan(0, _lib.PG_PREC_BF16, 2, T, 0, 2, 64, 0, bias, 1, 0, 256, buf, 256))
            kb = ar.expected_rung(T, bool(bias))
            assert buf.value.decode().startswith("whole kb%d hd64" % kb if kb else "long t288 hd64"), (T, bias, buf.value)


# ---- (4) refusals, without a device ----------------------------------------------------------------------------------------------------------
def _refused(rc, code, text):
    msg = (_lib.lib().pg_last_error() or b"").decode()
    assert rc == code and text in msg, (rc, msg)


def test_attention_debug_entries_refuse_bad_arguments_on_the_host():
    L = _lib.lib()
    B, T, H = 1, 4, 1
    qkv = np.zeros((B, T, 3 * 64), F32)
    ctx = np.zeros((B, T, 64), F32)
    bias = np.zeros((H, 64), F32)
    tok = np.full((B, T), 5, np.int32)
    plan = ctypes.create_string_buffer(64)
    P, I = _lib.ptr, _lib.PG_ERR_INVALID

    def kv(prec=_lib.PG_PREC_BF16, q=P(qkv), c=P(ctx), B=B, T=T, H=H, hd=64, bk=None, bv=None, plan=plan, nplan=64):
        return L.pg_dbg_attention_kv(0, prec, q, c, B, T, H, hd, P(tok), ar.PAD, bk, bv, plan, nplan)

    _refused(kv(prec=7), I, "unknown precision mode")
    _refused(kv(q=None), I, "bad argument")
    _refused(kv(c=None), I, "bad argument")
    _refused(kv(T=0), I, "bad argument")
    _refused(kv(H=0), I, "bad argument")
    _refused(kv(nplan=0), I, "bad argument")
    _refused(kv(hd=48), I, "head_dim must be 64 or 32")
    _refused(kv(bk=P(bias)), I, "bias_k and bias_v come together")
    _refused(kv(bv=P(bias)), I, "bias_k and bias_v come together")
    for prec in (_lib.PG_PREC_BF16, _lib.PG_PREC_F16, _lib.PG_PREC_FP32):
        _refused(kv(prec=prec, hd=32, bk=P(bias), bv=P(bias)), I, "the bias_k / bias_v key (ESM-1) is built for heads of 64 only")
    _refused(kv(B=1 << 20, T=1 << 10, H=4), I, "more than 2^31 - 1 qkv values")
    assert plan.value == b""

    msa = np.zeros((1, 2, 4, 3 * 64), F32)
    out = np.zeros((1, 2, 4, 64), F32)
    mtok = np.full((1, 2, 4), 5, np.int32)

    def mt(which=0, q=P(msa), c=P(out), B=1, R=2, C=4, H=1, tok=P(mtok), nplan=64):
        return L.pg_dbg_msa_attention_tok(0, which, q, c, B, R, C, H, 0.1, tok, ar.PAD, plan, nplan)

    _refused(mt(q=None), I, "bad argument")
    _refused(mt(c=None), I, "bad argument")
    _refused(mt(C=0), I, "bad argument")
    _refused(mt(nplan=0), I, "bad argument")
    _refused(mt(which=6), I, "which must be 0 ... 5")
    _refused(mt(which=-1), I, "which must be 0 ... 5")
    _refused(mt(B=1 << 12, R=1 << 10, C=1 << 10), I, "more than 2^31 - 1 qkv values")
    _refused(mt(which=4), _lib.PG_ERR_UNSUPPORTED, "fp16 precision mode: alignments wider than 576 columns take the split-bf16 row attention")
    assert plan.value == b""
