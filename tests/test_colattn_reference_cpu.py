"""Without a GPU: the operands, reference and bounds of tests/_colattn_reference.py are what its docstring says for every shape and
both formats of the GPU list, and pg_dbg_colattn refuses every bad argument on the host with its own text before it looks for a device."""
import numpy as np
import pytest

import _attention_reference as ar
import _colattn_reference as cr
from protein_gibbs_sampler_amd import _lib

F32 = np.float32
FMTS = ("bf16", "f16")
CASES = [(fmt, shape) for fmt in FMTS for shape in cr.SHAPES]
_QKV = {}


def _qkv(family, fmt, shape):
    """the exact 16-bit qkv of a case, computed once (exact_qkv makes the construction's assertions) and left unchanged"""
    key = (family, fmt, shape)
    if key not in _QKV:
        x, w, bias, g = cr.operands(family, shape)
        _QKV[key] = cr.exact_qkv(fmt, x, w, bias, g)
        _QKV[key].setflags(write=False)
    return _QKV[key]


def test_the_shape_list_is_the_one_the_kernel_needs():
    """every depth the kernel is instantiated for, 1, 2, 3 and 12 K-steps, a launch below one tile, ragged last tiles and groups"""
    assert {s[1] for s in cr.SHAPES} == {32, 64, 128, 256}
    assert {1, 2, 3, 12} <= {s[3] for s in cr.SHAPES}
    rows = [s[0] * s[1] * s[2] for s in cr.SHAPES]
    assert min(rows) < 256 and any(r % 256 for r in rows) and any(r % 256 == 0 for r in rows)
    assert {(r + 255) // 256 for r in rows} >= {1, 2, 3, 6, 7}
    assert max(s[0] * s[1] * s[2] for s in cr.SHAPES) <= 1600 and max(s[3] for s in cr.SHAPES) * 64 <= 768


@pytest.mark.parametrize("fmt,shape", CASES)
def test_projection_is_exact_in_every_family(fmt, shape):
    B, R, C, H = shape
    d = H * 64
    for family in cr.FAMILIES:
        x, w, bias, g = cr.operands(family, shape)
        assert x.shape == (B, R, C, d) and w.shape == (3 * d, d) and bias.shape == (3 * d,)
        qkv = _qkv(family, fmt, shape)                      # asserts representability, the grid and the 2^24 g ceiling
        # fp32 accumulation in two other orders gives the same bits: K-steps of 64 front to back, and back to front
        steps = [np.matmul(x[..., k:k + 64], w[:, k:k + 64].T, dtype=F32) for k in range(0, d, 64)]
        fwd = sum(steps[1:], steps[0]) + bias
        bwd = sum(steps[-2::-1], steps[-1]) + bias
        assert fwd.dtype == F32 and (ar.round_to(fmt, fwd) == qkv).all() and (ar.round_to(fmt, bwd) == qkv).all()
    q, k, v = (_qkv("integer", fmt, shape)[..., i * d:(i + 1) * d] for i in range(3))
    assert 0.15 < q.std() < 0.35 and 0.6 < k.std() < 1.1 and 0.6 < v.std() < 1.1, (q.std(), k.std(), v.std())


@pytest.mark.parametrize("shape", cr.SHAPES)
def test_integer_softmax_is_neither_flat_nor_one_hot(shape):
    B, R, C, H = shape
    qkv = _qkv("integer", "bf16", shape)
    q, k, _ = (x.transpose(0, 2, 3, 1, 4) for x in ar._heads(qkv, H, 64))       # [B][C][H][R][64]
    p = ar._softmax(q @ k.transpose(0, 1, 2, 4, 3))
    top = float(np.median(p.max(-1)))
    assert 2.0 / R < top < 0.5, top


@pytest.mark.parametrize("shape", cr.SHAPES)
def test_reference_equals_an_independent_einsum(shape):
    B, R, C, H = shape
    qkv = np.asarray(_qkv("integer", "f16", shape), np.float64)
    d = H * 64
    q, k, v = (qkv[..., i * d:(i + 1) * d].reshape(B, R, C, H, 64) for i in range(3))
    a = np.einsum("brchd,bjchd->bchrj", q, k)
    p = np.exp(a - a.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    want = np.einsum("bchrj,bjchd->brchd", p, v).reshape(B, R, C, d)
    ref, bound = cr.expected("integer", "f16", shape, qkv)
    assert np.abs(ref - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert bound.shape == ref.shape and (bound > 0).all()


def test_column_major_permutation_round_trips():
    for B, R, C in ((1, 32, 1), (2, 64, 3), (3, 32, 8)):
        tok = np.arange(B * R * C * 2, dtype=F32).reshape(B, R, C, 2)
        cm = cr.to_colmajor(tok)
        for b in range(B):
            for r in range(0, R, 7):
                for c in range(C):
                    assert (cm[(b * C + c) * R + r] == tok[b, r, c]).all()
        assert (cr.from_colmajor(cm, B, R, C) == tok).all()
        assert sorted(cm[:, 0].tolist()) == tok[..., 0].reshape(-1).tolist()


@pytest.mark.parametrize("fmt,shape", CASES)
def test_the_kernel_model_meets_every_family(fmt, shape):
    """ar.kernel_model, the numpy model of the 16-bit kernels' six steps: integer under the general bound, uniform under its own,
    rowcode exact -- the expectations are ones a correct kernel of that arithmetic meets"""
    for family in cr.FAMILIES:
        qkv = _qkv(family, fmt, shape)
        ref, bound = cr.expected(family, fmt, shape, qkv)
        got = cr.kernel_model_context(fmt, shape, qkv)
        err = np.abs(got - ref)
        assert (err <= bound).all(), (family, float((err / np.maximum(bound, 1e-300)).max()))
        if family == "rowcode":
            assert (got == ref).all() and np.abs(ref).max() <= 63 and len(np.unique(ref)) > 60


def test_uniform_bound_is_far_below_the_general_one_and_a_wrong_lane_misses_it():
    shape = (1, 32, 9, 2)
    for fmt in FMTS:
        qkv = _qkv("uniform", fmt, shape)
        ref, bound = cr.expected("uniform", fmt, shape, qkv)
        general = ar.bound(ar.column_attention(qkv, shape[3]), fmt)
        assert (bound <= general).all() and np.median(bound / general) < 0.75
        # the neighbouring feature, head or column in the place of the right one
        for wrong in (np.roll(ref, 1, -1), np.roll(ref, 64, -1), np.roll(ref, 1, 2)):
            assert (np.abs(wrong - ref) > bound).mean() > 0.9


@pytest.mark.parametrize("shape", [(1, 32, 9, 2), (3, 32, 8, 3), (1, 32, 13, 12)])
def test_a_dropped_k_step_moves_the_context_past_the_bound(shape):
    """what a main loop that loses one 64-wide K-step would give: nearly every context element leaves the bound"""
    d = shape[3] * 64
    x, w, bias, g = cr.operands("integer", shape)
    ref, bound = cr.expected("integer", "bf16", shape, _qkv("integer", "bf16", shape))
    for k0 in (0, d - 64):
        w2 = w.copy()
        w2[:, k0:k0 + 64] = 0
        got = cr.kernel_model_context("bf16", shape, cr.exact_qkv("bf16", x, w2, bias, g))
        assert (np.abs(got - ref) > bound).mean() > 0.9


# ---- the entry's host side -----------------------------------------------------------------------------------------------------
def _args(**kw):
    """valid tiny arguments of pg_dbg_colattn as a dict in argument order: (1, 32, 1, 1), 32 context rows"""
    a = dict(device=0, precision=_lib.PG_PREC_BF16, x=np.zeros((32, 64), F32), w=np.zeros((192, 64), F32), bias=np.zeros(192, F32),
             ctx=np.zeros((32, 64), F32), ctx_rows=32, B=1, R=32, C=1, H=1, fused=1, pad_fill=0.0, plan=None, plan_bytes=0)
    a.update(kw)
    return a


def _call(**kw):
    vals = [_lib.ptr(v) if isinstance(v, np.ndarray) else v for v in _args(**kw).values()]
    rc = _lib.lib().pg_dbg_colattn(*vals)
    msg = _lib.lib().pg_last_error()
    return rc, msg.decode() if msg else ""


REFUSALS = {
    "null_x": (dict(x=None), "pg_dbg_colattn: null argument"),
    "null_w": (dict(w=None), "pg_dbg_colattn: null argument"),
    "null_bias": (dict(bias=None), "pg_dbg_colattn: null argument"),
    "null_ctx": (dict(ctx=None), "pg_dbg_colattn: null argument"),
    "B_0": (dict(B=0), "pg_dbg_colattn: B, C and H must be at least 1"),
    "C_0": (dict(C=0), "pg_dbg_colattn: B, C and H must be at least 1"),
    "H_negative": (dict(H=-1), "pg_dbg_colattn: B, C and H must be at least 1"),
    "R_16": (dict(R=16), "pg_dbg_colattn: R must be 32, 64, 128 or 256"),
    "R_48": (dict(R=48), "pg_dbg_colattn: R must be 32, 64, 128 or 256"),
    "R_512": (dict(R=512, ctx_rows=512), "pg_dbg_colattn: R must be 32, 64, 128 or 256"),
    "fused_2": (dict(fused=2), "pg_dbg_colattn: fused is 0 or 1, and a plan buffer has room"),
    "plan_without_room": (dict(plan=b"12345678", plan_bytes=0), "pg_dbg_colattn: fused is 0 or 1, and a plan buffer has room"),
    "pad_fill_inf": (dict(pad_fill=float("inf")), "pg_dbg_colattn: pad_fill must be finite"),
    "pad_fill_nan": (dict(pad_fill=float("nan")), "pg_dbg_colattn: pad_fill must be finite"),
    "ctx_rows_31": (dict(ctx_rows=31), "pg_dbg_colattn: ctx_rows must be at least B*R*C"),
    "ctx_rows_one_short_of_two_columns": (dict(C=2, ctx_rows=63), "pg_dbg_colattn: ctx_rows must be at least B*R*C"),
    "too_many_operand_values": (dict(B=1 << 20, ctx_rows=1 << 25), "pg_dbg_colattn: more than 2^31 - 1 values"),
    "too_many_context_values": (dict(ctx_rows=1 << 26), "pg_dbg_colattn: more than 2^31 - 1 values"),
    "too_many_rows_for_an_int": (dict(B=1 << 28, C=1 << 28, ctx_rows=1 << 62), "pg_dbg_colattn: more than 2^31 - 1 values"),
    "fp32": (dict(precision=_lib.PG_PREC_FP32), "pg_dbg_colattn: precision must be PG_PREC_BF16 or PG_PREC_F16"),
    "unknown_precision": (dict(precision=7), "pg_dbg_colattn: precision must be PG_PREC_BF16 or PG_PREC_F16"),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_entry_refusals_precede_the_device_lookup(case):
    changes, message = REFUSALS[case]
    assert _call(**changes) == (_lib.PG_ERR_INVALID, message)


def test_each_kind_of_refusal_has_its_own_text():
    assert len({m for _, m in REFUSALS.values()}) == 8


@pytest.mark.parametrize("kw", [dict(), dict(fused=0), dict(precision=_lib.PG_PREC_F16), dict(ctx_rows=332, ctx=np.zeros((332, 64), F32), pad_fill=-240.0)])
def test_valid_tiny_arguments_without_a_gpu_are_no_device(kw):
    if _lib.lib().pg_device_count() > 0:
        pytest.skip("GPU present")
    assert _call(**kw) == (_lib.PG_ERR_NO_DEVICE, "no HIP device visible")
