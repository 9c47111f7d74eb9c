"""Without a GPU: every pg_dbg_* entry of include/pgibbs.h that takes a device (1) refuses a null required pointer on the host with
PG_ERR_INVALID and its own message, (2) refuses a precision mode it does not know, and (3) given valid, tiny arguments answers
PG_ERR_NO_DEVICE where there is no GPU -- it neither computes on the host nor touches a device it was not given.  These are the
return codes and texts the entries' shared host plumbing (csrc/api_dbg.hip) must keep."""
import ctypes

import numpy as np
import pytest

from protein_gibbs_sampler_amd import _lib

F32 = np.float32
BF16, FP32, F16 = _lib.PG_PREC_BF16, _lib.PG_PREC_FP32, _lib.PG_PREC_F16


def _z(*shape, dt=F32):
    return np.zeros(shape, dt)


def _dbl(n):
    return (ctypes.c_double * n)()


def _i32(*v):
    return np.asarray(v, dtype=np.int32)


# name -> (valid tiny arguments, index of a required pointer, the message of the refusal when that pointer is null).
# M = 4, d = 64, B = 1, T = 16, H = 1; the two benches take the smallest shapes they accept.
def _cases():
    x, w, b, g = _z(4, 64), _z(64, 64), _z(64), _z(64)
    qkv, ctx = _z(16, 192), _z(16, 64)
    mqkv, mctx = _z(32, 192), _z(32, 64)
    h16 = _z(4, 64, dt=np.uint16)
    return {
        "pg_dbg_gemm": ([0, BF16, x, w, b, _z(4, 64), 4, 64, 64, 0], 2, "pg_dbg_gemm: bad argument"),
        "pg_dbg_gemm_v": ([0, BF16, x, w, b, _z(4, 64), 4, 64, 64, 0, -1, -1, 4, None, 0], 2, "pg_dbg_gemm: bad argument"),
        "pg_dbg_gemm_bench": ([0, 16, 64, 64, 0, 1, 1, _dbl(1)], 7, "pg_dbg_gemm_bench: bad argument"),
        "pg_dbg_rowln_bench": ([0, 256, 128, 1, _dbl(5), _dbl(1)], 4, "pg_dbg_rowln_bench: bad argument"),
        "pg_dbg_qkv_attention_bench": ([0, 1, 32, 1, 1, _dbl(3), _dbl(1)], 5, "pg_dbg_qkv_attention_bench: T must be 32, 64, 128 or 256"),
        "pg_dbg_layernorm": ([0, x, g, g, _z(4, 64), 4, 64, 1e-5], 1, "pg_dbg_layernorm: bad argument"),
        "pg_dbg_layernorm_operand": ([0, BF16, x, g, g, _z(4, 64), 4, 64, 1e-5], 2, "pg_dbg_layernorm_operand: bad argument"),
        "pg_dbg_attention": ([0, BF16, qkv, ctx, 1, 16, 1], 2, "pg_dbg_attention: bad argument"),
        "pg_dbg_attention_hd": ([0, BF16, qkv, ctx, 1, 16, 1, 64, None, -1], 3, "pg_dbg_attention: bad argument"),
        "pg_dbg_attention_kv": ([0, BF16, qkv, ctx, 1, 16, 1, 64, None, -1, None, None, None, 0], 3, "pg_dbg_attention: bad argument"),
        "pg_dbg_rope": ([0, BF16, qkv, 1, 16, 1], 2, "pg_dbg_rope: bad argument"),
        "pg_dbg_rope_hd": ([0, BF16, qkv, 1, 16, 1, 64], 2, "pg_dbg_rope: bad argument"),
        "pg_dbg_msa_attention": ([0, 0, mqkv, mctx, 1, 2, 16, 1, 0.125], 2, "pg_dbg_msa_attention: bad argument"),
        "pg_dbg_msa_attention_tok": ([0, 1, mqkv, mctx, 1, 2, 16, 1, 0.125, _z(2, 16, dt=np.int32), 1, None, 0], 3,
                                     "pg_dbg_msa_attention: bad argument"),
        "pg_dbg_embed": ([0, BF16, _z(1, 16, dt=np.int32), 1, 16, _z(33, 64), 33, 64, _z(40, 64), 40, None, 0, None, None, None, None,
                          1, 32, 1, 1e-5, 1.0, _z(16, 64), None], 2, "pg_dbg_embed: bad argument"),
        "pg_dbg_layernorm_rows": ([0, BF16, x, g, g, h16, 4, 4, 64, 1e-5, 0, 0, 0, None], 2, "pg_dbg_layernorm_rows: bad argument"),
        "pg_dbg_gather_ln": ([0, BF16, _z(16, 64), 16, _i32(0, 1, 2, 3), None, 0, 1, 4, g, g, h16, 4, 4, 64, 1e-5, 0], 2,
                             "pg_dbg_gather_ln: bad argument"),
        "pg_dbg_gather_rows": ([0, _z(16, 16, dt=np.uint8), 16, _z(4, 16, dt=np.uint8), 4, _i32(0, 1, 2, 3), 0, 0, None, 0, 1, 4, 4, 16], 1,
                               "pg_dbg_gather_rows: bad argument"),
        "pg_dbg_split_rows": ([0, _z(4, 64), _z(4, 192, dt=np.uint16), 4, 4, 64, 1.0, 0, None], 1, "pg_dbg_split_rows: bad argument"),
        "pg_dbg_lm_tail": ([0, _z(4, 64), None, None, _z(33, 64), _z(33), _z(4, 33), 4, 64, 33, 1e-5, None], 1,
                           "pg_dbg_lm_tail: bad argument"),
    }


NAMES = sorted(_cases())


def _call(name, args):
    rc = getattr(_lib.lib(), name)(*[_lib.ptr(a) if isinstance(a, np.ndarray) else a for a in args])
    msg = _lib.lib().pg_last_error()
    print("%s -> rc %d, %r" % (name, rc, msg.decode() if msg else ""))
    return rc, msg.decode() if msg else ""


def _with(args, index, value):
    return args[:index] + [value] + args[index + 1:]


def test_every_entry_with_a_device_argument_is_covered():
    takes_device = {n for n, _, _ in _lib.SIGNATURES if n.startswith("pg_dbg_")} - {"pg_dbg_gemm_plan", "pg_dbg_attention_plan",
                                                                                  "pg_dbg_gather_tokens_host", "pg_dbg_gather_plan"}
    assert takes_device == set(NAMES)


@pytest.mark.parametrize("name", NAMES)
def test_null_required_pointer_is_refused_on_the_host(name):
    args, index, message = _cases()[name]
    assert _call(name, _with(args, index, None)) == (_lib.PG_ERR_INVALID, message)


@pytest.mark.parametrize("name", NAMES)
def test_valid_arguments_without_a_gpu_are_no_device(name):
    if _lib.lib().pg_device_count() > 0:
        pytest.skip("GPU present")
    args, _, _ = _cases()[name]
    assert _call(name, args) == (_lib.PG_ERR_NO_DEVICE, "no HIP device visible")


@pytest.mark.parametrize("name", ["pg_dbg_gemm", "pg_dbg_gemm_v", "pg_dbg_attention_kv", "pg_dbg_layernorm_operand", "pg_dbg_rope_hd"])
def test_unknown_precision_mode(name):
    args, _, _ = _cases()[name]
    assert _call(name, _with(args, 1, 7)) == (_lib.PG_ERR_INVALID, "unknown precision mode")


def test_unknown_precision_mode_of_the_attention_plan():
    buf = ctypes.create_string_buffer(256)
    assert _call("pg_dbg_attention_plan", [0, 7, 1, 16, 1, 1, 64, 0, 0, 1, 0, 256, buf, 256]) == (_lib.PG_ERR_INVALID, "unknown precision mode")


@pytest.mark.parametrize("name", ["pg_dbg_embed", "pg_dbg_layernorm_rows", "pg_dbg_gather_ln"])
def test_row_entries_take_16_bit_modes_only(name):
    args, _, _ = _cases()[name]
    assert _call(name, _with(args, 1, FP32)) == (_lib.PG_ERR_INVALID, name + ": precision must be PG_PREC_BF16 or PG_PREC_F16")


# Refusals that are argument checks like the rest and precede the device lookup like the rest: with or without a GPU the
# answer is the refusal, not PG_ERR_NO_DEVICE.
LATE = {
    "gemm_fused_gelu_split_needs_N_256": ("pg_dbg_gemm", {1: FP32, 9: 5}, _lib.PG_ERR_INVALID,
                                          "pg_dbg_gemm: the fused GELU-and-split epilogue needs N a multiple of 256"),
    "gemm_strict_epilogues": ("pg_dbg_gemm", {1: FP32, 9: 1}, _lib.PG_ERR_UNSUPPORTED,
                              "strict mode: plain (0), residual (2) and fused GELU-split (5) epilogues only"),
    "gemm_v_fused_gelu_split_needs_N_256": ("pg_dbg_gemm_v", {1: FP32, 9: 5}, _lib.PG_ERR_INVALID,
                                            "pg_dbg_gemm: the fused GELU-and-split epilogue needs N a multiple of 256"),
    "gemm_v_unknown_variant": ("pg_dbg_gemm_v", {10: 3}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_v: variant must be -1, 1, 2, 6, 7, 8, 20 or 80"),
    "gemm_v_ablation_pp": ("pg_dbg_gemm_v", {10: 21}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_v: variant must be -1, 1, 2, 6, 7, 8, 20 or 80"),
    "gemm_v_ablation_pp_60": ("pg_dbg_gemm_v", {10: 60}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_v: variant must be -1, 1, 2, 6, 7, 8, 20 or 80"),
    "gemm_v_ablation_w16": ("pg_dbg_gemm_v", {10: 81}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_v: variant must be -1, 1, 2, 6, 7, 8, 20 or 80"),
    "gemm_v_variant_90": ("pg_dbg_gemm_v", {10: 90}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_v: variant must be -1, 1, 2, 6, 7, 8, 20 or 80"),
    "gemm_v_variant_below_minus_1": ("pg_dbg_gemm_v", {10: -2}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_v: variant must be -1, 1, 2, 6, 7, 8, 20 or 80"),
    "gemm_v_strict_has_no_variant": ("pg_dbg_gemm_v", {1: FP32, 10: 2}, _lib.PG_ERR_UNSUPPORTED,
                                     "strict mode: launch_gemm_split3 has no variant (-1 only)"),
    "gemm_v_have_ws": ("pg_dbg_gemm_v", {11: 2}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_v: have_ws is -1, 0 or 1 and m_live 0 ... M"),
    "gemm_v_m_live": ("pg_dbg_gemm_v", {12: 5}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_v: have_ws is -1, 0 or 1 and m_live 0 ... M"),
    "gemm_v_plan_without_room": ("pg_dbg_gemm_v", {13: ctypes.create_string_buffer(8), 14: 0}, _lib.PG_ERR_INVALID, "pg_dbg_gemm: bad argument"),
    "split_rows_K_not_32": ("pg_dbg_split_rows", {5: 48}, _lib.PG_ERR_INVALID, "pg_dbg_split_rows: K must be a multiple of 32"),
    "split_rows_no_rows": ("pg_dbg_split_rows", {4: 0}, _lib.PG_ERR_INVALID, "pg_dbg_split_rows: bad argument"),
    "split_rows_unknown_form": ("pg_dbg_split_rows", {7: 4}, _lib.PG_ERR_INVALID, "pg_dbg_split_rows: form is weight (1) + through GELU (2)"),
    "split_rows_gelu_on_weight": ("pg_dbg_split_rows", {7: 3, 8: _z(4, 64)}, _lib.PG_ERR_INVALID, "pg_dbg_split_rows: GELU on a weight operand"),
    "split_rows_gelu_scale": ("pg_dbg_split_rows", {7: 2, 6: 0.37, 8: _z(4, 64)}, _lib.PG_ERR_INVALID, "pg_dbg_split_rows: the GELU form takes scale 1"),
    "gemm_bench_variant_90": ("pg_dbg_gemm_bench", {5: 90}, _lib.PG_ERR_INVALID, "variant 90: K = 3 x depth, fp32 epilogues"),
}


@pytest.mark.parametrize("case", sorted(LATE))
def test_shape_refusals_precede_the_device_lookup(case):
    name, changes, code, message = LATE[case]
    args, _, _ = _cases()[name]
    for index, value in changes.items():
        args = _with(args, index, value)
    assert _call(name, args) == (code, message)
