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


def _params(n_valid=20, first_valid=4):
    p = _lib.make_sample_params(False, 32, 0, 0, None, list(range(first_valid, first_valid + 20)), 0)
    p.n_valid = n_valid
    return ctypes.byref(p)


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
        "pg_dbg_gemm_ln": ([0, BF16, _z(4, 256), None, _z(256), _z(256), 1e-5, _z(32, 256), _z(32), _z(16, 32), 16, 4, 32, 256, 0, 0, None, 0], 2,
                           "pg_dbg_gemm_ln: bad argument"),
        "pg_dbg_gemm_bench": ([0, 16, 64, 64, 0, 1, 1, _dbl(1)], 7, "pg_dbg_gemm_bench: bad argument"),
        "pg_dbg_qkv_attention_bench": ([0, 1, 32, 1, 1, _dbl(3), _dbl(1)], 5, "pg_dbg_qkv_attention_bench: T must be 32, 64, 128 or 256"),
        # B = 1, R = 32, C = 1, H = 1, the fused launch, 32 context rows (tests/test_colattn_reference_cpu.py has every refusal)
        "pg_dbg_colattn": ([0, BF16, _z(32, 64), _z(192, 64), _z(192), _z(32, 64), 32, 1, 32, 1, 1, 1, 0.0, None, 0], 3,
                           "pg_dbg_colattn: null argument"),
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
        # 2 token rows of 8, compact logits [1][2 * 2][33], one index table [1][2][2], one step, no mask step
        "pg_dbg_sample": ([0, _z(2, 8, dt=np.int32), 2, 8, _z(1, 4, 33), 33, 1, _i32(1, 2, 3, -1), 1, None, 2, 2, _params(), 0, 1, 0, -1, 0,
                           _z(1, 2, 2, dt=np.int32), None, None], 4, "pg_dbg_sample: bad argument"),
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


@pytest.mark.parametrize("name", ["pg_dbg_embed", "pg_dbg_layernorm_rows", "pg_dbg_gather_ln", "pg_dbg_gemm_ln"])
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
    "gemm_ln_gamma": ("pg_dbg_gemm_ln", {4: None}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: bad argument"),
    "gemm_ln_beta": ("pg_dbg_gemm_ln", {5: None}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: bad argument"),
    "gemm_ln_w": ("pg_dbg_gemm_ln", {7: None}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: bad argument"),
    "gemm_ln_bias": ("pg_dbg_gemm_ln", {8: None}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: bad argument"),
    "gemm_ln_out": ("pg_dbg_gemm_ln", {9: None}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: bad argument"),
    "gemm_ln_plan_without_room": ("pg_dbg_gemm_ln", {16: ctypes.create_string_buffer(8), 17: 0}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: bad argument"),
    "gemm_ln_unknown_precision": ("pg_dbg_gemm_ln", {1: 7}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: precision must be PG_PREC_BF16 or PG_PREC_F16"),
    "gemm_ln_no_rows": ("pg_dbg_gemm_ln", {11: 0}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: M must be in 1 ... 32"),
    "gemm_ln_33_rows": ("pg_dbg_gemm_ln", {11: 33}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: M must be in 1 ... 32"),
    "gemm_ln_N_not_16": ("pg_dbg_gemm_ln", {12: 24}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: N must be a multiple of 16, at most 65536"),
    "gemm_ln_N_zero": ("pg_dbg_gemm_ln", {12: 0}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: N must be a multiple of 16, at most 65536"),
    "gemm_ln_K_not_256": ("pg_dbg_gemm_ln", {13: 320}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: K must be a multiple of 256"),
    "gemm_ln_K_zero": ("pg_dbg_gemm_ln", {13: 0}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: K must be a multiple of 256"),
    "gemm_ln_K_1536": ("pg_dbg_gemm_ln", {13: 1536}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: K / 256 must be in 1 ... 5"),
    "gemm_ln_gelu": ("pg_dbg_gemm_ln", {14: 2}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: gelu is 0 or 1 and nb 0, 1 or 2"),
    "gemm_ln_nb_3": ("pg_dbg_gemm_ln", {15: 3}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: gelu is 0 or 1 and nb 0, 1 or 2"),
    "gemm_ln_nb_negative": ("pg_dbg_gemm_ln", {15: -1}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: gelu is 0 or 1 and nb 0, 1 or 2"),
    "gemm_ln_nb_2_N_48": ("pg_dbg_gemm_ln", {12: 48, 15: 2}, _lib.PG_ERR_INVALID,
                          "pg_dbg_gemm_ln: two feature blocks per workgroup need N a multiple of 32"),
    "gemm_ln_eps": ("pg_dbg_gemm_ln", {6: -1e-5}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: eps must not be negative"),
    "gemm_ln_eps_nan": ("pg_dbg_gemm_ln", {6: float("nan")}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: eps must not be negative"),
    "gemm_ln_out_rows": ("pg_dbg_gemm_ln", {10: 15}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: out_rows must be in Mi ... 4096"),
    "gemm_ln_out_rows_17_live": ("pg_dbg_gemm_ln", {10: 31, 11: 17}, _lib.PG_ERR_INVALID, "pg_dbg_gemm_ln: out_rows must be in Mi ... 4096"),
    "sample_tokens": ("pg_dbg_sample", {1: None}, _lib.PG_ERR_INVALID, "pg_dbg_sample: bad argument"),
    "sample_idx": ("pg_dbg_sample", {7: None}, _lib.PG_ERR_INVALID, "pg_dbg_sample: bad argument"),
    "sample_params": ("pg_dbg_sample", {12: None}, _lib.PG_ERR_INVALID, "pg_dbg_sample: bad argument"),
    "sample_sampled_out": ("pg_dbg_sample", {18: None}, _lib.PG_ERR_INVALID, "pg_dbg_sample: bad argument"),
    "sample_no_steps": ("pg_dbg_sample", {14: 0}, _lib.PG_ERR_INVALID, "pg_dbg_sample: bad argument"),
    "sample_negative_first_iter": ("pg_dbg_sample", {13: -1}, _lib.PG_ERR_INVALID, "pg_dbg_sample: bad argument"),
    "sample_compact_2": ("pg_dbg_sample", {6: 2}, _lib.PG_ERR_INVALID, "pg_dbg_sample: compact, device_iter and permit_out_of_range are 0 or 1"),
    "sample_device_iter_2": ("pg_dbg_sample", {15: 2}, _lib.PG_ERR_INVALID,
                             "pg_dbg_sample: compact, device_iter and permit_out_of_range are 0 or 1"),
    "sample_permit_minus_1": ("pg_dbg_sample", {17: -1}, _lib.PG_ERR_INVALID,
                              "pg_dbg_sample: compact, device_iter and permit_out_of_range are 0 or 1"),
    "sample_masked_out_without_mask": ("pg_dbg_sample", {19: _z(1, 2, 8, dt=np.int32)}, _lib.PG_ERR_INVALID,
                                       "pg_dbg_sample: masked_tokens_out without a mask step (mask_idx < 0)"),
    "sample_too_few_tables": ("pg_dbg_sample", {13: 1}, _lib.PG_ERR_INVALID, "pg_dbg_sample: n_tables must be at least first_iter + n_steps"),
    "sample_too_few_tables_for_the_steps": ("pg_dbg_sample", {14: 2, 18: _z(2, 2, 2, dt=np.int32)}, _lib.PG_ERR_INVALID,
                                            "pg_dbg_sample: n_tables must be at least first_iter + n_steps"),
    "sample_n_valid_0": ("pg_dbg_sample", {12: _params(0)}, _lib.PG_ERR_INVALID, "pg_dbg_sample: n_valid must be in 1..32"),
    "sample_n_valid_33": ("pg_dbg_sample", {12: _params(33)}, _lib.PG_ERR_INVALID, "pg_dbg_sample: n_valid must be in 1..32"),
    "sample_valid_idx_is_V": ("pg_dbg_sample", {12: _params(20, 14)}, _lib.PG_ERR_INVALID, "pg_dbg_sample: valid_idx out of range"),
    "sample_valid_idx_negative": ("pg_dbg_sample", {12: _params(20, -1)}, _lib.PG_ERR_INVALID, "pg_dbg_sample: valid_idx out of range"),
    "sample_more_selected_than_token_rows": ("pg_dbg_sample", {2: 1}, _lib.PG_ERR_INVALID, "pg_dbg_sample: more selected rows than token rows"),
    "sample_row_map_entry": ("pg_dbg_sample", {9: _i32(0, 2)}, _lib.PG_ERR_INVALID, "pg_dbg_sample: row_map entry 2 is outside the 2 token rows"),
    "sample_row_map_negative": ("pg_dbg_sample", {9: _i32(-1, 0)}, _lib.PG_ERR_INVALID,
                                "pg_dbg_sample: row_map entry -1 is outside the 2 token rows"),
    "sample_position_is_width": ("pg_dbg_sample", {7: _i32(1, 2, 8, -1)}, _lib.PG_ERR_INVALID,
                                 "pg_dbg_sample: target position 8 is out of range for a token row of width 8"),
    "sample_shadowed_position_past_width": ("pg_dbg_sample", {7: _i32(1, 2, 3, 9 | 1 << 30)}, _lib.PG_ERR_INVALID,
                                            "pg_dbg_sample: target position 9 is out of range for a token row of width 8"),
    "gemm_bench_variant_90": ("pg_dbg_gemm_bench", {5: 90}, _lib.PG_ERR_INVALID, "variant 90: K = 3 x depth, fp32 epilogues"),
}


@pytest.mark.parametrize("case", sorted(LATE))
def test_shape_refusals_precede_the_device_lookup(case):
    name, changes, code, message = LATE[case]
    args, _, _ = _cases()[name]
    for index, value in changes.items():
        args = _with(args, index, value)
    assert _call(name, args) == (code, message)


def test_gemm_ln_is_refused_where_the_kernel_is_switched_off():
    """PGIBBS_LN_SKINNY is read once per process: a child with it set to 0 gets the refusal, before the device lookup"""
    import os
    import subprocess
    import sys
    code = ("import numpy as np; from protein_gibbs_sampler_amd import _lib; z = lambda *s: np.zeros(s, np.float32); "
            "a = [z(4, 256), None, z(256), z(256)], [z(32, 256), z(32), z(16, 32)]; p = lambda v: None if v is None else _lib.ptr(v); "
            "rc = _lib.lib().pg_dbg_gemm_ln(0, 0, *map(p, a[0]), 1e-5, *map(p, a[1]), 16, 4, 32, 256, 0, 0, None, 0); "
            "print(rc, _lib.lib().pg_last_error().decode())")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PGIBBS_LN_SKINNY="0", PYTHONPATH=root), cwd=root,
                         capture_output=True, text=True, timeout=120)
    assert out.stdout.strip() == "%d pg_dbg_gemm_ln: the kernel is switched off (PGIBBS_LN_SKINNY=0)" % _lib.PG_ERR_INVALID, out
