"""ESM-2 15B (esm2_t48_15B_UR50D: 40 heads of 128, d_model 5120) on the host: the tensor shapes at 5120, which sizes and head widths
load against the configuration, the attention plans at head dimension 128 (whole sequences up to 288 keys, 128-key tiles beyond) and
the row entries' acceptance of widths above 2560 in whole 512-feature units only; and, as shared bodies of tests/_esm2_cpu_common.py,
the rotary frequencies, the refusal of a head-128 file by the other sizes and the command-line model maps.  The configuration's values,
the v2 file's round trip and inv_freq check and models.ESM2_15B are the esm2_15b rows of tests/test_esm2_sizes_cpu.py.  Needs no GPU."""
import ctypes

import numpy as np
import pytest

import _esm2_cpu_common as common
from protein_gibbs_sampler_amd import _lib, weights
from test_attention_plan_cpu import F16, att, plans, strict


def test_tensor_names_and_shapes_at_5120():
    cfg = weights.make_config(weights.ESM2_T48_CONFIG, n_layers=1, d_ffn=512)
    sd = weights.synthetic_state_dict(cfg, seed=1)
    assert sd["embed_tokens.weight"].shape == (33, 5120)
    assert sd["layers.0.self_attn.q_proj.weight"].shape == (5120, 5120) and sd["layers.0.self_attn.out_proj.bias"].shape == (5120,)
    assert sd["layers.0.fc1.weight"].shape == (512, 5120) and sd["layers.0.fc2.weight"].shape == (5120, 512)
    assert sd["emb_layer_norm_after.weight"].shape == (5120,) and sd["lm_head.dense.weight"].shape == (5120, 5120)
    assert not any(k.startswith(("embed_positions", "emb_layer_norm_before")) for k in sd)


def test_t48_takes_the_15b_sizes_from_hyper_parameters_alone():
    cfg = weights.config_from_checkpoint_v2(dict(encoder_embed_dim=5120, encoder_layers=48, encoder_attention_heads=40, token_dropout=True),
                                            [], weights.ESM2_T48_CONFIG)
    assert (cfg["d_model"], cfg["n_heads"], cfg["d_ffn"], cfg["n_layers"]) == (5120, 40, 20480, 48)
    cfg = weights.config_from_checkpoint_v2(dict(encoder_embed_dim=2560, encoder_layers=36, encoder_attention_heads=40), [], weights.ESM2_T48_CONFIG)
    assert (cfg["d_model"], cfg["n_heads"]) == (2560, 40)                                   # heads of 64 load against every configuration


def test_more_than_40_heads_of_128_and_odd_widths_are_refused():
    with pytest.raises(ValueError, match="41 heads of dimension 128.*at most 40"):
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=41 * 128, encoder_layers=2, encoder_attention_heads=41), [], weights.ESM2_T48_CONFIG)
    with pytest.raises(ValueError, match="multiples of 512"):                               # 21 heads: 2688 features, no whole 512-unit
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=2688, encoder_layers=2, encoder_attention_heads=21), [], weights.ESM2_T48_CONFIG)
    with pytest.raises(ValueError, match="heads of dimension 24"):
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=480, encoder_layers=2, encoder_attention_heads=20), [], weights.ESM2_T48_CONFIG)
    with pytest.raises(ValueError, match="esm2_150m"):                                      # heads of 32 still load against t30 only
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=640, encoder_layers=2, encoder_attention_heads=20), [], weights.ESM2_T48_CONFIG)


# ---- attention plans at head dimension 128 (an MI355X: 256 CUs) ------------------------------------------------------------------------
def a128(n_seq, T, **kw):
    return att(n_seq, T, H=40, hd=128, **kw)


PLANS = [
    (a128(256, 258), "whole kb18 hd128 10240wg"),                     # config 2: 40 rounds of one workgroup per CU
    (a128(2, 288), "whole kb18 hd128 split3 0+240wg"),                # the tallest rung: 80 pairs on 256 slots
    (a128(2, 289), "long t128 hd128 400wg"),                          # one key more: 128-key tiles, five 64-query chunks per pair
    (a128(1, 577), "long t128 hd128 400wg"),
    (a128(1, 1026), "long t128 hd128 680wg"),
    (a128(1, 27), "whole kb2 hd128 40wg"),
    (a128(3, 258, pad=1), "whole kb18 hd128 pad 120wg"),
    (a128(3, 300, pad=1), "long t128 hd128 pad 600wg"),
    (a128(4, 130), "whole kb10 hd128 split2 0+320wg"),                # two workgroups per CU up to 10 key blocks: 512 slots; nine
                                                                      # query blocks allow two parts of at least one block per wave
    (a128(4, 100), "whole kb8 hd128 160wg"),                          # seven query blocks: too few to split
    (a128(2, 258, bias=1), "error: attention: the bias_k / bias_v key (ESM-1) is built for heads of 64 only"),
    (att(2, 258, hd=48), "error: attention: head dimension 48: the kernels are built for 64 (every architecture) or 32, 128, 16 (ESM-2 only)"),
    (strict(2, 27, H=40, hd=128), "split-f32 kb4 nqb1 hd128 80wg"),
    (strict(2, 100, H=40, hd=128), "split-f32 kb4 nqb2 hd128 80wg"),
    (strict(2, 258, H=40, hd=128), "split-f32 kb4 nqb3 hd128 160wg"),  # never five query blocks per wave at 128
    (strict(1, 1026, H=40, hd=128, pad=1), "split-f32 kb4 nqb3 hd128 pad 240wg"),
    (strict(2, 258, H=40, hd=128, bias=1), "error: attention: the bias_k / bias_v key (ESM-1) is built for heads of 64 only"),
    (att(2, 258, H=40, hd=128, precision=F16), "whole kb18 hd128 split3 0+240wg"),
    (att(256, 258), "whole kb18 hd64 5120wg"),                        # heads of 64 / 32 as they were
    (att(2, 577, hd=32), "long t288 hd32 400wg"),
]


def test_attention_plans_at_head_128():
    got = plans([list(c) for c, _ in PLANS])
    wrong = [(c, g, w) for (c, w), g in zip(PLANS, got) if g != w]
    assert not wrong, "\n".join("%r: plan %r, expected %r" % t for t in wrong)


# ---- rows wider than 2560 features -----------------------------------------------------------------------------------------------------
def _ln_rows(M, d):
    x = np.zeros((M, d), np.float32)
    g = np.zeros(d, np.float32)
    h = np.zeros((M, d), np.uint16)
    k = ctypes.c_int(-1)
    return _lib.lib().pg_dbg_layernorm_rows(0, _lib.PG_PREC_BF16, _lib.ptr(x), _lib.ptr(g), _lib.ptr(g), _lib.ptr(h), M, M, d, 1e-5, 0, 0, 0,
                                            ctypes.byref(k))


@pytest.mark.parametrize("d", [2564, 2688, 2816, 5632, 5124, 4100])
def test_row_entries_refuse_widths_that_are_no_whole_unit(d):
    rc = _ln_rows(4, d)
    msg = _lib.lib().pg_last_error().decode()
    assert rc == _lib.PG_ERR_INVALID and "2560" in msg and "multiple of 512 up to 5120" in msg, (rc, msg)


@pytest.mark.parametrize("d", [3072, 4096, 5120])
def test_row_entries_accept_whole_units_above_2560_on_the_host(d):
    """past the host-side checks: with a GPU the call runs, without one it ends at the device, never at the width"""
    rc = _ln_rows(4, d)
    msg = "" if rc == _lib.PG_OK else (_lib.lib().pg_last_error() or b"").decode()      # after a success the text is an earlier call's
    assert rc != _lib.PG_ERR_INVALID and "2560" not in msg, (rc, msg)


def test_rope_entry_takes_40_heads_of_128_and_refuses_41_on_the_host():
    L = _lib.lib()
    x = np.zeros((2, 3 * 41 * 128), np.float32)
    assert L.pg_dbg_rope_hd(0, _lib.PG_PREC_BF16, _lib.ptr(x), 1, 2, 41, 128) == _lib.PG_ERR_INVALID
    assert L.pg_dbg_rope(0, _lib.PG_PREC_BF16, _lib.ptr(x), 1, 2, 41) == _lib.PG_ERR_INVALID                  # head 64: still 40 at most
    assert L.pg_dbg_rope_hd(0, _lib.PG_PREC_BF16, _lib.ptr(x), 1, 2, 2, 48) == _lib.PG_ERR_INVALID


# ---- the shared bodies (tests/_esm2_cpu_common.py) at this size -------------------------------------------------------------------------
def test_inv_freq_128_is_torchs():
    common.check_inv_freq_is_torchs("esm2_15b")


@pytest.mark.parametrize("base", common.other_bases("esm2_15b"))
def test_heads_of_128_met_by_the_other_wrappers_name_esm2_15b(tmp_path_factory, base):
    common.check_met_by_another_size("esm2_15b", base, tmp_path_factory)


def test_command_lines_accept_esm2_15b():
    common.check_command_lines_accept("esm2_15b")
