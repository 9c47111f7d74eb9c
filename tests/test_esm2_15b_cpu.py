"""ESM-2 15B (esm2_t48_15B_UR50D: 40 heads of 128, d_model 5120) on the host: the configuration, the rotary frequencies for heads of
128, the v2 checkpoint reader and which head widths load against which configuration, models.ESM2_15B, the command-line model maps,
the attention plans at head dimension 128 (whole sequences up to 288 keys, 128-key tiles beyond) and the row entries' acceptance of
widths above 2560 in whole 512-feature units only.  Needs no GPU."""
import ctypes

import numpy as np
import pytest

from protein_gibbs_sampler_amd import _lib, weights
from test_attention_plan_cpu import F16, att, plans, strict


def test_t48_config_values():
    cfg = weights.ESM2_T48_CONFIG
    assert (cfg["arch"], cfg["d_model"], cfg["n_layers"], cfg["n_heads"], cfg["d_ffn"], cfg["vocab"]) == (_lib.PG_ARCH_ESM2, 5120, 48, 40, 20480, 33)
    assert weights.head_dim_of(cfg) == 128 and 128 in weights.HEAD_DIMS
    same = ("max_positions", "pad_idx", "mask_idx", "cls_idx", "eos_idx", "token_dropout", "max_msa_rows", "layer_norm_eps")
    assert all(cfg[k] == weights.ESM2_T33_CONFIG[k] for k in same)
    assert weights.MAX_D_MODEL == 2560 and weights.MAX_D_MODEL_HD128 == 5120 and weights.MAX_HEADS_OF_128 == 40
    assert weights.make_config(weights.ESM2_T48_CONFIG, d_model=256, n_layers=2, d_ffn=512)["n_heads"] == 2      # the base's head width
    assert weights.ESM2_T36_CONFIG["n_heads"] == 40 and weights.ESM2_T30_CONFIG["n_heads"] == 20                   # the others are untouched


def test_tensor_names_and_shapes_at_5120():
    cfg = weights.make_config(weights.ESM2_T48_CONFIG, n_layers=1, d_ffn=512)
    sd = weights.synthetic_state_dict(cfg, seed=1)
    assert sd["embed_tokens.weight"].shape == (33, 5120)
    assert sd["layers.0.self_attn.q_proj.weight"].shape == (5120, 5120) and sd["layers.0.self_attn.out_proj.bias"].shape == (5120,)
    assert sd["layers.0.fc1.weight"].shape == (512, 5120) and sd["layers.0.fc2.weight"].shape == (5120, 512)
    assert sd["emb_layer_norm_after.weight"].shape == (5120,) and sd["lm_head.dense.weight"].shape == (5120, 5120)
    assert not any(k.startswith(("embed_positions", "emb_layer_norm_before")) for k in sd)


def test_inv_freq_128_is_torchs():
    torch = pytest.importorskip("torch")
    want = (1.0 / (10000 ** (torch.arange(0, 128, 2).float() / 128))).numpy()
    assert np.array_equal(weights.rotary_inv_freq(128), want)
    want64 = (1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))).numpy()
    assert np.array_equal(weights.rotary_inv_freq(), want64)


@pytest.fixture(scope="module")
def hd128_file(tmp_path_factory):
    """A v2 checkpoint file of 2 layers x 256 with two heads of 128 and the state dict it was written from."""
    torch = pytest.importorskip("torch")
    cfg = weights.make_config(weights.ESM2_T48_CONFIG, d_model=256, n_layers=2, d_ffn=1024, max_positions=40)
    assert cfg["n_heads"] == 2
    sd = weights.synthetic_state_dict(cfg, seed=12, embed_std=0.3)
    path = tmp_path_factory.mktemp("esm2_15b") / "esm2_hd128.pt"
    torch.save(weights.to_fair_esm_checkpoint_v2(sd, cfg), path)
    return str(path), cfg, sd


def test_v2_round_trip_with_heads_of_128(hd128_file):
    torch = pytest.importorskip("torch")
    path, cfg, sd = hd128_file
    blob = torch.load(path, weights_only=False)
    stored = blob["model"]["encoder.sentence_encoder.layers.1.self_attn.rot_emb.inv_freq"].numpy()
    assert stored.shape == (64,) and np.array_equal(stored, weights.rotary_inv_freq(128))
    got, cfg2 = weights.load_fair_esm_checkpoint(path, weights.ESM2_T48_CONFIG, return_config=True)
    assert (cfg2["d_model"], cfg2["n_layers"], cfg2["n_heads"], cfg2["d_ffn"], cfg2["token_dropout"]) == (256, 2, 2, 1024, 1)
    assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)


def test_inv_freq_check_at_128(hd128_file, tmp_path):
    torch = pytest.importorskip("torch")
    path, cfg, sd = hd128_file
    blob = weights.to_fair_esm_checkpoint_v2(sd, cfg)
    key = "encoder.sentence_encoder.layers.0.self_attn.rot_emb.inv_freq"
    blob["model"][key] = torch.from_numpy(weights.rotary_inv_freq(64))                      # the head-64 table in a head-128 file
    p = tmp_path / "bad.pt"
    torch.save(blob, p)
    with pytest.raises(ValueError, match=r"inv_freq.*heads of 128"):
        weights.load_fair_esm_checkpoint(str(p), weights.ESM2_T48_CONFIG)
    blob["model"][key] = torch.from_numpy(weights.rotary_inv_freq(128) * np.float32(1.001))
    torch.save(blob, p)
    with pytest.raises(ValueError, match="inv_freq"):
        weights.load_fair_esm_checkpoint(str(p), weights.ESM2_T48_CONFIG)


def test_t48_takes_the_15b_sizes_from_hyper_parameters_alone():
    cfg = weights.config_from_checkpoint_v2(dict(encoder_embed_dim=5120, encoder_layers=48, encoder_attention_heads=40, token_dropout=True),
                                            [], weights.ESM2_T48_CONFIG)
    assert (cfg["d_model"], cfg["n_heads"], cfg["d_ffn"], cfg["n_layers"]) == (5120, 40, 20480, 48)
    cfg = weights.config_from_checkpoint_v2(dict(encoder_embed_dim=2560, encoder_layers=36, encoder_attention_heads=40), [], weights.ESM2_T48_CONFIG)
    assert (cfg["d_model"], cfg["n_heads"]) == (2560, 40)                                   # heads of 64 load against every configuration


@pytest.mark.parametrize("base", ["t33", "t36", "t30"])
def test_heads_of_128_met_by_the_other_wrappers_name_esm2_15b(hd128_file, base):
    path, cfg, sd = hd128_file
    base_cfg = {"t33": weights.ESM2_T33_CONFIG, "t36": weights.ESM2_T36_CONFIG, "t30": weights.ESM2_T30_CONFIG}[base]
    with pytest.raises(ValueError, match=r"heads of dimension 128: .*head dimension 64.*models\.ESM2_15B / --model esm2_15b"):
        weights.load_fair_esm_checkpoint(path, base_cfg)
    with pytest.raises(ValueError, match="esm2_15b"):
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=5120, encoder_layers=48, encoder_attention_heads=40), [], base_cfg)


def test_more_than_40_heads_of_128_and_odd_widths_are_refused():
    with pytest.raises(ValueError, match="41 heads of dimension 128.*at most 40"):
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=41 * 128, encoder_layers=2, encoder_attention_heads=41), [], weights.ESM2_T48_CONFIG)
    with pytest.raises(ValueError, match="multiples of 512"):                               # 21 heads: 2688 features, no whole 512-unit
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=2688, encoder_layers=2, encoder_attention_heads=21), [], weights.ESM2_T48_CONFIG)
    with pytest.raises(ValueError, match="heads of dimension 24"):
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=480, encoder_layers=2, encoder_attention_heads=20), [], weights.ESM2_T48_CONFIG)
    with pytest.raises(ValueError, match="esm2_150m"):                                      # heads of 32 still load against t30 only
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=640, encoder_layers=2, encoder_attention_heads=20), [], weights.ESM2_T48_CONFIG)


def test_models_esm2_15b_reads_a_v2_file_without_a_gpu(hd128_file):
    from protein_gibbs_sampler_amd import models
    path, cfg, sd = hd128_file
    m = models.ESM2_15B(checkpoint=path)
    assert m.cfg["arch"] == _lib.PG_ARCH_ESM2 and (m.cfg["d_model"], m.cfg["n_heads"], m.cfg["d_ffn"], m.cfg["n_layers"]) == (256, 2, 1024, 2)
    assert m.alphabet.mask_idx == 32 and len(m.alphabet.all_toks) == 33 and m.alphabet.prepend_bos and m.alphabet.append_eos
    for other in (models.ESM2, models.ESM2_3B, models.ESM2_150M):
        with pytest.raises(ValueError, match="esm2_15b"):
            other(checkpoint=path)
    if not weights.find_cached_checkpoint("esm2_t48_15B_UR50D.pt"):
        with pytest.raises(FileNotFoundError, match="esm2_t48_15B_UR50D"):
            models.ESM2_15B()


def test_command_lines_accept_esm2_15b():
    from protein_gibbs_sampler_amd import likelihood_esm, models, pgen_esm, pgen_esm_from_fasta
    for mod in (pgen_esm, pgen_esm_from_fasta, likelihood_esm):
        assert mod.model_map["esm2_15b"] is models.ESM2_15B and mod.model_map["esm2_3b"] is models.ESM2_3B
        assert mod.build_parser().parse_args(["--model", "esm2_15b"]).model == "esm2_15b"
    assert pgen_esm.build_parser().parse_args([]).model == "esm1b"                       # defaults unchanged


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


def test_strict_valu_switch_refuses_heads_of_128_by_name():
    got = plans([list(strict(2, 27, H=2, hd=128))], PGIBBS_ATTN_F32="valu")
    assert "PGIBBS_ATTN_F32=valu" in got[0] and "heads of 128" in got[0] and got[0].startswith("error: ")


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
