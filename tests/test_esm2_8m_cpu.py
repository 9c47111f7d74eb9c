"""ESM-2 8M (esm2_t6_8M_UR50D: 20 heads of 16, d_model 320) on the host: which sizes and head widths load against the configuration,
the numpy reference at heads of 16 against the HuggingFace fixture, the attention and GEMM plans at the 8M shapes, the LDS bank model
of the 32-byte key row, the host-side refusals of the debug entries and, as shared bodies of tests/_esm2_cpu_common.py, the rotary
frequencies, the refusal of a head-16 file by the other sizes and the command-line model maps.  The configuration's values, the v2
file's round trip and inv_freq check and models.ESM2_8M are the esm2_8m rows of tests/test_esm2_sizes_cpu.py.  Needs no GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _esm2_cpu_common as common
import _esm2_reference as ref
from protein_gibbs_sampler_amd import _lib, weights
from test_attention_plan_cpu import F16, att, plans, strict
from test_gemm_plan_cpu import layer, rows
from test_gemm_plan_cpu import plans as gemm_plans

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_t6_takes_the_8m_sizes_from_hyper_parameters_alone():
    cfg = weights.config_from_checkpoint_v2(dict(encoder_embed_dim=320, encoder_layers=6, encoder_attention_heads=20, token_dropout=True),
                                            [], weights.ESM2_T6_CONFIG)
    assert (cfg["d_model"], cfg["n_heads"], cfg["d_ffn"], cfg["n_layers"]) == (320, 20, 1280, 6)
    cfg = weights.config_from_checkpoint_v2(dict(encoder_embed_dim=1280, encoder_layers=33, encoder_attention_heads=20), [], weights.ESM2_T6_CONFIG)
    assert (cfg["d_model"], cfg["n_heads"]) == (1280, 20)                                   # heads of 64 load against every configuration


def test_more_than_32_heads_of_16_and_heads_of_24_are_refused():
    with pytest.raises(ValueError, match="33 heads of dimension 16.*at most 32"):
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=33 * 16, encoder_layers=2, encoder_attention_heads=33), [], weights.ESM2_T6_CONFIG)
    with pytest.raises(ValueError, match="heads of dimension 24"):                          # esm2_t12_35M_UR50D
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=480, encoder_layers=12, encoder_attention_heads=20), [], weights.ESM2_T6_CONFIG)
    with pytest.raises(ValueError, match="esm2_150m"):                                      # heads of 32 still load against t30 only
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=640, encoder_layers=2, encoder_attention_heads=20), [], weights.ESM2_T6_CONFIG)
    with pytest.raises(ValueError, match="esm2_15b"):
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=256, encoder_layers=2, encoder_attention_heads=2), [], weights.ESM2_T6_CONFIG)


# ---- the numpy reference at heads of 16 ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def hf16():
    z = np.load(os.path.join(HERE, "golden", "esm2_hf_hd16.npz"))
    cfg = weights.make_config(weights.ESM2_T6_CONFIG, **json.loads(str(z["cfg"])))
    sd = weights.synthetic_state_dict(cfg, seed=int(z["seed"]), std=float(z["std"]), embed_std=float(z["embed_std"]),
                                      ln_jitter=float(z["ln_jitter"]))
    return z, cfg, sd


def test_reference_at_16_agrees_with_huggingface(hf16):
    z, cfg, sd = hf16
    assert (cfg["d_model"], cfg["n_heads"], cfg["n_layers"]) == (320, 20, 6) and z["tokens"].shape == (2, 258)
    got = ref.esm2_forward(sd, ref.Esm2Config.of(cfg), z["tokens"][:1])
    assert np.abs(got - z["logits"][:1]).max() < 2e-4 and z["logits"].std() > 3.0


def test_the_same_weights_as_10_heads_of_32_are_a_different_model(hf16):
    z, cfg, sd = hf16
    other = dict(cfg, n_heads=10)
    got = ref.esm2_forward(sd, ref.Esm2Config.of(other), z["tokens"][:1, :40])
    mine = ref.esm2_forward(sd, ref.Esm2Config.of(cfg), z["tokens"][:1, :40])
    assert np.abs(got - mine).max() > 0.5


# ---- plans at the 8M shapes (an MI355X: 256 CUs) ---------------------------------------------------------------------------------------
def a16(n_seq, T, **kw):
    return att(n_seq, T, H=20, hd=16, **kw)


PLANS = [
    (a16(256, 258), "whole kb18 hd16 5120wg"),                       # config 2: 5 rounds of four workgroups per CU
    (a16(32, 258), "whole kb18 hd16 640wg"),                         # 640 of 1024 slots: one partial round, nothing to split
    (a16(64, 258), "whole kb18 hd16 split4 1024+1024wg"),
    (a16(1, 27), "whole kb2 hd16 20wg"),
    (a16(2, 576), "whole kb36 hd16 split4 0+160wg"),                 # the tallest rung: 40 pairs on 512 slots
    (a16(2, 577), "long t288 hd16 400wg"),
    (a16(1, 1026), "long t288 hd16 340wg"),
    (a16(3, 258, pad=1), "whole kb18 hd16 pad 60wg"),
    (a16(3, 600, pad=1), "long t288 hd16 pad 600wg"),
    (a16(2, 258, bias=1), "error: attention: the bias_k / bias_v key (ESM-1) is built for heads of 64 only"),
    (att(2, 258, hd=24), "error: attention: head dimension 24: the kernels are built for 64 (every architecture) or 32, 128, 16 (ESM-2 only)"),
    (att(2, 258, hd=48), "error: attention: head dimension 48: the kernels are built for 64 (every architecture) or 32, 128, 16 (ESM-2 only)"),
    (strict(2, 27, hd=16), "split-f32 kb4 nqb1 hd16 40wg"),
    (strict(2, 258, hd=16), "split-f32 kb6 nqb5 hd16 40wg"),
    (strict(2, 100, hd=16, pad=1), "split-f32 kb10 nqb2 hd16 pad 40wg"),
    (strict(2, 258, hd=16, bias=1), "error: attention: the bias_k / bias_v key (ESM-1) is built for heads of 64 only"),
    (att(2, 258, hd=16, precision=F16), "whole kb18 hd16 split4 0+160wg"),    # 40 pairs on 1024 slots: four parts each
    (att(256, 258), "whole kb18 hd64 5120wg"),                       # heads of 64 / 32 / 128 as they were
    (att(64, 258, hd=32), "whole kb18 hd32 split4 1024+1024wg"),
    (att(2, 289, H=40, hd=128), "long t128 hd128 400wg"),
]


def test_attention_plans_at_head_16():
    got = plans([list(c) for c, _ in PLANS])
    wrong = [(c, g, w) for (c, w), g in zip(PLANS, got) if g != w]
    assert not wrong, "\n".join("%r: plan %r, expected %r" % t for t in wrong)


def test_gemm_plans_at_the_8m_shapes():
    """N = 320 / 960 are no multiples of 128: 64 x 64 tiles at every height above the weight-streaming kernel's; fc1 (N = 1280,
    K = 320) is a shape of the 256 x 256 kernels at config 2; a single chain (32 rows) streams the weights."""
    shapes = layer(320, 1280)
    table = rows(66048, shapes, [""] * 4) + rows(8448, shapes, [""] * 4) + rows(32, shapes, [""] * 4)
    got = gemm_plans([list(c) for c, _ in table])
    qkv, out, fc1, fc2 = got[0:4]
    assert qkv.startswith("tile64x64 ") and out.startswith("tile64x64 ") and fc2.startswith("tile64x64 "), got[0:4]
    assert fc1.startswith("w16-256x256 "), fc1
    assert all(g.startswith("tile64x64 ") for g in (got[4], got[5], got[7])), got[4:8]
    assert all(g.startswith("skinny") for g in got[8:12]), got[8:12]
    assert not any(g.startswith("error") for g in got)
    bad = gemm_plans([[66048, 480, 480, 2, 2, 1, 0]])[0]                                   # esm2_t12_35M: K = 480
    assert bad == "error: gemm: K must be a multiple of 64"


# ---- the LDS bank model -----------------------------------------------------------------------------------------------------------------
def test_bank_model_reports_the_built_swizzle_conflict_free():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lds_bank_model.py")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = [l for l in out.stdout.splitlines() if l.startswith("HD 16 ")]
    by = lambda kind, what: [l for l in lines if l.startswith("HD 16 %s " % kind) and what in l]
    assert "(2 = conflict-free): {2}  tr_b16 cycles (2 = conflict-free): {2}" in by("built", "b64 cycles")[0]
    assert by("built", "staging-write")[0].endswith("{8}")
    assert "b64 cycles per read (2 = conflict-free): {4}" in by("none", "b64 cycles")[0]  # unswizzled: 2-way on every score read
    assert "b64 cycles per read (2 = conflict-free): {4}" in by("r1", "b64 cycles")[0]
    other = [l for l in out.stdout.splitlines() if l.startswith(("HD 64 built", "HD 32 built", "HD 128 built")) and "tr_b16" in l]
    assert len(other) == 3 and all("{4}  tr_b16 cycles (2 = conflict-free): {2}" in l for l in other)      # as they were


# ---- host-side refusals of the debug entries -------------------------------------------------------------------------------------------
def test_debug_entries_refuse_on_the_host():
    L = _lib.lib()
    x = np.zeros((2, 3 * 33 * 16), np.float32)
    assert L.pg_dbg_rope_hd(0, _lib.PG_PREC_BF16, _lib.ptr(x), 1, 2, 33, 16) == _lib.PG_ERR_INVALID              # 33 heads of 16
    assert L.pg_dbg_rope_hd(0, _lib.PG_PREC_BF16, _lib.ptr(x), 1, 2, 2, 24) == _lib.PG_ERR_INVALID
    H, T = 2, 16
    qkv = np.zeros((1, T, 3 * H * 16), np.float32)
    ctx = np.zeros((1, T, H * 16), np.float32)
    bias = np.zeros((H, 16), np.float32)
    rc = L.pg_dbg_attention_kv(0, _lib.PG_PREC_BF16, _lib.ptr(qkv), _lib.ptr(ctx), 1, T, H, 16, None, -1, _lib.ptr(bias), _lib.ptr(bias), None, 0)
    assert rc == _lib.PG_ERR_INVALID and b"heads of 64 only" in L.pg_last_error()
    rc = L.pg_dbg_attention_hd(0, _lib.PG_PREC_BF16, _lib.ptr(qkv), _lib.ptr(ctx), 1, T, H, 24, None, -1)
    assert rc == _lib.PG_ERR_INVALID and b"head_dim must be 64 or 32" in L.pg_last_error()


# ---- the shared bodies (tests/_esm2_cpu_common.py) at this size -------------------------------------------------------------------------
def test_inv_freq_16_is_torchs():
    common.check_inv_freq_is_torchs("esm2_8m")


@pytest.mark.parametrize("base", common.other_bases("esm2_8m"))
def test_heads_of_16_met_by_the_other_wrappers_name_esm2_8m(tmp_path_factory, base):
    common.check_met_by_another_size("esm2_8m", base, tmp_path_factory)


def test_command_lines_accept_esm2_8m():
    common.check_command_lines_accept("esm2_8m")
