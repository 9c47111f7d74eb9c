"""ESM-2 150M (esm2_t30_150M_UR50D: 20 heads of 32) on the host: make_config's head width, which head widths load against the
configuration, the numpy reference at heads of 32 against a HuggingFace fixture and, as shared bodies of tests/_esm2_cpu_common.py,
the rotary frequencies, the refusal of a head-32 file by the other sizes and the command-line model maps.  The configuration's values,
the v2 file's round trip and inv_freq check and models.ESM2_150M are the esm2_150m rows of tests/test_esm2_sizes_cpu.py.  Needs no GPU."""
import json
import os

import numpy as np
import pytest

import _esm2_cpu_common as common
import _esm2_reference as ref
from protein_gibbs_sampler_amd import _lib, weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_make_config_keeps_the_base_head_width():
    assert weights.make_config(weights.ESM2_T30_CONFIG, d_model=128, n_layers=2, d_ffn=512)["n_heads"] == 4
    assert weights.make_config(weights.ESM2_T33_CONFIG, d_model=128)["n_heads"] == 2
    assert weights.make_config(weights.ESM1B_CONFIG, d_model=256)["n_heads"] == 4
    assert weights.make_config(weights.MSA1B_CONFIG, d_model=256)["n_heads"] == 4
    assert weights.make_config(weights.ESM2_T30_CONFIG, d_model=128, n_heads=2)["n_heads"] == 2               # an explicit count wins


@pytest.mark.parametrize("d_model, heads, width", [(5120, 40, "128"), (480, 20, "24"), (320, 20, "16")])
def test_other_head_widths_raise_against_t30(d_model, heads, width):
    with pytest.raises(ValueError, match=r"heads of dimension %s: .*head dimension 64" % width):
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=d_model, encoder_layers=2, encoder_attention_heads=heads), [],
                                          weights.ESM2_T30_CONFIG)


def test_t30_takes_the_real_sizes_and_heads_of_64_and_bounds_the_head_count():
    cfg = weights.config_from_checkpoint_v2(dict(encoder_embed_dim=640, encoder_layers=30, encoder_attention_heads=20, token_dropout=True),
                                            [], weights.ESM2_T30_CONFIG)
    assert (cfg["d_model"], cfg["n_heads"], cfg["d_ffn"], cfg["n_layers"]) == (640, 20, 2560, 30)
    cfg = weights.config_from_checkpoint_v2(dict(encoder_embed_dim=256, encoder_layers=2, encoder_attention_heads=4), [], weights.ESM2_T30_CONFIG)
    assert (cfg["d_model"], cfg["n_heads"]) == (256, 4)                                   # heads of 64 load against every configuration
    with pytest.raises(ValueError, match="40 heads of dimension 32.*at most 32"):
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=1280, encoder_layers=2, encoder_attention_heads=40), [], weights.ESM2_T30_CONFIG)


def test_debug_entries_are_declared():
    names = {row[0] for row in _lib.SIGNATURES}
    assert {"pg_dbg_attention_hd", "pg_dbg_rope_hd", "pg_dbg_attention", "pg_dbg_rope"} <= names


def _recipe(name):
    z = np.load(os.path.join(GOLDEN, name))
    return z, json.loads(str(z["cfg"])), dict(seed=int(z["seed"]), std=float(z["std"]), embed_std=float(z["embed_std"]), ln_jitter=float(z["ln_jitter"]))


def test_reference_at_32_agrees_with_huggingface():
    z, over, kw = _recipe("esm2_hf_hd32.npz")
    cfg = weights.make_config(weights.ESM2_T30_CONFIG, **over)
    assert (cfg["d_model"], cfg["n_heads"], cfg["n_layers"]) == (640, 20, 6) and z["tokens"].shape == (2, 258)
    w = weights.synthetic_state_dict(cfg, **kw)
    got = ref.esm2_forward(w, ref.Esm2Config.of(cfg), z["tokens"])
    err = float(np.abs(got - z["logits"]).max())
    assert err < 2e-4, err
    # the head width matters: the same weights read as ten heads of 64 are a different model
    cfg64 = dict(cfg, n_heads=10)
    other = ref.esm2_forward(w, ref.Esm2Config.of(cfg64), z["tokens"])
    assert float(np.abs(other - z["logits"]).max()) > 0.1


# ---- the shared bodies (tests/_esm2_cpu_common.py) at this size -------------------------------------------------------------------------
def test_inv_freq_32_is_torchs():
    common.check_inv_freq_is_torchs("esm2_150m")


@pytest.mark.parametrize("base", common.other_bases("esm2_150m"))
def test_heads_of_32_met_by_the_other_wrappers_name_esm2_150m(tmp_path_factory, base):
    common.check_met_by_another_size("esm2_150m", base, tmp_path_factory)


def test_command_lines_accept_esm2_150m():
    common.check_command_lines_accept("esm2_150m")
