"""ESM-2 150M (esm2_t30_150M_UR50D: 20 heads of 32) on the host: the configuration, the rotary frequencies for heads of 32, the v2
checkpoint reader and which head widths load against which configuration, models.ESM2_150M, the command-line model maps, and the
numpy reference with the head dimension as a parameter (against the head-64 reference and a HuggingFace fixture).  Needs no GPU."""
import json
import os

import numpy as np
import pytest

import _esm2_reference as ref64
import _esm2_reference_hd as ref
from protein_gibbs_sampler_amd import _lib, weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def test_t30_config_values():
    cfg = weights.ESM2_T30_CONFIG
    assert (cfg["arch"], cfg["d_model"], cfg["n_layers"], cfg["n_heads"], cfg["d_ffn"], cfg["vocab"]) == (_lib.PG_ARCH_ESM2, 640, 30, 20, 2560, 33)
    assert cfg["n_heads"] * 32 == cfg["d_model"] and weights.head_dim_of(cfg) == 32
    same = ("max_positions", "pad_idx", "mask_idx", "cls_idx", "eos_idx", "token_dropout", "max_msa_rows", "layer_norm_eps")
    assert all(cfg[k] == weights.ESM2_T33_CONFIG[k] for k in same)
    assert weights.ESM2_T33_CONFIG["n_heads"] == 20 and weights.ESM2_T36_CONFIG["n_heads"] == 40          # the other two are untouched


def test_make_config_keeps_the_base_head_width():
    assert weights.make_config(weights.ESM2_T30_CONFIG, d_model=128, n_layers=2, d_ffn=512)["n_heads"] == 4
    assert weights.make_config(weights.ESM2_T33_CONFIG, d_model=128)["n_heads"] == 2
    assert weights.make_config(weights.ESM1B_CONFIG, d_model=256)["n_heads"] == 4
    assert weights.make_config(weights.MSA1B_CONFIG, d_model=256)["n_heads"] == 4
    assert weights.make_config(weights.ESM2_T30_CONFIG, d_model=128, n_heads=2)["n_heads"] == 2               # an explicit count wins


def test_inv_freq_32_is_torchs():
    torch = pytest.importorskip("torch")
    want = (1.0 / (10000 ** (torch.arange(0, 32, 2).float() / 32))).numpy()
    assert np.array_equal(weights.rotary_inv_freq(32), want) and np.array_equal(ref.inv_freq(32), want)
    want64 = (1.0 / (10000 ** (torch.arange(0, 64, 2).float() / 64))).numpy()
    assert np.array_equal(weights.rotary_inv_freq(), want64) and np.array_equal(weights.rotary_inv_freq(64), want64)


@pytest.fixture(scope="module")
def hd32_file(tmp_path_factory):
    """A v2 checkpoint file of 2 layers x 128 with four heads of 32 and the state dict it was written from."""
    torch = pytest.importorskip("torch")
    cfg = weights.make_config(weights.ESM2_T30_CONFIG, d_model=128, n_layers=2, d_ffn=512, max_positions=40)
    assert cfg["n_heads"] == 4
    sd = weights.synthetic_state_dict(cfg, seed=12, embed_std=0.3)
    path = tmp_path_factory.mktemp("esm2_150m") / "esm2_hd32.pt"
    torch.save(weights.to_fair_esm_checkpoint_v2(sd, cfg), path)
    return str(path), cfg, sd


def test_v2_round_trip_with_heads_of_32(hd32_file):
    torch = pytest.importorskip("torch")
    path, cfg, sd = hd32_file
    blob = torch.load(path, weights_only=False)
    stored = blob["model"]["encoder.sentence_encoder.layers.1.self_attn.rot_emb.inv_freq"].numpy()
    assert np.array_equal(stored, weights.rotary_inv_freq(32))
    got, cfg2 = weights.load_fair_esm_checkpoint(path, weights.ESM2_T30_CONFIG, return_config=True)
    assert (cfg2["d_model"], cfg2["n_layers"], cfg2["n_heads"], cfg2["d_ffn"], cfg2["token_dropout"]) == (128, 2, 4, 512, 1)
    assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)


def test_perturbed_inv_freq_raises(hd32_file, tmp_path):
    torch = pytest.importorskip("torch")
    path, cfg, sd = hd32_file
    blob = weights.to_fair_esm_checkpoint_v2(sd, cfg)
    blob["model"]["encoder.sentence_encoder.layers.0.self_attn.rot_emb.inv_freq"] = torch.from_numpy(weights.rotary_inv_freq(32) * np.float32(1.001))
    p = tmp_path / "bad.pt"
    torch.save(blob, p)
    with pytest.raises(ValueError, match=r"inv_freq.*heads of 32"):
        weights.load_fair_esm_checkpoint(str(p), weights.ESM2_T30_CONFIG)
    blob["model"]["encoder.sentence_encoder.layers.0.self_attn.rot_emb.inv_freq"] = torch.from_numpy(weights.rotary_inv_freq(64))
    torch.save(blob, p)
    with pytest.raises(ValueError, match="inv_freq"):                                    # the head-64 frequencies in a head-32 file
        weights.load_fair_esm_checkpoint(str(p), weights.ESM2_T30_CONFIG)


@pytest.mark.parametrize("base", ["t33", "t36"])
def test_heads_of_32_met_by_the_other_wrappers_name_esm2_150m(hd32_file, base):
    path, cfg, sd = hd32_file
    base_cfg = weights.ESM2_T33_CONFIG if base == "t33" else weights.ESM2_T36_CONFIG
    with pytest.raises(ValueError, match=r"heads of dimension 32: .*head dimension 64.*models\.ESM2_150M / --model esm2_150m"):
        weights.load_fair_esm_checkpoint(path, base_cfg)
    with pytest.raises(ValueError, match="esm2_150m"):
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=640, encoder_layers=30, encoder_attention_heads=20), [], base_cfg)


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


def test_models_esm2_150m_reads_a_v2_file_without_a_gpu(hd32_file):
    from protein_gibbs_sampler_amd import models
    path, cfg, sd = hd32_file
    m = models.ESM2_150M(checkpoint=path)
    assert m.cfg["arch"] == _lib.PG_ARCH_ESM2 and (m.cfg["d_model"], m.cfg["n_heads"], m.cfg["d_ffn"], m.cfg["n_layers"]) == (128, 4, 512, 2)
    assert m.alphabet.mask_idx == 32 and len(m.alphabet.all_toks) == 33 and m.alphabet.prepend_bos and m.alphabet.append_eos
    for other in (models.ESM2, models.ESM2_3B):
        with pytest.raises(ValueError, match="esm2_150m"):
            other(checkpoint=path)
    if not weights.find_cached_checkpoint("esm2_t30_150M_UR50D.pt"):
        with pytest.raises(FileNotFoundError, match="esm2_t30_150M_UR50D"):
            models.ESM2_150M()


def test_command_lines_accept_esm2_150m():
    from protein_gibbs_sampler_amd import likelihood_esm, models, pgen_esm, pgen_esm_from_fasta
    for mod in (pgen_esm, pgen_esm_from_fasta, likelihood_esm):
        assert mod.model_map["esm2_150m"] is models.ESM2_150M and mod.model_map["esm2"] is models.ESM2
    assert pgen_esm.build_parser().parse_args(["--model", "esm2_150m", "--synthetic-weights"]).model == "esm2_150m"
    assert likelihood_esm.build_parser().parse_args(["--model", "esm2_150m"]).model == "esm2_150m"
    assert pgen_esm_from_fasta.build_parser().parse_args(["--model", "esm2_150m"]).model == "esm2_150m"
    assert pgen_esm.build_parser().parse_args([]).model == "esm1b"                       # defaults unchanged


def test_debug_entries_are_declared():
    names = {row[0] for row in _lib.SIGNATURES}
    assert {"pg_dbg_attention_hd", "pg_dbg_rope_hd", "pg_dbg_attention", "pg_dbg_rope"} <= names


def _recipe(name):
    z = np.load(os.path.join(GOLDEN, name))
    return z, json.loads(str(z["cfg"])), dict(seed=int(z["seed"]), std=float(z["std"]), embed_std=float(z["embed_std"]), ln_jitter=float(z["ln_jitter"]))


def test_reference_at_64_equals_the_head_64_reference_bit_for_bit():
    z, over, kw = _recipe("esm2_hf_small.npz")
    cfg = weights.make_config(weights.ESM2_T33_CONFIG, **over)
    w = weights.synthetic_state_dict(cfg, **kw)
    tok = z["tokens"].copy()
    tok[1, -5:] = 1                                                                       # a right-padded row as well
    a = ref64.esm2_forward(w, ref64.Esm2Config.of(cfg), tok)
    b = ref.esm2_forward(w, ref.Esm2Config.of(cfg), tok)
    assert np.array_equal(a, b)
    rng = np.random.default_rng(5)
    qkv = rng.standard_normal((2 * 9, 3 * 3 * 64)).astype(np.float32)
    assert np.array_equal(ref64.rotate_qkv_rows(qkv, 2, 9, 3), ref.rotate_qkv_rows(qkv, 2, 9, 3, 64))
    assert all(np.array_equal(x, y) for x, y in zip(ref64.cos_sin(40), ref.cos_sin(40, 64)))


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
