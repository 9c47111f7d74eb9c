"""ESM-2 3B (esm2_t36_3B_UR50D) on the host: the configuration, the v2 checkpoint reader at d_model 2560, which widths are loaded
against which configuration, models.ESM2_3B and the command-line model maps (a shared body of tests/_esm2_cpu_common.py).  The
configuration's values are the esm2_3b row of tests/test_esm2_sizes_cpu.py.  Needs no GPU."""
import numpy as np
import pytest

import _esm2_cpu_common as common
from protein_gibbs_sampler_amd import _lib, weights


def test_t36_tensor_names_and_shapes():
    cfg = weights.make_config(weights.ESM2_T36_CONFIG, n_layers=2)
    shapes = weights.tensor_shapes(cfg)
    assert not any(n.startswith("embed_positions") or n.startswith("emb_layer_norm_before") for n in shapes)
    assert not any(n.startswith("layers.2.") for n in shapes)
    want = {"embed_tokens.weight": (33, 2560), "emb_layer_norm_after.weight": (2560,), "lm_head.dense.weight": (2560, 2560),
            "lm_head.layer_norm.bias": (2560,), "lm_head.bias": (33,), "layers.0.self_attn.q_proj.weight": (2560, 2560),
            "layers.1.self_attn.out_proj.bias": (2560,), "layers.1.fc1.weight": (10240, 2560), "layers.1.fc1.bias": (10240,),
            "layers.0.fc2.weight": (2560, 10240), "layers.0.self_attn_layer_norm.weight": (2560,),
            "layers.1.final_layer_norm.bias": (2560,)}
    for name, shape in want.items():
        assert tuple(shapes[name]) == shape, name


@pytest.fixture(scope="module")
def wide_file(tmp_path_factory):
    """A v2 checkpoint file of 2 layers x 2560 x 40 heads and the state dict it was written from."""
    torch = pytest.importorskip("torch")
    cfg = weights.make_config(weights.ESM2_T36_CONFIG, n_layers=2, max_positions=40)
    sd = weights.synthetic_state_dict(cfg, seed=11, embed_std=0.3)
    path = tmp_path_factory.mktemp("esm2_3b") / "esm2_wide.pt"
    torch.save(weights.to_fair_esm_checkpoint_v2(sd, cfg), path)
    return str(path), cfg, sd


def test_v2_round_trip_at_2560(wide_file):
    path, cfg, sd = wide_file
    base = weights.make_config(weights.ESM2_T36_CONFIG, max_positions=40)           # 36 layers: the count must come from the file
    got, cfg2 = weights.load_fair_esm_checkpoint(path, base, return_config=True)
    assert (cfg2["d_model"], cfg2["n_layers"], cfg2["n_heads"], cfg2["d_ffn"], cfg2["token_dropout"]) == (2560, 2, 40, 10240, 1)
    assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
    got2 = weights.load_fair_esm_checkpoint(path, cfg)                               # ... and against the 2-layer cut itself
    assert set(got2) == set(sd)


def test_config_from_checkpoint_v2_picks_3b_sizes():
    names = list(weights.tensor_shapes(weights.make_config(weights.ESM2_T36_CONFIG, n_layers=3)))
    file_cfg = dict(encoder_embed_dim=2560, encoder_layers=3, encoder_attention_heads=40, token_dropout=True)
    cfg = weights.config_from_checkpoint_v2(file_cfg, names, weights.ESM2_T36_CONFIG)
    assert (cfg["d_model"], cfg["n_heads"], cfg["d_ffn"], cfg["n_layers"]) == (2560, 40, 10240, 3)
    # a base config of another width above 2048 (a cut-down 3B-family config) also takes the file's sizes
    cfg = weights.config_from_checkpoint_v2(file_cfg, names, weights.make_config(weights.ESM2_T36_CONFIG, d_model=2304, n_heads=36, d_ffn=9216))
    assert (cfg["d_model"], cfg["n_heads"], cfg["d_ffn"]) == (2560, 40, 10240)


@pytest.mark.parametrize("base", ["t33", "t36"])
@pytest.mark.parametrize("d_model, heads, width", [(5120, 40, "128"), (640, 20, "32"), (480, 20, "24"), (320, 20, "16")])
def test_other_sizes_still_raise_by_head_width(base, d_model, heads, width):
    """esm2_t48_15B (heads of 128) and the small sizes (32 / 24 / 16) are refused whichever wrapper's config they meet, and the
    head-width check fires before the d_model one."""
    base_cfg = weights.ESM2_T33_CONFIG if base == "t33" else weights.ESM2_T36_CONFIG
    file_cfg = dict(encoder_embed_dim=d_model, encoder_layers=2, encoder_attention_heads=heads)
    with pytest.raises(ValueError, match=r"heads of dimension %s: .*head dimension 64" % width):
        weights.config_from_checkpoint_v2(file_cfg, [], base_cfg)


def test_wider_than_2560_raises():
    with pytest.raises(ValueError, match="d_model 3072 > 2560"):
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=3072, encoder_layers=2, encoder_attention_heads=48), [], weights.ESM2_T36_CONFIG)


def test_wide_file_loads_against_t36_and_not_against_t33(wide_file):
    path, cfg, sd = wide_file
    got, cfg2 = weights.load_fair_esm_checkpoint(path, weights.ESM2_T36_CONFIG, return_config=True)
    assert cfg2["d_model"] == 2560 and cfg2["n_layers"] == 2 and cfg2["max_positions"] == 1024
    assert np.array_equal(got["layers.1.fc2.weight"], sd["layers.1.fc2.weight"])
    for base in (weights.ESM2_T33_CONFIG, weights.make_config(weights.ESM2_T33_CONFIG, d_model=2048, n_heads=32, d_ffn=8192)):
        with pytest.raises(ValueError, match=r"d_model 2560 > 2048.*models\.ESM2_3B / --model esm2_3b"):
            weights.load_fair_esm_checkpoint(path, base)


def test_models_esm2_3b_reads_a_v2_file_without_a_gpu(wide_file, tmp_path):
    torch = pytest.importorskip("torch")
    from protein_gibbs_sampler_amd import models
    path, cfg, sd = wide_file
    m = models.ESM2_3B(checkpoint=path)
    assert m.cfg["arch"] == _lib.PG_ARCH_ESM2 and (m.cfg["d_model"], m.cfg["n_heads"], m.cfg["d_ffn"], m.cfg["n_layers"]) == (2560, 40, 10240, 2)
    assert m.alphabet.mask_idx == 32 and len(m.alphabet.all_toks) == 33 and m.alphabet.prepend_bos and m.alphabet.append_eos
    with pytest.raises(ValueError, match="esm2_3b"):                                 # the 650M wrapper refuses the same file by name
        models.ESM2(checkpoint=path)
    # a small file of the same layout loads through either wrapper: sizes come from the file
    small = weights.make_config(weights.ESM2_T33_CONFIG, d_model=128, n_layers=2, d_ffn=512, max_positions=40)
    p2 = tmp_path / "small.pt"
    torch.save(weights.to_fair_esm_checkpoint_v2(weights.synthetic_state_dict(small, seed=3), small), p2)
    assert models.ESM2_3B(checkpoint=str(p2)).cfg["d_model"] == 128
    if not weights.find_cached_checkpoint("esm2_t36_3B_UR50D.pt"):                   # no file, no opt-in to synthetic weights: refuse
        with pytest.raises(FileNotFoundError, match="esm2_t36_3B_UR50D"):
            models.ESM2_3B()


def test_command_lines_accept_esm2_3b():
    common.check_command_lines_accept("esm2_3b")
