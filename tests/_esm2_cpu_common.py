"""The host-side test bodies that are the same at every released ESM-2 size, each taking a --model name whose row of
tests/_esm2_sizes.py holds what differs.  tests/test_esm2_sizes_cpu.py runs the ones that are one item per size; each size's own file
(tests/test_esm2_cpu.py and its _3b, _150m, _15b, _8m, _35m siblings) runs the others."""
import numpy as np
import pytest

import _esm2_reference as ref
from _esm2_sizes import SIZES
from protein_gibbs_sampler_amd import _lib, models, weights

INV_FREQ_KEY = "encoder.sentence_encoder.layers.%d.self_attn.rot_emb.inv_freq"
# the other sizes under the names of their base configurations, as the per-size files' parameter ids have them
BASES = {"t33": "esm2", "t36": "esm2_3b", "t30": "esm2_150m", "t48": "esm2_15b", "t6": "esm2_8m", "t12": "esm2_35m"}


def other_bases(size):
    return [b for b, s in BASES.items() if s != size]


def check_config_values(size):
    row = SIZES[size]
    cfg, hd = row["base"], row["hd"]
    assert (cfg["arch"], cfg["d_model"], cfg["n_layers"], cfg["n_heads"], cfg["d_ffn"], cfg["vocab"]) == (_lib.PG_ARCH_ESM2, *row["shape"], 33)
    assert weights.head_dim_of(cfg) == hd and cfg["n_heads"] * hd == cfg["d_model"] and cfg["d_ffn"] == 4 * cfg["d_model"]
    assert hd in weights.HEAD_DIMS and 24 not in weights.HEAD_DIMS
    same = ("max_positions", "pad_idx", "mask_idx", "cls_idx", "eos_idx", "token_dropout", "max_msa_rows", "layer_norm_eps")
    assert all(cfg[k] == weights.ESM2_T33_CONFIG[k] for k in same)
    assert weights.HEAD_WIDTHS[hd]["max_heads"] == row["max_heads"] == getattr(weights, "MAX_HEADS_OF_%d" % hd, row["max_heads"])
    assert weights.MAX_D_MODEL == 2560 and weights.MAX_D_MODEL_HD128 == 5120
    if "cut" in row:
        assert weights.make_config(cfg, d_model=row["cut"][0], n_layers=2, d_ffn=512)["n_heads"] == row["cut"][1]      # the base's head width
    for other in SIZES.values():                                                                                       # the others are untouched
        assert (other["base"]["d_model"], other["base"]["n_layers"], other["base"]["n_heads"], other["base"]["d_ffn"]) == other["shape"]


def check_inv_freq_is_torchs(size):
    torch = pytest.importorskip("torch")
    hd = SIZES[size]["hd"]
    want = (1.0 / (10000 ** (torch.arange(0, hd, 2).float() / hd))).numpy()
    assert np.array_equal(weights.rotary_inv_freq(hd), want)
    if hd == 64:
        assert np.array_equal(weights.rotary_inv_freq(), want)
    if SIZES[size].get("ref_inv_freq_is_torchs", True):
        assert np.array_equal(ref.inv_freq(hd), want)


# ---- a v2 checkpoint file with heads of the size's width -------------------------------------------------------------------------------
_FILES = {}


def v2_file(size, tmp_path_factory):
    """-> (path, configuration, state dict) of the row's cut written as a v2 checkpoint file, once per session"""
    torch = pytest.importorskip("torch")
    if size not in _FILES:
        row = SIZES[size]
        cfg = weights.make_config(row["base"], max_positions=40, **row["v2_file"]["cut"])
        assert (cfg["d_model"], cfg["n_layers"], cfg["n_heads"], cfg["d_ffn"]) == row["v2_file"]["shape"]
        sd = weights.synthetic_state_dict(cfg, seed=12, embed_std=0.3)
        path = tmp_path_factory.mktemp(size) / ("esm2_hd%d.pt" % row["hd"])
        torch.save(weights.to_fair_esm_checkpoint_v2(sd, cfg), path)
        _FILES[size] = (str(path), cfg, sd)
    return _FILES[size]


def check_v2_round_trip(size, tmp_path_factory):
    import torch
    path, cfg, sd = v2_file(size, tmp_path_factory)
    hd = SIZES[size]["hd"]
    stored = torch.load(path, weights_only=False)["model"][INV_FREQ_KEY % 1].numpy()
    assert stored.shape == (hd // 2,) and np.array_equal(stored, weights.rotary_inv_freq(hd))
    got, cfg2 = weights.load_fair_esm_checkpoint(path, SIZES[size]["base"], return_config=True)
    assert (cfg2["d_model"], cfg2["n_layers"], cfg2["n_heads"], cfg2["d_ffn"], cfg2["token_dropout"]) == (*SIZES[size]["v2_file"]["shape"], 1)
    assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)


def check_inv_freq_check(size, tmp_path_factory, tmp_path):
    import torch
    path, cfg, sd = v2_file(size, tmp_path_factory)
    row = SIZES[size]
    blob = weights.to_fair_esm_checkpoint_v2(sd, cfg)
    p = tmp_path / "bad.pt"
    # another width's table in the file, then the width's own table a thousandth off
    for bad in (weights.rotary_inv_freq(row["other_table"]), weights.rotary_inv_freq(row["hd"]) * np.float32(1.001)):
        blob["model"][INV_FREQ_KEY % 0] = torch.from_numpy(bad)
        torch.save(blob, p)
        with pytest.raises(ValueError, match=r"inv_freq.*heads of %d" % row["hd"]):
            weights.load_fair_esm_checkpoint(str(p), row["base"])


def check_met_by_another_size(size, base, tmp_path_factory):
    """the file with heads of `size`'s width against the configuration named `base` (BASES): refused, naming `size`'s wrapper and --model"""
    path, cfg, sd = v2_file(size, tmp_path_factory)
    row, base_cfg = SIZES[size], SIZES[BASES[base]]["base"]
    with pytest.raises(ValueError, match=r"checkpoint has %d heads of dimension %d: .*head dimension 64.*models\.%s / --model %s$"
                       % (cfg["n_heads"], row["hd"], row["wrapper"].__name__, size)):
        weights.load_fair_esm_checkpoint(path, base_cfg)
    d_model, n_layers, n_heads, _ = row["shape"]
    with pytest.raises(ValueError, match=size):
        weights.config_from_checkpoint_v2(dict(encoder_embed_dim=d_model, encoder_layers=n_layers, encoder_attention_heads=n_heads), [], base_cfg)


def check_wrapper_reads_a_v2_file(size, tmp_path_factory):
    path, cfg, sd = v2_file(size, tmp_path_factory)
    row = SIZES[size]
    m = row["wrapper"](checkpoint=path)
    assert m.cfg["arch"] == _lib.PG_ARCH_ESM2 and (m.cfg["d_model"], m.cfg["n_layers"], m.cfg["n_heads"], m.cfg["d_ffn"]) == row["v2_file"]["shape"]
    assert m.alphabet.mask_idx == 32 and len(m.alphabet.all_toks) == 33 and m.alphabet.prepend_bos and m.alphabet.append_eos
    assert models.ESM2_MODELS[size] is row["wrapper"]
    for other in SIZES:
        if other != size:
            with pytest.raises(ValueError, match=size):
                SIZES[other]["wrapper"](checkpoint=path)
    if not weights.find_cached_checkpoint(row["file"] + ".pt"):                         # no file, no opt-in to synthetic weights: refuse
        with pytest.raises(FileNotFoundError, match=row["file"]):
            row["wrapper"]()


def check_command_lines_accept(size):
    from protein_gibbs_sampler_amd import likelihood_esm, pgen_esm, pgen_esm_from_fasta, seq_probs_esm
    for mod in (pgen_esm, pgen_esm_from_fasta, likelihood_esm):
        assert all(mod.model_map[cli] is row["wrapper"] for cli, row in SIZES.items())
        assert mod.build_parser().parse_args(["--model", size]).model == size
    assert pgen_esm.build_parser().parse_args(["--model", size, "--synthetic-weights"]).model == size
    assert seq_probs_esm.model_map[size] is SIZES[size]["wrapper"]
    assert pgen_esm_from_fasta.model_map.keys() >= {"esm1b", size}
    assert pgen_esm.build_parser().parse_args([]).model == "esm1b"                       # defaults unchanged
    assert likelihood_esm.build_parser().parse_args([]).model == "esm1v"
