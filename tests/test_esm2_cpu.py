"""ESM-2 on the host: the numpy reference against an independent implementation (HuggingFace rotary ESM, stored logits), the
rotate-half identities, the v2 checkpoint reader and, as shared bodies of tests/_esm2_cpu_common.py, the rotary frequencies against
torch's and the command-line model maps.  Needs no GPU."""
import json
import os

import numpy as np
import pytest

import _esm2_cpu_common as common
import _esm2_reference as ref
from protein_gibbs_sampler_amd import _lib, weights

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def hf_case(name):
    """-> (config, weights, tokens, HuggingFace logits) of tests/golden/esm2_hf_<name>.npz (make_golden_esm2.py)."""
    z = np.load(os.path.join(GOLDEN, "esm2_hf_%s.npz" % name))
    cfg = weights.make_config(weights.ESM2_T33_CONFIG, **json.loads(str(z["cfg"])))
    w = weights.synthetic_state_dict(cfg, seed=int(z["seed"]), std=float(z["std"]), embed_std=float(z["embed_std"]),
                                     ln_jitter=float(z["ln_jitter"]))
    return cfg, w, z["tokens"].astype(np.int64), z["logits"]


@pytest.mark.parametrize("name", ["small", "mid"])
def test_reference_reproduces_huggingface_rotary_esm(name):
    cfg, w, tok, want = hf_case(name)
    assert (tok != cfg["pad_idx"]).all() and (tok == cfg["mask_idx"]).any()
    got = ref.esm2_forward(w, ref.Esm2Config.of(cfg), tok)
    assert np.abs(got - want).max() < 2e-4


def test_config_and_tensor_names():
    cfg = weights.ESM2_T33_CONFIG
    assert (cfg["arch"], cfg["d_model"], cfg["n_layers"], cfg["n_heads"], cfg["d_ffn"], cfg["vocab"]) == (_lib.PG_ARCH_ESM2, 1280, 33, 20, 5120, 33)
    assert (cfg["pad_idx"], cfg["mask_idx"], cfg["cls_idx"], cfg["eos_idx"], cfg["token_dropout"], cfg["max_positions"]) == (1, 32, 0, 2, 1, 1024)
    small = weights.make_config(cfg, d_model=128, n_layers=2, d_ffn=256)
    names = set(weights.tensor_shapes(small))
    assert not any(n.startswith("embed_positions") or n.startswith("emb_layer_norm_before") for n in names)
    assert {"embed_tokens.weight", "emb_layer_norm_after.weight", "lm_head.dense.weight", "layers.1.self_attn.q_proj.bias",
            "layers.0.fc2.weight"} <= names
    assert set(weights.synthetic_state_dict(small, seed=1)) == names


def test_rotation_preserves_pair_norms_and_is_relative():
    rng = np.random.default_rng(0)
    T = 300
    cos, sin = ref.cos_sin(T)
    u = rng.standard_normal((T, 64)).astype(np.float32)
    r = ref.rotate(u, cos, sin).astype(np.float64)
    n0 = u[:, :32].astype(np.float64) ** 2 + u[:, 32:].astype(np.float64) ** 2
    n1 = r[:, :32] ** 2 + r[:, 32:] ** 2
    assert np.abs(n1 - n0).max() < 1e-5 * n0.max()                  # every (i, i + 32) pair keeps its length
    assert np.array_equal(r[0], u[0].astype(np.float64))            # position 0 (<cls>) is the identity
    # q'(t) . k'(s) depends on t - s only: the same two vectors placed at (t, s) and (t + 40, s + 40)
    q, k = rng.standard_normal(64).astype(np.float32), rng.standard_normal(64).astype(np.float32)
    qs = ref.rotate(np.tile(q, (T, 1)), cos, sin).astype(np.float64)
    ks = ref.rotate(np.tile(k, (T, 1)), cos, sin).astype(np.float64)
    for t, s in ((5, 3), (17, 60), (200, 100)):
        assert abs(qs[t] @ ks[s] - qs[t + 40] @ ks[s + 40]) < 2e-4
    assert abs(qs[5] @ ks[3] - qs[5] @ ks[4]) > 1e-3                # ... and does depend on it


def test_rotate_qkv_rows_leaves_v_alone():
    rng = np.random.default_rng(1)
    B, T, H = 2, 7, 3
    x = rng.standard_normal((B * T, 3 * H * 64)).astype(np.float32)
    y = ref.rotate_qkv_rows(x, B, T, H)
    assert np.array_equal(y[:, 2 * H * 64:], x[:, 2 * H * 64:])
    assert np.array_equal(y[0], x[0]) and np.array_equal(y[T], x[T])         # t = 0 rows
    assert not np.array_equal(y[1, :2 * H * 64], x[1, :2 * H * 64])


# ---- the v2 checkpoint layout -----------------------------------------------------------------------------------------------------
def _small():
    cfg = weights.make_config(weights.ESM2_T33_CONFIG, d_model=128, n_layers=2, d_ffn=512, max_positions=40)
    return cfg, weights.synthetic_state_dict(cfg, seed=3, embed_std=0.3)


@pytest.mark.parametrize("namespace", [True, False])
def test_v2_checkpoint_round_trip(tmp_path, namespace):
    torch = pytest.importorskip("torch")
    cfg, sd = _small()
    blob = weights.to_fair_esm_checkpoint_v2(sd, cfg, namespace=namespace)
    assert "args" not in blob and "encoder.sentence_encoder.layers.1.self_attn.rot_emb.inv_freq" in blob["model"]
    assert "encoder.lm_head.weight" in blob["model"] and "encoder.sentence_encoder.embed_tokens.weight" in blob["model"]
    blob["model"]["contact_head.regression.weight"] = torch.zeros(1, 2 * cfg["n_heads"])
    blob["model"]["contact_head.regression.bias"] = torch.zeros(1)
    path = tmp_path / "esm2.pt"
    torch.save(blob, path)
    base = weights.make_config(weights.ESM2_T33_CONFIG, max_positions=40)          # 33 x 1280: sizes must come from the file
    got, cfg2 = weights.load_fair_esm_checkpoint(str(path), base, return_config=True)
    assert (cfg2["d_model"], cfg2["n_layers"], cfg2["n_heads"], cfg2["d_ffn"], cfg2["token_dropout"]) == (128, 2, 2, 512, 1)
    assert set(got) == set(sd) and all(np.array_equal(got[k], sd[k]) for k in sd)
    assert np.abs(got["embed_tokens.weight"][cfg["mask_idx"]]).max() > 0           # ESM-2: the <mask> row is NOT zeroed on load


def test_v2_checkpoint_errors(tmp_path):
    torch = pytest.importorskip("torch")
    cfg, sd = _small()
    path = tmp_path / "f.pt"

    blob = weights.to_fair_esm_checkpoint_v2(sd, cfg)
    blob["model"]["encoder.sentence_encoder.layers.0.self_attn.rot_emb.inv_freq"] = torch.from_numpy(weights.rotary_inv_freq() * np.float32(1.001))
    torch.save(blob, path)
    with pytest.raises(ValueError, match="inv_freq"):
        weights.load_fair_esm_checkpoint(str(path), cfg)

    blob = weights.to_fair_esm_checkpoint_v2(sd, cfg)
    blob["cfg"]["model"].encoder_attention_heads = 4                               # heads of 32, as esm2_t30_150M
    torch.save(blob, path)
    with pytest.raises(ValueError, match="head dimension 64"):
        weights.load_fair_esm_checkpoint(str(path), cfg)

    blob = weights.to_fair_esm_checkpoint_v2(sd, cfg)
    blob["cfg"]["model"].encoder_embed_dim, blob["cfg"]["model"].encoder_attention_heads = 2560, 40      # esm2_t36_3B
    torch.save(blob, path)
    with pytest.raises(ValueError, match="d_model 2560 > 2048"):
        weights.load_fair_esm_checkpoint(str(path), cfg)

    blob = weights.to_fair_esm_checkpoint_v2(sd, cfg)
    blob["model"]["encoder.lm_head.weight"] = blob["model"]["encoder.lm_head.weight"] + 1
    torch.save(blob, path)
    with pytest.raises(ValueError, match="untied"):
        weights.load_fair_esm_checkpoint(str(path), cfg)

    # a v2 file is not an ESM-1b model, and a v1 file is not an ESM-2 one
    torch.save(weights.to_fair_esm_checkpoint_v2(sd, cfg), path)
    with pytest.raises(ValueError, match="v2 layout"):
        weights.load_fair_esm_checkpoint(str(path), weights.make_config(weights.ESM1B_CONFIG, d_model=128, n_layers=2, d_ffn=512, max_positions=40))
    torch.save({"args": {"arch": "roberta_large"}, "model": {}}, path)
    with pytest.raises(ValueError, match="v1 layout"):
        weights.load_fair_esm_checkpoint(str(path), cfg)


def test_models_esm2_reads_a_v2_file_without_a_gpu(tmp_path):
    torch = pytest.importorskip("torch")
    from protein_gibbs_sampler_amd import models
    cfg, sd = _small()
    path = tmp_path / "esm2.pt"
    torch.save(weights.to_fair_esm_checkpoint_v2(sd, cfg), path)
    m = models.ESM2(checkpoint=str(path))
    assert m.cfg["arch"] == _lib.PG_ARCH_ESM2 and m.cfg["d_model"] == 128 and m.alphabet.mask_idx == 32 and len(m.alphabet.all_toks) == 33
    assert m.alphabet.prepend_bos and m.alphabet.append_eos
    if not weights.find_cached_checkpoint("esm2_t33_650M_UR50D.pt"):               # no file, no opt-in to synthetic weights: refuse
        with pytest.raises(FileNotFoundError, match="esm2_t33_650M_UR50D"):
            models.ESM2()


# ---- the shared bodies (tests/_esm2_cpu_common.py) at this size -------------------------------------------------------------------------
def test_inv_freq_is_torchs():
    common.check_inv_freq_is_torchs("esm2")


def test_command_lines_accept_esm2():
    common.check_command_lines_accept("esm2")
