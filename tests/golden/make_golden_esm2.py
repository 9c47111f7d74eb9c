"""Regenerates tests/golden/esm2_hf_*.npz: logits of HuggingFace `transformers.EsmForMaskedLM` with ROTARY positions -- an implementation
of the ESM-2 architecture independent of this repository -- on seeded synthetic weights, cross-checked against the numpy reference
tests/_esm2_reference.py at record time (max |difference| < 2e-4).  Modelled on gen_hf of make_golden.py.  One fixture per head width
beside the two at 64: hd32 (the esm2_t30_150M_UR50D head width: 6 layers x 640 with 20 heads), hd128 (esm2_t48_15B_UR50D's: 6 layers x
512 with 4 heads), hd16 (esm2_t6_8M_UR50D itself in shape: 6 layers x 320 with 20 heads) and hd24 (esm2_t12_35M_UR50D itself in shape:
12 layers x 480 with 20 heads; the engine runs this model embedded in slots of 32).

Needs `transformers` (the test suite does not: it only reads the .npz files, which hold the tokens, the logits and the recipe of the
weights -- weights.synthetic_state_dict(cfg, seed, std, embed_std, ln_jitter)).  Token batches are UNPADDED: HuggingFace derives
rotary positions for padded input its own way, so padding is pinned by the contract and the numpy reference, not by these files.

    python tests/golden/make_golden_esm2.py [--out DIR] [NAME ...]         (no name: every fixture; DIR: this directory)
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

# name -> (base configuration of weights, its overrides, B, L, seed of the weights, std, embed_std, ln_jitter, seed of the tokens)
CASES = {
    "small": ("ESM2_T33_CONFIG", dict(d_model=256, n_layers=4, d_ffn=1024, max_positions=128), 3, 64, 21, 0.05, 0.3, 0.1, 301),
    "mid": ("ESM2_T33_CONFIG", dict(d_model=640, n_layers=6, d_ffn=2560, max_positions=512), 2, 256, 22, 0.03, 0.3, 0.1, 302),
    "hd32": ("ESM2_T30_CONFIG", dict(n_layers=6, max_positions=512), 2, 256, 23, 0.03, 0.3, 0.1, 303),
    "hd128": ("ESM2_T48_CONFIG", dict(n_layers=6, d_model=512, d_ffn=2048, max_positions=512), 2, 256, 29, 0.035, 0.3, 0.1, 1283),
    "hd16": ("ESM2_T6_CONFIG", dict(n_layers=6, max_positions=512), 2, 256, 29, 0.03, 0.3, 0.1, 161),
    "hd24": ("ESM2_T12_CONFIG", dict(n_layers=12, max_positions=512), 2, 256, 31, 0.03, 0.3, 0.1, 241),
}


def tokens_for(name, B, L):
    rng = np.random.default_rng(CASES[name][-1])
    tok = rng.integers(4, 24, size=(B, L + 2))
    tok[:, 0] = 0
    tok[:, -1] = 2
    for b in range(B):
        pos = rng.choice(np.arange(1, L + 1), size=max(1, (b + 1) * L // 10), replace=False)
        tok[b, pos] = 32
    return tok


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("names", nargs="*", help="the fixtures to write, of %s (default: all)" % ", ".join(CASES))
    ap.add_argument("--out", default=HERE, help="directory to write esm2_hf_NAME.npz into")
    args = ap.parse_args()
    import torch
    from transformers import EsmConfig as HC, EsmForMaskedLM

    import _esm2_reference as ref
    from protein_gibbs_sampler_amd import weights

    for name in args.names or CASES:
        base, over, B, L, seed, std, estd, jit, _ = CASES[name]
        cfg = weights.make_config(getattr(weights, base), **over)
        assert weights.head_dim_of(cfg) == weights.head_dim_of(getattr(weights, base))       # the width the fixture is named for
        w = weights.synthetic_state_dict(cfg, seed=seed, std=std, embed_std=estd, ln_jitter=jit)
        hc = HC(vocab_size=33, hidden_size=cfg["d_model"], num_hidden_layers=cfg["n_layers"], num_attention_heads=cfg["n_heads"],
                intermediate_size=cfg["d_ffn"], max_position_embeddings=cfg["max_positions"] + 2, position_embedding_type="rotary",
                emb_layer_norm_before=False, token_dropout=True, mask_token_id=32, pad_token_id=1, layer_norm_eps=1e-5,
                hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        m = EsmForMaskedLM(hc).eval()
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
        sd = {"esm.embeddings.word_embeddings.weight": T(w["embed_tokens.weight"])}
        for i in range(cfg["n_layers"]):
            p, q = "layers.%d." % i, "esm.encoder.layer.%d." % i
            for a, b in (("q_proj", "attention.self.query"), ("k_proj", "attention.self.key"), ("v_proj", "attention.self.value"),
                         ("out_proj", "attention.output.dense")):
                sd[q + b + ".weight"] = T(w[p + "self_attn." + a + ".weight"])
                sd[q + b + ".bias"] = T(w[p + "self_attn." + a + ".bias"])
            for a, b in (("self_attn_layer_norm", "attention.LayerNorm"), ("fc1", "intermediate.dense"), ("fc2", "output.dense"),
                         ("final_layer_norm", "LayerNorm")):
                sd[q + b + ".weight"] = T(w[p + a + ".weight"])
                sd[q + b + ".bias"] = T(w[p + a + ".bias"])
        for a, b in (("emb_layer_norm_after", "esm.encoder.emb_layer_norm_after"), ("lm_head.dense", "lm_head.dense"),
                     ("lm_head.layer_norm", "lm_head.layer_norm")):
            sd[b + ".weight"] = T(w[a + ".weight"])
            sd[b + ".bias"] = T(w[a + ".bias"])
        sd["lm_head.bias"] = T(w["lm_head.bias"])
        sd["lm_head.decoder.weight"] = T(w["embed_tokens.weight"])
        missing, unexpected = m.load_state_dict(sd, strict=False)
        missing = [k for k in missing if "contact_head" not in k and "position_ids" not in k and "inv_freq" not in k]
        assert not missing and not unexpected, (missing, unexpected)
        tok = tokens_for(name, B, L)
        with torch.no_grad():
            hf_logits = m(input_ids=torch.from_numpy(tok), attention_mask=None).logits.numpy()
        mine = ref.esm2_forward(w, ref.Esm2Config.of(cfg), tok)
        err = float(np.abs(mine - hf_logits).max())
        print("HF cross-check %s: max|reference - HF| = %.3e  (logit std %.3f)" % (name, err, hf_logits.std()))
        assert err < 2e-4, err
        np.savez_compressed(os.path.join(args.out, "esm2_hf_%s.npz" % name), tokens=tok.astype(np.int32),
                            logits=hf_logits.astype(np.float32), cfg=json.dumps(over), seed=seed, std=std, embed_std=estd, ln_jitter=jit)


if __name__ == "__main__":
    main()
