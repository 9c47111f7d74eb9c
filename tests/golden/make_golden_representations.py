"""Regenerates tests/golden/esm_hf_repr.npz and esm2_hf_repr.npz: the hidden states (output_hidden_states=True) of HuggingFace
`transformers.EsmForMaskedLM` -- an implementation of both architectures independent of this repository -- on seeded synthetic
weights: ESM-1b (absolute positions, emb_layer_norm_before) and ESM-2 (rotary positions), 3 layers x 128 with two heads of 64, tokens
[3, 27] with a few <mask>.  The state-dict mapping is that of make_golden.py::gen_hf and make_golden_esm2.py.

Layer numbering is fair-esm's: hidden_states[0] = the embedding output, [l] = the stream after block l, [n] = after block n through
emb_layer_norm_after.  Each file holds, for all n + 1 layers, the mean over every sequence's residues (tokens 1 .. T - 2, taken in
float64) and the per-token states of a seeded subset of the 81 token rows -- all rows would be three times the largest fixture here.
At record time each layer is cross-checked against this repository's fp32 references (oracle.esm_forward.esm1b_trunk's return_layers,
tests/_repr_reference.esm2_layers): max |difference| < 2e-4, the existing generators' bound.

Needs `transformers` (the test suite does not: it reads the .npz files, which hold tokens, states and the recipe of the weights).

    python tests/golden/make_golden_representations.py [--out DIR]
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

SHAPE = dict(d_model=128, n_layers=3, n_heads=2, d_ffn=512, max_pos=64)
B, T, N_ROWS = 3, 27, 20
# file -> (rotary, seed of the weights, std, embed_std, ln_jitter, seed of the tokens and of the row subset)
CASES = {"esm_hf_repr": (False, 41, 0.05, 0.3, 0.1, 411), "esm2_hf_repr": (True, 42, 0.05, 0.3, 0.1, 421)}


def tokens_for(seed):
    rng = np.random.default_rng(seed)
    tok = rng.integers(4, 24, size=(B, T))
    tok[:, 0] = 0
    tok[:, -1] = 2
    for b in range(B):
        tok[b, rng.choice(np.arange(1, T - 1), size=b + 1, replace=False)] = 32
    rows = np.sort(rng.choice(B * T, size=N_ROWS, replace=False))
    return tok, rows


def hf_state_dict(w, n_layers, rotary):
    import torch
    T_ = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    sd = {"esm.embeddings.word_embeddings.weight": T_(w["embed_tokens.weight"])}
    if not rotary:
        sd["esm.embeddings.position_embeddings.weight"] = T_(w["embed_positions.weight"])
        sd["esm.embeddings.layer_norm.weight"] = T_(w["emb_layer_norm_before.weight"])
        sd["esm.embeddings.layer_norm.bias"] = T_(w["emb_layer_norm_before.bias"])
    for i in range(n_layers):
        p, q = "layers.%d." % i, "esm.encoder.layer.%d." % i
        for a, b in (("self_attn.q_proj", "attention.self.query"), ("self_attn.k_proj", "attention.self.key"),
                     ("self_attn.v_proj", "attention.self.value"), ("self_attn.out_proj", "attention.output.dense"),
                     ("self_attn_layer_norm", "attention.LayerNorm"), ("fc1", "intermediate.dense"), ("fc2", "output.dense"),
                     ("final_layer_norm", "LayerNorm")):
            sd[q + b + ".weight"] = T_(w[p + a + ".weight"])
            sd[q + b + ".bias"] = T_(w[p + a + ".bias"])
    for a, b in (("emb_layer_norm_after", "esm.encoder.emb_layer_norm_after"), ("lm_head.dense", "lm_head.dense"),
                 ("lm_head.layer_norm", "lm_head.layer_norm")):
        sd[b + ".weight"] = T_(w[a + ".weight"])
        sd[b + ".bias"] = T_(w[a + ".bias"])
    sd["lm_head.bias"] = T_(w["lm_head.bias"])
    sd["lm_head.decoder.weight"] = T_(w["embed_tokens.weight"])
    return sd


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=HERE, help="directory to write the two .npz files into")
    args = ap.parse_args()
    import torch
    from transformers import EsmConfig as HC, EsmForMaskedLM

    import _esm2_reference as ref2
    import _repr_reference as rr
    from oracle.esm_forward import EsmConfig, esm1b_trunk, synthetic_esm_weights
    from protein_gibbs_sampler_amd import weights

    for name, (rotary, seed, std, estd, jit, tok_seed) in CASES.items():
        n = SHAPE["n_layers"]
        if rotary:
            over = dict(d_model=SHAPE["d_model"], n_layers=n, d_ffn=SHAPE["d_ffn"], max_positions=SHAPE["max_pos"])
            cfg = weights.make_config(weights.ESM2_T33_CONFIG, **over)
            assert cfg["n_heads"] == SHAPE["n_heads"]
            w = weights.synthetic_state_dict(cfg, seed=seed, std=std, embed_std=estd, ln_jitter=jit)
            recipe = over
        else:
            ocfg = EsmConfig(**SHAPE)
            w = synthetic_esm_weights(ocfg, seed=seed, std=std, embed_std=estd, ln_jitter=jit)
            recipe = SHAPE
        hc = HC(vocab_size=33, hidden_size=SHAPE["d_model"], num_hidden_layers=n, num_attention_heads=SHAPE["n_heads"],
                intermediate_size=SHAPE["d_ffn"], max_position_embeddings=SHAPE["max_pos"] + 2,
                position_embedding_type="rotary" if rotary else "absolute", emb_layer_norm_before=not rotary, token_dropout=True,
                mask_token_id=32, pad_token_id=1, layer_norm_eps=1e-5, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        m = EsmForMaskedLM(hc).eval()
        missing, unexpected = m.load_state_dict(hf_state_dict(w, n, rotary), strict=False)
        missing = [k for k in missing if "contact_head" not in k and "position_ids" not in k and "inv_freq" not in k]
        assert not missing and not unexpected, (missing, unexpected)
        tok, rows = tokens_for(tok_seed)
        with torch.no_grad():
            out = m(input_ids=torch.from_numpy(tok), attention_mask=None, output_hidden_states=True)
        states = np.stack([h.numpy() for h in out.hidden_states]).astype(np.float32)             # [n + 1][B][T][d]
        assert states.shape == (n + 1, B, T, SHAPE["d_model"])
        if rotary:
            mine = rr.esm2_layers(w, ref2.Esm2Config.of(cfg), tok)
        else:
            x, mine = esm1b_trunk(w, ocfg, tok, return_layers=True)
            mine[-1] = x
        for l in range(n + 1):
            err = float(np.abs(mine[l] - states[l]).max())
            print("HF cross-check %s layer %d: max|reference - HF| = %.3e  (state std %.3f)" % (name, l, err, states[l].std()))
            assert err < 2e-4, (name, l, err)
        means = states[:, :, 1:T - 1].astype(np.float64).mean(axis=2).astype(np.float32)          # [n + 1][B][d]
        per_token = states.reshape(n + 1, B * T, -1)[:, rows]                                    # [n + 1][N_ROWS][d]
        np.savez_compressed(os.path.join(args.out, name + ".npz"), tokens=tok.astype(np.int32), rows=rows.astype(np.int32), means=means,
                            per_token=per_token, cfg=json.dumps(recipe), seed=seed, std=std, embed_std=estd, ln_jitter=jit)


if __name__ == "__main__":
    main()
