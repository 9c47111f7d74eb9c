"""Regenerates tests/golden/esm_hf_contacts.npz and esm2_hf_contacts.npz: the contact probabilities (predict_contacts) and attention
maps (output_attentions=True) of HuggingFace `transformers.EsmForMaskedLM` -- an implementation of both architectures independent of
this repository -- on seeded synthetic weights and a seeded contact regression.  The recipe is make_golden_representations.py's
(3 layers x 128, two heads of 64, tokens [3, 27] with a few <mask>), plus one right-padded ragged batch [3, 27] with rows of 27, 19 and
11 tokens (<eos> before the <pad> tail, attention_mask given).

Each file holds, for both batches: the tokens, the regression (weight [n_layers * n_heads], bias), the contact probabilities
[B][T-2][T-2] and the attention rows of a seeded subset of (layer, sequence, head, query) quadruples -- all maps would be six times
the largest fixture here.  In the ragged batch HuggingFace's own convention differs from this engine's at the window entries whose row
or column is <eos> or <pad>: HuggingFace leaves the APC of a zeroed row in place, the engine writes logit = bias; the file also holds
the live mask so a test compares the live block.

At record time the numpy reference (tests/_contact_reference.py) is cross-checked against HuggingFace: attention probabilities must
agree below 2e-4 (the existing generators' bound); the worst contact-logit difference is printed and stored (`logit_err`).

Needs `transformers` (the test suite does not: it reads the .npz files).

    python tests/golden/make_golden_contacts.py [--out DIR]
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
sys.path.insert(0, HERE)

from make_golden_representations import SHAPE, B, T, hf_state_dict, tokens_for      # noqa: E402

N_ROWS = 24
RAGGED_LENGTHS = (27, 19, 11)
# file -> (rotary, seed of the weights, std, embed_std, ln_jitter, seed of the tokens / the row subset / the head)
CASES = {"esm_hf_contacts": (False, 51, 0.05, 0.3, 0.1, 511), "esm2_hf_contacts": (True, 52, 0.05, 0.3, 0.1, 521)}
HEAD_STD, HEAD_BIAS = 40.0, -0.5


def ragged(tok):
    """the batch right-padded to RAGGED_LENGTHS: <eos> at the end of every row's own length, <pad> behind it"""
    out = np.array(tok)
    for b, n in enumerate(RAGGED_LENGTHS):
        out[b, n - 1] = 2
        out[b, n:] = 1
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", default=HERE, help="directory to write the two .npz files into")
    args = ap.parse_args()
    import torch
    from transformers import EsmConfig as HC, EsmForMaskedLM

    import _contact_reference as cr
    import _esm2_reference as ref2
    from oracle.esm_forward import EsmConfig, synthetic_esm_weights
    from protein_gibbs_sampler_amd import weights

    for name, (rotary, seed, std, estd, jit, tok_seed) in CASES.items():
        n, H = SHAPE["n_layers"], SHAPE["n_heads"]
        if rotary:
            over = dict(d_model=SHAPE["d_model"], n_layers=n, d_ffn=SHAPE["d_ffn"], max_positions=SHAPE["max_pos"])
            cfg = weights.make_config(weights.ESM2_T33_CONFIG, **over)
            w = weights.synthetic_state_dict(cfg, seed=seed, std=std, embed_std=estd, ln_jitter=jit)
            recipe = over
        else:
            ocfg = EsmConfig(**SHAPE)
            w = synthetic_esm_weights(ocfg, seed=seed, std=std, embed_std=estd, ln_jitter=jit)
            recipe = SHAPE
        rng = np.random.default_rng(tok_seed)
        head_w = (HEAD_STD * rng.standard_normal(n * H)).astype(np.float32)
        hc = HC(vocab_size=33, hidden_size=SHAPE["d_model"], num_hidden_layers=n, num_attention_heads=H,
                intermediate_size=SHAPE["d_ffn"], max_position_embeddings=SHAPE["max_pos"] + 2,
                position_embedding_type="rotary" if rotary else "absolute", emb_layer_norm_before=not rotary, token_dropout=True,
                mask_token_id=32, pad_token_id=1, layer_norm_eps=1e-5, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
        try:
            m = EsmForMaskedLM(HC(**{**hc.to_dict(), "attn_implementation": "eager"})).eval()
        except Exception:
            m = EsmForMaskedLM(hc).eval()
        sd = hf_state_dict(w, n, rotary)
        sd["esm.contact_head.regression.weight"] = torch.from_numpy(head_w[None])
        sd["esm.contact_head.regression.bias"] = torch.tensor([HEAD_BIAS], dtype=torch.float32)
        missing, unexpected = m.load_state_dict(sd, strict=False)
        missing = [k for k in missing if "position_ids" not in k and "inv_freq" not in k]
        assert not missing and not unexpected, (missing, unexpected)
        tok, _ = tokens_for(tok_seed)
        save = dict(head_w=head_w, head_b=np.float32(HEAD_BIAS), cfg=json.dumps(recipe), seed=seed, std=std, embed_std=estd, ln_jitter=jit)
        for tag, t in (("full", tok), ("ragged", ragged(tok))):
            ids = torch.from_numpy(t)
            mask = torch.from_numpy((t != 1).astype(np.int64))
            with torch.no_grad():
                out = m(input_ids=ids, attention_mask=mask, output_attentions=True)
                con = m.predict_contacts(ids, mask).numpy().astype(np.float32)
            assert out.attentions is not None and len(out.attentions) == n, "the model returned no attention maps"
            att = np.stack([a.numpy() for a in out.attentions]).astype(np.float32)           # [n][B][H][T][T]
            assert att.shape == (n, B, H, T, T) and con.shape == (B, T - 2, T - 2)
            mine = cr.esm2_attentions(w, ref2.Esm2Config.of(cfg), t) if rotary else cr.esm1b_attentions(w, ocfg, t)
            real_q = (t != 1)[None, :, None, :, None]                                       # rows of <pad> queries: whatever each side does
            a_err = float(np.abs(np.where(real_q, mine - att, 0)).max())
            print("HF cross-check %s %s: attention max|reference - HF| = %.3e" % (name, tag, a_err))
            assert a_err < 2e-4, (name, tag, a_err)
            lg64, con64 = cr.contacts_from_attentions_f64(mine, t, head_w, HEAD_BIAS, 2, 1)
            live = cr.live_window(t, 2, 1)
            block = live[:, :, None] & live[:, None, :]
            hf_logit = np.log(con.astype(np.float64)) - np.log1p(-con.astype(np.float64))
            l_err = float(np.abs(np.where(block, lg64 - hf_logit, 0)).max())
            print("HF cross-check %s %s: contact logit max|reference - HF| over the live block = %.3e  (logit std %.2f)"
                  % (name, tag, l_err, lg64[block].std()))
            pick = np.sort(rng.choice(n * B * H * T, size=N_ROWS, replace=False))
            save.update({tag + "_tokens": t.astype(np.int32), tag + "_contacts": con, tag + "_live": block,
                         tag + "_rows": pick.astype(np.int32), tag + "_attn_rows": att.reshape(n * B * H * T, T)[pick],
                         tag + "_logit_err": l_err, tag + "_attn_err": a_err})
        np.savez_compressed(os.path.join(args.out, name + ".npz"), **save)


if __name__ == "__main__":
    main()
