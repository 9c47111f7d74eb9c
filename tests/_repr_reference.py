"""fp32 numpy references of the sequence representations (test infrastructure only -- never imported by the product path).

  sequential_mean   the pool arithmetic contract of pg_esm_forward_representations / repr.hip, in np.float32:
                    acc = 0; acc = acc + x[t] for t ascending; acc / float32(count); a count of 0 gives zeros
  esm2_layers       the n + 1 hidden states of an ESM-2 model, composed from tests/_esm2_reference.py's own steps (the same
                    operations in the same order as esm2_forward, so layer n pushed through lm_head equals its logits exactly)
  esm2_lm_head      that head

Layer numbering (fair-esm's repr_layers, HuggingFace's hidden_states): 0 = the embedding output, l = the residual stream after block
l, n = the stream after block n through emb_layer_norm_after.
"""
import numpy as np

import _esm2_reference as r2

F32 = np.float32


def sequential_mean(x, begin, count):
    """x [T][d] float32 -> the mean of rows begin .. begin + count - 1, summed one row at a time in float32."""
    x = np.asarray(x, dtype=F32)
    acc = np.zeros(x.shape[1:], dtype=F32)
    if count == 0:
        return acc
    for t in range(begin, begin + count):
        acc = (acc + x[t]).astype(F32)
    return (acc / F32(count)).astype(F32)


def pooled(rows, pools):
    """rows [B][T][d], pools [n_pools][B][2] = (begin, count) -> [n_pools][B][d] of sequential means."""
    pools = np.asarray(pools)
    return np.stack([np.stack([sequential_mean(rows[b], int(pools[p, b, 0]), int(pools[p, b, 1])) for b in range(rows.shape[0])])
                     for p in range(pools.shape[0])])


def esm2_layers(w, cfg, tokens):
    """tokens [B][T] -> list of n_layers + 1 float32 arrays [B][T][d]."""
    tokens = np.asarray(tokens)
    B, T = tokens.shape
    pad = tokens == cfg.pad_idx
    x = w["embed_tokens.weight"][tokens].astype(F32)
    if cfg.token_dropout:
        is_mask = tokens == cfg.mask_idx
        x = np.where(is_mask[..., None], F32(0), x)
        ratio = is_mask.sum(axis=1).astype(F32) / (~pad).sum(axis=1).astype(F32)
        x = (x * (F32(1 - 0.15 * 0.8) / (F32(1) - ratio)).astype(F32)[:, None, None]).astype(F32)
    x = np.where(pad[..., None], F32(0), x).astype(F32)
    cos, sin = r2.cos_sin(T, cfg.head_dim)
    states = [x]
    for i in range(cfg.n_layers):
        p = "layers.%d." % i
        h = r2.layer_norm(x, w[p + "self_attn_layer_norm.weight"], w[p + "self_attn_layer_norm.bias"], cfg.eps)
        x = x + r2._attention(w, p + "self_attn.", cfg, h, pad, cos, sin)
        h = r2.layer_norm(x, w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"], cfg.eps)
        h = r2.gelu(r2.linear(h, w[p + "fc1.weight"], w[p + "fc1.bias"]))
        x = (x + r2.linear(h, w[p + "fc2.weight"], w[p + "fc2.bias"])).astype(F32)
        states.append(x)
    states[-1] = r2.layer_norm(x, w["emb_layer_norm_after.weight"], w["emb_layer_norm_after.bias"], cfg.eps)
    return states


def esm2_lm_head(w, cfg, x):
    """x [..., d] = layer n -> logits [..., V] float32: the tail of esm2_forward."""
    g = r2.gelu(r2.linear(x, w["lm_head.dense.weight"], w["lm_head.dense.bias"]))
    g = r2.layer_norm(g, w["lm_head.layer_norm.weight"], w["lm_head.layer_norm.bias"], cfg.eps)
    return (g @ w["embed_tokens.weight"].T + w["lm_head.bias"]).astype(F32)
