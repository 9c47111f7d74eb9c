"""numpy references of contact prediction (test infrastructure only -- never imported by the product path).

  esm1b_attentions / esm2_attentions   the per-layer attention probabilities [n_layers][B][H][T][T] float32 of an ESM-1b / ESM-2
                                       model, composed from oracle/esm_forward.py's and tests/_esm2_reference.py's own steps (the
                                       same operations in the same order as their forwards)
  contacts_from_attentions_f64         fair-esm's ContactPredictionHead in float64 with this engine's two conventions (a channel
                                       with a12 == 0 contributes 0; a window entry at a not-live row or column gets logit = bias)
  contacts_from_attentions_f32         the same, restating csrc/contact.hip's fp32 contract operation for operation: S = A + A^T in
                                       one add, wave_sum for a1 and a12, N = S - (a1[i] * a1[j]) / a12, logit = logit + w[c] * N
                                       with c = l * H + h ascending, + bias last
  softmax_probs_f64                    float64 softmax(q . k) of a qkv buffer as pg_contact_dbg_probs reads it
  round_bf16 / round_f16               the operand roundings of the two 16-bit modes (round to nearest even)

A[l][b][h][i][j] is block l's probability of query i over key j; <pad> keys are masked in the softmax, as the forward does.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import _esm2_reference as r2                      # noqa: E402
from oracle import esm_forward as r1              # noqa: E402

F32 = np.float32
F64 = np.float64


# ---- attention probabilities of the two architectures ---------------------------------------------------------------------------
def _probs(q, k, pad):
    """q, k [B][H][T][hd] float32 -> softmax over the keys, float32, <pad> keys masked: the softmax of r1.mha / r2._attention"""
    a = (q @ k.transpose(0, 1, 3, 2)).astype(F32)
    if pad.any():
        a = np.where(pad[:, None, None, :], F32(-np.inf), a)
    a = a - a.max(axis=-1, keepdims=True)
    e = np.exp(a, dtype=F32)
    return (e / e.sum(axis=-1, keepdims=True, dtype=F32)).astype(F32)


def _heads(w, p, h, H, hd):
    B, T, _ = h.shape
    q = r1.linear(h, w[p + "q_proj.weight"], w[p + "q_proj.bias"]) * F32(hd ** -0.5)
    k = r1.linear(h, w[p + "k_proj.weight"], w[p + "k_proj.bias"])
    return q.reshape(B, T, H, hd).transpose(0, 2, 1, 3), k.reshape(B, T, H, hd).transpose(0, 2, 1, 3)


def esm1b_attentions(w, cfg, tokens):
    """cfg: oracle.esm_forward.EsmConfig -> [n_layers][B][H][T][T] float32"""
    x, pad = r1.esm1b_embed(w, cfg, tokens)
    out = []
    for i in range(cfg.n_layers):
        p = "layers.%d." % i
        h = r1.layer_norm(x, w[p + "self_attn_layer_norm.weight"], w[p + "self_attn_layer_norm.bias"])
        q, k = _heads(w, p + "self_attn.", h, cfg.n_heads, cfg.d_model // cfg.n_heads)
        out.append(_probs(q, k, pad))
        x = x + r1.mha(w, p + "self_attn.", cfg, h, pad)
        h = r1.layer_norm(x, w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"])
        h = r1.gelu(r1.linear(h, w[p + "fc1.weight"], w[p + "fc1.bias"]))
        x = (x + r1.linear(h, w[p + "fc2.weight"], w[p + "fc2.bias"])).astype(F32)
    return np.stack(out)


def esm2_attentions(w, cfg, tokens):
    """cfg: _esm2_reference.Esm2Config -> [n_layers][B][H][T][T] float32"""
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
    out = []
    for i in range(cfg.n_layers):
        p = "layers.%d." % i
        h = r2.layer_norm(x, w[p + "self_attn_layer_norm.weight"], w[p + "self_attn_layer_norm.bias"], cfg.eps)
        q, k = _heads(w, p + "self_attn.", h, cfg.n_heads, cfg.head_dim)
        out.append(_probs(r2.rotate(q, cos, sin), r2.rotate(k, cos, sin), pad))
        x = x + r2._attention(w, p + "self_attn.", cfg, h, pad, cos, sin)
        h = r2.layer_norm(x, w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"], cfg.eps)
        h = r2.gelu(r2.linear(h, w[p + "fc1.weight"], w[p + "fc1.bias"]))
        x = (x + r2.linear(h, w[p + "fc2.weight"], w[p + "fc2.bias"])).astype(F32)
    return np.stack(out)


# ---- the head -------------------------------------------------------------------------------------------------------------------
def live_window(tokens, eos, pad):
    """[B][T-2] bool: the window positions t = 1 .. T-2 whose token is neither <eos> nor <pad>"""
    tokens = np.asarray(tokens)
    return ((tokens != eos) & (tokens != pad))[:, 1:-1]


def contacts_from_attentions_f64(A, tokens, w, bias, eos, pad):
    """A [L][B][H][T][T], w [L * H] -> (logits, contacts) float64 [B][T-2][T-2]"""
    A = np.asarray(A, dtype=F64)
    L, B, H, T, _ = A.shape
    live = live_window(tokens, eos, pad)
    m = (live[:, :, None] & live[:, None, :])[None, :, None]
    win = np.where(m, A[:, :, :, 1:-1, 1:-1], 0.0)
    S = win + win.transpose(0, 1, 2, 4, 3)
    a1 = S.sum(axis=-1)
    a12 = a1.sum(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        N = S - a1[..., :, None] * a1[..., None, :] / a12[..., None, None]
    N = np.where(a12[..., None, None] == 0, 0.0, N)
    wv = np.asarray(w, dtype=F64).reshape(L, 1, H, 1, 1)
    logits = (wv * N).sum(axis=(0, 2)) + float(bias)
    return logits, 1.0 / (1.0 + np.exp(-logits))


def wave_sum(x):
    """contact.hip's wave_sum over the last axis, in float32: lane L adds x[L], x[L + 64], ... in ascending order from 0.0f, then the
    butterfly acc = acc + acc_of_lane(L ^ off) for off = 32, 16, 8, 4, 2, 1"""
    x = np.asarray(x, dtype=F32)
    n = x.shape[-1]
    acc = np.zeros(x.shape[:-1] + (64,), dtype=F32)
    for k0 in range(0, n, 64):
        part = x[..., k0:k0 + 64]
        acc[..., :part.shape[-1]] = (acc[..., :part.shape[-1]] + part).astype(F32)
    lanes = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        acc = (acc + acc[..., lanes ^ off]).astype(F32)
    return acc[..., 0]


def fold_layer_f32(P, tokens, w_layer, bias, first, last, logits, eos, pad):
    """One launch_contact_accumulate: P [B][H][T][T] float32, w_layer [H] -> the new logits float32 [B][T-2][T-2]"""
    P = np.asarray(P, dtype=F32)
    B, H, T, _ = P.shape
    live = live_window(tokens, eos, pad)
    m = (live[:, :, None] & live[:, None, :])[:, None]
    win = np.where(m, P[:, :, 1:-1, 1:-1], F32(0)).astype(F32)
    S = (win + win.transpose(0, 1, 3, 2)).astype(F32)
    a1 = wave_sum(S)                   # [B][H][W]
    a12 = wave_sum(a1)                 # [B][H]
    out = np.zeros((B, T - 2, T - 2), dtype=F32) if first else np.array(logits, dtype=F32)
    w_layer = np.asarray(w_layer, dtype=F32)
    for h in range(H):
        for b in range(B):
            if a12[b, h] == 0:
                continue
            prod = (a1[b, h][:, None] * a1[b, h][None, :]).astype(F32)
            N = (S[b, h] - (prod / a12[b, h]).astype(F32)).astype(F32)
            out[b] = (out[b] + (w_layer[h] * N).astype(F32)).astype(F32)
    if last:
        out = (out + F32(bias)).astype(F32)
    return out


def contacts_from_attentions_f32(A, tokens, w, bias, eos, pad):
    """A [L][B][H][T][T] float32, w [L * H] -> logits float32 [B][T-2][T-2], layer by layer as the engine folds them"""
    L, B, H = A.shape[:3]
    w = np.asarray(w, dtype=F32).reshape(L, H)
    logits = None
    for l in range(L):
        logits = fold_layer_f32(A[l], tokens, w[l], bias, l == 0, l == L - 1, logits, eos, pad)
    return logits


# ---- kernel-level reference of the probabilities ----------------------------------------------------------------------------------
def round_bf16(x):
    u = np.ascontiguousarray(x, dtype=F32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return (r.astype(np.uint32) << 16).view(F32).reshape(np.shape(x))


def round_f16(x):
    return np.asarray(x, dtype=F32).astype(np.float16).astype(F32)


def scores_f64(qkv, n_seq, T, H, hd):
    """qkv [n_seq * T][3 * H * hd] -> (scores [n_seq][H][T][T] float64, sum_d |q_d k_d| of the same shape)"""
    x = np.asarray(qkv, dtype=F64).reshape(n_seq, T, 3, H, hd).transpose(2, 0, 3, 1, 4)
    return x[0] @ x[1].transpose(0, 1, 3, 2), np.abs(x[0]) @ np.abs(x[1]).transpose(0, 1, 3, 2)


def softmax_probs_f64(qkv, n_seq, T, H, hd, pad=None):
    """-> (P [n_seq][H][T][T] float64 with exact zeros at masked keys, scores, sum |q k|)"""
    s, mag = scores_f64(qkv, n_seq, T, H, hd)
    a = s if pad is None else np.where(np.asarray(pad, bool)[:, None, None, :], -np.inf, s)
    a = a - a.max(axis=-1, keepdims=True)
    e = np.exp(a)
    return e / e.sum(axis=-1, keepdims=True), s, mag
