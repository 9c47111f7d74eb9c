"""numpy references of the MSA Transformer's contact prediction (test infrastructure only -- never imported by the product path, never
a rerun of the engine).

  msa_row_attentions             the oracle's MSA trunk (oracle/msa_forward.py), restated only as far as needed to collect every block's
                                 tied row-attention map: -> (A [n_layers][B][H][C][C] float32, the trunk's output).  The map is
                                 row_attention's own q, k, scale, <pad> handling and softmax; the stream is advanced by the oracle's
                                 own row_attention / column_attention
  row_probs_f64                  float64 scores and softmax of a given qkv buffer (16-bit-rounded, or fp32 operands) with the ragged
                                 semantics, as pg_msa_contact_dbg_probs reads it: -> (P, scores, sum |q k| scaled)
  fold_layer_f32                 csrc/contact.hip's fp32 contract with a window of W = T - 1 - tail positions and the live mask of a given
                                 token row, operation for operation (tail = 0, row 0 of the MSA: the MSA Transformer's; tail = 1:
                                 tests/_contact_reference.py's)
  row_contacts_f32 / _f64        all layers folded: the fp32 order, and the float64 form of the same contract

Conventions (include/pgibbs.h): only the <cls> row and column are cut (window t = 1 .. C-1), channel c = l * H + h, a channel with
a12 == 0 contributes 0, a window entry whose row or column is not live (row 0's token there is <pad>) gets logit = bias exactly.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from _contact_reference import F32, F64, round_bf16, round_f16, wave_sum      # noqa: E402,F401
from oracle import msa_forward as M                                          # noqa: E402
from oracle.esm_forward import layer_norm, linear, gelu, softmax_lastdim      # noqa: E402


# ---- the trunk, collecting the row maps -------------------------------------------------------------------------------------------
def row_map(w, p, cfg, h, pad):
    """oracle.msa_forward.row_attention up to its softmax: [B][H][C][C] float32"""
    B, R, C, d = h.shape
    H = cfg.n_heads
    dh = d // H
    scale = F32(dh ** -0.5) / F32(np.sqrt(R))
    q = linear(h, w[p + "q_proj.weight"], w[p + "q_proj.bias"]).reshape(B, R, C, H, dh) * scale
    k = linear(h, w[p + "k_proj.weight"], w[p + "k_proj.bias"]).reshape(B, R, C, H, dh)
    if pad is not None:
        q = np.where(pad[..., None, None], F32(0), q)
    qc = np.ascontiguousarray(q.transpose(0, 3, 2, 1, 4)).reshape(B, H, C, R * dh)
    kc = np.ascontiguousarray(k.transpose(0, 3, 2, 1, 4)).reshape(B, H, C, R * dh)
    a = np.matmul(qc, kc.transpose(0, 1, 3, 2)).astype(F32)
    if pad is not None:
        a = np.where(pad[:, 0][:, None, None, :], F32(-10000.0), a)
    return softmax_lastdim(a)


def msa_row_attentions(w, cfg, tokens):
    """cfg: oracle.msa_forward.MsaConfig -> (A [n_layers][B][H][C][C] float32, trunk output [B][R][C][d])"""
    x = M.msa_embed(w, cfg, tokens)
    pad = np.asarray(tokens) == cfg.pad_idx
    pad = pad if pad.any() else None
    maps = []
    for i in range(cfg.n_layers):
        p = "layers.%d." % i
        h = layer_norm(x, w[p + "row_self_attention.layer_norm.weight"], w[p + "row_self_attention.layer_norm.bias"])
        maps.append(row_map(w, p + "row_self_attention.layer.", cfg, h, pad))
        x = (x + M.row_attention(w, p + "row_self_attention.layer.", cfg, h, pad)).astype(F32)
        h = layer_norm(x, w[p + "column_self_attention.layer_norm.weight"], w[p + "column_self_attention.layer_norm.bias"])
        x = (x + M.column_attention(w, p + "column_self_attention.layer.", cfg, h, pad)).astype(F32)
        h = layer_norm(x, w[p + "feed_forward_layer.layer_norm.weight"], w[p + "feed_forward_layer.layer_norm.bias"])
        h = gelu(linear(h, w[p + "feed_forward_layer.layer.fc1.weight"], w[p + "feed_forward_layer.layer.fc1.bias"]))
        x = (x + linear(h, w[p + "feed_forward_layer.layer.fc2.weight"], w[p + "feed_forward_layer.layer.fc2.bias"])).astype(F32)
    return np.stack(maps), layer_norm(x, w["emb_layer_norm_after.weight"], w["emb_layer_norm_after.bias"])


# ---- kernel-level reference of the maps ---------------------------------------------------------------------------------------------
def row_scores_f64(qkv, B, R, C, H, scale, tok=None, pad_idx=1, hd=64):
    """qkv [B * R * C][3 * H * hd] -> (scores [B][H][C][C] float64 = scale * sum_r sum_d q k with q zeroed at <pad> positions and the key
    columns that are <pad> in row 0 filled with -10000, scale * sum |q k| of the same shape, filled [B][C] bool)"""
    x = np.asarray(qkv, dtype=F64).reshape(B, R, C, 3, H, hd)
    q, k = x[:, :, :, 0], x[:, :, :, 1]                                   # [B][R][C][H][hd]
    filled = np.zeros((B, C), bool)
    if tok is not None:
        pad = np.asarray(tok).reshape(B, R, C) == pad_idx
        q = np.where(pad[..., None, None], 0.0, q)
        filled = pad[:, 0]
    s = np.einsum("brihd,brjhd->bhij", q, k) * float(scale)
    mag = np.einsum("brihd,brjhd->bhij", np.abs(q), np.abs(k)) * float(scale)
    s = np.where(filled[:, None, None, :], -10000.0, s)
    return s, mag, filled


def row_probs_f64(qkv, B, R, C, H, scale, tok=None, pad_idx=1):
    """-> (P [B][H][C][C] float64, scores, sum |q k|, filled)"""
    s, mag, filled = row_scores_f64(qkv, B, R, C, H, scale, tok, pad_idx)
    a = s - s.max(axis=-1, keepdims=True)
    e = np.exp(a)
    return e / e.sum(axis=-1, keepdims=True), s, mag, filled


# ---- the head -------------------------------------------------------------------------------------------------------------------
def live_window(tok_row, eos, pad, tail):
    """tok_row [B][T] -> [B][T - 1 - tail] bool: the window positions whose token is neither eos nor pad (eos -1: none is)"""
    tok_row = np.asarray(tok_row)
    return ((tok_row != eos) & (tok_row != pad))[:, 1:tok_row.shape[1] - tail]


def fold_layer_f32(P, tok_row, w_layer, bias, first, last, logits, eos, pad, tail):
    """One launch_contact_accumulate_window: P [B][H][T][T] float32, w_layer [H] -> the new logits float32 [B][W][W], W = T - 1 - tail"""
    P = np.asarray(P, dtype=F32)
    B, H, T, _ = P.shape
    W = T - 1 - tail
    live = live_window(tok_row, eos, pad, tail)
    m = (live[:, :, None] & live[:, None, :])[:, None]
    win = np.where(m, P[:, :, 1:1 + W, 1:1 + W], F32(0)).astype(F32)
    S = (win + win.transpose(0, 1, 3, 2)).astype(F32)
    a1 = wave_sum(S)
    a12 = wave_sum(a1)
    out = np.zeros((B, W, W), dtype=F32) if first else np.array(logits, dtype=F32)
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


def row_contacts_f32(A, tok0, w, bias, pad):
    """A [L][B][H][C][C] float32, tok0 [B][C] (row 0 of every MSA), w [L * H] -> logits float32 [B][C-1][C-1], layer by layer"""
    L, B, H = A.shape[:3]
    w = np.asarray(w, dtype=F32).reshape(L, H)
    logits = None
    for l in range(L):
        logits = fold_layer_f32(A[l], tok0, w[l], bias, l == 0, l == L - 1, logits, -1, pad, 0)
    return logits


def row_contacts_f64(A, tok0, w, bias, pad, eos=-1, tail=0):
    """The float64 form of the same contract: -> (logits, contacts) float64 [B][W][W]"""
    A = np.asarray(A, dtype=F64)
    L, B, H, T, _ = A.shape
    W = T - 1 - tail
    live = live_window(tok0, eos, pad, tail)
    m = (live[:, :, None] & live[:, None, :])[None, :, None]
    win = np.where(m, A[:, :, :, 1:1 + W, 1:1 + W], 0.0)
    S = win + win.transpose(0, 1, 2, 4, 3)
    a1 = S.sum(axis=-1)
    a12 = a1.sum(axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        N = S - a1[..., :, None] * a1[..., None, :] / a12[..., None, None]
    N = np.where(a12[..., None, None] == 0, 0.0, N)
    wv = np.asarray(w, dtype=F64).reshape(L, 1, H, 1, 1)
    logits = (wv * N).sum(axis=(0, 2)) + float(bias)
    return logits, 1.0 / (1.0 + np.exp(-logits))
