"""fp32 numpy reference of the ESM-2 forward (test infrastructure only -- never imported by the product path).

Written from the published algorithm of fair-esm's `ESM2.forward` (include/pgibbs.h PG_ARCH_ESM2 restates the contract):

  x = embed_tokens[tok]                                            (embed scale 1, NO position embedding)
  token dropout: x[tok == <mask>] = 0;  x *= (1 - 0.12) / (1 - n_mask_b / n_nonpad_b)
  x *= (tok != <pad>)                                              (no emb_layer_norm_before)
  L x { x += out_proj(MHA_rotary(LN1(x)));  x += fc2(gelu(fc1(LN2(x)))) }        (pre-LN, erf GELU, <pad> keys masked)
  x = emb_layer_norm_after(x)
  logits = LN(gelu(dense(x))) @ embed_tokens^T + lm_head.bias      (tied decoder)

MHA_rotary: per head of hd = d_model / n_heads (64 by default), q = (h W_q^T + b_q) * hd^-0.5 (a float32 factor) and k = h W_k^T + b_k
are rotated before q k^T:
  inv_freq[i] = 1 / 10000^(2i/hd), ang[t][i] = float32(t) * inv_freq[i], t = index along the token axis (0 for <cls>, padding or not)
  u'[i] = u[i] cos - u[i+hd/2] sin,  u'[i+hd/2] = u[i+hd/2] cos + u[i] sin  ("rotate-half": pairs (i, i + hd/2)); v is not rotated.

Corroborated against an independent implementation, HuggingFace `transformers.EsmForMaskedLM` with rotary positions, at heads of 64,
32, 128, 16 and 24 (tests/golden/make_golden_esm2.py -> esm2_hf_*.npz; tests/test_esm2_cpu.py, tests/test_esm2_sizes_cpu.py).
Weights: a dict keyed by fair-esm state-dict names.
"""
import numpy as np
from scipy.special import erf

F32 = np.float32


def layer_norm(x, w, b, eps=1e-5):
    x = x.astype(F32)
    xc = x - x.mean(axis=-1, keepdims=True, dtype=F32)
    var = (xc * xc).mean(axis=-1, keepdims=True, dtype=F32)
    return (xc / np.sqrt(var + F32(eps)) * w + b).astype(F32)


def gelu(x):
    x = np.ascontiguousarray(x, dtype=F32)
    out = np.empty_like(x)
    flat, oflat = x.reshape(-1), out.reshape(-1)
    step = 1 << 22                                   # blocks bound the float64 temporaries of scipy's erf
    for i in range(0, flat.size, step):
        a = flat[i:i + step]
        oflat[i:i + step] = F32(0.5) * a * (F32(1.0) + erf(a * F32(0.7071067811865476)).astype(F32))
    return out


def linear(x, w, b):
    return (x @ w.T + b).astype(F32)


def inv_freq(hd=64):
    """float32, as torch computes 1.0 / (10000 ** (arange(0, hd, 2).float() / hd)): the power in double, rounded to float32."""
    half = hd // 2
    return (F32(1.0) / (10000.0 ** (np.arange(half, dtype=np.float64) / float(half))).astype(F32)).astype(F32)


def cos_sin(T, hd=64):
    """cos / sin [T][hd/2] float32 of the float32 angle t * inv_freq[i], evaluated in double and rounded."""
    ang = (np.arange(T, dtype=F32)[:, None] * inv_freq(hd)[None, :]).astype(F32)
    return np.cos(ang.astype(np.float64)).astype(F32), np.sin(ang.astype(np.float64)).astype(F32)


def rotate(u, cos, sin):
    """u [..., T, hd] float32 -> rotated, every product and the add / subtract rounded to float32 separately."""
    u = u.astype(F32)
    half = u.shape[-1] // 2
    lo, hi = u[..., :half], u[..., half:]
    return np.concatenate([(lo * cos).astype(F32) - (hi * sin).astype(F32), (hi * cos).astype(F32) + (lo * sin).astype(F32)],
                          axis=-1).astype(F32)


def rotate_qkv_rows(qkv, B, T, H, hd=64):
    """[B*T][3*H*hd] float32 -> the q and k thirds rotated (row r at position r % T), v untouched: what pg_dbg_rope_hd computes."""
    cos, sin = cos_sin(T, hd)
    x = np.array(qkv, dtype=F32).reshape(B, T, 3, H, hd)
    for part in (0, 1):
        x[:, :, part] = rotate(x[:, :, part].transpose(0, 2, 1, 3), cos, sin).transpose(0, 2, 1, 3)
    return x.reshape(B * T, 3 * H * hd)


def softmax_attention(qkv, B, T, H, hd, pad=None):
    """qkv [B][T][3*H*hd] float32 (q already scaled) -> ctx [B][T][H*hd] in float64 arithmetic: what pg_dbg_attention_hd computes.
    pad [B][T] bool: keys to mask."""
    x = np.asarray(qkv, dtype=np.float64).reshape(B, T, 3, H, hd).transpose(2, 0, 3, 1, 4)
    a = x[0] @ x[1].transpose(0, 1, 3, 2)
    if pad is not None:
        a = np.where(np.asarray(pad, bool)[:, None, None, :], -np.inf, a)
    a = a - a.max(axis=-1, keepdims=True)
    e = np.exp(a)
    return ((e / e.sum(axis=-1, keepdims=True)) @ x[2]).transpose(0, 2, 1, 3).reshape(B, T, H * hd)



class Esm2Config:
    def __init__(self, d_model=1280, n_layers=33, n_heads=20, vocab=33, pad_idx=1, mask_idx=32, token_dropout=True, eps=1e-5):
        self.d_model, self.n_layers, self.n_heads, self.vocab = d_model, n_layers, n_heads, vocab
        self.pad_idx, self.mask_idx, self.token_dropout, self.eps = pad_idx, mask_idx, token_dropout, eps
        assert d_model % n_heads == 0
        self.head_dim = d_model // n_heads

    @classmethod
    def of(cls, cfg):
        """from an engine configuration dict (weights.ESM2_T33_CONFIG and friends)"""
        return cls(cfg["d_model"], cfg["n_layers"], cfg["n_heads"], cfg["vocab"], cfg["pad_idx"], cfg["mask_idx"],
                   bool(cfg["token_dropout"]), cfg["layer_norm_eps"])


def _attention(w, p, cfg, h, pad, cos, sin):
    B, T, d = h.shape
    H, hd = cfg.n_heads, cfg.head_dim
    q = linear(h, w[p + "q_proj.weight"], w[p + "q_proj.bias"]) * F32(hd ** -0.5)
    k = linear(h, w[p + "k_proj.weight"], w[p + "k_proj.bias"])
    v = linear(h, w[p + "v_proj.weight"], w[p + "v_proj.bias"])
    q = rotate(q.reshape(B, T, H, hd).transpose(0, 2, 1, 3), cos, sin)
    k = rotate(k.reshape(B, T, H, hd).transpose(0, 2, 1, 3), cos, sin)
    v = v.reshape(B, T, H, hd).transpose(0, 2, 1, 3)
    a = (q @ k.transpose(0, 1, 3, 2)).astype(F32)
    if pad.any():
        a = np.where(pad[:, None, None, :], F32(-np.inf), a)
    a = a - a.max(axis=-1, keepdims=True)
    e = np.exp(a, dtype=F32)
    prob = (e / e.sum(axis=-1, keepdims=True, dtype=F32)).astype(F32)
    ctx = (prob @ v).transpose(0, 2, 1, 3).reshape(B, T, d).astype(F32)
    return linear(ctx, w[p + "out_proj.weight"], w[p + "out_proj.bias"])


def esm2_forward(w, cfg, tokens):
    """tokens [B][T] -> logits [B][T][V] float32."""
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
    cos, sin = cos_sin(T, cfg.head_dim)
    for i in range(cfg.n_layers):
        p = "layers.%d." % i
        h = layer_norm(x, w[p + "self_attn_layer_norm.weight"], w[p + "self_attn_layer_norm.bias"], cfg.eps)
        x = x + _attention(w, p + "self_attn.", cfg, h, pad, cos, sin)
        h = layer_norm(x, w[p + "final_layer_norm.weight"], w[p + "final_layer_norm.bias"], cfg.eps)
        h = gelu(linear(h, w[p + "fc1.weight"], w[p + "fc1.bias"]))
        x = (x + linear(h, w[p + "fc2.weight"], w[p + "fc2.bias"])).astype(F32)
    x = layer_norm(x, w["emb_layer_norm_after.weight"], w["emb_layer_norm_after.bias"], cfg.eps)
    g = gelu(linear(x, w["lm_head.dense.weight"], w["lm_head.dense.bias"]))
    g = layer_norm(g, w["lm_head.layer_norm.weight"], w["lm_head.layer_norm.bias"], cfg.eps)
    return (g @ w["embed_tokens.weight"].T + w["lm_head.bias"]).astype(F32)


def log_softmax(logits):
    a = logits.astype(np.float64)
    a = a - a.max(axis=-1, keepdims=True)
    return (a - np.log(np.exp(a).sum(axis=-1, keepdims=True))).astype(F32)
