"""Plain float64 references of the row kernels of csrc/elementwise.hip (token embedding, LM-head tail) and the seeded token patterns
their tests share.  tests/test_row_reference_cpu.py checks the embedding reference against the oracle's three embeddings without a
GPU; tests/test_gpu_row_kernels.py then trusts it."""
import numpy as np

PAD, MASK, CLS, EOS = 1, 32, 0, 2
PATTERNS = ("no_pad", "right_pad", "interior_pad", "leading_pad", "no_mask", "half_masked", "mask_next_to_pad")


def make_tokens(pattern, n_seq, T, seed, pad=PAD, mask=MASK):
    """tokens[n_seq][T] for one of PATTERNS: residues 4 .. 23, rows that differ from one another, <pad> and <mask> placed as the
    pattern says.  No sequence ever has all its non-pad tokens masked: token dropout divides by 1 - n_mask / n_nonpad, which is a
    division by zero there -- in fair-esm's own forward as well, so no caller can rely on that case."""
    assert pattern in PATTERNS
    rng = np.random.default_rng(seed)
    tok = rng.integers(4, 24, (n_seq, T)).astype(np.int32)
    if T >= 3:
        tok[:, 0], tok[:, -1] = CLS, EOS
    rows = np.arange(n_seq)
    if pattern in ("right_pad", "no_mask", "half_masked") and T >= 2:
        for i in rows:                                                  # rows of different lengths, each at least one token
            n = max(1, T - 1 - ((i * 5 + 2) % max(1, T // 2)))
            tok[i, n:] = pad
    if pattern in ("interior_pad", "mask_next_to_pad") and T >= 3:
        tok[:, T // 2] = pad
        if T >= 9:
            tok[rows % 2 == 1, T // 3] = pad                            # odd rows: a second gap
    if pattern == "leading_pad" and T >= 2:
        for i in rows:
            tok[i, :1 + (i % 2 if T >= 3 else 0)] = pad
    nonpad = tok != pad
    if pattern == "half_masked":
        for i in rows:
            at = np.flatnonzero(nonpad[i])
            tok[i, at[1::2]] = mask
    elif pattern == "mask_next_to_pad" and T >= 3:
        for j in (T // 2 - 1, T // 2 + 1):
            if 0 <= j < T:
                tok[nonpad[:, j], j] = mask
    elif pattern != "no_mask":
        sel = np.zeros_like(nonpad)
        sel[:, 2::7] = True
        tok[sel & nonpad] = mask
    for i in rows:                                                      # never all <pad>, never every non-pad token masked
        if not (tok[i] != pad).any():
            tok[i, 0] = 5
        live = np.flatnonzero(tok[i] != pad)
        if (tok[i, live] == mask).all():
            tok[i, live[0]] = 4 + (i % 20)
    return tok


def embed_reference(tokens, embed, pos=None, msa_pos=None, rows_per_msa=0, gamma=None, beta=None, pad=PAD, mask=MASK,
                    token_dropout=False, eps=1e-5, embed_scale=1.0):
    """x[n_seq][T][d] in float64, as fair-esm computes it: embed[tok] * scale (token dropout: <mask> rows zero, every row times
    0.88 / (1 - n_mask / n_nonpad) of its sequence; else embed_scale) + pos[count of non-pad tokens up to t + pad] (+ msa_pos[seq %
    rows_per_msa]), LayerNorm when gamma is given, <pad> rows zero.  Also returns |e * scale| + |pos| + |msa_pos|, the magnitude a
    rounding-error bound of the sum scales with."""
    tokens = np.asarray(tokens)
    n_seq, T = tokens.shape
    is_pad = tokens == pad
    e = embed.astype(np.float64)[tokens]
    if token_dropout:
        is_mask = tokens == mask
        ratio = is_mask.sum(1) / (~is_pad).sum(1)
        scale = np.where(is_mask, 0.0, ((1 - 0.15 * 0.8) / (1 - ratio))[:, None])[..., None]
    else:
        scale = np.float64(embed_scale)
    x = e * scale
    mag = np.abs(x)
    if pos is not None:
        live = (~is_pad).astype(np.int64)
        p = pos.astype(np.float64)[np.cumsum(live, axis=1) * live + pad]
        x, mag = x + p, mag + np.abs(p)
    if rows_per_msa > 0:
        r = msa_pos.astype(np.float64)[np.arange(n_seq) % rows_per_msa][:, None, :]
        x, mag = x + r, mag + np.abs(r)
    if gamma is not None:
        x = (x - x.mean(-1, keepdims=True)) / np.sqrt(x.var(-1, keepdims=True) + eps) * gamma.astype(np.float64) + beta.astype(np.float64)
    x = np.where(is_pad[..., None], 0.0, x)
    return x, mag


def layernorm_reference(x, gamma, beta, eps=1e-5):
    x = x.astype(np.float64)
    return (x - x.mean(-1, keepdims=True)) / np.sqrt(x.var(-1, keepdims=True) + eps) * gamma.astype(np.float64) + beta.astype(np.float64)


def lm_tail_reference(g, embed, bias, gamma=None, beta=None, eps=1e-5):
    """logits[n][V] in float64 = (LayerNorm(g) when gamma is given, else g) . embed^T + bias; also sum_i |v_i e_i| + |bias| per logit,
    max |v| and sum_i |e_i| per vocabulary row: the terms of the tests' error bounds."""
    v = layernorm_reference(g, gamma, beta, eps) if gamma is not None else g.astype(np.float64)
    e = embed.astype(np.float64)
    b = bias.astype(np.float64)
    return v @ e.T + b, np.abs(v) @ np.abs(e).T + np.abs(b), float(np.abs(v).max()), np.abs(e).sum(1)
