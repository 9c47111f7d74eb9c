"""The float64 reference of the attention kernels, the element-wise error bound the kernel tests assert, and the input families
they run (numpy only; tests/test_attention_reference_cpu.py checks this file against the oracles without a GPU,
tests/test_gpu_attention_kernels.py holds the kernels to it).

Semantics, as the kernels state them (csrc/attention.hip, csrc/msa_attention.hip, csrc/attention_f32.hip):
  * full attention of a sequence: ctx_i = sum_j softmax_j(q_i . k_j) v_j, q already scaled;
  * a key whose token is <pad> scores -inf in a chain (fair-esm's key_padding_mask) and -10000 in the strided sequences of the
    MSA column attention (ColumnSelfAttention: an all-<pad> column softmaxes to the uniform row);
  * ESM-1's bias key (add_bias_kv) is one more key behind the T token keys, attended by every query, never masked;
  * tied row attention: one C x C map per (alignment, head) from scores summed over the R rows, times `scale`; with <pad>,
    q is zeroed at padded positions and the key columns that are <pad> in ROW 0 score -10000 (RowSelfAttention).

The bound
---------
Inputs are handed over already rounded to the operand type, so nothing is granted for them.  A 16-bit kernel then does, per
query i (attn_frag.h softmax_exact / attention_long_kernel):
  1. s_j = q_i . k_j            products of two 16-bit values are exact in fp32; accumulated in fp32 by the MFMA,
  2. e_j = exp2(fma(s_j, log2e, -max * log2e))      v_exp_f32,
  3. l = sum_j e_j              fp32, over the UNROUNDED e_j,
  4. P_j = round16(e_j)         the operand type: unit roundoff u = 2^-8 (bf16, 8 significant bits) or 2^-11 (fp16),
  5. o = sum_j P_j v_j          fp32 MFMA accumulation,
  6. ctx = round16(o * (1 / l)) rounded once, same u.
With A = sum_j p_j |v_j| (p = the exact softmax) and r = |ref|:
  * step 4 perturbs each term of the numerator by at most u e_j |v_j|: u A after normalisation.  fp16 only: an e_j below 2^-14
    is rounded on the subnormal grid, absolute error 2^-25 each, l >= 1 (the maximum's e is 1): at most 2^-25 sum_j |v_j|;
  * step 6 is u r (fp16: + 2^-25 for a subnormal result);
  * the fp32 steps.  A relative error eps on every e_j moves ctx by at most eps (A + r) (numerator and denominator).  The
    exponent: the accumulated score is off by at most n_dot 2^-24 S, S = max_i |q_i| max_j |k_j| >= sum_d |q_d k_d| >= |s_j|
    (Cauchy-Schwarz; n_dot = products per score); log2e as a float, the fma's rounding of an exponent of magnitude <= 2 S log2e
    and the rounding of -max * log2e add at most 4 S log2e 2^-24; times ln 2: (n_dot + 4) S 2^-24 <= n_dot S 2^-23 relative.
    v_exp_f32 is accurate to 1 ulp (CDNA4 ISA guide, "V_EXP_F32 ... 1 ULP accuracy"): 2^-23.  The sums of steps 3 and 5 run over
    n_keys terms, each at most n_keys 2^-24 relative in any order; 1 / l and the product with it are 1.5 ulp.  Together
        eps32 = 2^-23 (n_keys + 4 + n_dot S)
    -- the term "proportional to (1 + max|score|) 2^-23", with max|score| taken as S so that cancellation inside a score is paid for;
  * second-order terms: everything times (1 + 2u).
      bound = (1 + 2u) [ (u + eps32) (A + r) + fp16 subnormal terms ].
The tied-row kernel rounds the normalised p_j instead of e_j and stores o unscaled: the same six terms.

The strict kernels (PG_PREC_FP32) carry every operand as a bf16 (hi, lo) pair: hi is within 2^-9 of the value and lo within
2^-9 of the rest, so a pair holds the value to 2^-18, and the dropped lo.lo product is at most 2^-18 of |a||b|.  Scores: q pair,
k pair and the dropped product, 3 2^-18 S absolute = relative on e_j; P pair, V pair and their dropped product 3 2^-18 on the
numerator; the context pair 2^-18 r:
      bound = (3 2^-18 (S + 1) + eps32) (A + r) + u_out r,     u_out = 2^-18,
or the 16-bit u when the kernel writes plain 16-bit context rows (the ragged tied-row route of the engine).
None of these figures is fitted to what a kernel returns.
"""
from collections import namedtuple

import numpy as np

F64 = np.float64
PAD = 1                      # <pad> in every alphabet of the project
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
FAMILIES = ("gaussian", "negative", "late_last", "late_tile", "unity", "intcode")

Result = namedtuple("Result", "ref pabs smax vabs n_keys n_dot")
Result.__doc__ = """ref: the context; pabs: sum_j p_j |v_j| per element; smax: S per element's (sequence, head), broadcastable to ref;
vabs: sum_j |v_j| over the keys, per element; n_keys / n_dot: keys per softmax / products per score"""


# ---- operand types -----------------------------------------------------------------------------------------------------------------
def round_to(fmt, a):
    """round-to-nearest-even to the operand type, as float32; "f32": unchanged"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if fmt == "f32":
        return a
    if fmt == "f16":
        return a.astype(np.float16).astype(np.float32)
    u = a.view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


# ---- the reference -----------------------------------------------------------------------------------------------------------------
def _softmax(a):
    p = np.exp(a - a.max(-1, keepdims=True))
    return p / p.sum(-1, keepdims=True)


def _norm_max(x):
    """max over the token axis (-2) of the Euclidean norm over d"""
    return np.sqrt((x * x).sum(-1)).max(-1)


def attention(q, k, v, key_pad=None, fill=-np.inf, bias_k=None, bias_v=None):
    """q, k, v [N][H][T][HD] (any float type, taken as exact); key_pad bool [N][T]: True = the key is <pad>, its score becomes `fill`;
    bias_k / bias_v [H][HD]: ESM-1's extra key behind the T keys, never masked.  Result fields are [N][H][T][HD] (smax [N][H][1][1])."""
    q, k, v = (np.asarray(x, F64) for x in (q, k, v))
    N, H, T, HD = q.shape
    if bias_k is not None:
        k = np.concatenate([k, np.broadcast_to(np.asarray(bias_k, F64)[None, :, None, :], (N, H, 1, HD))], 2)
        v = np.concatenate([v, np.broadcast_to(np.asarray(bias_v, F64)[None, :, None, :], (N, H, 1, HD))], 2)
    a = q @ k.transpose(0, 1, 3, 2)
    if key_pad is not None:
        m = np.zeros((N, k.shape[2]), bool)
        m[:, :T] = key_pad
        a = np.where(m[:, None, None, :], fill, a)
    p = _softmax(a)
    smax = (_norm_max(q) * _norm_max(k))[..., None, None]
    vabs = np.broadcast_to(np.abs(v).sum(2, keepdims=True), q.shape)
    return Result(p @ v, p @ np.abs(v), smax, vabs, k.shape[2], HD)


def _heads(qkv, H, hd):
    """[..][T][3*H*hd] -> q, k, v [..][T][H][hd]"""
    d = H * hd
    r = np.asarray(qkv, F64)
    return (r[..., i * d:(i + 1) * d].reshape(r.shape[:-1] + (H, hd)) for i in range(3))


def chain_attention(qkv, H, hd, tok=None, pad_idx=PAD, bias_k=None, bias_v=None):
    """qkv [B][T][3*H*hd] -> Result with fields [B][T][H*hd] (smax [B][1][H*hd]): the contiguous sequences of the ESM models; <pad> keys -inf"""
    B, T = qkv.shape[:2]
    q, k, v = (x.transpose(0, 2, 1, 3) for x in _heads(qkv, H, hd))
    res = attention(q, k, v, None if tok is None else np.asarray(tok) == pad_idx, -np.inf, bias_k, bias_v)
    back = [np.broadcast_to(x, q.shape).transpose(0, 2, 1, 3).reshape(B, T, H * hd) for x in res[:4]]
    back[2] = back[2][:, :1]
    return Result(*back, res.n_keys, res.n_dot)


def column_attention(qkv, H, tok=None, pad_idx=PAD):
    """qkv [B][R][C][3*H*64] -> fields [B][R][C][H*64]: every column of an alignment is a sequence of R keys; <pad> keys -10000"""
    B, R, C = qkv.shape[:3]
    q, k, v = (x.transpose(0, 2, 3, 1, 4).reshape(B * C, H, R, 64) for x in _heads(qkv, H, 64))
    pad = None if tok is None else (np.asarray(tok) == pad_idx).transpose(0, 2, 1).reshape(B * C, R)
    res = attention(q, k, v, pad, -10000.0)
    back = [np.broadcast_to(x, q.shape).reshape(B, C, H, R, 64).transpose(0, 3, 1, 2, 4).reshape(B, R, C, H * 64) for x in res[:4]]
    return Result(*back, res.n_keys, res.n_dot)


def tied_row_attention(qkv, H, scale, tok=None, pad_idx=PAD):
    """qkv [B][R][C][3*H*64] -> fields [B][R][C][H*64]; with tok: q zeroed at <pad>, key columns that are <pad> in row 0 score -10000"""
    B, R, C = qkv.shape[:3]
    q, k, v = _heads(qkv, H, 64)                                   # [B][R][C][H][64]
    if tok is not None:
        pad = np.asarray(tok) == pad_idx
        q = np.where(pad[..., None, None], 0.0, q)
    # one matrix product per (b, h) over the R * 64 concatenated features, as oracle/msa_forward.py does
    qc, kc, vc = (np.ascontiguousarray(x.transpose(0, 3, 2, 1, 4)).reshape(B, H, C, R * 64) for x in (q, k, v))
    a = (qc @ kc.transpose(0, 1, 3, 2)) * float(scale)
    if tok is not None:
        a = np.where(pad[:, 0][:, None, None, :], -10000.0, a)
    p = _softmax(a)
    shape = (B, R, C, H * 64)
    ref, pabs = ((p @ x).reshape(B, H, C, R, 64).transpose(0, 3, 2, 1, 4).reshape(shape) for x in (vc, np.abs(vc)))
    # S: |sum_r q_r . k_r| <= sqrt(sum_r |q_r|^2) sqrt(sum_r |k_r|^2) over the concatenated rows
    qn = np.sqrt((q * q).sum((1, 4))).max(1)                       # [B][H]
    kn = np.sqrt((k * k).sum((1, 4))).max(1)
    smax = np.repeat((qn * kn * abs(float(scale)))[:, None, None, :], 64, -1)
    vabs = np.broadcast_to(np.abs(v).sum(2, keepdims=True), v.shape).reshape(shape)
    return Result(ref, pabs, smax, vabs, C, R * 64)


def eps32(res):
    return 2.0 ** -23 * (res.n_keys + 4 + res.n_dot * res.smax)


def bound(res, fmt):
    """the element-wise bound of a 16-bit kernel with operands of type fmt ("bf16" / "f16"): module docstring"""
    u = U[fmt]
    ar = res.pabs + np.abs(res.ref)
    sub = 2.0 ** -25 * (res.vabs + 1.0) if fmt == "f16" else 0.0
    return (1 + 2 * u) * ((u + eps32(res)) * ar + sub)


def bound_strict(res, out_fmt=None):
    """the strict (split-bf16 / all-fp32) kernels; out_fmt: the 16-bit type of plain context rows, None = the (hi, lo) pair"""
    ar = res.pabs + np.abs(res.ref)
    u_out = 2.0 ** -18 if out_fmt is None else U[out_fmt]
    return (1 + 2 * u_out) * ((3 * 2.0 ** -18 * (res.smax + 1) + eps32(res)) * ar + u_out * np.abs(res.ref))


# ---- input families ----------------------------------------------------------------------------------------------------------------
def family_qkv(family, seed, n_seq, T, H, hd, peak=None, gain=1.0):
    """float32 [n_seq][T][3*H*hd], not yet rounded to an operand type.
    gain: what multiplies a score beyond its hd products (tied rows: R * scale), so that the families keep their score range there.
    peak [n_seq]: the key that holds the row maximum of the late_* families (default: late_last T - 1, late_tile the first key of
    the last 288-key tile).
      gaussian   q, k, v ~ N(0, 1), q scaled by 0.35: what the older tests use
      negative   q in [m, 1.25 m], k in [-1.25 m, -m], m^2 hd gain = 24: every real score lies in [-37.5, -24], so a key that
                 scores 0 -- zero-filled and unmasked, a <pad> key let through, a stale LDS row of zeros -- outweighs all real keys
                 together by e^24 / T and takes the softmax
      late_*     scores of a few units except on one key, about 40: the running maximum of a tiled kernel jumps there, everything
                 accumulated before it is rescaled by e^-36, and in fp16 the other P fall on the subnormal grid
      unity      q = 0, v = 1: every exponential is exactly 1, the context exactly 1 whatever the keys -- provided every unmasked
                 key is counted once and no other
      intcode    gaussian q, k; v of key j, head h, sequence n is the integer ((5 n + 3 h + j) % 15) - 7 in every d
    """
    rng = np.random.default_rng([seed, n_seq, T, H, hd, FAMILIES.index(family)])
    d = H * hd
    q, k, v = (rng.standard_normal((n_seq, T, H, hd)) for _ in range(3))
    if family in ("gaussian", "intcode"):
        q *= 0.35
    if family == "intcode":
        n, j, h = np.ogrid[:n_seq, :T, :H]
        v = np.broadcast_to((((5 * n + 3 * h + j) % 15) - 7)[..., None], v.shape).astype(F64)
    elif family == "negative":
        m = np.sqrt(24.0 / (hd * gain))
        q = m * (1 + 0.25 * rng.random(q.shape))
        k = -m * (1 + 0.25 * rng.random(k.shape))
    elif family in ("late_last", "late_tile"):
        s = np.where(rng.random(hd) < 0.5, -1.0, 1.0)
        q = (0.5 * s + 0.1 * q) / np.sqrt(gain)
        k = 0.3 * k / np.sqrt(gain)
        if peak is None:
            peak = np.full(n_seq, T - 1 if family == "late_last" else (T - 1) // 288 * 288)
        k[np.arange(n_seq), np.asarray(peak)] = (40.0 / (0.5 * hd)) * s / np.sqrt(gain)
    elif family == "unity":
        q[:] = 0.0
        v[:] = 1.0
    return np.concatenate([x.reshape(n_seq, T, d) for x in (q, k, v)], -1).astype(np.float32)


def family_bias(family, seed, H, hd):
    """bias_k, bias_v [H][hd] float32 of ESM-1's extra key for a family.  negative: the bias key scores -12 ... -9, so it outweighs the
    token keys by e^12 and the context is bias_v -- a bias key dropped, masked or given another value shows in every element, and a
    key that scores 0 still outweighs it by e^9; unity: bias_v = 1; intcode: the integer 8, which no token key holds; late_*: a key of a
    few units"""
    rng = np.random.default_rng([seed, H, hd, 99, FAMILIES.index(family)])
    bk, bv = rng.standard_normal((H, hd)), rng.standard_normal((H, hd))
    if family == "negative":
        bk = -0.37 * np.sqrt(24.0 / hd) * (1 + 0.1 * rng.random((H, hd)))
    elif family in ("late_last", "late_tile"):
        bk *= 0.3
    elif family == "unity":
        bv[:] = 1.0
    elif family == "intcode":
        bv[:] = 8.0
    return bk.astype(np.float32), bv.astype(np.float32)


# ---- <pad> patterns of a batch of chains --------------------------------------------------------------------------------------------
def pad_tokens(T):
    """int32 [3][T]: token 5 = a residue, PAD = <pad>.  Row 0: a ragged tail (the last five keys); row 1: padded down to a single
    real key; row 2: a run of <pad> that ends exactly on the last 288-key boundary below T (T > 288) or else on the last 16-key
    boundary, real keys behind it.  Rows whose pattern does not fit a short T keep what fits (at least one real key each)."""
    tok = np.full((3, T), 5, np.int32)
    tok[0, max(1, T - 5):] = PAD
    tok[1, 1:] = PAD
    end = (T - 1) // 288 * 288 if T > 288 else (T - 1) // 16 * 16
    if end > 1:
        tok[2, max(1, end - 7):end] = PAD
    return tok


def last_real_key(tok):
    real = np.asarray(tok) != PAD
    return real.shape[1] - 1 - real[:, ::-1].argmax(1)


def poison_pad(qkv, tok, H, hd, pad_idx=PAD):
    """k = 0 and v = 64 at <pad> tokens (in place): a <pad> key that a kernel lets through scores 0 and drags the context towards 64
    -- in the negative family it takes the softmax.  (A model leaves whatever its projections give there; masked, it cannot matter.)"""
    d = H * hd
    pad = np.asarray(tok) == pad_idx
    qkv[..., d:2 * d][pad] = 0.0
    qkv[..., 2 * d:][pad] = 64.0
    return qkv


def rung_edge_lengths():
    """every edge of the key-block ladder (attn_frag.h): for each even rung kb = 2 ... 36 the first length it serves on the fine ladder,
    its last odd length and its full length 16 kb -- which are also the lengths whose bias key (key T) sits alone in the next rung's
    first new block, for every coarse rung, and alone in a 288-key tile (288, 576, 864) -- then the long kernel's 577, 864, 865, 1024"""
    out = []
    for kb in range(2, 37, 2):
        out += [16 * (kb - 2) + 1, 16 * kb - 1, 16 * kb]
    return out + [577, 864, 865, 1024]


def expected_rung(T, bias, fine=True):
    """attention_rung of attn_frag.h restated: 0 = the long kernel"""
    n = T + (1 if bias else 0)
    if n > 576:
        return 0
    if fine and not bias:
        return (((n + 15) // 16) + 1) & ~1
    return next(r for r in (2, 4, 8, 12, 18, 24, 30, 36) if n <= 16 * r)


# ---- a numpy model of the 16-bit kernels' arithmetic (the six steps of the module docstring, float32 where the kernel is) -----------
def kernel_model(q, k, v, fmt, key_pad=None, fill=-3.0e38, bias_k=None, bias_v=None, dead_key=False):
    """q, k, v float32 [N][H][T][HD], already of type fmt; returns the context the six steps give.  dead_key: one more key of zeros
    that nothing masks (what an off-by-one in the tail mask leaves alive)."""
    f = np.float32
    N, H, T, HD = q.shape
    extra = [] if bias_k is None else [(bias_k, bias_v)]
    if dead_key:
        extra.append((np.zeros((H, HD), f), np.zeros((H, HD), f)))
    for ek, ev in extra:
        k = np.concatenate([k, np.broadcast_to(np.asarray(ek, f)[None, :, None, :], (N, H, 1, HD))], 2)
        v = np.concatenate([v, np.broadcast_to(np.asarray(ev, f)[None, :, None, :], (N, H, 1, HD))], 2)
    a = np.matmul(q, k.transpose(0, 1, 3, 2), dtype=f)
    if key_pad is not None:
        m = np.zeros((N, k.shape[2]), bool)
        m[:, :T] = key_pad
        a = np.where(m[:, None, None, :], f(fill), a)
    log2e = f(1.44269504088896341)
    with np.errstate(over="ignore", invalid="ignore"):
        mneg = (-a.max(-1, keepdims=True) * log2e).astype(f)
        e = np.exp2((a * log2e).astype(f) + mneg, dtype=f)
    l = e.sum(-1, keepdims=True, dtype=f)
    o = np.matmul(round_to(fmt, e), v, dtype=f)
    return round_to(fmt, o * (f(1) / l))
