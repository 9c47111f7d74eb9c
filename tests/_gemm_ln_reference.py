"""The references of the single-chain GEMM with the folded LayerNorm (gemm_ln_skinny_kernel, csrc/gemm_bf16.hip), the input families its
tests run, a float32 model of the kernel's stated order with five wrong variants, and the case table (numpy only;
tests/test_gemm_ln_reference_cpu.py checks this file without a GPU, tests/test_gpu_gemm_ln_kernels.py holds the kernel to it).

Semantics:  out[Mi][N] = round16( LayerNorm(x[Mi][K]; gamma, beta, eps) . w[N][K]^T + bias[N] ), optionally through GELU; x, gamma, beta,
bias fp32, w 16-bit, the LayerNorm output rounded ONCE to the 16-bit operand type on its way into the MFMA, fp32 accumulation.

Family a: exact
---------------
Row r is x[r][k] = m_r + s_rk a_r with s_rk = +/-1 (exactly K/2 of each, shuffled per row), m_r an integer that differs per row and
a_r a power of two in 1/4 ... 8 that differs between neighbouring rows and between rows 16 apart; eps = 0.  Every x is a multiple of
1/4 below 2^7, so every partial sum of a row (at most 1280 terms) is a multiple of 1/4 below 2^18: exact in fp32 in any order, and
sum_k x = K m_r.  The kernel's mean is fl(fl(K m) fl(1 / K)), which equals m for the values kept (`stats_exact`: 1 / K is inexact at
K = 768 and 1280, so the pools are filtered with the kernel's own float32 expressions).  The centred values are +/-a_r exactly, their
squares a_r^2, every partial sum a multiple of a_r^2 up to K a_r^2, exact; fl(fl(K a^2) fl(1 / K)) = a^2 by the same filter (+ eps = 0:
the same value with or without a fused multiply-add), sqrt(a^2) = a and 1 / a are exact.  The operand is (+/-a)(1 / a) gamma_k + beta_k
= +/-gamma_k + beta_k: an integer in [-7, 7] for integer gamma in [-4, 4] and beta in [-3, 3], exact whether or not the compiler
contracts a r g + b.  With w integers in [-8, 8] and integer bias of magnitude 3000 ... 40000 the product is the exact-integer case of
_gemm_reference.py: sum_k |h w| + |bias| < 2^24 (asserted), every partial sum exact, the output the round-to-nearest-even conversion
of ONE int64 value, compared bit for bit.  A row normalised with a neighbour's statistics gives (m_r - m_q +/- a_r) / a_q, gamma or
beta eight columns off another integer, a dropped K slice or a foreign bias a sum that differs by at least 1.
gamma and beta vary along k without a period of 8, 32 or 256 (asserted).
GELU sub-family: gamma in {0, +/-1} with density sqrt(3.5 / K), beta = 0, w in {-1, 0, 1} at the same density and bias in eighths:
the pre-activation is exact and each output is held to _gemm_reference.gelu_bound (gelu_poly2, 16-bit output).

Family b: realistic
-------------------
x[r][k] = sigma_r (R_r + t_rk): sigma_r a power of two in 1/4 ... 4, t a standard Gaussian, R_r = |mean| / sigma between 0 and 100
(row 0 holds 100; the signs alternate).  gamma = 1 +/- 0.1, beta = 0.1 +/- 0.05, w = 0.03 x Gaussian on the 16-bit grid of both types,
bias = 0.1 x Gaussian, eps 1e-5 and 1e-12.  One-pass variance formulas cancel at R = 100: E[x^2] = 10^4 sigma^2 carries an fp32
rounding of 6e-4 sigma^2 per term against a variance of sigma^2.
The reference: float64 LayerNorm, the operand rounded once to the 16-bit type, float64 product, bias, optional erf-GELU.

The bound, per output element, has four terms.  u = 2^-24; u16 = 2^-8 (bf16) or 2^-11 (fp16), the half ulp of a 16-bit value.
 1. LayerNorm in fp32.  D = 13 + K / 256 bounds the additions any input passes through in the kernel's two sums (a tree over 8 values,
    K / 256 k-steps, two lane exchanges, 8 waves).  With d_k = x_k - mean, n_k = |d_k| / sqrt(var + eps), X = max_k |x_k|:
      * mean: |mean^ - mean| <= (D + 2) u X  (any summation of depth D: D u sum |x| <= D u K X; 1 / K and the product: 2 u).  In units
        of sigma that is m = (D + 2) u X / sigma -- the mean-cancellation term, proportional to max |x| / sigma.  At R = 100 it is
        2 10^-4: a fifth of an fp16 ulp of every operand of the row, which alone would put 20 % of them next to a rounding boundary.
        Family b therefore takes t on the grid 2^-6 with sum_k t_rk = 0 exactly and R_r from the filtered pool: every partial sum of
        pass 1 is a multiple of sigma 2^-6 below 2^24 of them and the mean is exact, m = 0 (`pass1_exact`, evaluated per row with the
        kernel's float32 expressions; a row that does not qualify -- none of the table -- pays the term in full).
      * centred values: v_k = (x_k - mean^)(1 + u).
      * variance: sum_k v_k^2 = Q + K dm^2 + 2 sum (d_k - dm) e_k with sum d_k = 0, |e_k| <= u (|d_k| + |dm|); squares and additions add
        (D + 1) u: relative error rho_Q <= m^2 + (D + 3) u (1 + m)^2.  q / K + eps: 3 u more; sqrtf and the division are correctly rounded
        (hipcc's default for fp32, u each; 3 u with room to spare): rho_r <= (rho_Q + 3 u) / 2 + 3 u.  Pass 2 is NOT exact in family b (the squares of the centred values are summed
        in fp32 like any others).
      * operand before rounding, a r g + b as two products and a sum or a product and a fused multiply-add (either form: at most
        3 u): delta_k = |gamma_k| (m (1 + u) + n_k (rho_r + 3 u)) + u |h_k|, times (1 + 2^-10) for the second-order terms.
 2. The 16-bit rounding of the operand: the kernel rounds a value within delta_k of the float64 h_k, so its operand lies between
    round16(h_k - delta_k) and round16(h_k + delta_k): flip_k = their difference -- one 16-bit ulp where a rounding boundary lies within
    delta_k of h_k, 0 elsewhere.  Operand term: sum_k |w_k| (delta_k + flip_k).  The share of elements with flip_k != 0 is kept at or
    below 0.5 % in every case by the choice of the seed (`realistic_rows` walks the seeds; asserted on the CPU): the term stays
    below a tenth of the output's half ulp.
 3. fp32 accumulation of K products, 7 partial sums and the bias in any order: (K + 10) u (sum_k |w_k h16_k| + |bias|).
 4. The output's half ulp: u16 (|ref| + terms 2 + 3) (+ 2^-25 absolute for fp16).  GELU epilogue: |d gelu / dz| <= 1.13, so the
    pre-activation error enters 1.13-fold, plus the documented error of gelu_poly2 (gemm_epilogue.h: 3.2e-6) x 2, before the half ulp.
None of these figures is fitted to what a kernel or the model returns.

Family c: row independence
--------------------------
Family b, with the rows behind the live ones (M ... Mi - 1) holding in turn zeros, values near 1e30 and NaN: the live rows' bits must
not depend on them.

The model
---------
`model` restates the kernel in numpy float32: per lane ((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7)) per k-step, k-steps in
sequence, the four lanes of a row as (s0 + s1) + (s2 + s3) (rows4_sum: xor 16, then xor 32), the 8 waves in order; s * (1 / K); the
centred squares as (v0^2 + v1^2) + (v2^2 + v3^2) per half k-step; 1 / sqrtf(q * (1 / K) + eps); a * r * g + b in both forms
(`contract`: the last product and the sum as one fused multiply-add, emulated through float64, as is q * (1 / K) + eps); each wave's
32-wide MFMA steps accumulated in sequence, waves 1 ... 7 added to wave 0, bias, rounding.  It is exact on family a and stays inside
bound b; `WRONG` lists five wrong variants, each of which leaves the bits of family a or the bound of family b.
"""
import functools
from collections import namedtuple

import numpy as np

import _gemm_reference as gr

F32, F64, I64 = np.float32, np.float64, np.int64
U32 = 2.0 ** -24
U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}
KS = (256, 512, 768, 1024, 1280)
MS = (1, 15, 16, 17, 31, 32)
FORCED = ((1, 16), (1, 48), (1, 64), (2, 32), (2, 64), (2, 96))      # (nb, N): one, three, four workgroups; one, two, three
# the engine's own launches at d_model = 1280 (engine.hip: QKV 3 d x d and fc1 d_ffn x d; the out-projection d x d does not take this
# kernel, so 1280 x 1280 is not in the table), nb = 0: the launcher's rule
ENGINE = ((3840, 1280), (5120, 1280))
ACC_C = 10
MAX_FLIP_SHARE = 0.005
WRONG = ("one-pass variance", "statistics of the next row", "gamma and beta shifted 8 columns", "wave 7's K slice dropped",
         "block 1 of an nb = 2 workgroup with block 0's bias")


def padded(M):
    return (M + 15) // 16 * 16


def eps_of(K):
    """family b's eps per depth: 1e-12 (ESM-1) at K = 512 and 1024, 1e-5 elsewhere; the engine widths run 1e-12 as well"""
    return 1e-12 if (K // 256) % 2 == 0 else 1e-5


def expected_nb(N, n_cu):
    """launch_gemm_ln_skinny's rule for nb = 0"""
    return 2 if N // 16 > n_cu and N % 32 == 0 else 1


def round16(fmt, a):
    """float64 -> the nearest (ties to even) value of the 16-bit type, as float64; values far from either type's range limits"""
    a = np.asarray(a, F64)
    if fmt == "f16":
        return a.astype(np.float16).astype(F64)
    m, e = np.frexp(a)
    return np.ldexp(np.rint(m * 256.0), e - 8)


def gelu64(z):
    from scipy.special import erf
    return 0.5 * z * (1.0 + erf(z / np.sqrt(2.0)))


# ---- exactness of the kernel's statistics, in its own float32 expressions ------------------------------------------------------------
def stats_exact(m, a=1.0):
    """fl(fl(K m) fl(1 / K)) == m and fl(fl(K a^2) fl(1 / K)) == a^2 for every K of the table"""
    for K in KS:
        inv_k = F32(1.0) / F32(K)
        if F32(K * float(m)) * inv_k != F32(m) or F32(K * float(a) * float(a)) * inv_k != F32(a * a):
            return False
    return True


A_POW = tuple(a for a in (0.25, 0.5, 1.0, 2.0, 4.0, 8.0) if stats_exact(1.0, a))
M_POOL = tuple(m for m in ((-1) ** i * (5 + 3 * i) for i in range(48)) if stats_exact(m))[:32]      # 5, -8, 11, ... up to about 100
R_POOL = tuple(r for r in (100, 0, 30, 1, 10, 3, 64, 0, 96, 2, 50, 0, 20, 5, 80, 1) if stats_exact(r))


def pass1_exact(x):
    """per row of float32 x: True when every partial sum of the row is exact in fp32 whatever the order (all values multiples of one
    power of two g, K max|x| / g < 2^24) and the kernel's fl(fl(sum) fl(1 / K)) is the exact mean"""
    x = np.asarray(x, F32)
    K = x.shape[1]
    m, e = np.frexp(x.astype(F64))
    i = np.abs(np.rint(m * 2.0 ** 24)).astype(I64)                       # 24-bit significands
    lsb = np.where(i > 0, e - 24 + np.log2(np.maximum(i & -i, 1)).astype(I64), 10 ** 6)
    g = np.ldexp(1.0, np.minimum(lsb.min(1), 1000).astype(np.int32))      # the row's grid
    fits = np.abs(x.astype(F64)).max(1) / g * K < 2.0 ** 24
    s = x.astype(F64).sum(1)
    mean32 = s.astype(F32) * (F32(1.0) / F32(K))
    return fits & (mean32.astype(F64) * K == s)


# ---- family a ------------------------------------------------------------------------------------------------------------------------
ExactLN = namedtuple("ExactLN", "x gamma beta w bias h ref mag m a")
ExactLN.__doc__ = """x[32][K] (callers take the first M rows as live and the rest of the first Mi as x_pad), gamma, beta, w, bias: float32
inputs; h: the integer operand; ref: int64 result [32][N]; mag: sum_k |h w| + |bias|; m, a: per-row mean and deviation"""


@functools.lru_cache(maxsize=None)
def _exact_rows(K, seed):
    rng = np.random.default_rng([seed, K, 11])
    m = np.asarray(M_POOL, F64)
    a = np.asarray([A_POW[r % len(A_POW)] for r in range(32)], F64)
    s = np.stack([rng.permutation(np.repeat([-1.0, 1.0], K // 2)) for _ in range(32)])
    x = (m[:, None] + s * a[:, None]).astype(F32)
    for v in (x, s, m, a):
        v.setflags(write=False)
    return x, s, m, a


@functools.lru_cache(maxsize=8)
def exact(N, K, seed=1):
    x, s, m, a = _exact_rows(K, seed)
    rng = np.random.default_rng([seed, N, K, 12])
    gamma = rng.integers(-4, 5, K).astype(F32)
    beta = rng.integers(-3, 4, K).astype(F32)
    w = rng.integers(-8, 9, (N, K)).astype(F32)
    w[:, 1] = (np.arange(N) % 15) - 7                                   # column-dependent
    bias = (rng.integers(3000, 40001, N) * rng.choice([-1, 1], N)).astype(F32)
    h = np.rint(s * gamma + beta).astype(I64)
    ref = h @ w.astype(I64).T + bias.astype(I64)
    mag = np.abs(h) @ np.abs(w).astype(I64).T + np.abs(bias).astype(I64)
    return ExactLN(x, gamma, beta, w, bias, h, ref, mag, m, a)


GeluLN = namedtuple("GeluLN", "x gamma beta w bias z ref")


@functools.lru_cache(maxsize=8)
def exact_gelu(N, K, seed=1):
    """the GELU sub-family: z exact; z and ref are what _gemm_reference.gelu_bound reads"""
    x, s, _, _ = _exact_rows(K, seed)
    rng = np.random.default_rng([seed, N, K, 13])
    p = min(1.0, np.sqrt(3.5 / K))
    gamma = (rng.integers(-1, 2, K) * (rng.random(K) < p * 1.5)).astype(F32)
    w = (rng.integers(-1, 2, (N, K)) * (rng.random((N, K)) < p * 1.5)).astype(F32)
    bias = (rng.integers(-8, 9, N) / 8.0).astype(F32)
    z = (s * gamma) @ w.astype(F64).T + bias.astype(F64)
    return GeluLN(x, gamma, np.zeros(K, F32), w, bias, z, gelu64(z))


# ---- family b ------------------------------------------------------------------------------------------------------------------------
Rows = namedtuple("Rows", "x gamma beta eps ratio sigma seed")


def _rows(K, eps, seed):
    rng = np.random.default_rng([seed, K, 21])
    t = np.clip(np.rint(rng.standard_normal((32, K)) * 64.0), -6 * 64, 6 * 64)
    t -= np.rint(t.sum(1, keepdims=True) / K)
    for r in range(32):                                                  # the rest of the row sum, one grid unit per element
        left = int(t[r].sum())
        t[r, :abs(left)] -= np.sign(left)
    assert (t.sum(1) == 0).all()
    ratio = np.asarray([R_POOL[r % len(R_POOL)] * (-1) ** r for r in range(32)], F64)
    sigma = np.asarray([2.0 ** ((3 * r) % 5 - 2) for r in range(32)], F64)
    x = (sigma[:, None] * (ratio[:, None] + t / 64.0)).astype(F32)
    gamma = (1.0 + rng.uniform(-0.1, 0.1, K)).astype(F32)
    beta = (0.1 + 0.05 * rng.standard_normal(K)).astype(F32)
    return Rows(x, gamma, beta, eps, ratio, sigma, seed)


def flip_shares(rows):
    """largest share of operand elements next to a rounding boundary over the live-row counts of the table and both types"""
    worst = 0.0
    for fmt in U16:
        _, delta = ln_delta(rows.x, rows.gamma, rows.beta, rows.eps)
        flip = operand_flip(fmt, layernorm64(rows.x, rows.gamma, rows.beta, rows.eps), delta)
        worst = max([worst] + [float((flip[:M] != 0).mean()) for M in MS])
    return worst


@functools.lru_cache(maxsize=None)
def realistic_rows(K, eps):
    """the first seed whose rows keep the flip share within MAX_FLIP_SHARE for every M of the table in both types (a property of the
    reference alone)"""
    for seed in range(200):
        rows = _rows(K, eps, seed)
        if flip_shares(rows) <= MAX_FLIP_SHARE:
            for v in rows[:3]:
                v.setflags(write=False)
            return rows
    raise AssertionError("no seed below 200 keeps the flip share within %.3f at K = %d" % (MAX_FLIP_SHARE, K))


@functools.lru_cache(maxsize=8)
def weights(N, K, seed=5):
    """w on the 16-bit grid of both operand types, bias fp32"""
    rng = np.random.default_rng([seed, N, K, 22])
    w = gr.round_to("f16", gr.round_to("bf16", 0.03 * rng.standard_normal((N, K))))
    return w.astype(F32), (0.1 * rng.standard_normal(N)).astype(F32)


# ---- the float64 reference and the bound ---------------------------------------------------------------------------------------------
def layernorm64(x, gamma, beta, eps):
    x = np.asarray(x, F64)
    d = x - x.mean(1, keepdims=True)
    return d / np.sqrt((d * d).mean(1, keepdims=True) + eps) * np.asarray(gamma, F64) + np.asarray(beta, F64)


def ln_delta(x, gamma, beta, eps):
    """(h, delta): the float64 LayerNorm of float32 rows and the bound on the fp32 kernel's error per element, before the 16-bit rounding"""
    x64 = np.asarray(x, F64)
    K = x64.shape[1]
    D = 13 + K // 256
    g, b = np.asarray(gamma, F64), np.asarray(beta, F64)
    d = x64 - x64.mean(1, keepdims=True)
    r = 1.0 / np.sqrt((d * d).mean(1, keepdims=True) + eps)
    h = d * r * g + b
    m = np.where(pass1_exact(x), 0.0, (D + 2) * U32 * np.abs(x64).max(1))[:, None] * r
    rho_q = m * m + (D + 3) * U32 * (1 + m) ** 2
    rho_r = (rho_q + 3 * U32) / 2 + 3 * U32
    delta = np.abs(g) * (m * (1 + U32) + np.abs(d) * r * (rho_r + 3 * U32)) + U32 * np.abs(h)
    return h, delta * (1 + 2.0 ** -10)


def operand_flip(fmt, h, delta):
    return round16(fmt, h + delta) - round16(fmt, h - delta)


Ref = namedtuple("Ref", "ref bound h h16 delta flip z")


def reference(x, gamma, beta, eps, w, bias, fmt, gelu):
    """float64 reference and per-element bound of out[rows of x][N] in the 16-bit type fmt"""
    h, delta = ln_delta(x, gamma, beta, eps)
    h16, flip = round16(fmt, h), operand_flip(fmt, h, delta)
    K = h.shape[1]
    w64, b64 = np.asarray(w, F64), np.asarray(bias, F64)
    z = h16 @ w64.T + b64
    e_z = (delta + flip) @ np.abs(w64).T + (K + ACC_C) * U32 * (np.abs(h16) @ np.abs(w64).T + np.abs(b64))
    ref, e = (gelu64(z), 1.13 * e_z + 2 * gr.POLY_DOC) if gelu else (z, e_z)
    bound = e + U16[fmt] * (np.abs(ref) + e) + (2.0 ** -25 if fmt == "f16" else 0.0)
    return Ref(ref, bound, h, h16, delta, flip, z)


# ---- the float32 model of the kernel and its wrong variants --------------------------------------------------------------------------
def _fma(a, b, c):
    """fl(a b + c) of float32 values: the product is exact in float64; the one double rounding left is below the model's purpose"""
    return (a.astype(F64) * b.astype(F64) + c.astype(F64)).astype(F32)


def _rows4_waves(s):
    """per-lane values [rows][wave][fq] -> the four lanes of a row as rows4_sum adds them, then the 8 waves in order"""
    s = (s[..., 0] + s[..., 1]) + (s[..., 2] + s[..., 3])
    tot = np.zeros(s.shape[0], F32)
    for wv in range(8):
        tot = tot + s[:, wv]
    return tot


def _pass1(xa):
    s = np.zeros(xa.shape[:2] + (4,), F32)
    for u in range(xa.shape[2]):
        v = xa[:, :, u]
        s = s + (((v[..., 0] + v[..., 1]) + (v[..., 2] + v[..., 3])) + ((v[..., 4] + v[..., 5]) + (v[..., 6] + v[..., 7])))
    return _rows4_waves(s)


def _pass2(va):
    q = np.zeros(va.shape[:2] + (4,), F32)
    for u in range(va.shape[2]):
        for hh in (0, 4):
            v = va[:, :, u, :, hh:hh + 4]
            q = q + ((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + (v[..., 2] * v[..., 2] + v[..., 3] * v[..., 3]))
    return _rows4_waves(q)


def model(x, gamma, beta, eps, w, bias, fmt, gelu=False, contract=False, wrong=None, nb=1):
    """x[Mi][K] float32 (all the rows the kernel reads) -> out[Mi][N] float32 on the 16-bit grid of fmt"""
    assert wrong is None or wrong in WRONG
    x, gamma, beta, w, bias = (np.asarray(v, F32) for v in (x, gamma, beta, w, bias))
    (Mi, K), N = x.shape, w.shape[0]
    nks = K // 256
    if wrong == WRONG[2]:
        gamma, beta = np.roll(gamma, -8), np.roll(beta, -8)
    if wrong == WRONG[4] and nb == 2:
        n = np.arange(N)
        bias = bias[np.where((n // 16) % 2 == 1, n - 16, n)]
    inv_k, eps32 = F32(1.0) / F32(K), F32(eps)
    with np.errstate(all="ignore"):
        xa = x.reshape(Mi, 8, nks, 4, 8)                                 # k = wave * (K / 8) + u * 32 + fq * 8 + j
        mean = _pass1(xa) * inv_k
        va = xa - mean[:, None, None, None, None]
        if wrong == WRONG[0]:
            var = _pass1(xa * xa) * inv_k - mean * mean
            var = var + eps32
        else:
            q = _pass2(va)
            var = _fma(q, np.full_like(q, inv_k), np.full_like(q, eps32)) if contract else q * inv_k + eps32
        rstd = F32(1.0) / np.sqrt(var)
        if wrong == WRONG[1]:
            mean, rstd = np.roll(mean, -1), np.roll(rstd, -1)
            va = xa - mean[:, None, None, None, None]
        v = va.reshape(Mi, K) * rstd[:, None]
        op = _fma(v, np.broadcast_to(gamma, v.shape), np.broadcast_to(beta, v.shape)) if contract else v * gamma + beta
        h16 = gr.round_to(fmt, op).astype(F64)
        acc = np.zeros((8, Mi, N), F32)
        for wv in range(8):
            for u in range(nks):
                k0 = wv * (K // 8) + u * 32
                acc[wv] = acc[wv] + (h16[:, k0:k0 + 32] @ w[:, k0:k0 + 32].astype(F64).T).astype(F32)
        out = acc[0]
        for wv in range(1, 7 if wrong == WRONG[3] else 8):
            out = out + acc[wv]
        out = out + bias
        if gelu:
            out = gelu64(out.astype(F64))
        return gr.round_to(fmt, out)
