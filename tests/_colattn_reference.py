"""Operands, reference and bounds of the kernel-level tests of the fused column QKV + attention kernel (csrc/gemm_colattn.hip; numpy
only; tests/test_colattn_reference_cpu.py checks this file without a GPU, tests/test_gpu_colattn_kernel.py holds the kernel to it).

The kernel computes, for an alignment batch x[B][R][C][d] (d = H * 64) and the engine's col_qkv weights w[3 d][d] / bias[3 d],
    [q | k | v] = round16(x w^T + bias),    ctx[b, r, c, h] = softmax_j(q[b, r, c, h] . k[b, j, c, h]) v[b, :, c, h],
the attention being the column attention of tests/_attention_reference.py on the 16-bit q, k, v.

Exact projection
----------------
The operands are built so that the projection has no rounding before its one 16-bit store: x holds integers, w integers times a power
of two g_w, bias integers times g = g_w (or a finer power of two), every one of them representable in bf16 and fp16.  A product of two
16-bit values is exact in fp32, so every partial sum of x w^T + bias, in any order, is an integer multiple of g; `exact_qkv` asserts
that sum_k |x_k| |w_k| + |bias| stays below 2^24 g, so no fp32 accumulation rounds, whatever its order or its K-step.  round16 of
that sum is then what ANY correct kernel stores, bit for bit: nothing is granted for the projection.

Families
--------
  integer   x in [-2, 2], w in [-2, 2] s with the q rows times a further 2^-2, bias in [-4, 4] s, s = 2^-ceil(log2(2 sqrt(d))): q of
            standard deviation 0.2 ... 0.3, k and v of 0.7 ... 1, a softmax that is neither flat nor one-hot.  Reference and bound:
            column_attention and bound of _attention_reference.py, unchanged -- the fused kernel claims the column kernel's arithmetic.
  uniform   integer with the q rows of w and the q bias zero: every score is 0, every exponential exactly 1, l = R a power of two, the
            numerator an exact fp32 sum of the 16-bit v (multiples of g below 2^24 g, asserted).  The context is the column mean of the
            exact v, rounded once: 16-bit rounding u |mean|, plus 1 / l and the product with it at 1.5 ulp, granted as 3 2^-24 |mean|,
            plus 2^-25 for an fp16 result on the subnormal grid:
                bound = u |mean| + 3 2^-24 |mean| (+ 2^-25, fp16).
            Derived, not fitted, and far tighter than the general bound: a wrong row, head, bias lane or weight permutation misses it by
            whole units.
  rowcode   one row r*(b, c) of every column holds a one-hot x (lane j(b, c), spread over the K-steps), every other row is zero.
            w_q = 0 and the q bias is 1, so every query is the all-ones vector; w_k = 1 and the k bias 0, so the key of r* scores 64 and
            every other key 0: margin 64 > 40, the other exponentials are below 2^-92 and multiply v = 0 exactly (the v bias is 0, x is
            zero there), l rounds to 1.  The context of EVERY row of column (b, c) in head h is therefore v of row r* exactly, and that
            is w_v[h*64 + f][j] = code(j, h, f), an integer in [-63, 63]: a context row stored at the wrong token row, alignment or head
            slice, a weight row fetched for the wrong head, is an exact mismatch.  Bound 0.
"""
import math

import numpy as np

import _attention_reference as ar

F32, F64 = np.float32, np.float64
FAMILIES = ("integer", "uniform", "rowcode")

# (B, R, C, H): the smallest shapes that reach each mechanism of the kernel (DESIGN.md has the table)
SHAPES = [
    (1, 32, 1, 1),       # 32 live rows in one tile, 7 pad sequences, a single K-step: no prefetch
    (1, 128, 1, 1),      # half a tile at KB = 8
    (1, 32, 9, 2),       # 288 rows: the second M-tile is 1 live + 7 pad sequences; two K-steps; two heads
    (3, 32, 8, 3),       # 3 full tiles x 3 heads = 9 workgroups (no multiple of the 8 XCDs); three K-steps; b changes inside the grid
    (2, 64, 3, 1),       # the alignment boundary (seq / C) falls inside one tile
    (1, 64, 5, 3),       # 320 rows, 6 workgroups
    (2, 128, 3, 2),      # two sequences of different (b, c) in one tile
    (1, 256, 3, 1),      # KB = 16: one sequence per tile, all 16 waves on it
    (2, 256, 1, 2),
    (5, 64, 5, 1),       # 7 M-tiles: grouped_tile<4> with a ragged last group
    (1, 32, 41, 2),      # 6 M-tiles
    (1, 32, 13, 12),     # the production width d = 768, twelve K-steps, 24 workgroups
]


def weight_scale(d):
    """s = 2^-ceil(log2(2 sqrt(d)))"""
    return 2.0 ** -math.ceil(math.log2(2.0 * math.sqrt(d)))


def rowcode_row(b, c, R, C):
    """r*: the one row of column (b, c) that holds a nonzero x"""
    return (3 * (b * C + c) + 1) % R


def rowcode_lane(b, c, C, d):
    """j: the lane of that row's one-hot x"""
    return (37 * (b * C + c) + 5) % d


def rowcode_value(j, h, f):
    return (5 * j + 3 * h + f) % 127 - 63


def operands(family, shape, seed=0):
    """x [B][R][C][d], w [3 d][d] (q rows first), bias [3 d] as float32, and g: the power of two every partial sum is a multiple of"""
    B, R, C, H = shape
    d = H * 64
    if family == "rowcode":
        x = np.zeros((B, R, C, d), F32)
        w = np.zeros((3 * d, d), F32)
        bias = np.zeros(3 * d, F32)
        bias[:d] = 1.0
        w[d:2 * d] = 1.0
        j, h, f = np.ogrid[:d, :H, :64]
        w[2 * d:] = rowcode_value(j, h, f).transpose(1, 2, 0).reshape(d, d)
        for b in range(B):
            for c in range(C):
                x[b, rowcode_row(b, c, R, C), c, rowcode_lane(b, c, C, d)] = 1.0
        return x, w, bias, 1.0
    rng = np.random.default_rng([seed, B, R, C, H, FAMILIES.index(family)])
    s = weight_scale(d)
    x = rng.integers(-2, 3, (B, R, C, d)).astype(F32)
    w = rng.integers(-2, 3, (3 * d, d)).astype(F64) * s
    bias = rng.integers(-4, 5, 3 * d).astype(F64) * s
    w[:d] *= 0.25
    if family == "uniform":
        w[:d] = 0.0
        bias[:d] = 0.0
    return x, w.astype(F32), bias.astype(F32), s / 4


def exact_qkv(fmt, x, w, bias, g):
    """round16(x w^T + bias) [B][R][C][3 d] as float32, after asserting the construction of the module docstring: operands representable
    in fmt, everything on the grid g, every partial sum below 2^24 g -- so that fp32 accumulation in any order is exact"""
    for a in (x, w, bias):
        assert (ar.round_to(fmt, a) == a).all(), "an operand is not representable in " + fmt
        assert (np.asarray(a, F64) / g == np.rint(np.asarray(a, F64) / g)).all(), "an operand is off the grid"
    x64, w64, b64 = (np.asarray(a, F64) for a in (x, w, bias))
    worst = (np.abs(x64) @ np.abs(w64).T + np.abs(b64)).max() / g
    assert worst < 2.0 ** 24, worst
    acc = x64 @ w64.T + b64
    assert (acc.astype(F32).astype(F64) == acc).all()
    return ar.round_to(fmt, acc.astype(F32))


def to_colmajor(x):
    """rows in token order (b*R + r)*C + c, given as [B][R][C][d] -> [B*C*R][d] with row (b*C + c)*R + r: the fused kernel's operand"""
    B, R, C, d = x.shape
    return np.ascontiguousarray(x.transpose(0, 2, 1, 3)).reshape(B * C * R, d)


def from_colmajor(rows, B, R, C):
    return np.ascontiguousarray(rows.reshape(B, C, R, -1).transpose(0, 2, 1, 3))


def uniform_bound(mean, fmt):
    m = np.abs(mean)
    return ar.U[fmt] * m + 3 * 2.0 ** -24 * m + (2.0 ** -25 if fmt == "f16" else 0.0)


def expected(family, fmt, shape, qkv):
    """(ref, bound) [B][R][C][d] float64 for the exact 16-bit qkv of a family; the family's own assertions on qkv are made here"""
    B, R, C, H = shape
    d = H * 64
    if family == "integer":
        res = ar.column_attention(qkv, H)
        return res.ref, ar.bound(res, fmt)
    q, k, v = (np.asarray(qkv[..., i * d:(i + 1) * d], F64) for i in range(3))
    if family == "uniform":
        assert not q.any()
        mean = np.broadcast_to(v.mean(1, keepdims=True), v.shape).copy()      # exact: R is a power of two, the sum below 2^24 g
        return mean, uniform_bound(mean, fmt)
    assert family == "rowcode"
    ref = np.empty((B, R, C, d))
    for b in range(B):
        for c in range(C):
            rs = rowcode_row(b, c, R, C)
            ref[b, :, c] = v[b, rs, c]
            others = np.arange(R) != rs
            assert not v[b, others, c].any()
            for h in range(H):
                sl = slice(h * 64, (h + 1) * 64)
                a = q[b, :, c, sl] @ k[b, :, c, sl].T                      # [query][key]
                assert (a[:, rs] - a[:, others].max(1) > 40.0).all()
            j = rowcode_lane(b, c, C, d)
            hh, ff = np.ogrid[:H, :64]
            assert (ref[b, 0, c] == rowcode_value(j, hh, ff).reshape(d)).all()
    return ref, np.zeros_like(ref)


def kernel_model_context(fmt, shape, qkv):
    """ar.kernel_model (the numpy model of the 16-bit kernels' six steps) on the columns of qkv -> [B][R][C][d] float32"""
    B, R, C, H = shape
    q, k, v = (x.transpose(0, 2, 3, 1, 4).reshape(B * C, H, R, 64).astype(F32) for x in ar._heads(qkv, H, 64))
    out = ar.kernel_model(q, k, v, fmt)
    return out.reshape(B, C, H, R, 64).transpose(0, 3, 1, 2, 4).reshape(B, R, C, H * 64)
