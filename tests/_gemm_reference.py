"""The references of the GEMM kernel tests, the input families they run and the table of cases (numpy only;
tests/test_gemm_reference_cpu.py checks this file without a GPU, tests/test_gpu_gemm_kernels.py holds the kernels to it).

Semantics (csrc/gemm_bf16.hip):  out[M][N] = x[M][K] . w[N][K]^T + bias[N]  (+ residual, or through GELU), fp32 accumulation of
16-bit operands by the MFMA, every epilogue fused.  The debug entry takes fp32 host arrays and converts them on the device.

The exact families
------------------
`integers`: x and w are integers in [-8, 8].  They convert exactly to bf16 (8 significant bits) and to fp16 (11), every product
is an integer of magnitude <= 64, and with
        sum_k |x_k| |w_k| + |bias| + |residual| < 2^24          (asserted per case; K <= 5120 gives at most 327 680 + 2^21)
every partial sum any kernel can form -- any k order, any split of K over waves or workgroups, bias and residual added at any point
-- is an integer below 2^24 and therefore exact in fp32.  The output is then ONE value whatever the summation order: the int64
result, bit for bit.  A dropped, doubled or misplaced k, row, column, tile, split, bias or residual moves an output by at least 1.
Column 0 of x carries a row-dependent and column 1 of w a column-dependent entry, so a transposed operand or output cannot pass.
16-bit outputs (dbg epi 3) are the round-to-nearest-even conversion of that integer: bias magnitudes of 3000 ... 40000 put |out|
above 2048, where neither bf16 (integers exact up to 256) nor fp16 (up to 2048) holds every integer, and below fp16's largest
finite value 65504; at least a quarter of the outputs are changed by the rounding in either flavour (asserted per case; in practice
more than 85 %) and exact ties -- bf16: out = 8 mod 16 at |out| in [2048, 4096) -- make up about 1 % (bf16) and 9 % (fp16) of the
outputs, hundreds per case, which pins the tie rule.

`strict_integers` (PG_PREC_FP32): the same small integers, and in every row of x and of w a few 9-bit values +/-257 and +/-385.
Their split (split_operand.h) is hi = 256 or 384 (a tie, rounded to even) and lo = 1 -- both exact bf16.  The kernels sum, per
32 columns, x_lo.w_hi + x_hi.w_lo + x_hi.w_hi and never x_lo.w_lo; the reference is that definition in int64,
        ref = sum_k (xh wh + xl wh + xh wl) + bias (+ residual)   =   x . w^T - sum_k xl wl + ...
again exact in fp32 under the same headroom condition (asserted), again bit for bit.  Some 9-bit values of an x row share their k
with one of a w row (there the dropped xl wl = +/-1 shows) and most do not; a lo block read from the wrong group or the wrong block of
the layout changes a product of lo = 1 with a non-zero hi.

The GELU family
---------------
`gelu_inputs`: x, w in {-1, 0, 1} with density sqrt(3.5 / K) and bias in multiples of 1/8 in [-1, 1]: the pre-activation
z = x . w^T + b is exact in every mode (var z about 4; at least half of the |z| are <= 4, asserted), so the only error left is the
epilogue's, against float64 erf-GELU, per element:
  * gelu_erf (dbg epi 1, fp32 out): gemm_epilogue.h documents |erf error| <= 1.5e-7, which enters as 0.5 |z| times it;
  * gelu_poly2 (dbg epi 4, 16-bit out; strict epi 5, (hi, lo) pair out): documented absolute error 3.2e-6;
  * both documented figures are taken TIMES 2 (nobody measured them through a kernel: one ulp each for v_exp_f32 and v_rcp_f32);
  * plus the output type's half ulp on the computed value: 2^-24 (fp32), 2^-8 (bf16), 2^-11 (fp16; 2^-25 absolute below 2^-14),
    2^-16 for the pair, relative.
None of these figures is fitted to what a kernel returns; the worst measured fraction of the bound is recorded in DESIGN.md.

The cases
---------
CASES lists (kernel, how it is reached, shape, epilogues); which shapes and why: see the comment above it.  `launched_rows` restates
the debug entry's row rule, `expected_plan` the text the launch must record where it does not depend on the CU count.
"""
from collections import namedtuple

import numpy as np

F32, F64, I64 = np.float32, np.float64, np.int64
EPI_INTERNAL = {0: 3, 1: 4, 2: 2, 3: 0, 4: 1}      # dbg epi -> EPI_* of csrc/kernels.h (pg_dbg_gemm_plan's argument)
HEADROOM = 2 ** 24
ERF_DOC, POLY_DOC = 1.5e-7, 3.2e-6                # gemm_epilogue.h
U_OUT = {"f32": 2.0 ** -24, "bf16": 2.0 ** -8, "f16": 2.0 ** -11, "pair": 2.0 ** -16}


def round_to(fmt, a):
    """round-to-nearest-even of float64 / integer values to bf16 or fp16, as float32"""
    if fmt == "f16":
        return np.asarray(a, F64).astype(np.float16).astype(F32)
    a32 = np.asarray(a, F64).astype(F32)              # the exact families' values are integers below 2^24: exact
    u = np.ascontiguousarray(a32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(F32)


def _matmul_exact(a, b):
    """integer-valued a . b^T through float64 BLAS: every partial sum is an integer far below 2^53"""
    return np.rint(a.astype(F64) @ b.astype(F64).T).astype(I64)


Exact = namedtuple("Exact", "x w bias res ref mag")
Exact.__doc__ = """x, w, bias, res: float32 inputs (res: the residual the output buffer holds; None without one); ref: int64 result;
mag: sum_k |x||w| + |bias| + |res| per output, the headroom condition's left side"""


def _small_ints(rng, M, N, K):
    x = rng.integers(-8, 9, (M, K)).astype(F32)
    w = rng.integers(-8, 9, (N, K)).astype(F32)
    x[:, 0] = (np.arange(M) % 17) - 8               # row-dependent
    w[:, 1 % K] = (np.arange(N) % 15) - 7           # column-dependent
    return x, w


def integers(M, N, K, seed, residual=False, out16=False):
    rng = np.random.default_rng([seed, M, N, K])
    x, w = _small_ints(rng, M, N, K)
    if out16:
        bias = (rng.integers(3000, 40001, N) * rng.choice([-1, 1], N)).astype(F32)
    else:
        bias = rng.integers(-2 ** 20, 2 ** 20 + 1, N).astype(F32)
    res = rng.integers(-2 ** 20, 2 ** 20 + 1, (M, N)).astype(F32) if residual else None
    ref = _matmul_exact(x, w) + bias.astype(I64)
    mag = _matmul_exact(np.abs(x), np.abs(w)) + np.abs(bias).astype(I64)
    if residual:
        ref = ref + res.astype(I64)
        mag = mag + np.abs(res).astype(I64)
    return Exact(x, w, bias, res, ref, mag)


def split_pair(a):
    """bf16 (hi, lo) of float32 values, as split_operand.h defines them: hi = bf16(v), lo = bf16(v - hi)"""
    hi = round_to("bf16", a)
    return hi, round_to("bf16", np.asarray(a, F32) - hi)


NINE_BIT = (257, -385, 385, -257)


def strict_integers(M, N, K, seed, residual=False):
    rng = np.random.default_rng([seed, M, N, K, 3])
    x, w = _small_ints(rng, M, N, K)
    for t, v in enumerate(NINE_BIT[:3]):            # three per row: k = (3 i + 11 t) % K in x, (5 j + 11 t + 1) % K in w
        x[np.arange(M), (3 * np.arange(M) + 11 * t) % K] = v
        w[np.arange(N), (5 * np.arange(N) + 11 * t + 1) % K] = NINE_BIT[t + 1]
    bias = rng.integers(-2 ** 20, 2 ** 20 + 1, N).astype(F32)
    res = rng.integers(-2 ** 20, 2 ** 20 + 1, (M, N)).astype(F32) if residual else None
    (xh, xl), (wh, wl) = split_pair(x), split_pair(w)
    assert (xh + xl == x).all() and (wh + wl == w).all()
    ref = _matmul_exact(xh, wh) + _matmul_exact(xl, wh) + _matmul_exact(xh, wl) + bias.astype(I64)
    ax, aw = np.abs(xh) + np.abs(xl), np.abs(wh) + np.abs(wl)
    mag = _matmul_exact(ax, aw) + np.abs(bias).astype(I64)
    if residual:
        ref = ref + res.astype(I64)
        mag = mag + np.abs(res).astype(I64)
    return Exact(x, w, bias, res, ref, mag)


def shared_nine_bit(e):
    """fraction of the (row of x, row of w) pairs in which a 9-bit value of one meets a 9-bit value of the other at the same k"""
    return float((_matmul_exact(np.abs(e.x) > 8, np.abs(e.w) > 8) > 0).mean())


Gelu = namedtuple("Gelu", "x w bias z ref")


def gelu_inputs(M, N, K, seed):
    rng = np.random.default_rng([seed, M, N, K, 7])
    p = min(1.0, np.sqrt(3.5 / K))
    x = (rng.integers(-1, 2, (M, K)) * (rng.random((M, K)) < p * 1.5)).astype(F32)      # P(non-zero) = 2/3 * 1.5 p = p
    w = (rng.integers(-1, 2, (N, K)) * (rng.random((N, K)) < p * 1.5)).astype(F32)
    x[:, 0] = (np.arange(M) % 3) - 1
    w[:, 1 % K] = (np.arange(N) % 3) - 1
    bias = (rng.integers(-8, 9, N) / 8.0).astype(F32)
    z = x.astype(F64) @ w.astype(F64).T + bias.astype(F64)
    from scipy.special import erf
    return Gelu(x, w, bias, z, 0.5 * z * (1.0 + erf(z / np.sqrt(2.0))))


def gelu_bound(g, epi, out):
    """per element; epi: dbg epi 1 (gelu_erf), 4 or 5 (gelu_poly2); out: "f32", "bf16", "f16" or "pair" """
    fit = 2 * ERF_DOC * 0.5 * np.abs(g.z) if epi == 1 else np.full(g.z.shape, 2 * POLY_DOC)
    b = fit + U_OUT[out] * (np.abs(g.ref) + fit)
    return b + (2.0 ** -25 if out == "f16" else 0.0)


# ---- the float32 restatement and the wrong models (test_gemm_reference_cpu.py) -------------------------------------------------------
def restate_f32(x, w, bias, res, splits, rng, products=None):
    """The kernels' arithmetic in float32 numpy: k walked in 64-wide tiles in a shuffled order, per-split partials summed in fixed
    order, then bias and residual.  products: [(a, b), ...] operand pairs summed per tile (the strict three products); default x . w"""
    products = products or [(x, w)]
    K = x.shape[1]
    Ks = K // splits
    parts = []
    for s in range(splits):
        acc = np.zeros((x.shape[0], w.shape[0]), F32)
        for t in rng.permutation(Ks // 64 if Ks % 64 == 0 else Ks // 32):
            step = 64 if Ks % 64 == 0 else 32
            k0 = s * Ks + t * step
            for a, b in products:
                acc = acc + (a[:, k0:k0 + step] @ b[:, k0:k0 + step].T).astype(F32)
        parts.append(acc)
    out = bias.astype(F32)[None, :] + parts[0] if splits > 1 else parts[0] + bias.astype(F32)[None, :]
    for p in parts[1:]:
        out = out + p
    return out + res if res is not None else out


def wrong_models(e, splits, tail_row0, products=None):
    """name -> int64 result of four wrong kernels on the exact inputs e (None where the model does not apply)"""
    products = products or [(e.x, e.w)]
    K, N = e.x.shape[1], e.w.shape[0]
    out = {}
    d = sum(_matmul_exact(a[:16, K - 64:], b[:, K - 64:]) for a, b in products)     # rows 0..15 lose the last k-tile
    out["last k-tile dropped for one 16-row block"] = e.ref.copy()
    out["last k-tile dropped for one 16-row block"][:16] -= d
    b = e.bias.astype(I64)
    out["bias shifted by four columns"] = e.ref - b + np.roll(b, -4)
    out["residual added twice on the first tail-tile row"] = None
    if e.res is not None and tail_row0 is not None:
        r = e.ref.copy()
        r[tail_row0] += e.res[tail_row0].astype(I64)
        out["residual added twice on the first tail-tile row"] = r
    out["one K-split left out"] = None
    if splits > 1:
        Ks = K // splits
        out["one K-split left out"] = e.ref - sum(_matmul_exact(a[:, K - Ks:], b[:, K - Ks:]) for a, b in products)
    return out


# ---- the cases -----------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "kernel variant have_ws M N K epis strict")
Case.__doc__ = """kernel: the plan text's label the case is meant to run (a second label after " + "); variant / have_ws:
pg_dbg_gemm_v's; epis: dbg epilogues; strict: PG_PREC_FP32 (else both 16-bit flavours)"""


def launched_rows(M):
    """the rows pg_dbg_gemm_v hands the 16-bit launcher: 16-row padding up to 256 rows, 256-row padding above (strict: always)"""
    return (M + 15) // 16 * 16 if M <= 256 else (M + 255) // 256 * 256


def splitk_splits(K):
    return K // 1280 if K % 1280 == 0 else (K // 1024 if K % 1024 == 0 else 1)


def _cases():
    """The smallest shapes at which each kernel can still go wrong: more than one tile per grid dimension; K-tile counts minimal
    (64, or 128 where the kernel needs two), odd (192 = 3, 320 = 5) and deep (1280); M below, at and above a tile / padding edge
    where the plan admits it.  Per kernel: every (M, N) at the odd K and every K at one (M, N), not the full product."""
    c = []

    def grid(kernel, variant, Ms, Ns, Ks, epis, have_ws=-1, strict=False):
        seen = set()
        for M in Ms:
            for N in Ns:
                seen.add((M, N, Ks[1]))
        for K in Ks:
            seen.add((Ms[-1], Ns[-1], K))
        for M, N, K in sorted(seen):
            c.append(Case(kernel, variant, have_ws, M, N, K, epis, strict))

    # weight streaming: 16 / 32 / 64 rows per workgroup (M 48 is the 64-row instance), 4 waves (K % 256 != 0) and 8 waves
    grid("skinny4w", 2, (1, 16, 17, 32, 48), (64, 320), (64, 192, 320), (0, 1, 2, 3, 4))
    grid("skinny8w", 2, (1, 16, 17, 32, 48), (64, 320), (256, 1280, 768), (0, 2, 3))
    grid("tile64x64", 2, (49, 64, 65, 129, 256), (64, 192), (64, 192, 320, 1280), (0, 1, 2, 3, 4))
    grid("tile64x64", 6, (320,), (64, 192), (64, 192, 320), (0, 2, 3))
    grid("tile128x128", 7, (128, 384), (128, 384), (64, 192, 320, 1280), (0, 1, 2, 3, 4))
    grid("tile256x256-lockstep", 1, (512,), (256, 512), (128, 192, 320, 1280), (0, 1, 2, 3, 4))
    grid("pp256x256", 20, (512, 768), (256, 512), (128, 192, 320, 1280), (0, 1, 2, 3, 4))
    grid("pp192x256", 8, (256, 512, 768), (256, 512), (128, 192, 320, 1280), (2,))          # leftovers 64, 128, 0 as tail tiles
    grid("w16-256x256", 80, (512, 768), (256, 512), (128, 192, 320, 1280), (0, 1, 2, 3, 4))
    # split-K (residual, scratch on offer): every split count of gemm_splitk_splits for K = 2048 (2), 3072 (3), 5120 (4), on the
    # three kernels that split; (8 x 16, 8 x 11, 8 x 8) tiles of 128^2 are what "enough128" and "small" of plan_gemm admit together
    for K, n128 in ((2048, 2048), (3072, 1408), (5120, 1024)):
        for ws in (1, 0):
            c.append(Case("skinny8w", 2, ws, 32, 128, K, (2,), False))
            c.append(Case("tile64x64", 2, ws, 129, 128, K, (2,), False))
            c.append(Case("tile128x128" if ws else "tile64x64", 2, ws, 1024, n128, K, (2,), False))
    # strict plain (the 16-bit tile kernels over K' = 3 K, every row padded to 256) and the fused fc1 epilogue; below one round of
    # 256 x 256 tiles the fused kernel's grid is tail tiles only, its 256 x 256 form runs in BIG_STRICT
    grid("tile64x64", -1, (40, 256, 513), (128, 256), (64, 192), (0, 2), strict=True)
    grid("gemm_split3_w16", -1, (256, 512), (256, 512), (64, 192), (5,), strict=True)
    return c


CASES = _cases()
# one production-dispatch shape whose grid holds 256 x 256 tiles and a panel of tail tiles: on 256 CUs 272 tiles = one round + 16
PRODUCTION_TAIL = (4352, 4096, 128)
# strict fused kernel at the smallest shapes with a full round of tiles on 256 CUs: 256 tiles, and 260 = one round + a tail panel
BIG_STRICT = ((16384, 1024, 64), (16640, 1024, 64))


def expected_plan(c):
    """the text a case's launch must record, where it does not depend on the CU count (else the label alone)"""
    rows, n = launched_rows(c.M), c.N
    if c.strict:
        rows = (c.M + 255) // 256 * 256
    splits = splitk_splits(c.K) if c.have_ws == 1 and 2 in c.epis else 1
    sk = " x%dk" % splits if splits > 1 else ""
    k = c.kernel
    if k.startswith("skinny"):
        return "%s %dt%s" % (k, n // 16, sk)
    if k == "tile64x64":
        return "%s %dt%s" % (k, (rows + 63) // 64 * (n // 64), sk)
    if k == "tile128x128":
        return "%s %dt%s" % (k, rows // 128 * (n // 128), sk)
    if k == "pp192x256":
        left = rows % 192
        return "%s %dt" % (k, rows // 192 * (n // 256)) + (" + tail64 %dt" % (left // 64 * (n // 64)) if left else "")
    if k == "gemm_split3_w16":
        return k                                        # how many rows are tail tiles depends on the CU count
    return "%s %dt" % (k, rows // 256 * (n // 256))
