"""Host restatements, in numpy float32, of the per-row arithmetic every LayerNorm-bearing kernel shares (csrc/ln_row.h): the wave
reduction, ln_inplace operation for operation, and store_row_bf16 -- the 16-bit rounding and the strict mode's split rows.  GPU tests
compare kernels with these bit for bit; the functions themselves need no GPU."""
import numpy as np

F32 = np.float32


def _fma32(a, b, c):
    """float32 fma(a, b, c) on arrays: the product is exact in double; the sum is rounded to double and then to float32, and the rare
    double rounding (the double sum lands exactly on a float32 tie) is repaired from the exact error of the double addition."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)                              # TwoSum: p + c = s + err exactly
    r = s.astype(F32)
    tie = (err != 0) & (((s.view(np.uint64) & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28)))
    if tie.any():
        up = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))  # move off the tie in the direction of the exact value
        r = np.where(tie, up.astype(F32), r)
    return r


def _wave_sum(v):
    """wave_sum of ln_row.h on [rows][64] float32: v += shfl_xor(v, o) for o = 32, 16, ... 1."""
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[:, lanes ^ o]).astype(F32)
    return v


def _ln_inplace_host(x, g, b, eps, sqrt_ulps=0):
    """ln_inplace (csrc/ln_row.h) in numpy float32, operation for operation: lane l holds float4 chunks l, l + 64, ...; per lane the
    chunks in ascending order, then the butterfly.  The one operation a host cannot restate is the square root: the device's is the
    hardware instruction, accurate to one ulp and not always the correctly rounded value -- `sqrt_ulps` moves the host's root by
    that many ulps."""
    M, d = x.shape
    nch4 = d // 4
    n_i = (nch4 + 63) // 64
    v = np.zeros((M, n_i, 64, 4), dtype=F32)
    have = np.zeros((n_i, 64), dtype=bool)
    for i in range(n_i):
        n = min(64, nch4 - 64 * i)
        v[:, i, :n] = x[:, 256 * i:256 * i + 4 * n].reshape(M, n, 4)
        have[i, :n] = True
    s = np.zeros((M, 64), dtype=F32)
    for i in range(n_i):
        t = ((v[:, i, :, 0] + v[:, i, :, 1]).astype(F32) + (v[:, i, :, 2] + v[:, i, :, 3]).astype(F32)).astype(F32)
        s = np.where(have[i], (s + t).astype(F32), s)
    mean = (_wave_sum(s) / F32(d)).astype(F32)                  # [M][64], every lane the same value
    q = np.zeros((M, 64), dtype=F32)
    for i in range(n_i):
        v[:, i] = (v[:, i] - mean[:, :, None]).astype(F32)
        c = v[:, i]
        t = (_fma32(c[..., 0], c[..., 0], (c[..., 1] * c[..., 1]).astype(F32)) +
             _fma32(c[..., 2], c[..., 2], (c[..., 3] * c[..., 3]).astype(F32))).astype(F32)
        q = np.where(have[i], (q + t).astype(F32), q)
    var = ((_wave_sum(q) / F32(d)).astype(F32) + F32(eps)).astype(F32)
    root = np.sqrt(var).astype(F32)
    for _ in range(abs(sqrt_ulps)):
        root = np.nextafter(root, F32(np.inf if sqrt_ulps > 0 else 0.0))
    rstd = (F32(1.0) / root).astype(F32)
    out = np.empty_like(x)
    for i in range(n_i):
        n = min(64, nch4 - 64 * i)
        gg = g[256 * i:256 * i + 4 * n].reshape(n, 4)
        bb = b[256 * i:256 * i + 4 * n].reshape(n, 4)
        y = _fma32((v[:, i, :n] * rstd[:, :n, None]).astype(F32), np.broadcast_to(gg, (M, n, 4)), np.broadcast_to(bb, (M, n, 4)))
        out[:, 256 * i:256 * i + 4 * n] = y.reshape(M, 4 * n)
    return out


# ---- store_row_bf16 -----------------------------------------------------------------------------------------------------------------
def bf16_bits(v):
    """float32 -> bfloat16 bits, round to nearest even (finite inputs): gfx950's v_cvt_pk_bf16_f32."""
    u = np.ascontiguousarray(v, dtype=F32).view(np.uint32)
    return ((u + (((u >> 16) & 1) + np.uint32(0x7fff))) >> 16).astype(np.uint16)


def f16_bits(v):
    """float32 -> IEEE half bits, round to nearest even."""
    return np.ascontiguousarray(v, dtype=F32).astype(np.float16).view(np.uint16)


def bf16_value(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


PLAIN, SPLIT_DUP, SPLIT_NODUP = 0, 1, 2      # the `form` of pg_dbg_layernorm_rows


def store_rows_host(v, form=PLAIN, f16=False, fill=None):
    """store_row_bf16 on rows v[M][d] float32 -> uint16 bits.  PLAIN: [M][d], each value rounded to the operand type.  Split forms
    (bf16): [M][3 d], per group of 32 columns 96 values [lo(32) | hi(32) | hi(32)] with hi = bf16(v), lo = bf16(v - hi), the
    subtraction in float32; SPLIT_NODUP leaves the third block of every group as `fill` (what the destination held before)."""
    v = np.ascontiguousarray(v, dtype=F32)
    M, d = v.shape
    if form == PLAIN:
        return f16_bits(v) if f16 else bf16_bits(v)
    assert not f16 and d % 32 == 0
    hi = bf16_bits(v)
    lo = bf16_bits((v - bf16_value(hi)).astype(F32))
    out = np.empty((M, d // 32, 3, 32), dtype=np.uint16)
    out[:, :, 0] = lo.reshape(M, d // 32, 32)
    out[:, :, 1] = hi.reshape(M, d // 32, 32)
    if form == SPLIT_DUP:
        out[:, :, 2] = out[:, :, 1]
    else:
        assert fill is not None
        out[:, :, 2] = np.asarray(fill, dtype=np.uint16).reshape(M, d // 32, 3, 32)[:, :, 2] if np.ndim(fill) else np.uint16(fill)
    return out.reshape(M, 3 * d)


def rows_not_from_host_loop(got, x, g, b, eps, form=PLAIN, f16=False, fill=None):
    """Indices of the rows of `got` (uint16 bits [M][d or 3 d]) that are NOT store(ln_host(x)) with the root of the variance at the
    correctly rounded value or one ulp either side -- the rule of test_layernorm_bits_equal_the_host_loop, row by row."""
    bad = np.arange(x.shape[0])
    for ulps in (0, -1, 1):
        if bad.size == 0:
            break
        f = fill[bad] if fill is not None and np.ndim(fill) else fill
        want = store_rows_host(_ln_inplace_host(np.ascontiguousarray(x[bad]), g, b, eps, ulps), form, f16, f)
        bad = bad[(got[bad] != want).any(axis=1)]
    return bad
