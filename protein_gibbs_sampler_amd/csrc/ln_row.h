// One LayerNorm row on one 64-lane wave -- the ONLY definition of the arithmetic, shared by every row kernel (elementwise.hip):
// a row's bf16 operand is bit-identical whichever kernel produced it.  Every floating-point operation is an explicitly rounded
// intrinsic, so no translation unit's contraction choices can differ.
#pragma once
#include "pg_common.h"
#include "split_operand.h"

PG_OPS_BEGIN

// A lane holds chunks lane, lane + 64, ... of the row as float4 v[NCH]: NCH is a template parameter of everything below, deduced
// from the array.  kMaxCh = 8 (d <= 2048) is the form every model up to d_model 2048 runs; kMaxChWide = 10 (d <= 2560: ESM-2 3B) costs 40 VGPRs per row instead of 32.
// kMaxCh5k = 20 (d <= 5120: ESM-2 15B) holds 80 VGPRs of row; above 2560 only whole 512-feature units are accepted (3072, 3584, ..
// 5120: kRowUnit5k), so every lane holds the same number of chunks there.
// The arithmetic and its order -- per lane the chunks in ascending order, then wave_sum -- do not depend on NCH.
constexpr int kMaxCh = 8;       // d <= 8 * 256 = 2048
constexpr int kMaxChWide = 10;  // d <= 10 * 256 = 2560
constexpr int kMaxCh5k = 20;    // d <= 20 * 256 = 5120, in units of kRowUnit5k
constexpr int kRowUnit5k = 512;
// the row widths the instantiations above cover: what the row launchers (elementwise.hip), their debug entries and the engine admit
constexpr bool row_d_ok(int d) {
  return d >= 4 && d % 4 == 0 && (d <= kMaxChWide * 256 || (d % kRowUnit5k == 0 && d <= kMaxCh5k * 256));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = __fadd_rn(v, __shfl_xor(v, o));
  return v;
}

// normalise the row held in v[] (chunk c = lane + 64*i) in place: (x-mean)/sqrt(var+eps)*g + b
template <int NCH>
__device__ __forceinline__ void ln_inplace(float4 (&v)[NCH], int nch4, int lane, int d, float eps,
                                           const float* __restrict__ gamma, const float* __restrict__ beta) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (lane + 64 * i < nch4) s = __fadd_rn(s, __fadd_rn(__fadd_rn(v[i].x, v[i].y), __fadd_rn(v[i].z, v[i].w)));
  const float mean = __fdiv_rn(wave_sum(s), (float)d);
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (lane + 64 * i < nch4) {
      v[i].x = __fsub_rn(v[i].x, mean); v[i].y = __fsub_rn(v[i].y, mean); v[i].z = __fsub_rn(v[i].z, mean); v[i].w = __fsub_rn(v[i].w, mean);
      q = __fadd_rn(q, __fadd_rn(__fmaf_rn(v[i].x, v[i].x, __fmul_rn(v[i].y, v[i].y)), __fmaf_rn(v[i].z, v[i].z, __fmul_rn(v[i].w, v[i].w))));
    }
  const float rstd = __fdiv_rn(1.0f, __fsqrt_rn(__fadd_rn(__fdiv_rn(wave_sum(q), (float)d), eps)));
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (lane + 64 * i < nch4) {
      const int c = lane + 64 * i;
      const float4 g = ((const float4*)gamma)[c], b = ((const float4*)beta)[c];
      v[i].x = __fmaf_rn(__fmul_rn(v[i].x, rstd), g.x, b.x);
      v[i].y = __fmaf_rn(__fmul_rn(v[i].y, rstd), g.y, b.y);
      v[i].z = __fmaf_rn(__fmul_rn(v[i].z, rstd), g.z, b.z);
      v[i].w = __fmaf_rn(__fmul_rn(v[i].w, rstd), g.w, b.w);
    }
}

// The row as 16-bit operand values; split3 (strict precision mode): as the split operand row of 3 * d bf16 values (split_operand.h:
// hi = bf16(v), lo = bf16(v - hi), per group of 32 columns [lo | hi | hi]); dup = false leaves the third block of every group unwritten.
template <int NCH>
__device__ __forceinline__ void store_row_bf16(bf16_t* dst, const float4 (&v)[NCH], int nch4, int lane, bool split3 = false,
                                               bool dup = true) {
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (lane + 64 * i < nch4) {
      const int ci = lane + 64 * i;              // float4 index = columns 4 ci .. 4 ci + 3
      uint2 p;
      p.x = pack_op2(v[i].x, v[i].y);
      p.y = pack_op2(v[i].z, v[i].w);
      if (!split3) {
        ((uint2*)dst)[ci] = p;
      } else {
        uint2 hi, lo;
        split4(v[i].x, v[i].y, v[i].z, v[i].w, hi, lo);
        split_store4(dst + split_group_offset(ci >> 3, (ci & 7) * 4), hi, lo, dup);
      }
    }
}

// Live width (an embedded model: engine.h d_live): the row is d wide in memory, its first d_live features are the model's own and
// the rest are structural zeros.  The kernels then load, normalise (ln_inplace with nch4 = d_live / 4 and d = d_live: the bits of a
// row of d_live features) and store the live chunks as above, and this writes the pad chunks nl4 .. nch4 - 1 of the output row as
// zeros, in the same two forms -- the buffer is reused and may hold anything, NaN patterns included.  No trip when d_live == d.
__device__ __forceinline__ void zero_row_pad_bf16(bf16_t* dst, int nl4, int nch4, int lane, bool split3 = false, bool dup = true) {
  const uint2 z = make_uint2(0u, 0u);
  for (int ci = nl4 + lane; ci < nch4; ci += 64) {
    if (!split3) ((uint2*)dst)[ci] = z;
    else split_store4(dst + split_group_offset(ci >> 3, (ci & 7) * 4), z, z, dup);
  }
}
// d_live of a row of d features: a multiple of 4, at most d
constexpr bool row_live_ok(int d, int d_live) { return d_live >= 4 && d_live % 4 == 0 && d_live <= d; }

PG_OPS_END
