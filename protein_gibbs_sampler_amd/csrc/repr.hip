// Sequence representations: the residual stream x[M][d] of a requested layer as compact fp32 rows out[M][d_live] (with the final
// LayerNorm where the architecture has one), and sequential means of those rows over per-sequence token ranges.  Memory-bound, fp32 in
// and out: compiled once, no fp16 flavour.
//
// Layout rule of the row kernels (elementwise.hip): one 64-lane wave per token row, float4 per lane (16 B loads and stores), row bases
// as 64-bit products.  The LayerNorm is ln_row.h's ln_inplace on the same NCH ladder, so a normalised row equals launch_layernorm_f32's
// on the live columns bit for bit.
#include <type_traits>

#include "kernels.h"
#include "ln_row.h"

namespace pg {

// x[M][d] -> out[M][d_live]: the live columns of every row, normalised when gamma is given; a row whose token is pad_idx -> zeros
template <int NCH>
__global__ __launch_bounds__(256) void repr_rows_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const int32_t* __restrict__ tokens, int pad_idx,
                                                       float* __restrict__ out, int64_t M, int d, int d_live, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const int nl4 = d_live >> 2;
  float4* o = (float4*)(out + (size_t)row * d_live);
  if (tokens && tokens[row] == pad_idx) {
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      if (lane + 64 * i < nl4) o[lane + 64 * i] = make_float4(0.f, 0.f, 0.f, 0.f);
    return;
  }
  const float4* x4 = (const float4*)(x + (size_t)row * d);
  float4 v[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (lane + 64 * i < nl4) v[i] = x4[lane + 64 * i];
  if (gamma) ln_inplace(v, nl4, lane, d_live, eps, gamma, beta);
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (lane + 64 * i < nl4) o[lane + 64 * i] = v[i];
}

// in[B][T][d_live], ranges[n_pools][B][2] = (begin, count) -> out[n_pools][B][d_live].  One thread owns one float4 column of one
// (pool, sequence) and walks its rows in ascending order: acc = 0; acc = acc + v[t] per row; acc / float(count), every operation an
// explicitly rounded intrinsic.  No cross-lane step, no atomics.  The loads of eight rows are issued ahead; the adds stay in order.
__device__ __forceinline__ void pool_add(float4& a, const float4& v) {
  a.x = __fadd_rn(a.x, v.x); a.y = __fadd_rn(a.y, v.y); a.z = __fadd_rn(a.z, v.z); a.w = __fadd_rn(a.w, v.w);
}
__global__ __launch_bounds__(256) void repr_pool_kernel(const float* __restrict__ in, const int32_t* __restrict__ ranges,
                                                       float* __restrict__ out, int64_t n_items, int B, int T, int nl4) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n_items) return;
  const int64_t pb = i / nl4;                 // pool * B + sequence
  const int c4 = (int)(i - pb * nl4);
  const int b = (int)(pb % B);
  const int begin = ranges[2 * pb], count = ranges[2 * pb + 1];
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  if (count > 0) {
    const float4* p = (const float4*)in + ((size_t)b * T + begin) * nl4 + c4;
    int t = 0;
    for (; t + 8 <= count; t += 8) {
      float4 v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = p[(size_t)(t + j) * nl4];
#pragma unroll
      for (int j = 0; j < 8; ++j) pool_add(acc, v[j]);
    }
    for (; t < count; ++t) pool_add(acc, p[(size_t)t * nl4]);
    const float n = (float)count;
    acc.x = __fdiv_rn(acc.x, n); acc.y = __fdiv_rn(acc.y, n); acc.z = __fdiv_rn(acc.z, n); acc.w = __fdiv_rn(acc.w, n);
  }
  ((float4*)out)[i] = acc;
}

int launch_repr_rows(hipStream_t s, const float* x, const float* gamma, const float* beta, const int32_t* tokens, int pad_idx, float* out,
                     int64_t M, int d, int d_live, float eps) {
  if (d_live == 0) d_live = d;
  if (!row_d_ok(d)) return fail(1, "repr_rows: d must be a multiple of 4 and <= 2560, or a multiple of 512 up to 5120");
  if (!row_live_ok(d, d_live)) return fail(1, "repr_rows: the live width must be a multiple of 4, at most d");
  if ((gamma == nullptr) != (beta == nullptr)) return fail(1, "repr_rows: gamma and beta come together");
  if (M < 0 || (M + 3) / 4 > 0x7fffffffLL) return fail(1, "repr_rows: too many rows");
  if (M == 0) return 0;
  const dim3 grid((unsigned)((M + 3) / 4)), block(256);
  if (d > kMaxChWide * 256) hipLaunchKernelGGL(repr_rows_kernel<kMaxCh5k>, grid, block, 0, s, x, gamma, beta, tokens, pad_idx, out, M, d, d_live, eps);
  else if (d > kMaxCh * 256) hipLaunchKernelGGL(repr_rows_kernel<kMaxChWide>, grid, block, 0, s, x, gamma, beta, tokens, pad_idx, out, M, d, d_live, eps);
  else hipLaunchKernelGGL(repr_rows_kernel<kMaxCh>, grid, block, 0, s, x, gamma, beta, tokens, pad_idx, out, M, d, d_live, eps);
  PG_HIP(hipGetLastError());
  return 0;
}

// the ranges are device-resident: the caller has checked 0 <= begin, 0 <= count, begin + count <= T on the host (repr_pools_check)
int launch_repr_pool(hipStream_t s, const float* in, const int32_t* ranges, float* out, int n_pools, int B, int T, int d_live) {
  if (d_live < 4 || d_live % 4) return fail(1, "repr_pool: the row width must be a multiple of 4");
  if (n_pools < 0 || B < 0 || T < 1) return fail(1, "repr_pool: bad shape");
  const int64_t n_items = (int64_t)n_pools * B * (d_live >> 2);
  if (n_items == 0) return 0;
  if ((n_items + 255) / 256 > 0x7fffffffLL) return fail(1, "repr_pool: too many pooled values");
  hipLaunchKernelGGL(repr_pool_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, s, in, ranges, out, n_items, B, T, d_live >> 2);
  PG_HIP(hipGetLastError());
  return 0;
}

int repr_pools_check(const char* who, const int32_t* pools, int n_pools, int B, int T) {
  for (int64_t i = 0; i < (int64_t)n_pools * B; ++i) {
    const int64_t begin = pools[2 * i], count = pools[2 * i + 1];
    if (count < 0) return fail(PG_ERR_INVALID, std::string(who) + ": pool " + std::to_string(i / B) + " of sequence " + std::to_string(i % B) + " has a negative count");
    if (begin < 0 || begin + count > T)
      return fail(PG_ERR_INVALID, std::string(who) + ": pool " + std::to_string(i / B) + " of sequence " + std::to_string(i % B) + " leaves the token row [0, " + std::to_string(T) + "]");
  }
  return PG_OK;
}

}  // namespace pg
