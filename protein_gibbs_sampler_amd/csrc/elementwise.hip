// Memory-bound kernels of the forward pass (HBM roofline): token embedding + token-dropout rescale +
// learned positions + LayerNorm, LayerNorm (fp32 residual -> bf16 GEMM operand), gather+LayerNorm of
// the sampled rows, and the LM-head tail (LayerNorm -> tied decoder -> logits).
//
// They restate, for the GPU, steps 1-4, the pre-LN of step 5, and steps 6-7 of the ESM-1b forward
// (fair-esm ProteinBertModel.forward) that the reference reaches through
// `self.model.model(batch)["logits"]` (/root/reference/src/pgen/esm_sampler.py:223), and step 1-2/4
// of MSATransformer.forward (A.3; esm_msa_sampler.py:136,236).
//
// Layout rule: one 64-lane wave per token row; a row of d fp32 is read as float4 per lane
// (16 B x 64 lanes = 1 KiB coalesced per instruction); mean/variance by wave shuffle reductions;
// nothing goes through LDS.
#include <stdlib.h>

#include <type_traits>

#include "kernels.h"
#include "ln_row.h"

PG_OPS_BEGIN

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// the row of this wave: 256 threads = four rows per workgroup (rows_grid)
__device__ __forceinline__ int64_t wave_row() { return (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); }
// the lane's chunks lane, lane + 64, ... of a row of nch4 float4 that starts at src
template <int NCH>
__device__ __forceinline__ void load_row(float4 (&v)[NCH], const float* src, int nch4, int lane) {
  const float4* x4 = (const float4*)src;
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (lane + 64 * i < nch4) v[i] = x4[lane + 64 * i];
}

// ---- embedding -------------------------------------------------------------------------------
// tokens[n_seq][T] -> x[n_seq*T][d] fp32 = LN_before(embed[tok]*scale + pos[...] (+ msa_row_pos[r]))
// pos == nullptr (ESM-2): nothing is added; gamma == nullptr (ESM-1, ESM-2): no LN_before.
// token_dropout (ESM-1b): mask rows zeroed, all rows scaled by 0.88 / (1 - n_mask/src_len) per sequence.
// rows_per_msa > 0 (MSA-1b): adds msa_pos[seq % rows_per_msa].
template <int NCH>
__global__ __launch_bounds__(256) void embed_ln_kernel(const int32_t* __restrict__ tokens, const float* __restrict__ embed,
                                                      const float* __restrict__ pos, const float* __restrict__ msa_pos,
                                                      const float* __restrict__ gamma, const float* __restrict__ beta,
                                                      float* __restrict__ x, int64_t n_tok, int T, int d, int pad_idx,
                                                      int mask_idx, int token_dropout, int rows_per_msa, float eps,
                                                      const float* __restrict__ gamma2, const float* __restrict__ beta2,
                                                      bf16_t* __restrict__ h2, float embed_scale, int d_live) {
  const int lane = threadIdx.x & 63;
  const int64_t row = wave_row();
  if (row >= n_tok) return;
  const int64_t seq = row / T;
  const int t = (int)(row - seq * T);
  const int32_t* trow = tokens + seq * T;
  const int tok = trow[t];
  // per-sequence counts: masks, non-pad tokens, non-pad tokens at or before t
  int n_mask = 0, n_nonpad = 0, n_before = 0;
  for (int j = lane; j < T; j += 64) {
    const int tj = trow[j];
    n_mask += (tj == mask_idx);
    n_nonpad += (tj != pad_idx);
    n_before += (tj != pad_idx) && (j <= t);
  }
  n_mask = wave_sum_i(n_mask);
  n_nonpad = wave_sum_i(n_nonpad);
  n_before = wave_sum_i(n_before);
  const bool is_pad = (tok == pad_idx);
  float scale = embed_scale;               // 1 (ESM-1b, MSA-1b); sqrt(d) for ESM-1
  if (token_dropout) {
    scale = (1.0f - 0.15f * 0.8f) / (1.0f - (float)n_mask / (float)n_nonpad);
    if (tok == mask_idx) scale = 0.0f;
  }
  const int p = is_pad ? pad_idx : n_before + pad_idx;
  const int nch4 = d >> 2;
  const float4* e4 = (const float4*)(embed + (size_t)tok * d);
  const float4* p4 = pos ? (const float4*)(pos + (size_t)p * d) : nullptr;      // pos == nullptr: no position table (ESM-2: rotary)
  const float4* r4 = rows_per_msa > 0 ? (const float4*)(msa_pos + (size_t)(seq % rows_per_msa) * d) : nullptr;
  float4 v[NCH];
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (lane + 64 * i < nch4) {
      const int c = lane + 64 * i;
      const float4 e = e4[c], q = p4 ? p4[c] : make_float4(0.f, 0.f, 0.f, 0.f);
      v[i] = make_float4(e.x * scale + q.x, e.y * scale + q.y, e.z * scale + q.z, e.w * scale + q.w);
      if (r4) {
        const float4 r = r4[c];
        v[i].x += r.x; v[i].y += r.y; v[i].z += r.z; v[i].w += r.w;
      }
    }
  if (gamma) ln_inplace(v, nch4, lane, d, eps, gamma, beta);      // gamma == nullptr: no emb_layer_norm_before (ESM-1)
  float4* o = (float4*)(x + (size_t)row * d);
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (lane + 64 * i < nch4) {
      if (is_pad) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
      o[lane + 64 * i] = v[i];
    }
  if (h2) {      // the first layer's LayerNorm on the row just written (same values, same code as layernorm_bf16_kernel: same bits)
    const int nl4 = d_live >> 2;      // an embedded model (ln_row.h): over the live features, zeros behind them
    ln_inplace(v, nl4, lane, d_live, eps, gamma2, beta2);
    store_row_bf16(h2 + (size_t)row * d, v, nl4, lane);
    zero_row_pad_bf16(h2 + (size_t)row * d, nl4, nch4, lane);
  }
}

// ---- LayerNorm: x fp32 [M][d] -> h bf16 [M][d] ------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(256) void layernorm_bf16_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, bf16_t* __restrict__ h,
                                                            int split3, int64_t M, int d, float eps, int d_live) {
  const int lane = threadIdx.x & 63;
  const int64_t row = wave_row();
  if (row >= M) return;
  const int nch4 = d >> 2, nl4 = d_live >> 2;      // d_live < d: an embedded model's row (ln_row.h)
  float4 v[NCH];
  load_row(v, x + (size_t)row * d, nl4, lane);
  ln_inplace(v, nl4, lane, d_live, eps, gamma, beta);
  bf16_t* o = h + (size_t)row * d * (split3 ? 3 : 1);
  store_row_bf16(o, v, nl4, lane, split3, split3 != 2);       // split3 == 2: no duplicate hi block
  zero_row_pad_bf16(o, nl4, nch4, lane, split3, split3 != 2);
}

// Mid-size batches (a 32 ... 128-chain shard of a multi-GPU job: 8 k ... 33 k token rows): with one row per wave the grid is 1.03 ...
// 4 "rounds" of what the chip holds at once (8 workgroups of 4 waves per CU), and the last, nearly empty round costs a whole
// row latency -- 14.9 us for 8448 rows where an eighth of the full-size launch is 10.4 (profiles/r05_shard_timeline_32chains.txt).
// Here the grid is exactly one resident round and every wave walks its rows (row, row + waves, ...) with the NEXT row's loads issued
// before the current row is normalised.  Same per-row arithmetic (ln_inplace, store_row_bf16): same bits.
// (the row width is a template parameter: with it the chunks a lane does not hold leave the register file -- 2 x 5 float4 at
// d = 1280 instead of 2 x 8 -- and eight workgroups per CU stay resident, as for the plain kernel)
template <int D>
__global__ __launch_bounds__(256) void layernorm_bf16_stride_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta, bf16_t* __restrict__ h,
                                                                   int split3, int64_t M, float eps) {
  constexpr int d = D, nch4 = D >> 2;
  const int lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * 4;
  int64_t row = wave_row();
  if (row >= M) return;
  float4 v[kMaxCh], vn[kMaxCh];
  load_row(v, x + (size_t)row * d, nch4, lane);
  for (;;) {
    const int64_t next = row + stride;
    if (next < M) load_row(vn, x + (size_t)next * d, nch4, lane);      // wave-uniform
    ln_inplace(v, nch4, lane, d, eps, gamma, beta);
    store_row_bf16(h + (size_t)row * d * (split3 ? 3 : 1), v, nch4, lane, split3, split3 != 2);
    if (next >= M) break;
#pragma unroll
    for (int i = 0; i < kMaxCh; ++i) v[i] = vn[i];
    row = next;
  }
}

// The same with the output rows in COLUMN-MAJOR token order: token row (b*R + r)*C + c -> operand row (b*C + c)*R + r, so that a
// column's R tokens are contiguous rows for the fused column QKV + attention kernel (gemm_colattn.hip).  A separate kernel: the hot
// LayerNorm above stays as it is.
__global__ __launch_bounds__(256) void layernorm_bf16_colmajor_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                                     const float* __restrict__ beta, bf16_t* __restrict__ h,
                                                                     int64_t M, int d, float eps, int R, int C) {
  const int lane = threadIdx.x & 63;
  const int64_t row = wave_row();
  if (row >= M) return;
  const int nch4 = d >> 2;
  float4 v[kMaxCh];
  load_row(v, x + (size_t)row * d, nch4, lane);
  ln_inplace(v, nch4, lane, d, eps, gamma, beta);
  const int64_t br = row / C;
  const int c = (int)(row - br * C);
  const int64_t b = br / R;
  const int r = (int)(br - b * R);
  store_row_bf16(h + (size_t)((b * C + c) * R + r) * d, v, nch4, lane);
}

// fp32 -> fp32 LayerNorm (debug entry / strict paths)
template <int NCH>
__global__ __launch_bounds__(256) void layernorm_f32_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ y,
                                                           int64_t M, int d, float eps, int d_live) {
  const int lane = threadIdx.x & 63;
  const int64_t row = wave_row();
  if (row >= M) return;
  const int nch4 = d >> 2, nl4 = d_live >> 2;
  float4 v[NCH];
  load_row(v, x + (size_t)row * d, nl4, lane);
  ln_inplace(v, nl4, lane, d_live, eps, gamma, beta);
  float4* o = (float4*)(y + (size_t)row * d);
#pragma unroll
  for (int i = 0; i < NCH; ++i)
    if (lane + 64 * i < nl4) o[lane + 64 * i] = v[i];
  for (int ci = nl4 + lane; ci < nch4; ci += 64) o[ci] = make_float4(0.f, 0.f, 0.f, 0.f);      // an embedded model's pad features
}

// ---- gather the sampled rows + final LayerNorm -> bf16 (LM-head dense operand) ---------------
// sel r -> token row row_of(r) * width + idx[r]; idx < 0 (ragged padding) -> row of zeros.
// row_map == nullptr: selected row s = r / P maps to token row s.
template <int NCH>
__global__ __launch_bounds__(256) void gather_ln_bf16_kernel(const float* __restrict__ x, const int32_t* __restrict__ idx,
                                                            const int32_t* __restrict__ row_map, int P, int width,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            bf16_t* __restrict__ h, int split3, int64_t n_sel, int d, float eps,
                                                            int d_live) {
  const int lane = threadIdx.x & 63;
  const int64_t r = wave_row();
  if (r >= n_sel) return;
  const int nch4 = d >> 2, nl4 = d_live >> 2;
  int pos = idx ? idx[r] : 0;
  float4 v[NCH];
  if (pos < 0 || (idx && (pos & 0x3fffffff) >= width)) {
#pragma unroll
    for (int i = 0; i < NCH; ++i) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  } else {
    int64_t src;
    if (idx) {
      pos &= 0x3fffffff;
      const int64_t s = r / P;
      src = (row_map ? (int64_t)row_map[s] : s) * width + pos;
    } else {
      src = r;
    }
    load_row(v, x + (size_t)src * d, nl4, lane);
    ln_inplace(v, nl4, lane, d_live, eps, gamma, beta);
  }
  bf16_t* o = h + (size_t)r * d * (split3 ? 3 : 1);
  store_row_bf16(o, v, nl4, lane, split3);
  zero_row_pad_bf16(o, nl4, nch4, lane, split3);
}

// ---- plain row gathers (last-layer pruning: only the sampled rows go through out-proj / FFN of the final layer) ----
// dst[r] = src[row_of(r) * width + idx[r]] for 16-byte chunks; idx < 0 -> row 0 (value never read back)
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                         const int32_t* __restrict__ idx, const int32_t* __restrict__ row_map,
                                                         int P, int width, int64_t n_sel, int chunks,
                                                         const int32_t* __restrict__ d_iter) {
  const int64_t r = wave_row();
  if (r >= n_sel) return;
  if (d_iter) idx += (size_t)(*d_iter) * n_sel;
  int pos = idx[r];
  pos = pos < 0 ? 0 : (pos & 0x3fffffff);
  if (pos >= width) pos = 0;          // out-of-range entries are never sampled (sample_writeback_kernel skips them)
  const int64_t s = r / P;
  const int64_t row = (row_map ? (int64_t)row_map[s] : s) * width + pos;
  for (int c = threadIdx.x & 63; c < chunks; c += 64) dst[r * chunks + c] = src[row * chunks + c];
}

// ---- LM-head tail: logits[r][V] = LN(g[r]) . embed^T + bias ----------------------------------
// g = gelu(dense(x)) fp32 [n][d] (GEMM epilogue); the 33 x d tied decoder stays L2-resident.
template <int NCH>
__global__ __launch_bounds__(256) void lm_tail_kernel(const float* __restrict__ g, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, const float* __restrict__ embed,
                                                     const float* __restrict__ out_bias, float* __restrict__ logits,
                                                     int64_t n, int d, int V, float eps, int d_live) {
  const int lane = threadIdx.x & 63;
  const int64_t r = wave_row();
  if (r >= n) return;
  // rows of g and of the decoder are d apart; the LayerNorm and the dot products run over the d_live live features (ln_row.h)
  const int nch4 = d_live >> 2;
  float4 v[NCH];
  load_row(v, g + (size_t)r * d, nch4, lane);
  if (gamma) ln_inplace(v, nch4, lane, d_live, eps, gamma, beta);      // gamma == nullptr: ESM-1's head has no LayerNorm
  float mine = 0.f;  // lane t keeps logit t (V <= 64)
  // four decoder rows per trip: their loads are all in flight before the first reduction (one row per trip was a chain
  // of V dependent L2 round trips: 81 us for a handful of rows)
  for (int t0 = 0; t0 < V; t0 += 4) {
    float s[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int t = t0 + u < V ? t0 + u : V - 1;
      const float4* e4 = (const float4*)(embed + (size_t)t * d);
      float a = 0.f;
#pragma unroll
      for (int i = 0; i < NCH; ++i)
        if (lane + 64 * i < nch4) {
          const float4 e = e4[lane + 64 * i];
          a += (v[i].x * e.x + v[i].y * e.y) + (v[i].z * e.z + v[i].w * e.w);
        }
      s[u] = a;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float r = wave_sum(s[u]);
      if (t0 + u < V && lane == t0 + u) mine = r + out_bias[t0 + u];
    }
  }
  if (lane < V) logits[(size_t)r * V + lane] = mine;
}

// Few rows (a single chain samples 2 positions per iteration; generate_single ~50): the row-per-wave kernel above walks the 33
// decoder rows one trip after the other (84 us for 2 rows).  Here one workgroup per row, one wave per 4 decoder rows: every wave
// normalises the row itself (1280 values) and all decoder rows are in flight at once.
template <int NCH>
__global__ __launch_bounds__(1024) void lm_tail_small_kernel(const float* __restrict__ g, const float* __restrict__ gamma,
                                                            const float* __restrict__ beta, const float* __restrict__ embed,
                                                            const float* __restrict__ out_bias, float* __restrict__ logits,
                                                            int d, int V, float eps, int d_live) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r = blockIdx.x;
  const int nch4 = d_live >> 2;      // as lm_tail_kernel: strides of d, arithmetic over d_live
  float4 v[NCH];
  load_row(v, g + (size_t)r * d, nch4, lane);
  if (gamma) ln_inplace(v, nch4, lane, d_live, eps, gamma, beta);
  float s[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int t = wave * 4 + u < V ? wave * 4 + u : V - 1;
    const float4* e4 = (const float4*)(embed + (size_t)t * d);
    float a = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i)
      if (lane + 64 * i < nch4) {
        const float4 e = e4[lane + 64 * i];
        a += (v[i].x * e.x + v[i].y * e.y) + (v[i].z * e.z + v[i].w * e.w);      // same per-lane order as lm_tail_kernel
      }
    s[u] = a;
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const float tot = wave_sum(s[u]);
    const int t = wave * 4 + u;
    if (t < V && lane == 0) logits[(size_t)r * V + t] = tot + out_bias[t];
  }
}

// ---- strict mode helpers: fp32 -> (hi, lo) bf16 pair, optionally through erf-GELU ----------------
__device__ __forceinline__ float gelu_erf_exact(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

// src fp32 [rows][K] -> dst bf16 [rows][3K]: the split operand row of an activation or, WEIGHT, of a weight (split_operand.h)
template <bool GELU, bool WEIGHT>
__global__ void split3_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int64_t n4, int k4, float scale) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n4; i += stride) {
    float4 v = ((const float4*)src)[i];
    v.x *= scale; v.y *= scale; v.z *= scale; v.w *= scale;
    if (GELU) { v.x = gelu_erf_exact(v.x); v.y = gelu_erf_exact(v.y); v.z = gelu_erf_exact(v.z); v.w = gelu_erf_exact(v.w); }
    uint2 hi, lo;
    split4(v.x, v.y, v.z, v.w, hi, lo);
    const int64_t row = i / k4;
    const int ci = (int)(i - row * k4);                      // float4 index in the row = columns 4 ci .. 4 ci + 3
    bf16_t* g = dst + row * 3 * (4 * k4) + split_lo_offset(4 * ci);
    if (WEIGHT) split_store4_weight(g, hi, lo);
    else split_store4(g, hi, lo, true);
  }
}
__global__ void gelu_f32_kernel(float* __restrict__ p, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] = gelu_erf_exact(p[i]);
}

// ---- fp32 <-> bf16 conversion (weights at load time, debug entries) ---------------------------
__global__ void f32_to_bf16_kernel(const float* __restrict__ src, bf16_t* __restrict__ dst, int64_t n, float scale) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = f32_to_op16_dev(src[i] * scale);
}
__global__ void bf16_to_f32_kernel(const bf16_t* __restrict__ src, float* __restrict__ dst, int64_t n) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) dst[i] = op16_to_f32(src[i]);
}
__global__ void scale_f32_kernel(float* __restrict__ p, int64_t n, float scale) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (; i < n; i += stride) p[i] *= scale;
}

// ---- launchers --------------------------------------------------------------------------------
static inline unsigned rows_grid(int64_t rows) { return (unsigned)((rows + 3) / 4); }
// rows_grid's result is a 32-bit workgroup count; past it the launch would cover the first rows only
static inline bool rows_fit(int64_t rows) { return rows >= 0 && (rows + 3) / 4 <= 0x7fffffffLL; }
// the row kernels hold a row as float4 v[NCH] per lane: the 8-chunk instantiation up to d = 2048 (every model before ESM-2 3B runs
// it, unchanged), the 10-chunk one up to d = 2560, the 20-chunk one for the whole 512-feature units above it up to d = 5120
// (row_d_ok of ln_row.h)
static inline bool row_wide(int d) { return d > kMaxCh * 256; }
// f(integral_constant<int, NCH>) for the NCH of a row of d values: a launcher names its kernel template once
template <class F>
static inline void by_row_width(int d, F&& f) {
  if (d > kMaxChWide * 256) f(std::integral_constant<int, kMaxCh5k>{});
  else if (row_wide(d)) f(std::integral_constant<int, kMaxChWide>{});
  else f(std::integral_constant<int, kMaxCh>{});
}
// A row launcher's admission of (d, rows) under the kernel's name `who`.  false: the launcher returns *rc -- 1, refused with the
// error set, or 0, no rows and nothing to do
// d_live (0 = d): the live width of an embedded model's rows (ln_row.h); resolved in place
static bool rows_go(const char* who, int d, int64_t rows, int* rc, int* d_live = nullptr) {
  *rc = 0;
  if (d_live && *d_live == 0) *d_live = d;
  if (!row_d_ok(d)) *rc = fail(1, std::string(who) + ": d must be a multiple of 4 and <= 2560, or a multiple of 512 up to 5120");
  else if (d_live && !row_live_ok(d, *d_live)) *rc = fail(1, std::string(who) + ": the live width must be a multiple of 4, at most d");
  else if (rows != 0 && !rows_fit(rows)) *rc = fail(1, std::string(who) + ": too many rows");
  return *rc == 0 && rows != 0;
}
// n > 0 items over at most `cap` workgroups of 256 threads that stride the rest
template <class Kernel, class... Args>
static int launch_grid_stride(hipStream_t s, Kernel* kernel, int64_t n, int cap, Args... args) {
  const unsigned grid = (unsigned)((n + 255) / 256 < cap ? (n + 255) / 256 : cap);
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, s, args...);
  PG_HIP(hipGetLastError());
  return 0;
}

int launch_embed_ln(hipStream_t s, const int32_t* tokens, const float* embed, const float* pos, const float* msa_pos,
                    const float* gamma, const float* beta, float* x, int64_t n_tok, int T, int d, int pad_idx,
                    int mask_idx, int token_dropout, int rows_per_msa, float eps, const float* gamma2, const float* beta2,
                    bf16_t* h2, float embed_scale, int d_live) {
  int rc;
  if (!rows_go("embed", d, n_tok, &rc, &d_live)) return rc;
  if (d_live != d && gamma) return fail(1, "embed: emb_layer_norm_before has no live-width form");
  by_row_width(d, [&](auto nch) {
    hipLaunchKernelGGL(embed_ln_kernel<decltype(nch)::value>, dim3(rows_grid(n_tok)), dim3(256), 0, s, tokens, embed, pos, msa_pos, gamma, beta,
                       x, n_tok, T, d, pad_idx, mask_idx, token_dropout, rows_per_msa, eps, gamma2, beta2, h2, embed_scale, d_live);
  });
  PG_HIP(hipGetLastError());
  return 0;
}

// The argument refusals of launch_layernorm_bf16 (0 = the launch may go ahead; touches no device) ...
int layernorm_bf16_check(int64_t M, int d, bool split3, int colmajor_R, int colmajor_C, int d_live) {
  int rc;
  if (!rows_go("layernorm", d, M, &rc, &d_live)) return rc;
  if (colmajor_R > 0) {
    if (d_live != d) return fail(1, "layernorm: column-major output has no live-width form");
    if (row_wide(d)) return fail(1, "layernorm: column-major output needs d <= 2048");
    if (split3 || M % ((int64_t)colmajor_R * colmajor_C)) return fail(1, "layernorm: column-major output needs whole MSAs and plain bf16 rows");
  }
  return 0;
}
// ... and its choice of kernel for M > 0 rows on the current device (LN_KERNEL_*; *stride_grid = the stride kernel's workgroups):
// the launcher and pg_dbg_layernorm_rows, which reports it, both ask here
int layernorm_bf16_choice(int64_t M, int d, int colmajor_R, unsigned* stride_grid, int d_live) {
  if (colmajor_R > 0) return LN_KERNEL_COLMAJOR;
  if (d_live && d_live != d) return LN_KERNEL_PLAIN;      // the stride kernel has no live-width form
  // one resident round of workgroups walking their rows when the plain grid would be 1 ... 4 rounds (layernorm_bf16_stride_kernel)
  static const int on = env_int("PGIBBS_LN_STRIDE", 1);
  const int n_cu = device_cu_count();
  const unsigned g1 = rows_grid(M);
  if (on && (d == 1280 || d == 768) && g1 > (unsigned)n_cu * 8 && g1 <= (unsigned)n_cu * 32) {
    // the grid = what is resident at once (occupancy of this very kernel x CUs, asked once per width)
    static int occ[2] = {0, 0};
    int& oc = occ[d == 768];
    if (oc == 0) {
      int v = 0;
      const hipError_t e = d == 1280 ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, layernorm_bf16_stride_kernel<1280>, 256, 0)
                                     : hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, layernorm_bf16_stride_kernel<768>, 256, 0);
      oc = (e == hipSuccess && v > 0) ? v : -1;
    }
    if (oc > 0 && g1 > (unsigned)(n_cu * oc)) {
      *stride_grid = (unsigned)(n_cu * oc);
      return LN_KERNEL_STRIDE;
    }
  }
  return LN_KERNEL_PLAIN;
}

int launch_layernorm_bf16(hipStream_t s, const float* x, const float* gamma, const float* beta, bf16_t* h, int64_t M,
                          int d, float eps, bool split3, int colmajor_R, int colmajor_C, bool split3_dup, int d_live) {
  const int rc = layernorm_bf16_check(M, d, split3, colmajor_R, colmajor_C, d_live);
  if (rc) return rc;
  if (M == 0) return 0;
  if (d_live == 0) d_live = d;
  const int sp = split3 ? (split3_dup ? 1 : 2) : 0;
  unsigned stride_grid = 0;
  switch (layernorm_bf16_choice(M, d, colmajor_R, &stride_grid, d_live)) {
    case LN_KERNEL_COLMAJOR:
      hipLaunchKernelGGL(layernorm_bf16_colmajor_kernel, dim3(rows_grid(M)), dim3(256), 0, s, x, gamma, beta, h, M, d, eps, colmajor_R, colmajor_C);
      break;
    case LN_KERNEL_STRIDE:
      if (d == 1280) hipLaunchKernelGGL(layernorm_bf16_stride_kernel<1280>, dim3(stride_grid), dim3(256), 0, s, x, gamma, beta, h, sp, M, eps);
      else hipLaunchKernelGGL(layernorm_bf16_stride_kernel<768>, dim3(stride_grid), dim3(256), 0, s, x, gamma, beta, h, sp, M, eps);
      break;
    default:
      by_row_width(d, [&](auto nch) {
        hipLaunchKernelGGL(layernorm_bf16_kernel<decltype(nch)::value>, dim3(rows_grid(M)), dim3(256), 0, s, x, gamma, beta, h, sp, M, d, eps, d_live);
      });
  }
  PG_HIP(hipGetLastError());
  return 0;
}

int launch_layernorm_f32(hipStream_t s, const float* x, const float* gamma, const float* beta, float* y, int64_t M, int d,
                         float eps, int d_live) {
  int rc;
  if (!rows_go("layernorm", d, M, &rc, &d_live)) return rc;
  by_row_width(d, [&](auto nch) {
    hipLaunchKernelGGL(layernorm_f32_kernel<decltype(nch)::value>, dim3(rows_grid(M)), dim3(256), 0, s, x, gamma, beta, y, M, d, eps, d_live);
  });
  PG_HIP(hipGetLastError());
  return 0;
}

int launch_gather_ln_bf16(hipStream_t s, const float* x, const int32_t* idx, const int32_t* row_map, int P, int width,
                          const float* gamma, const float* beta, bf16_t* h, int64_t n_sel, int d, float eps, bool split3, int d_live) {
  int rc;
  if (!rows_go("gather_ln", d, n_sel, &rc, &d_live)) return rc;
  by_row_width(d, [&](auto nch) {
    hipLaunchKernelGGL(gather_ln_bf16_kernel<decltype(nch)::value>, dim3(rows_grid(n_sel)), dim3(256), 0, s, x, idx, row_map, P, width, gamma,
                       beta, h, split3 ? 1 : 0, n_sel, d, eps, d_live);
  });
  PG_HIP(hipGetLastError());
  return 0;
}

int launch_gather_rows(hipStream_t s, const void* src, void* dst, const int32_t* idx, const int32_t* row_map, int P, int width,
                       int64_t n_sel, int row_bytes, const int32_t* d_iter) {
  if (n_sel == 0) return 0;
  if (row_bytes % 16) return fail(1, "gather: rows must be multiples of 16 bytes");
  hipLaunchKernelGGL(gather_rows_kernel, dim3(rows_grid(n_sel)), dim3(256), 0, s, (const uint4*)src, (uint4*)dst, idx, row_map, P,
                     width, n_sel, row_bytes / 16, d_iter);
  PG_HIP(hipGetLastError());
  return 0;
}

// launch_lm_tail's choice between lm_tail_small_kernel (true) and lm_tail_kernel; pg_dbg_lm_tail reports it
// Rows wider than 2560 features always take lm_tail_kernel: a 1024-thread workgroup has 128 VGPRs per lane, which do not hold the 80
// of a 20-chunk row next to the decoder chunks in flight (that instantiation spilled 28 bytes and is not built).  Same bits either way
bool lm_tail_small(int64_t n, int d) {
  static const int small_max = env_int("PGIBBS_LM_TAIL_SMALL", 1024);
  return n <= small_max && d <= kMaxChWide * 256;
}

int launch_lm_tail(hipStream_t s, const float* g, const float* gamma, const float* beta, const float* embed,
                   const float* out_bias, float* logits, int64_t n, int d, int V, float eps, int d_live) {
  if (V < 1 || V > 64) return fail(1, "lm_tail: vocab must be in 1..64");      // lane t keeps logit t; 64 * ceil(V / 4) <= 1024 threads
  int rc;
  if (!rows_go("lm_tail", d, n, &rc, &d_live)) return rc;
  // identical arithmetic per logit (same per-lane partial sums, same wave reduction): bit-equal results.  Up to 1024 rows (round 5;
  // it was 128): a 32-chain shard's 800 sampled rows took 81 us on the row-per-wave kernel -- 200 workgroups, each wave walking the
  // decoder rows in nine dependent trips -- PGIBBS_LM_TAIL_SMALL=n moves the switch
  const bool small = lm_tail_small(n, d);
  by_row_width(d, [&](auto nch) {
    constexpr int NCH = decltype(nch)::value;
    // small: no shared memory; every wave holds the row and four decoder rows' chunks (NCH + 4 float4 in flight at most: far below
    // the 128 VGPRs a 1024-thread workgroup may use per lane)
    if constexpr (NCH <= kMaxChWide) {
      if (small) {
        hipLaunchKernelGGL(lm_tail_small_kernel<NCH>, dim3((unsigned)n), dim3(64 * ((V + 3) / 4)), 0, s, g, gamma, beta, embed, out_bias,
                           logits, d, V, eps, d_live);
        return;
      }
    }
    hipLaunchKernelGGL(lm_tail_kernel<NCH>, dim3(rows_grid(n)), dim3(256), 0, s, g, gamma, beta, embed, out_bias, logits, n, d, V, eps, d_live);
  });
  PG_HIP(hipGetLastError());
  return 0;
}

int launch_split3_bf16(hipStream_t s, const float* src, bf16_t* dst, int64_t rows, int K, float scale, bool gelu, bool weight) {
  if (rows == 0) return 0;
  if (K % kSplitCols) return fail(1, "split: K must be a multiple of 32");
  if (gelu && weight) return fail(1, "split: GELU on a weight operand");
  const int64_t n4 = rows * (K / 4);
  auto* kernel = gelu ? split3_bf16_kernel<true, false> : weight ? split3_bf16_kernel<false, true> : split3_bf16_kernel<false, false>;
  return launch_grid_stride(s, kernel, n4, 8192, src, dst, n4, K / 4, scale);
}
int launch_gelu_f32(hipStream_t s, float* p, int64_t n) { return n ? launch_grid_stride(s, gelu_f32_kernel, n, 8192, p, n) : 0; }

int launch_f32_to_bf16(hipStream_t s, const float* src, bf16_t* dst, int64_t n, float scale) {
  return n ? launch_grid_stride(s, f32_to_bf16_kernel, n, 4096, src, dst, n, scale) : 0;
}
int launch_bf16_to_f32(hipStream_t s, const bf16_t* src, float* dst, int64_t n) {
  return n ? launch_grid_stride(s, bf16_to_f32_kernel, n, 4096, src, dst, n) : 0;
}
int launch_scale_f32(hipStream_t s, float* p, int64_t n, float scale) {
  return n ? launch_grid_stride(s, scale_f32_kernel, n, 4096, p, n, scale) : 0;
}

PG_OPS_END
