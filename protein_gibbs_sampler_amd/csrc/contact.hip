// Contact prediction (fair-esm's predict_contacts / return_contacts=True): the attention maps the fused attention kernels never
// hold, and the average product correction + logistic regression head over them.  Two launchers, called once per layer:
//
//   launch_attn_probs[_f32]    P[n_seq][H][T][T] fp32 = softmax_j(q_i . k_j) of one layer's qkv buffer, read exactly as that layer's
//                              fused attention launch reads it (after the rotary kernel, q pre-scaled, same ld / k_off / SeqLayout;
//                              v is not looked at).  16-bit operands: one v_mfma_f32_16x16x32 (bf16 / f16; heads of 16: the half-depth
//                              16x16x16) step per 32 d, attn_frag.h's geometry -- compiled per operand flavour.  Strict mode: fp32
//                              qkv, every operand split into a bf16 (hi, lo) pair, kl.qh + kh.ql per 32 d and then kh.qh, fp32
//                              accumulation, small terms first (attention_f32.hip's scheme) -- bf16 flavour only.
//   launch_contact_accumulate  logits[B][W][W] (W = T - 2) (+)= sum_h w[h] . APC(symmetrised, live-masked P[b][h]) -- one flavour.
//                              launch_contact_accumulate_window: the same with W = T - 1 - tail and a token-row stride (the MSA
//                              Transformer's maps: tail 0, row 0 of tokens[B][R][C], eos_idx = -1; the kernels say how).
//
// launch_attn_probs: how a row of any length is held.  One workgroup = (sequence, head, 64 queries), wave w its queries 16 w .. +15;
// the keys go through the LDS in tiles of 64 and are swept TWICE at every T: sweep 1 keeps the row's running maximum m and sum l
// (the online recurrence of attention_long_kernel), sweep 2 computes the same scores again -- same instructions on the same
// operands: same bits -- and writes exp2(s log2e - m log2e) * (1 / l).  There is no length up to which a row stays in registers and
// therefore no T-dependent branch: T = 3 and T = 1024 run the same code, only the tile count differs (T <= 64: one tile).  The
// second score product costs MFMA time the fp32 stores hide (4 T^2 bytes written per T^2 HD MACs).
// A query's result depends on its own row of q, the sequence's k and the sequence's tokens alone: not on the batch, the grid or the
// other heads.  No atomics, fixed order: deterministic.
// Masked keys (token == pad_idx, as the fused kernels mask them) get exactly 0; a row without any live key is all zeros.
//
// launch_contact_accumulate: the arithmetic contract (tests/_contact_reference.py restates it operation for operation; every
// operation below is ONE fp32 operation rounded to nearest -- the file is compiled with -ffp-contract=off and uses the _rn intrinsics):
//   live[t]  = tokens[b][t] != eos_idx && tokens[b][t] != pad_idx;  window index i <-> token t = i + 1, i in 0 .. W - 1
//   A[i][j]  = live[i + 1] && live[j + 1] ? P[b][h][i + 1][j + 1] : 0.0f
//   S[i][j]  = A[i][j] + A[j][i]                          (one add; commutative, so S is exactly symmetric)
//   a1[i]    = wave_sum_j S[i][j],  a12 = wave_sum_i a1[i] where wave_sum over n terms x[0 .. n-1] is:
//                lane L (0 .. 63): acc = 0.0f; for k = L, L + 64, L + 128, ... < n ascending: acc = acc + x[k];
//                then for off in 32, 16, 8, 4, 2, 1: acc = acc + acc_of_lane(L ^ off)      (all 64 lanes end with the same value)
//   per head h ascending, skipped altogether when a12 == 0 (no live residue in the window: that channel contributes 0 -- fair-esm
//   divides by zero there and yields NaN):
//       N = S[i][j] - (a1[i] * a1[j]) / a12;   logit = logit + w[h] * N
//   logit starts from 0.0f when `first`, else from the stored value; when `last`: logit = logit + bias, and with a contacts buffer
//   contacts = 1.0f / (1.0f + expf(-logit)).
// A window entry whose row or column is not live has S = 0 and a1 = 0 on that side, so every term is w[h] * (0 - 0 / a12) = +-0 and
// its logit is exactly bias.  The caller folds layers in ascending order: the channel order c = l * H + h is fixed.
// Both kernels: 64-bit row bases, vector stores, no cross-workgroup communication.
#include <type_traits>

#include "attn_frag.h"
#include "split_operand.h"

PG_OPS_BEGIN

constexpr int kProbsTileKeys = 64, kProbsTileKB = 4;      // keys per LDS tile = 4 blocks of 16

// F32: the strict form -- fp32 qkv, split operands (tiles Kh and Kl)
template <int HD, bool F32>
__global__ __launch_bounds__(256) void attn_probs_kernel(const void* __restrict__ qkv_, float* __restrict__ P, int T, int H, int ld_qkv_,
                                                        int k_off, SeqLayout sl, int n_qchunk, const int32_t* __restrict__ key_tok,
                                                        int pad_idx) {
  constexpr int TK = kProbsTileKeys, KB = kProbsTileKB, ROW = HD * 2, NKK = score_steps(HD), CPR = HD / 8;
  constexpr float LOG2E = 1.44269504088896341f;
  typedef typename std::conditional<F32, float, bf16_t>::type in_t;
  typedef kfrag_t<HD> kf_t;
  __shared__ __attribute__((aligned(16))) char smem[(F32 ? 2 : 1) * TK * ROW + TK];
  char* Kh = smem;
  char* Kl = smem + TK * ROW;                               // F32 only
  char* maskf = smem + (F32 ? 2 : 1) * TK * ROW;            // one byte per key of the tile: 1 = past the last key, or a <pad> token

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qc = blockIdx.x % n_qchunk, sh = blockIdx.x / n_qchunk;
  const int seq = sh / H, h = sh % H;
  const size_t row0 = (size_t)(seq / sl.inner_count) * sl.outer_rows + (size_t)(seq % sl.inner_count) * sl.inner_rows;
  const size_t ld = (size_t)ld_qkv_ * sl.row_step;
  const in_t* base = (const in_t*)qkv_ + row0 * ld_qkv_ + h * HD;
  const int fr = lane & 15, fq = lane >> 4;
  const int q0 = qc * 64 + wave * 16;
  const bool active = q0 < T;                               // wave-uniform
  const int q = q0 + fr;

  // Q fragments (MFMA B operand): query fr, d = kk*32 + fq*8 .. +7 (head 16: d = fq*4 .. +3); a query past the end reads the last row
  kf_t qh[NKK], ql[NKK];
  {
    const in_t* qrow = base + (size_t)(q < T ? q : T - 1) * ld;
    if constexpr (!F32) {
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) qh[kk] = q_frag<HD>(qrow, kk, fq);
    } else if constexpr (HD == 16) {
      const float4 p = *(const float4*)(qrow + fq * 4);
      uint2 hi, lo;
      split4(p.x, p.y, p.z, p.w, hi, lo);
      qh[0] = __builtin_bit_cast(bf16x4, hi);
      ql[0] = __builtin_bit_cast(bf16x4, lo);
    } else {
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        const float4* p = (const float4*)(qrow + kk * 32 + fq * 8);
        uint4 hi, lo;
        split8(p[0], p[1], hi, lo);
        qh[kk] = __builtin_bit_cast(bf16x8, hi);
        ql[kk] = __builtin_bit_cast(bf16x8, lo);
      }
    }
  }

  // keys k0 .. k0 + 63 of the sequence into the tile(s) (rows past T as zeros) and their mask bytes; one item = 8 d of one key
  auto stage = [&](int k0) {
    constexpr int NIT = (TK * CPR + 255) / 256;
    if constexpr (!F32) {
      uint4 r[NIT];
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int i = tid + it * 256, row = i / CPR, c = i & (CPR - 1);
        r[it] = make_uint4(0, 0, 0, 0);
        if (i < TK * CPR && k0 + row < T) r[it] = *(const uint4*)(base + (size_t)(k0 + row) * ld + k_off + c * 8);
      }
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int i = tid + it * 256, row = i / CPR, c = i & (CPR - 1);
        if (i < TK * CPR) *(uint4*)(Kh + tile_addr<HD>(row, c)) = r[it];
      }
    } else {
      float4 r0[NIT], r1[NIT];
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int i = tid + it * 256, row = i / CPR, c = i & (CPR - 1);
        r0[it] = make_float4(0.f, 0.f, 0.f, 0.f);
        r1[it] = r0[it];
        if (i < TK * CPR && k0 + row < T) {
          const float4* p = (const float4*)(base + (size_t)(k0 + row) * ld + k_off + c * 8);
          r0[it] = p[0];
          r1[it] = p[1];
        }
      }
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int i = tid + it * 256, row = i / CPR, c = i & (CPR - 1);
        if (i < TK * CPR) {
          uint4 hi, lo;
          split8(r0[it], r1[it], hi, lo);
          const int a = tile_addr<HD>(row, c);
          *(uint4*)(Kh + a) = hi;
          *(uint4*)(Kl + a) = lo;
        }
      }
    }
    if (tid < TK) {
      const int key = k0 + tid;
      maskf[tid] = (key >= T || (key_tok && key_tok[row0 + (size_t)key * sl.row_step] == pad_idx)) ? 1 : 0;
    }
  };
  // the tile's scores of the lane's query: st[kb][r] = S[query fr][key k0 + kb*16 + fq*4 + r], masked keys -3e38
  auto scores = [&](f32x4 (&st)[KB]) {
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
      const int krow = kb * 16 + fr;
      if constexpr (!F32) {
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) a = score_mfma(k_frag<HD>(Kh, krow, kk, fq), qh[kk], a);
      } else {
        kf_t kh[NKK];
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) {
          kh[kk] = k_frag<HD>(Kh, krow, kk, fq);
          const kf_t kl = k_frag<HD>(Kl, krow, kk, fq);
          a = score_mfma(kl, qh[kk], a);
          a = score_mfma(kh[kk], ql[kk], a);
        }
#pragma unroll
        for (int kk = 0; kk < NKK; ++kk) a = score_mfma(kh[kk], qh[kk], a);
      }
      st[kb] = mask_pad(a, *(const uint32_t*)(maskf + kb * 16 + fq * 4), -3.0e38f);
    }
  };

  // ---- sweep 1: the row's maximum and sum
  float m = -3.0e38f, l = 0.f;
  for (int k0 = 0; k0 < T; k0 += TK) {
    __syncthreads();
    stage(k0);
    __syncthreads();
    if (!active) continue;
    f32x4 st[KB];
    scores(st);
    const float mn = fmaxf(m, rows4_max(lane_max(st)));
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * LOG2E);
    const float mneg = -mn * LOG2E;
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) psum += st[kb][r] < -1.0e38f ? 0.f : __builtin_amdgcn_exp2f(fmaf(st[kb][r], LOG2E, mneg));      // a NaN score stays NaN
    l = l * alpha + rows4_sum(psum);
    m = mn;
  }
  // ---- sweep 2: the same scores again, normalised and written
  const float inv = l == 0.f ? 0.f : 1.0f / l;              // every key masked: a row of zeros; a NaN sum stays NaN
  const float mneg = -m * LOG2E;
  float* prow = P + ((size_t)sh * T + (q < T ? q : T - 1)) * (size_t)T;
  const bool vec = (T & 3) == 0;                            // rows of T floats: 16-byte stores when every row starts on 16 bytes
  for (int k0 = 0; k0 < T; k0 += TK) {
    __syncthreads();
    stage(k0);
    __syncthreads();
    if (!active) continue;
    f32x4 st[KB];
    scores(st);
    if (q >= T) continue;
#pragma unroll
    for (int kb = 0; kb < KB; ++kb) {
      float p[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) p[r] = st[kb][r] < -1.0e38f ? 0.f : __builtin_amdgcn_exp2f(fmaf(st[kb][r], LOG2E, mneg)) * inv;
      const int key = k0 + kb * 16 + fq * 4;
      if (vec) {
        if (key < T) *(float4*)(prow + key) = make_float4(p[0], p[1], p[2], p[3]);
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (key + r < T) prow[key + r] = p[r];
      }
    }
  }
}

// ---- the plan: a pure function of the shape (pg_contact_dbg_probs reports it; no HIP call) ----
struct ProbsPlan {
  std::string error;
  int hd = 64, n_qchunk = 0, n_tiles = 0;
  bool pad = false, strict = false;
  unsigned grid = 0;               // 0: nothing to launch
};
static ProbsPlan plan_attn_probs(int64_t n_seq, int T, int H, int head_dim, bool has_pad, bool strict) {
  ProbsPlan p;
  p.hd = head_dim, p.pad = has_pad, p.strict = strict;
  p.error = attention_head_error(head_dim, false);
  if (!p.error.empty() || n_seq == 0) return p;
  if (T <= 0) { p.error = "attn_probs: empty sequence"; return p; }
  if (H < 1) { p.error = "attn_probs: no heads"; return p; }
  p.n_qchunk = (T + 63) / 64;
  p.n_tiles = (T + kProbsTileKeys - 1) / kProbsTileKeys;
  if (n_seq * H * p.n_qchunk > 0x7fffffff) { p.error = "attn_probs: too many sequences"; return p; }
  p.grid = (unsigned)(n_seq * H * p.n_qchunk);
  return p;
}
static std::string plan_text(const ProbsPlan& p) {
  if (!p.error.empty()) return "error: " + p.error;
  if (!p.grid) return "nothing";
  return std::string(p.strict ? "probs-f32" : "probs") + " two-sweep t64 x" + std::to_string(p.n_tiles) + " hd" + std::to_string(p.hd) + (p.pad ? " pad " : " ") +
         std::to_string(p.grid) + "wg";
}
static int probs_args_check(int T, int H, int ld_qkv, int k_off, int head_dim, bool f32) {
  // 16-byte fragment and tile loads: every row and the k block start on 16 bytes
  const int per16 = f32 ? 4 : 8;
  if (ld_qkv % per16 || k_off % per16 || k_off < 0 || ld_qkv < H * head_dim) return fail(1, "attn_probs: ld_qkv / k_off must keep the rows 16-byte aligned");
  return 0;
}

void attn_probs_plan_text(int64_t n_seq, int T, int H, int head_dim, bool has_pad, std::string* text) {
  *text = plan_text(plan_attn_probs(n_seq, T, H, head_dim, has_pad, false));
}

int launch_attn_probs(hipStream_t s, const bf16_t* qkv, float* P, int64_t n_seq, int T, int H, int ld_qkv, int k_off, SeqLayout sl,
                      const int32_t* key_tok, int pad_idx, int head_dim) {
  const ProbsPlan p = plan_attn_probs(n_seq, T, H, head_dim, key_tok != nullptr, false);
  if (!p.error.empty()) return fail(1, p.error);
  if (!p.grid) return 0;
  if (int rc = probs_args_check(T, H, ld_qkv, k_off, head_dim, false)) return rc;
  note_kernel(plan_text(p).c_str());
  visit_head_width(head_dim, [&](auto hd) {
    hipLaunchKernelGGL((attn_probs_kernel<decltype(hd)::value, false>), dim3(p.grid), dim3(256), 0, s, (const void*)qkv, P, T, H, ld_qkv, k_off, sl,
                       p.n_qchunk, key_tok, pad_idx);
  });
  PG_HIP(hipGetLastError());
  return 0;
}

#ifndef PG_F16
void attn_probs_f32_plan_text(int64_t n_seq, int T, int H, int head_dim, bool has_pad, std::string* text) {
  *text = plan_text(plan_attn_probs(n_seq, T, H, head_dim, has_pad, true));
}

int launch_attn_probs_f32(hipStream_t s, const float* qkv, float* P, int64_t n_seq, int T, int H, int ld_qkv, int k_off, SeqLayout sl,
                          const int32_t* key_tok, int pad_idx, int head_dim) {
  const ProbsPlan p = plan_attn_probs(n_seq, T, H, head_dim, key_tok != nullptr, true);
  if (!p.error.empty()) return fail(1, p.error);
  if (!p.grid) return 0;
  if (int rc = probs_args_check(T, H, ld_qkv, k_off, head_dim, true)) return rc;
  note_kernel(plan_text(p).c_str());
  visit_head_width(head_dim, [&](auto hd) {
    hipLaunchKernelGGL((attn_probs_kernel<decltype(hd)::value, true>), dim3(p.grid), dim3(256), 0, s, (const void*)qkv, P, T, H, ld_qkv, k_off, sl,
                       p.n_qchunk, key_tok, pad_idx);
  });
  PG_HIP(hipGetLastError());
  return 0;
}
#endif

PG_OPS_END

#ifndef PG_F16
namespace pg {

// ---- average product correction + regression head: fp32, one flavour (the contract: top of the file) ----
__device__ __forceinline__ bool contact_live(int32_t t, int eos_idx, int pad_idx) { return t != eos_idx && t != pad_idx; }
// wave_sum's second half: the butterfly over the 64 lanes
__device__ __forceinline__ float contact_wave_tree(float acc) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, off, 64));
  return acc;
}

// The window form: the window is token positions 1 .. T - 1 - tail (W = T - 1 - tail: tail = 1 cuts a trailing <eos> position -- the
// ESM family --, tail = 0 none -- the MSA Transformer, whose alphabet appends no <eos>), and the tokens of batch item b start at
// tokens + b * tok_stride (T for a [B][T] batch; R * C for tokens[B][R][C], so that row 0 of each MSA is what is read).
// One workgroup of 4 waves per (b, h): wave w sums the window rows i = w, w + 4, ... (a1), then wave 0 sums a1 (a12)
__global__ __launch_bounds__(256) void contact_sums_kernel(const float* __restrict__ P, const int32_t* __restrict__ tokens, int eos_idx,
                                                          int pad_idx, float* __restrict__ a1, float* __restrict__ a12, int H, int T, int W,
                                                          size_t tok_stride) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t bh = blockIdx.x;
  const int32_t* tok = tokens + (bh / H) * tok_stride;
  const float* A = P + bh * (size_t)T * T;
  float* a1o = a1 + bh * (size_t)W;
  for (int i = wave; i < W; i += 4) {
    const bool li = contact_live(tok[i + 1], eos_idx, pad_idx);
    float acc = 0.f;
    for (int j = lane; j < W; j += 64) {
      const bool on = li && contact_live(tok[j + 1], eos_idx, pad_idx);
      const float x = on ? A[(size_t)(i + 1) * T + (j + 1)] : 0.f, y = on ? A[(size_t)(j + 1) * T + (i + 1)] : 0.f;
      acc = __fadd_rn(acc, __fadd_rn(x, y));
    }
    acc = contact_wave_tree(acc);
    if (lane == 0) a1o[i] = acc;
  }
  __syncthreads();                                         // the workgroup's own a1 stores, visible to wave 0
  if (wave == 0) {
    float acc = 0.f;
    for (int i = lane; i < W; i += 64) acc = __fadd_rn(acc, a1o[i]);
    acc = contact_wave_tree(acc);
    if (lane == 0) a12[bh] = acc;
  }
}

// One thread per (b, i, j) in 16 x 16 tiles (the transposed read A[j][i] then comes in 64-byte runs too)
__global__ __launch_bounds__(256) void contact_fold_kernel(const float* __restrict__ P, const int32_t* __restrict__ tokens, int eos_idx,
                                                          int pad_idx, const float* __restrict__ a1, const float* __restrict__ a12,
                                                          const float* __restrict__ w, float bias, int first, int last,
                                                          float* __restrict__ logits, float* __restrict__ contacts, int H, int T, int W,
                                                          size_t tok_stride) {
  const int j = blockIdx.x * 16 + (threadIdx.x & 15), i = blockIdx.y * 16 + (threadIdx.x >> 4);
  const size_t b = blockIdx.z;
  if (i >= W || j >= W) return;
  const int32_t* tok = tokens + b * tok_stride;
  const bool on = contact_live(tok[i + 1], eos_idx, pad_idx) && contact_live(tok[j + 1], eos_idx, pad_idx);
  const size_t o = (b * W + i) * (size_t)W + j;
  float logit = first ? 0.f : logits[o];
  for (int h = 0; h < H; ++h) {
    const size_t bh = b * H + h;
    const float d = a12[bh];
    if (d == 0.f) continue;
    const float* A = P + bh * (size_t)T * T;
    const float x = on ? A[(size_t)(i + 1) * T + (j + 1)] : 0.f, y = on ? A[(size_t)(j + 1) * T + (i + 1)] : 0.f;
    const float S = __fadd_rn(x, y);
    const float n = __fsub_rn(S, __fdiv_rn(__fmul_rn(a1[bh * W + i], a1[bh * W + j]), d));
    logit = __fadd_rn(logit, __fmul_rn(w[h], n));
  }
  if (last) logit = __fadd_rn(logit, bias);
  logits[o] = logit;
  if (last && contacts) contacts[o] = __fdiv_rn(1.0f, __fadd_rn(1.0f, expf(-logit)));
}

size_t contact_window_sums_floats(int B, int H, int T, int tail) { return (size_t)B * H * (T - 1 - tail) + (size_t)B * H; }
size_t contact_sums_floats(int B, int H, int T) { return contact_window_sums_floats(B, H, T, 1); }

int launch_contact_accumulate_window(hipStream_t s, const float* P, const int32_t* tokens, int eos_idx, int pad_idx, const float* w, float bias,
                                     bool first, bool last, float* sums, float* logits, float* contacts, int B, int T, int H, int tail,
                                     size_t tok_stride) {
  if (tail != 0 && tail != 1) return fail(1, "contact_accumulate: tail must be 0 or 1");
  if (B < 0 || T < 2 + tail || H < 1)
    return fail(1, tail ? "contact_accumulate: bad shape (T >= 3: <cls>, at least one position, <eos>)"
                        : "contact_accumulate: bad shape (T >= 2: <cls> and at least one position)");
  if (tok_stride < (size_t)T) return fail(1, "contact_accumulate: token rows overlap");
  if (B == 0) return 0;
  const int W = T - 1 - tail;
  if ((int64_t)B * H > 0x7fffffff || B > 65535 || (W + 15) / 16 > 65535) return fail(1, "contact_accumulate: too many sequences");
  float* a1 = sums;
  float* a12 = sums + (size_t)B * H * W;
  hipLaunchKernelGGL(contact_sums_kernel, dim3((unsigned)(B * H)), dim3(256), 0, s, P, tokens, eos_idx, pad_idx, a1, a12, H, T, W, tok_stride);
  hipLaunchKernelGGL(contact_fold_kernel, dim3((W + 15) / 16, (W + 15) / 16, B), dim3(256), 0, s, P, tokens, eos_idx, pad_idx, a1, a12, w, bias,
                     first ? 1 : 0, last ? 1 : 0, logits, contacts, H, T, W, tok_stride);
  PG_HIP(hipGetLastError());
  return 0;
}

int launch_contact_accumulate(hipStream_t s, const float* P, const int32_t* tokens, int eos_idx, int pad_idx, const float* w, float bias,
                              bool first, bool last, float* sums, float* logits, float* contacts, int B, int T, int H) {
  return launch_contact_accumulate_window(s, P, tokens, eos_idx, pad_idx, w, bias, first, last, sums, logits, contacts, B, T, H, 1, (size_t)T);
}

}  // namespace pg
#endif
