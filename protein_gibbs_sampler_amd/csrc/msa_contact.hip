// Contact prediction of the MSA Transformer (fair-esm's return_contacts=True on esm_msa1b): the tied row-attention maps the fused
// row kernel never holds.  Two launchers, called once per block by Engine::tap_row_attention:
//
//   launch_msa_row_scores     S[B*H*C][ldS] fp32 (ldS = msa_row_scores_ld(C)) = scale * sum_r sum_d q[b,r,i,h,d] k[b,r,j,h,d] of one block's
//                             row qkv buffer, read exactly as that block's row-attention launch reads it (ld 3 d, k at d, heads of 64).
//                             16-bit operands, compiled per operand flavour.  The strict mode's form is msa_row_scores_split_kernel
//                             (attention_f32.hip, launch_msa_row_scores_f32), whose shape this kernel has: one workgroup = (msa, head,
//                             64 queries, one key tile of 64 or 160 keys), wave w its queries 16 w .. +15; the R alignment rows stream
//                             through an LDS K tile (attn_frag.h's row layout and swizzle) and the S^T = K Q^T blocks of the wave stay in
//                             the v_mfma_f32_16x16x32 accumulators over all r ascending; the scale is applied once, at the end.
//                             The key tiling makes every C up to max_positions the same code -- no register-budget bound such as the
//                             fused kernel's C <= 576.
//   launch_row_softmax_probs  P[B][H][C][C] fp32 dense = softmax_j of the S rows; one wave per row -- one flavour.
//
// The K tiles alternate between two LDS buffers and row r + 1 is fetched into registers while row r's MFMAs run (one barrier per row,
// msa_row_attention_kernel's scheme with one row of look-ahead): a workgroup issues 8 MFMAs per key block and row against a tile load
// of 128 strided bytes per key, so without the look-ahead every row would wait a full memory round trip.
// Ragged batches (tok given: fair-esm's RowSelfAttention, oracle/msa_forward.py::row_attention): q is zeroed at <pad> positions of any
// row, the scores of key columns that are <pad> in ROW 0 are -10000 (finite), R is the padded depth.
// A score depends on its own (msa, head, query, key) operands alone -- not on the grid, the batch or the other heads; no atomics, fixed
// order: deterministic, and an MSA alone has the bits it has inside a batch.
// Softmax arithmetic (attn_probs_kernel's second sweep): m = max_j s_j; e_j = exp2(fma(s_j, log2e, -m log2e)); l = wave_sum e_j
// (lane L adds j = L, L + 64, ... ascending from 0, then the xor butterfly 32 .. 1); p_j = e_j * (1 / l).  A row that holds a
// non-finite score is written as NaN throughout, so the host's scan of the maps sees it whatever the other scores are.
#include "attn_frag.h"

PG_OPS_BEGIN

template <int MAXKB>
__global__ __launch_bounds__(256) void msa_row_scores_kernel(const bf16_t* __restrict__ qkv, float* __restrict__ S, int R, int C, int H,
                                                            int ld_qkv, int k_off, float scale, int n_qchunk, int n_ktile, int ldS,
                                                            const int32_t* __restrict__ tok, int pad_idx) {
  constexpr int tpad = MAXKB * 16, BUF = tpad * 128;
  using KRegs = TileRegs<tpad, 256>;
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kt = blockIdx.x % n_ktile, qc = (blockIdx.x / n_ktile) % n_qchunk, bh = blockIdx.x / (n_ktile * n_qchunk);
  const int b = bh / H, h = bh % H;
  const bf16_t* base = qkv + (size_t)b * R * C * ld_qkv + h * 64;      // token row r * C + i of this msa
  const int fr = lane & 15, fq = lane >> 4;
  const int q0 = qc * 64 + wave * 16, k0 = kt * tpad;
  const bool active = q0 < C;                                          // wave-uniform
  const int qrow = q0 + fr < C ? q0 + fr : C - 1;
  f32x4 st[MAXKB];
#pragma unroll
  for (int kb = 0; kb < MAXKB; ++kb) st[kb] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // keys k0 .. k0 + tpad - 1 of alignment row r (keys past C as zeros): one item = 8 d of one key
  KRegs g;
  auto load_k = [&](int r) {
    const bf16_t* rb = base + (size_t)r * C * ld_qkv + k_off;
#pragma unroll
    for (int it = 0; it < KRegs::NIT; ++it) {
      const int i = tid + it * 256, key = k0 + (i >> 3), c = i & 7;
      g.r[it] = make_uint4(0, 0, 0, 0);
      if (i < tpad * 8 && key < C) g.r[it] = *(const uint4*)(rb + (size_t)key * ld_qkv + c * 8);
    }
  };
  load_k(0);
  for (int r = 0; r < R; ++r) {
    char* Ks = smem + (r & 1) * BUF;
    tile_store(g, tid, Ks);
    const bf16_t* qp = base + ((size_t)r * C + qrow) * ld_qkv;
    bf16x8 qf0 = q_frag(qp, 0, fq), qf1 = q_frag(qp, 1, fq);
    if (tok && tok[((size_t)b * R + r) * C + qrow] == pad_idx) {
      const bf16x8 z = __builtin_bit_cast(bf16x8, make_uint4(0, 0, 0, 0));
      qf0 = z;
      qf1 = z;
    }
    __syncthreads();                                  // tile r visible; everybody is done with tile r - 1 (the other buffer)
    if (r + 1 < R) load_k(r + 1);
    if (active) {
      // the two k-halves of a key block accumulate into the same registers: keep them MAXKB MFMAs apart
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int kb = 0; kb < MAXKB; ++kb) st[kb] = mfma_op16(k_frag(Ks, kb * 16 + fr, kk, fq), kk ? qf1 : qf0, st[kb]);
      }
    }
  }
  const int q = q0 + fr;
  if (active && q < C) {
    float* dst = S + ((size_t)bh * C + q) * ldS + k0 + fq * 4;
    const int32_t* t0 = tok ? tok + (size_t)b * R * C : nullptr;      // row 0 of this MSA
#pragma unroll
    for (int kb = 0; kb < MAXKB; ++kb) {
      const int key = k0 + kb * 16 + fq * 4;
      if (key < ldS) {                                // ldS is a multiple of 4: key + 3 < ldS
        float4 v = make_float4(st[kb][0] * scale, st[kb][1] * scale, st[kb][2] * scale, st[kb][3] * scale);
        if (t0) {
          if (key < C && t0[key] == pad_idx) v.x = -10000.f;
          if (key + 1 < C && t0[key + 1] == pad_idx) v.y = -10000.f;
          if (key + 2 < C && t0[key + 2] == pad_idx) v.z = -10000.f;
          if (key + 3 < C && t0[key + 3] == pad_idx) v.w = -10000.f;
        }
        *(float4*)(dst + kb * 16) = v;
      }
    }
  }
}

// ---- the plan: a pure function of the shape (pg_msa_contact_dbg_probs reports it; no HIP call).  The tiling is the strict scores
// kernel's (plan_msa_row_f32): 64-key tiles up to 64 columns, 160-key tiles beyond
struct RowScoresPlan {
  std::string error;
  int kb = 10, n_qchunk = 0, n_ktile = 1;
  bool pad = false;
  unsigned grid = 0;               // 0: nothing to launch
};
static RowScoresPlan plan_msa_row_scores(int B, int R, int C, int H, bool has_pad) {
  RowScoresPlan p;
  p.pad = has_pad;
  if (B == 0 || R == 0) return p;
  if (B < 0 || R < 0 || C <= 0) { p.error = "row scores: empty alignment"; return p; }
  if (H < 1) { p.error = "row scores: no heads"; return p; }
  p.n_qchunk = (C + 63) / 64;
  p.kb = C <= 64 ? 4 : 10;
  p.n_ktile = C <= 64 ? 1 : (C + 159) / 160;
  const int64_t grid = (int64_t)B * H * p.n_qchunk * p.n_ktile;
  if (grid > 0x7fffffff || (int64_t)B * H * C > 0x7fffffff) { p.error = "row scores: too many alignments"; return p; }
  p.grid = (unsigned)grid;
  return p;
}
static std::string plan_text(const RowScoresPlan& p) {
  if (!p.error.empty()) return "error: " + p.error;
  if (!p.grid) return "nothing";
  return "row-scores kb" + std::to_string(p.kb) + " kt" + std::to_string(p.n_ktile) + (p.pad ? " pad " : " ") + std::to_string(p.grid) + "wg";
}
void msa_row_scores_plan_text(int B, int R, int C, int H, bool has_pad, std::string* text) {
  *text = plan_text(plan_msa_row_scores(B, R, C, H, has_pad));
}

int launch_msa_row_scores(hipStream_t s, const bf16_t* qkv, float* S, int B, int R, int C, int H, int ld_qkv, int k_off, float scale,
                          const int32_t* tok, int pad_idx) {
  const RowScoresPlan p = plan_msa_row_scores(B, R, C, H, tok != nullptr);
  if (!p.error.empty()) return fail(1, p.error);
  if (!p.grid) return 0;
  // 16-byte fragment and tile loads: every row and the k block start on 16 bytes
  if (ld_qkv % 8 || k_off % 8 || k_off < 0 || ld_qkv < H * 64) return fail(1, "row scores: ld_qkv / k_off must keep the rows 16-byte aligned");
  note_kernel(plan_text(p).c_str());
  const int ldS = msa_row_scores_ld(C);
  auto go = [&](auto kb) {
    hipLaunchKernelGGL(msa_row_scores_kernel<decltype(kb)::value>, dim3(p.grid), dim3(256), 0, s, qkv, S, R, C, H, ld_qkv, k_off, scale,
                       p.n_qchunk, p.n_ktile, ldS, tok, pad_idx);
  };
  if (p.kb == 4) go(std::integral_constant<int, 4>{});
  else go(std::integral_constant<int, 10>{});
  PG_HIP(hipGetLastError());
  return 0;
}

PG_OPS_END

#ifndef PG_F16
namespace pg {

// One wave per score row; 4 rows per workgroup
__global__ __launch_bounds__(256) void row_softmax_probs_kernel(const float* __restrict__ S, float* __restrict__ P, int64_t n_rows, int C,
                                                               int ldS) {
  constexpr float LOG2E = 1.44269504088896341f;
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= n_rows) return;                                   // wave-uniform; no barrier below
  const float* srow = S + (size_t)row * ldS;
  float* prow = P + (size_t)row * C;
  float m = -3.0e38f, bad = 0.f;
  for (int j = lane; j < C; j += 64) {
    const float s = srow[j];
    m = fmaxf(m, s);
    bad += s * 0.f;                                            // NaN from a NaN or an infinity, else +-0
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    m = fmaxf(m, __shfl_xor(m, off, 64));
    bad += __shfl_xor(bad, off, 64);
  }
  const float mneg = -m * LOG2E;
  float l = 0.f;
  for (int j = lane; j < C; j += 64) l += __builtin_amdgcn_exp2f(fmaf(srow[j], LOG2E, mneg));
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) l += __shfl_xor(l, off, 64);
  const float inv = 1.0f / l + bad;
  for (int j = lane; j < C; j += 64) prow[j] = __builtin_amdgcn_exp2f(fmaf(srow[j], LOG2E, mneg)) * inv;
}

int launch_row_softmax_probs(hipStream_t s, const float* S, float* P, int64_t n_rows, int C, int ldS) {
  if (n_rows < 0 || C < 1 || ldS < C) return fail(1, "row softmax: bad shape");
  if (n_rows == 0) return 0;
  if ((n_rows + 3) / 4 > 0x7fffffff) return fail(1, "row softmax: too many rows");
  hipLaunchKernelGGL(row_softmax_probs_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, s, S, P, n_rows, C, ldS);
  PG_HIP(hipGetLastError());
  return 0;
}

}  // namespace pg
#endif
