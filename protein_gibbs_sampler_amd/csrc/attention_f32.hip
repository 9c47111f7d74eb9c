// Strict-precision attention (PG_PREC_FP32): the same softmax(q k^T) v per (sequence, head) as attention.hip from
// fp32 q, k, v, for the 1e-3 logit-parity mode.
//
// attention_split_kernel: the MFMA formulation of attention.hip's attention_long_kernel with every
// operand split into a bf16 (hi, lo) pair in registers -- S = ql.kh + qh.kl + qh.kh and O = vl.ph + vh.pl + vh.ph, fp32
// accumulation, small terms first -- so q, k, v and P keep ~16 mantissa bits (the dropped lo.lo terms are ~2^-17
// relative).  One workgroup = (sequence, head, 64 queries); K and V tiles of MAXKB*16 keys are split while they are
// staged (four LDS tiles: Kh, Kl, Vh, Vl); online softmax across tiles; exp2 on fp32 scores.
#include "attn_frag.h"
#include "split_operand.h"

PG_OPS_BEGIN

// Building blocks shared by the three split-bf16 MFMA kernels (full attention, tied-row scores, tied-row apply).
// Fragment geometry, tile layout and the transposing V^T read: attn_frag.h.
// HD: the head dimension, 64, 32, 128 or 16 (attn_frag.h; 32, 128 and 16 are built for the full attention only)
template <int MAXKB, int HD = 64>
struct SplitAttn {
  static constexpr int tpad = MAXKB * 16, nkc = MAXKB / 2;
  static constexpr int CPR = HD / 8, NKK = score_steps(HD), NDB = HD / 16;      // 16-byte chunks per key row, score MFMAs per key block, output blocks
  typedef kfrag_t<HD> kf_t;                                                      // the score product's fragment (attn_frag.h)
  static_assert(MAXKB % 2 == 0, "two 16-key blocks per 32-wide PV step");
  static constexpr float LOG2E = 1.44269504088896341f;

  // rows 0 .. tpad-1 of HD fp32 at src + row*ld (rows >= n_valid read as zero) -> (hi, lo) bf16 tiles (tile_addr).  All
  // global loads in flight first.
  // extra (optional): 64 fp32 that stand in for row n_valid (ESM-1: the head's bias_k / bias_v behind the last token)
  template <bool EXTRA = false>
  static __device__ __forceinline__ void stage(const float* __restrict__ src, size_t ld, int n_valid, char* Xh, char* Xl, int tid,
                                               const float* __restrict__ extra = nullptr) {
    constexpr int NIT = (tpad * CPR + 255) / 256;      // one item = 8 d of one key
    float4 r0[NIT], r1[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + it * 256, row = i / CPR, c = i & (CPR - 1);
      r0[it] = make_float4(0.f, 0.f, 0.f, 0.f);
      r1[it] = r0[it];
      if (i < tpad * CPR && row < n_valid) {
        const float4* p = (const float4*)(src + (size_t)row * ld + c * 8);
        r0[it] = p[0];
        r1[it] = p[1];
      } else if (EXTRA && row == n_valid && i < tpad * CPR) {
        const float4* p = (const float4*)(extra + c * 8);
        r0[it] = p[0];
        r1[it] = p[1];
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + it * 256, row = i / CPR, c = i & (CPR - 1);
      if (i < tpad * CPR) {
        uint4 hi, lo;
        split8(r0[it], r1[it], hi, lo);
        const int a = tile_addr<HD>(row, c);
        *(uint4*)(Xh + a) = hi;
        *(uint4*)(Xl + a) = lo;
      }
    }
  }

  // Q fragments (MFMA B operand) of the query whose HD fp32 start at qrow: d = kk*32 + fq*8 .. +7; head 16: d = fq*4 .. +3
  static __device__ __forceinline__ void load_q(const float* __restrict__ qrow, int fq, kf_t (&qh)[NKK], kf_t (&ql)[NKK]) {
    if constexpr (HD == 16) {
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

  // st[kb] += (K tile rows kb*16 .. +15) . q :  kl.qh + kh.ql + kh.qh
  static __device__ __forceinline__ void qk(const char* Kh, const char* Kl, const kf_t (&qh)[NKK], const kf_t (&ql)[NKK],
                                            f32x4 (&st)[MAXKB], int fr, int fq) {
#pragma unroll
    for (int kb = 0; kb < MAXKB; ++kb) {
      f32x4 a = st[kb];
      const int krow = kb * 16 + fr;
      kf_t kh[NKK];
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) {
        // head 16: the 8-byte piece fq & 1 of chunk fq >> 1 (k_frag's address, once for the hi and the lo tile)
        const int ad = HD == 16 ? tile_addr<HD>(krow, fq >> 1) + (fq & 1) * 8 : tile_addr<HD>(krow, kk * 4 + fq);
        kf_t kl;
        if constexpr (HD == 16) kh[kk] = lds_read_b64(Kh + ad), kl = lds_read_b64(Kl + ad);      // kept ds_read_b64 (attn_frag.h)
        else kh[kk] = *(const kf_t*)(Kh + ad), kl = *(const kf_t*)(Kl + ad);
        a = score_mfma(kl, qh[kk], a);
        a = score_mfma(kh[kk], ql[kk], a);
      }
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) a = score_mfma(kh[kk], qh[kk], a);
      st[kb] = a;
    }
  }

  // One online-softmax step over the tile's scores st (masked entries hold -3e38), then O += V^T P^T with P and V split.
  // K-slot (fq*8 + j) of 32-key chunk c <-> key (2c + (j>>2))*16 + fq*4 + (j&3): exactly the order the lane holds P in.
  static __device__ __forceinline__ void softmax_pv(f32x4 (&st)[MAXKB], f32x4 (&o)[NDB], float& m, float& l, const char* Vh,
                                                    const char* Vl, int fr, int fq) {
    float tmax = -3.0e38f;
#pragma unroll
    for (int kb = 0; kb < MAXKB; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) tmax = fmaxf(tmax, st[kb][r]);
    tmax = rows4_max(tmax);
    const float mn = fmaxf(m, tmax);
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * LOG2E);
    const float mneg = -mn * LOG2E;
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < MAXKB; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = st[kb][r] > -1.0e38f ? __builtin_amdgcn_exp2f(fmaf(st[kb][r], LOG2E, mneg)) : 0.f;
        st[kb][r] = e;
        psum += e;
      }
    psum = rows4_sum(psum);
    l = l * alpha + psum;
    m = mn;
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      o[db][0] *= alpha; o[db][1] *= alpha; o[db][2] *= alpha; o[db][3] *= alpha;
    }
#pragma unroll
    for (int c = 0; c < nkc; ++c) {
      const f32x4 p0 = st[2 * c], p1 = st[2 * c + 1];
      uint4 ph, pl;
      split8(make_float4(p0[0], p0[1], p0[2], p0[3]), make_float4(p1[0], p1[1], p1[2], p1[3]), ph, pl);
      const bf16x8 pfh = __builtin_bit_cast(bf16x8, ph), pfl = __builtin_bit_cast(bf16x8, pl);
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        VtFrag vh, vl;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) {           // vt_half's address, once for the hi and the lo tile
          const int krow = (2 * c + hh) * 16 + fq * 4 + (fr >> 2);
          const int dcol = db * 16 + (fr & 3) * 4;
          const int ad = tile_addr<HD>(krow, dcol >> 3) + ((dcol >> 2) & 1) * 8;
          vh.h[hh] = lds_read_tr16(Vh + ad);
          vl.h[hh] = lds_read_tr16(Vl + ad);
        }
        o[db] = mfma_op16(vl.v, pfh, o[db]);
        o[db] = mfma_op16(vh.v, pfl, o[db]);
        o[db] = mfma_op16(vh.v, pfh, o[db]);
      }
    }
  }

  // row = the query's context row; the lane holds columns h*HD + db*16 + fq*4 .. +3.  bf16, or the strict mode's split operand
  // row (split_operand.h: a head of 64 is two groups, a head of 32 one, a head of 16 half of one -- heads 2 g and 2 g + 1 share group g).
  // split_d != 0: the split row, 3 * |split_d| values; split_d < 0: without the duplicate hi block -- the out-projection that reads
  // the rows is the fused three-product kernel (gemm_split3_fused)
  static __device__ __forceinline__ void store_ctx(const f32x4 (&o)[NDB], float l, bf16_t* row, int h, int fq, int split_d) {
    const float inv = l > 0.f ? 1.0f / l : 0.f;     // every key masked (an all-<pad> sequence): zero context, not NaN
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      const float a = o[db][0] * inv, b = o[db][1] * inv, c = o[db][2] * inv, d = o[db][3] * inv;
      // The split and the stores of split_operand.h, spelled out from its pieces (this file is built for bf16 operands only, so
      // pack_op2 is the header's pack): with split4 + split_store4 here every form of attention_split_kernel and both
      // msa_row_apply_split_kernel forms changed register allocation -- <4,1,bias,pad,64> 126 -> 128 VGPRs, <8,5,bias,pad,64>
      // 253 -> 254 -- and <10,5,bias,pad,64> went from 64 to 68 bytes of scratch; as written they compile to the same code as before
      uint2 p, r;
      p.x = pack_op2(a, b);
      p.y = pack_op2(c, d);
      if (!split_d) {
        *(uint2*)(row + h * HD + db * 16 + fq * 4) = p;
      } else {
        r.x = pack_op2(split_rest(a, p.x << 16), split_rest(b, p.x & 0xffff0000u));
        r.y = pack_op2(split_rest(c, p.y << 16), split_rest(d, p.y & 0xffff0000u));
        bf16_t* g = HD == 16 ? row + split_lo_offset(h * 16 + fq * 4) : row + (NKK * h + (db >> 1)) * kSplitVals + (db & 1) * 16 + fq * 4;
        *(uint2*)g = r;
        *(uint2*)(g + kSplitHi) = p;
        if (split_d > 0) *(uint2*)(g + kSplitDup) = p;
      }
    }
  }
};

// ---- full attention: one workgroup = (sequence, head, 64 * NQB queries); wave w owns the 16-query blocks w, w + 4, ... of the
// chunk.  The K / V tiles are read from HBM / L2 and split ONCE per workgroup and tile and every query block of the chunk runs
// against them, its online-softmax state (O, m, l: 18 registers) carried across the tiles: at T = 258 one workgroup per
// (sequence, head) instead of five that each re-staged and re-split the same 132 KB of fp32 K and V (round 3: 28 ms of the strict
// config-2 iteration were this kernel, 4x the bf16 mode's, most of it the 5x redundant fp32 tile traffic).  The per-query
// arithmetic (tile order, products, rounding points) is unchanged: identical bits.
template <int MAXKB, int NQB, bool BIASKV = false, bool PADMASK = false, int HD = 64>
__global__ __launch_bounds__(256, 2) void attention_split_kernel(
    const float* __restrict__ qkv, bf16_t* __restrict__ ctx, int split_d, int T, int H, int ld_qkv_, int ld_ctx_, int k_off,
    int v_off, SeqLayout sl, int n_qchunk, const int32_t* __restrict__ key_tok, int pad_idx, const float* __restrict__ bias_kv) {
  using A = SplitAttn<MAXKB, HD>;
  constexpr int tpad = A::tpad, ROW = HD * 2;
  __shared__ __attribute__((aligned(16))) char smem[4 * tpad * ROW];
  char *Kh = smem, *Kl = smem + tpad * ROW, *Vh = smem + 2 * tpad * ROW, *Vl = smem + 3 * tpad * ROW;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qc = blockIdx.x % n_qchunk, sh = blockIdx.x / n_qchunk;
  const int seq = sh / H, h = sh % H;
  const size_t row0 = (size_t)(seq / sl.inner_count) * sl.outer_rows + (size_t)(seq % sl.inner_count) * sl.inner_rows;
  const size_t ld_qkv = (size_t)ld_qkv_ * sl.row_step, ld_ctx = (size_t)ld_ctx_ * sl.row_step;
  const float* base = qkv + row0 * ld_qkv_ + h * HD;
  const int fr = lane & 15, fq = lane >> 4;
  const int qbase = qc * (64 * NQB) + wave * 16;     // block j of this wave: queries qbase + j*64 .. +15
  f32x4 o[NQB][A::NDB];
  float m[NQB], l[NQB];
#pragma unroll
  for (int j = 0; j < NQB; ++j) {
#pragma unroll
    for (int db = 0; db < A::NDB; ++db) o[j][db] = (f32x4){0.f, 0.f, 0.f, 0.f};
    m[j] = -3.0e38f;
    l[j] = 0.f;
  }

  // ESM-1 (add_bias_kv): key T = this head's bias_k / bias_v -- one more key, never masked (attention.hip)
  const int Tk = T + (BIASKV ? 1 : 0);
  const float* bk = BIASKV ? bias_kv + h * HD : nullptr;
  const float* bv = BIASKV ? bias_kv + (H + h) * HD : nullptr;
  for (int k0 = 0; k0 < Tk; k0 += tpad) {
    __syncthreads();
    A::template stage<BIASKV>(base + (size_t)k0 * ld_qkv + k_off, ld_qkv, T - k0, Kh, Kl, tid, bk);
    A::template stage<BIASKV>(base + (size_t)k0 * ld_qkv + v_off, ld_qkv, T - k0, Vh, Vl, tid, bv);
    // the tile's <pad> flags once per tile and wave, as wave-uniform bit masks (read per key, per query block and per
    // tile inside the score loop they were the pattern that made the ragged bf16 attention 5x slower before its flags were staged;
    // here the four fp32 tiles already fill the LDS two workgroups per CU may hold, so the flags live in scalar registers)
    unsigned long long pm[(tpad + 63) / 64];
    if (PADMASK) {
#pragma unroll
      for (int w = 0; w < (tpad + 63) / 64; ++w) {
        const int key = w * 64 + lane;
        pm[w] = __ballot(key < tpad && k0 + key < T && key_tok[row0 + (size_t)(k0 + key) * sl.row_step] == pad_idx);
      }
    }
    __syncthreads();
    const int tl = Tk - k0 - fq * 4;             // key k0 + kb*16 + fq*4 + r is padding iff kb*16 + r >= tl
#pragma unroll
    for (int j = 0; j < NQB; ++j) {
      const int q0 = qbase + j * 64;
      if (q0 >= T) continue;                       // wave-uniform
      typename A::kf_t qh[A::NKK], ql[A::NKK];
      A::load_q(base + (size_t)(q0 + fr < T ? q0 + fr : T - 1) * ld_qkv, fq, qh, ql);
      f32x4 st[MAXKB];
#pragma unroll
      for (int kb = 0; kb < MAXKB; ++kb) st[kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
      A::qk(Kh, Kl, qh, ql, st, fr, fq);
#pragma unroll
      for (int kb = 0; kb < MAXKB; ++kb)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (kb * 16 + r >= tl) st[kb][r] = -3.0e38f;
      if (PADMASK) {      // <pad> keys of a ragged batch: token of key t at key_tok[row0 + t * row_step]; -inf for chains, fair-esm's
                          // finite -10000 for the MSA Transformer's column attention (attention.hip)
        const float fill = sl.row_step == 1 ? -3.0e38f : -10000.0f;
#pragma unroll
        for (int kb = 0; kb < MAXKB; ++kb) {
          const uint32_t f4 = (uint32_t)(pm[kb >> 2] >> ((kb & 3) * 16 + fq * 4)) & 0xfu;      // keys kb*16 + fq*4 .. +3 of the tile
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if ((f4 >> r) & 1u) st[kb][r] = fill;
        }
      }
      A::softmax_pv(st, o[j], m[j], l[j], Vh, Vl, fr, fq);
    }
  }
#pragma unroll
  for (int j = 0; j < NQB; ++j) {
    const int q = qbase + j * 64 + fr;
    if (qbase + j * 64 < T && q < T) A::store_ctx(o[j], l[j], ctx + row0 * ld_ctx_ + (size_t)q * ld_ctx, h, fq, split_d);
  }
}

// ---- tied row attention (MSA), step 1: S[b,h][i][j] = scale * sum_r q_r[i] . k_r[j] ---------------------------------
// One workgroup = (msa b, head h, 64 queries, one key tile); the score blocks stay in the MFMA accumulators while the
// R alignment rows stream through the K tile.  S rows are ldS floats (C rounded up to 4) for 16-byte accesses.
template <int MAXKB>
__global__ __launch_bounds__(256, 2) void msa_row_scores_split_kernel(const float* __restrict__ qkv, float* __restrict__ S, int R,
                                                                      int C, int H, int ld_qkv, int k_off, float scale,
                                                                      int n_qchunk, int n_ktile, int ldS,
                                                                      const int32_t* __restrict__ tok, int pad_idx) {
  // tok (optional: a ragged list of MSAs padded to one [B][R][C] tensor, esm_msa_sampler.py:341): fair-esm's RowSelfAttention
  // zeroes q at <pad> positions before the sum over alignment rows and fills the scores of the key columns that are <pad> in
  // ROW 0 with -10000 (finite; the softmax in the apply kernel sees ordinary numbers)
  using A = SplitAttn<MAXKB>;
  constexpr int tpad = A::tpad;
  __shared__ __attribute__((aligned(16))) char smem[2 * tpad * 128];
  char *Kh = smem, *Kl = smem + tpad * 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kt = blockIdx.x % n_ktile, qc = (blockIdx.x / n_ktile) % n_qchunk, bh = blockIdx.x / (n_ktile * n_qchunk);
  const int b = bh / H, h = bh % H;
  const float* base = qkv + (size_t)b * R * C * ld_qkv + h * 64;
  const int fr = lane & 15, fq = lane >> 4;
  const int q0 = qc * 64 + wave * 16, k0 = kt * tpad;
  const bool active = q0 < C;
  const int qrow = q0 + fr < C ? q0 + fr : C - 1;
  f32x4 st[MAXKB];
#pragma unroll
  for (int kb = 0; kb < MAXKB; ++kb) st[kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int r = 0; r < R; ++r) {
    const float* rb = base + (size_t)r * C * ld_qkv;
    bf16x8 qh[2], ql[2];
    A::load_q(rb + (size_t)qrow * ld_qkv, fq, qh, ql);
    if (tok && tok[((size_t)b * R + r) * C + qrow] == pad_idx) {
      const bf16x8 z = __builtin_bit_cast(bf16x8, make_uint4(0, 0, 0, 0));
      qh[0] = z; qh[1] = z; ql[0] = z; ql[1] = z;
    }
    __syncthreads();
    A::stage(rb + (size_t)k0 * ld_qkv + k_off, ld_qkv, C - k0, Kh, Kl, tid);
    __syncthreads();
    if (active) A::qk(Kh, Kl, qh, ql, st, fr, fq);
  }
  const int q = q0 + fr;
  if (active && q < C) {
    float* dst = S + ((size_t)bh * C + q) * ldS + k0 + fq * 4;
#pragma unroll
    for (int kb = 0; kb < MAXKB; ++kb)
      if (k0 + kb * 16 + fq * 4 < ldS) {
        float4 v = make_float4(st[kb][0] * scale, st[kb][1] * scale, st[kb][2] * scale, st[kb][3] * scale);
        if (tok) {
          const int32_t* t0 = tok + (size_t)b * R * C;            // row 0 of this MSA
          const int key = k0 + kb * 16 + fq * 4;
          if (key < C && t0[key] == pad_idx) v.x = -10000.f;
          if (key + 1 < C && t0[key + 1] == pad_idx) v.y = -10000.f;
          if (key + 2 < C && t0[key + 2] == pad_idx) v.z = -10000.f;
          if (key + 3 < C && t0[key + 3] == pad_idx) v.w = -10000.f;
        }
        *(float4*)(dst + kb * 16) = v;
      }
  }
}

// ---- tied row attention, step 2: ctx_r = softmax_j(S) v_r; one workgroup = (b, h, alignment row r, 64 queries) ---------
template <int MAXKB>
__global__ __launch_bounds__(256, 2) void msa_row_apply_split_kernel(const float* __restrict__ qkv, const float* __restrict__ S,
                                                                     bf16_t* __restrict__ ctx, int split_d, int R, int C, int H,
                                                                     int ld_qkv, int ld_ctx, int v_off, int n_qchunk, int ldS) {
  using A = SplitAttn<MAXKB>;
  constexpr int tpad = A::tpad;
  __shared__ __attribute__((aligned(16))) char smem[2 * tpad * 128];
  char *Vh = smem, *Vl = smem + tpad * 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qc = blockIdx.x % n_qchunk, r = (blockIdx.x / n_qchunk) % R, bh = blockIdx.x / (n_qchunk * R);
  const int b = bh / H, h = bh % H;
  const float* rb = qkv + ((size_t)b * R + r) * C * ld_qkv + h * 64;
  const int fr = lane & 15, fq = lane >> 4;
  const int q0 = qc * 64 + wave * 16;
  const bool active = q0 < C;
  const int q = q0 + fr;
  const float* srow = S + ((size_t)bh * C + (q < C ? q : C - 1)) * ldS + fq * 4;
  f32x4 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) o[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m = -3.0e38f, l = 0.f;
  for (int k0 = 0; k0 < C; k0 += tpad) {
    f32x4 st[MAXKB];
#pragma unroll
    for (int kb = 0; kb < MAXKB; ++kb) {
      const int key0 = k0 + kb * 16 + fq * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (key0 < ldS) v = *(const float4*)(srow + k0 + kb * 16);
      st[kb][0] = key0 < C ? v.x : -3.0e38f;
      st[kb][1] = key0 + 1 < C ? v.y : -3.0e38f;
      st[kb][2] = key0 + 2 < C ? v.z : -3.0e38f;
      st[kb][3] = key0 + 3 < C ? v.w : -3.0e38f;
    }
    __syncthreads();
    A::stage(rb + (size_t)k0 * ld_qkv + v_off, ld_qkv, C - k0, Vh, Vl, tid);
    __syncthreads();
    if (active) A::softmax_pv(st, o, m, l, Vh, Vl, fr, fq);
  }
  if (active && q < C) A::store_ctx(o, l, ctx + (((size_t)b * R + r) * C + q) * ld_ctx, h, fq, split_d);
}

// ------------------------------------------------------------------------------------------------
// The dispatch: pure plans (no HIP call; pg_dbg_attention_plan prints them, tests/test_attention_plan_cpu.py pins them) and one
// launch switch per launcher, as in attention.hip.
// ------------------------------------------------------------------------------------------------
struct StrictRowPlan {
  int kb = 10;                     // key blocks per tile, 4 (up to 64 columns) or 10
  int n_chunk = 0, n_ktile = 1;    // 64-query chunks, and key tiles of the scores kernel
  unsigned grid_scores = 0, grid_apply = 0;      // 0: nothing to launch
};
static StrictRowPlan plan_msa_row_f32(int B, int R, int C, int H) {
  StrictRowPlan p;
  if (B == 0 || R == 0) return p;
  p.n_chunk = (C + 63) / 64;
  p.kb = C <= 64 ? 4 : 10;
  p.n_ktile = C <= 64 ? 1 : (C + 159) / 160;
  p.grid_scores = (unsigned)(B * H * p.n_chunk * p.n_ktile);
  p.grid_apply = (unsigned)(B * H * R * p.n_chunk);
  return p;
}
static std::string plan_text(const StrictRowPlan& p) {
  if (!p.grid_apply) return "nothing";
  return "row-split-f32 kb" + std::to_string(p.kb) + " kt" + std::to_string(p.n_ktile) + " " + std::to_string(p.grid_scores) + "wg, " +
         std::to_string(p.grid_apply) + "wg";
}
// <pad> tokens change what the kernels compute, not the plan
void msa_row_f32_plan_text(int B, int R, int C, int H, std::string* text) { *text = plan_text(plan_msa_row_f32(B, R, C, H)); }

// step 1 of the plan: launch_msa_row_attention_f32's first launch, and launch_msa_row_scores_f32's only one
static void launch_row_scores_split(hipStream_t s, const StrictRowPlan& p, const float* qkv, float* scores, int R, int C, int H, int ld_qkv,
                                    int k_off, float scale, const int32_t* tok, int pad_idx) {
  const int ldS = msa_row_scores_ld(C);
  auto go = [&](auto kb) {
    hipLaunchKernelGGL(msa_row_scores_split_kernel<decltype(kb)::value>, dim3(p.grid_scores), dim3(256), 0, s, qkv, scores, R, C, H, ld_qkv,
                       k_off, scale, p.n_chunk, p.n_ktile, ldS, tok, pad_idx);
  };
  if (p.kb == 4) go(std::integral_constant<int, 4>{});
  else go(std::integral_constant<int, 10>{});
}

int launch_msa_row_attention_f32(hipStream_t s, const float* qkv, float* scores, bf16_t* ctx, int split_d, int B, int R,
                                 int C, int H, int ld_qkv, int ld_ctx, int k_off, int v_off, float scale, const int32_t* tok,
                                 int pad_idx) {
  const StrictRowPlan p = plan_msa_row_f32(B, R, C, H);
  if (!p.grid_apply) return 0;
  note_kernel(plan_text(p).c_str());
  const int ldS = msa_row_scores_ld(C);         // `scores` holds B*H*C rows of ldS floats
  launch_row_scores_split(s, p, qkv, scores, R, C, H, ld_qkv, k_off, scale, tok, pad_idx);
  auto apply = [&](auto kb) {
    constexpr int KB = decltype(kb)::value;
    hipLaunchKernelGGL(msa_row_apply_split_kernel<KB>, dim3(p.grid_apply), dim3(256), 0, s, qkv, scores, ctx, split_d, R, C, H,
                       ld_qkv, ld_ctx, v_off, p.n_chunk, ldS);
  };
  if (p.kb == 4) apply(std::integral_constant<int, 4>{});
  else apply(std::integral_constant<int, 10>{});
  PG_HIP(hipGetLastError());
  return 0;
}

// The scores launch alone (the contacts tap): the same kernel, grid and arguments as the first launch above
void msa_row_scores_f32_plan_text(int B, int R, int C, int H, bool has_pad, std::string* text) {
  const StrictRowPlan p = plan_msa_row_f32(B, R, C, H);
  *text = !p.grid_scores ? "nothing"
                         : "row-scores-f32 kb" + std::to_string(p.kb) + " kt" + std::to_string(p.n_ktile) + (has_pad ? " pad " : " ") +
                               std::to_string(p.grid_scores) + "wg";
}
int launch_msa_row_scores_f32(hipStream_t s, const float* qkv, float* scores, int B, int R, int C, int H, int ld_qkv, int k_off, float scale,
                              const int32_t* tok, int pad_idx) {
  if (B < 0 || R < 0 || C <= 0 || H < 1) return fail(1, "row scores: bad shape");
  if ((int64_t)B * H * ((C + 63) / 64) * ((C + 159) / 160) > 0x7fffffff) return fail(1, "row scores: too many alignments");
  const StrictRowPlan p = plan_msa_row_f32(B, R, C, H);
  if (!p.grid_scores) return 0;
  std::string text;
  msa_row_scores_f32_plan_text(B, R, C, H, tok != nullptr, &text);
  note_kernel(text.c_str());
  launch_row_scores_split(s, p, qkv, scores, R, C, H, ld_qkv, k_off, scale, tok, pad_idx);
  PG_HIP(hipGetLastError());
  return 0;
}

// The (key blocks per tile, 16-query blocks per wave) pairs attention_split_kernel is built for -- every pair plan_attention_f32
// can produce -- and the head widths each is built at.  Head 128 runs 64-key tiles with 1, 2 or 3 query blocks per wave; heads 64 /
// 32 / 16 pair 64-key tiles with one query block only, so <4, 2> and <4, 3> exist at head 128 alone.
struct SplitPair {
  int kb, nqb;
  bool hd128, narrow;      // built at head 128; at heads 64 (with and without ESM-1's bias key), 32 and 16
};
constexpr SplitPair kSplitPairs[] = {{4, 1, true, true},   {4, 2, true, false},  {4, 3, true, false},  {6, 5, false, true}, {8, 5, false, true},
                                     {10, 1, false, true}, {10, 2, false, true}, {10, 3, false, true}, {10, 5, false, true}};
constexpr int kNSplitPairs = sizeof(kSplitPairs) / sizeof(kSplitPairs[0]);
// The launch switch over the pairs, as visit_rung (attn_frag.h): f(std::integral_constant<int, i>) for the entry i that is
// <kb, nqb>, and what it returns.  false: no such pair.
template <int I = 0, class F>
static bool visit_split_pair(int kb, int nqb, F&& f) {
  if constexpr (I == kNSplitPairs) {
    return false;
  } else {
    if (kb != kSplitPairs[I].kb || nqb != kSplitPairs[I].nqb) return visit_split_pair<I + 1>(kb, nqb, f);
    return f(std::integral_constant<int, I>{});
  }
}

struct StrictAttentionPlan {
  std::string error;               // not empty: the call is refused (error code 1)
  int kb = 0, nqb = 1, hd = 64;    // key blocks per tile and 16-query blocks per wave: one of kSplitPairs
  bool pad = false, bias = false;  // the kernel's PADMASK / BIASKV form
  unsigned grid = 0;               // 0: no sequences, nothing to launch
  int n_qchunk = 0;                // chunks of 64 * nqb queries per (sequence, head) pair
};
static StrictAttentionPlan plan_attention_f32(int64_t n_seq, int T, int H, int head_dim, bool has_pad, bool has_bias) {
  StrictAttentionPlan p;
  p.hd = head_dim, p.pad = has_pad, p.bias = has_bias;
  auto refuse = [&](const std::string& why) { p.error = why; return p; };
  p.error = attention_head_error(head_dim, has_bias);
  if (!p.error.empty()) return p;
  if (n_seq == 0) return p;
  if (T <= 0) return refuse("attention: empty sequence");
  // 16-query blocks per wave (the workgroup = 64 * nqb queries, all of them against each staged K / V tile): the smallest of 1, 2,
  // 3, 5 that covers the sequence with one workgroup, else 5
  const int Tk = T + (has_bias ? 1 : 0);           // every form: plain, <pad> mask, ESM-1's bias key (round 5)
  const bool one_tile = Tk <= 64;                  // at most 64 keys: a single 64-key tile, one query block per wave
  const int blocks = (T + 15) / 16;
  p.nqb = blocks <= 4 ? 1 : (blocks <= 8 ? 2 : (blocks <= 12 ? 3 : 5));
  if (one_tile) p.nqb = 1;
  p.n_qchunk = (T + 64 * p.nqb - 1) / (64 * p.nqb);
  if (n_seq * H * p.n_qchunk > 0x7fffffff) return refuse("attention: too many sequences");
  p.grid = (unsigned)(n_seq * H * p.n_qchunk);
  // key tile: 64 keys for short sequences, else 160 (80 KB of LDS: two workgroups per CU; at T = 258 a single 288-key
  // tile with one workgroup per CU was 1.6x slower)
  p.kb = one_tile ? 4 : 10;
  if (!one_tile && p.nqb == 5) {
    // Long sequences (five query blocks per wave): the tile height of 6, 8 or 10 key blocks that pads the keys least -- the
    // kernel's time follows the padded key count (T = 258: 3 x 96 = 288 keys 18.8 ms per config-2 iteration, 2 x 160 = 320 keys
    // 20.5, 3 x 128 = 384 keys 25.7); ties go to the taller tile.
    long best = ((long)Tk + 159) / 160 * 160;
    for (int k : {8, 6}) {
      const long padded = ((long)Tk + 16 * k - 1) / (16 * k) * (16 * k);
      if (padded < best) { best = padded; p.kb = k; }
    }
  }
  // Head 128: the four tiles (hi + lo of K and of V, 256-byte rows) are 1 KB per key, so the 80 KB that leave room for two workgroups
  // per CU hold 80 keys and the tallest even block count is 4: 64-key tiles (64 KB) at every length.  The taller tiles of heads 64 /
  // 32 would be 96 - 160 KB, one workgroup per CU -- the form that was 1.6x slower at head 64.
  // Five query blocks per wave would be o[5][8] = 160 accumulator registers and spill under the two-workgroup bound: three at most.
  if (head_dim == 128) {
    p.kb = 4;
    if (p.nqb > 3) {
      p.nqb = 3;
      p.n_qchunk = (T + 64 * 3 - 1) / (64 * 3);
      if (n_seq * H * p.n_qchunk > 0x7fffffff) return refuse("attention: too many sequences");
      p.grid = (unsigned)(n_seq * H * p.n_qchunk);
    }
  }
  return p;
}
static std::string plan_text(const StrictAttentionPlan& p) {
  if (!p.error.empty()) return "error: " + p.error;
  if (!p.grid) return "nothing";
  std::string t = "split-f32 kb" + std::to_string(p.kb) + " nqb" + std::to_string(p.nqb) + " hd" + std::to_string(p.hd);
  if (p.pad) t += " pad";
  if (p.bias) t += " bias";
  return t + " " + std::to_string(p.grid) + "wg";
}
void attention_f32_plan_text(int64_t n_seq, int T, int H, int head_dim, bool has_pad, bool has_bias, std::string* text) {
  *text = plan_text(plan_attention_f32(n_seq, T, H, head_dim, has_pad, has_bias));
}

// entry I of kSplitPairs: its <BIASKV, PADMASK, HD> form for this call; no bias key at head 32 / 128 / 16.
// false: the pair is not built at this head width and nothing was launched
template <int I, class... Args>
static bool launch_split(int hd, bool pad, bool bias, dim3 grid, hipStream_t s, Args... args) {
  constexpr SplitPair P = kSplitPairs[I];
  auto form = [&](auto bias_c, auto hd_c) {
    constexpr bool BIASKV = decltype(bias_c)::value;
    constexpr int HD = decltype(hd_c)::value;
    if (pad) hipLaunchKernelGGL((attention_split_kernel<P.kb, P.nqb, BIASKV, true, HD>), grid, dim3(256), 0, s, args...);
    else hipLaunchKernelGGL((attention_split_kernel<P.kb, P.nqb, BIASKV, false, HD>), grid, dim3(256), 0, s, args...);
    return true;
  };
  using std::false_type;
  using std::integral_constant;
  if (hd == 128) {
    if constexpr (P.hd128) return form(false_type{}, integral_constant<int, 128>{});
  } else if constexpr (P.narrow) {
    if (hd == 32) return form(false_type{}, integral_constant<int, 32>{});
    if (hd == 16) return form(false_type{}, integral_constant<int, 16>{});
    return bias ? form(std::true_type{}, integral_constant<int, 64>{}) : form(false_type{}, integral_constant<int, 64>{});
  }
  return false;
}

int launch_attention_f32(hipStream_t s, const float* qkv, bf16_t* ctx, int split_d, int64_t n_seq, int T, int H,
                         int ld_qkv, int ld_ctx, int k_off, int v_off, SeqLayout sl, const int32_t* key_tok, int pad_idx,
                         const float* bias_kv, int head_dim) {
  const StrictAttentionPlan p = plan_attention_f32(n_seq, T, H, head_dim, key_tok != nullptr, bias_kv != nullptr);
  if (!p.error.empty()) return fail(1, p.error);
  if (!p.grid) return 0;
  note_kernel(plan_text(p).c_str());
  const bool launched = visit_split_pair(p.kb, p.nqb, [&](auto i) {
    return launch_split<decltype(i)::value>(p.hd, p.pad, p.bias, dim3(p.grid), s, qkv, ctx, split_d, T, H, ld_qkv, ld_ctx, k_off, v_off, sl,
                                            p.n_qchunk, key_tok, pad_idx, bias_kv);
  });
  // the plan produced a pair outside kSplitPairs, or one that is not built at this head width: a bug in plan_attention_f32
  if (!launched) return fail(1, "attention: the strict kernel is not built for this (key tile, query blocks, head dimension)");
  PG_HIP(hipGetLastError());
  return 0;
}

PG_OPS_END
