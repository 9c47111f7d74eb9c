// Fused multi-head self-attention for one sequence per workgroup (ESM-1b layers):
//   ctx[b, t, h*HD:(h+1)*HD] = softmax_j( q[b,t,h] . k[b,j,h] ) @ v[b,:,h]        (q pre-scaled by HD^-0.5)
// This is the attention inside fair-esm's ProteinBertModel that the reference reaches through
// `self.model.model(batch)["logits"]` (/root/reference/src/pgen/esm_sampler.py:223).
//
// CDNA4 mapping, written for head dim HD = 64 (ESM-1b, MSA-1b, ESM-2 650M / 3B); HD = 32 (ESM-2 150M) is the same kernel with half
// the LDS row, one score MFMA per key block and two output blocks; HD = 128 (ESM-2 15B) with twice the row, four score MFMAs and eight
// output blocks, whole sequences up to 288 keys and 128-key tiles beyond; HD = 16 (ESM-2 8M) with a 32-byte row, one half-depth score
// MFMA per key block and one output block (attn_frag.h):
//   * grid = B*H workgroups of 4 waves; K and V (both row-major, XOR-swizzled 16-B chunks) live in LDS for
//     the whole sequence (T <= 576: 2 x 72 KB) and are shared by all query blocks; longer sequences use
//     attention_long_kernel (288-key tiles, online softmax).
//   * per wave, 16 queries at a time (the block arithmetic and its fragment layouts: attn_frag.h): S^T = K.Q^T with
//     v_mfma_f32_16x16x32_bf16 ("swapped" product), so a lane holds, for ONE query (lane & 15), 4 consecutive keys of every
//     16-key block: the whole score row is lane-local except for a 4-lane reduction -> exact (non-online) softmax in
//     registers, no LDS round trip for P.
//   * the K-slot order of the PV contraction is free, so it is chosen to be exactly the order the lane
//     already holds P in (two 16-key blocks per 32-wide MFMA step); the matching V^T fragment (4 + 4 keys of one d per
//     lane) comes straight out of the row-major V tile through gfx950's transposing LDS read ds_read_b64_tr_b16 -- no
//     transposition pass when the tile is staged (that pass and its 4-byte LDS writes were 16 % of the kernel).
//   * O^T = V^T.P^T, so a lane ends with 4 consecutive d for one query -> 8-byte row-major stores.
#include <stdlib.h>

#include "attn_frag.h"

PG_OPS_BEGIN

// MAXKB = number of 16-key blocks computed (T <= 16*MAXKB), even.  The dispatch ladder guarantees
// T > 16*(MAXKB-6), so only the last 6 blocks can hold masked (>= T) keys.

// Phase timestamps for tools/probes/attention_phases.hip (compiled out of the library): lane 0 of every wave records the
// shader clock at the phase boundaries of its first query blocks.
#ifdef PG_ATT_PROF
__device__ unsigned long long* pg_att_prof;      // [workgroup][wave][8 slots][8 stamps]
#define PG_T(slot, i)                                                                                              \
  do {                                                                                                             \
    if ((slot) < 8 && (threadIdx.x & 63) == 0)                                                                     \
      pg_att_prof[(((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 8 + (slot)) * 8 + (i)] = __builtin_readcyclecounter(); \
  } while (0)
#else
#define PG_T(slot, i)
#endif

// BIASKV: ESM-1's extra bias_k / bias_v key (a template parameter: the extra staging branch and the runtime key count cost the
// config-2 kernel 8 % when they were runtime conditions)
// SPLIT (round 6): the grid's LAST workgroups each take 1 / split of one (sequence, head) pair's query blocks instead of a whole pair
// -- workgroups [0, split_from) whole pairs, workgroup split_from + u the blocks part, part + split, ... (part = u % split) of pair
// split_from + u / split -- so that the partial last round of a launch (a 32-chain shard: 640 pairs on 512 resident workgroups =
// one full round + a quarter-full one that takes as long) becomes short workgroups that fill the chip.  A query block's arithmetic
// does not depend on which workgroup runs it: same bits.  The plain launch (SPLIT = false) is the kernel of rounds 1-5, unchanged.
// HD: the head dimension, 64 or 32 (attn_frag.h).  At 32 a key is 64 bytes of LDS, K + V of 576 keys 72 KB: at least two
// workgroups per CU on every rung (what limits a rung is the score row in registers, 4 VGPRs per key block, not the LDS -- which is
// also why the whole-sequence kernel still ends at 576 keys).  The plain and SPLIT head-32 forms compile to <= 128 VGPRs up to 20 key
// blocks and <= 168 up to 26 without a tighter bound, so four / three workgroups are resident there (DESIGN 10 has the table).
// HD = 128: K + V are MAXKB * 8 KB of LDS, so two workgroups share a CU up to 10 key blocks (2 x 80 KB, as head 64's rung 20) and one
// holds it alone on rungs 12 .. 18; the launch bound follows the LDS.  The K look-ahead is two key blocks there (kbuf[2][2][4] = 64
// VGPRs; the six of head 64 would be 192), the V look-ahead stays two chunks (vbuf[3][8] = 96 VGPRs).
// (the PADMASK form of 10 blocks adds 160 flag bytes to the 80 KB and is alone on its CU: pad = true asks for 1 there)
// HD = 16: K + V are MAXKB KB of LDS (36 KB at 576 keys) and never the limit; the launch bound stays the 2 of head 32 (the score row
// st[MAXKB] alone is 144 VGPRs on rung 36) and the compiler's own register counts give more on the lower rungs (attention_resident).
constexpr int attention_occupancy(int maxkb, int hd, bool pad = false) {
  return hd == 128 ? (maxkb <= 8 || (maxkb == 10 && !pad) ? 2 : 1) : hd == 64 ? (maxkb <= 18 ? 2 : 1) : 2;
}
// Workgroups per CU that the HOST counts with when it splits a partial last round (plan_attention): what is resident, not what the
// launch bound asks the compiler for.  Head 64: two up to 20 key blocks, one beyond.  The two functions differ at kb = 20: its
// 2 x 80 KB of LDS fit a CU and the plain and SPLIT forms, compiled under the looser bound of 1, still come out at 158 VGPRs + 88
// AGPRs = two waves per SIMD, so two workgroups do share a CU there and the split counts two.  Head 32: four / three / two (the
// VGPR figures above).
// Head 128 (the plain and SPLIT forms; DESIGN 10 has the table): four at 4 key blocks (32 KB, 124 VGPRs), three at 6 (48 KB, 160
// VGPRs), two up to 10 (80 KB), one beyond -- the LDS decides from 8 blocks on.
// Head 16 (the plain and SPLIT forms, as compiled: waves per SIMD = workgroups per CU, the hardware's 8 at most): 8 up to 6 key
// blocks (<= 54 VGPRs), 7 at 8 (66), 6 at 10 (78), 5 up to 14 (92), 4 up to 22 (126), 3 up to 34 (166), 2 at 36 (174).
constexpr int attention_resident16(int kb) {
  return kb <= 6 ? 8 : kb <= 8 ? 7 : kb <= 10 ? 6 : kb <= 14 ? 5 : kb <= 22 ? 4 : kb <= 34 ? 3 : 2;
}
constexpr int attention_resident(int kb, int hd) {
  return hd == 16 ? attention_resident16(kb) : hd == 128 ? (kb <= 4 ? 4 : (kb <= 6 ? 3 : (kb <= 10 ? 2 : 1))) : hd == 64 ? (kb <= 20 ? 2 : 1) : (kb <= 20 ? 4 : (kb <= 26 ? 3 : 2));
}
template <int MAXKB, bool PADMASK, bool BIASKV = false, bool SPLIT = false, int HD = 64>
__global__ __launch_bounds__(256, attention_occupancy(MAXKB, HD, PADMASK)) void attention_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ ctx, int T,
                                                       int H, int ld_qkv_, int ld_ctx_, int k_off, int v_off,
                                                       SeqLayout sl, const int32_t* __restrict__ key_tok, int pad_idx,
                                                       const bf16_t* __restrict__ bias_kv, int split_from = 0, int split = 1) {
  constexpr int ROW = HD * 2, NKK = score_steps(HD), NDB = HD / 16;      // bytes per key in LDS, score MFMAs per key block, 16-wide output blocks
  typedef kfrag_t<HD> kf_t;                                              // the score product's fragment (attn_frag.h)
  __shared__ __attribute__((aligned(16))) char smem[2 * MAXKB * 16 * ROW + (PADMASK ? MAXKB * 16 : 0)];
  char* Ks = smem;
  char* Vs = smem + MAXKB * 16 * ROW;          // V rows, same layout as K (tile_addr)
  char* padf = smem + 2 * MAXKB * 16 * ROW;    // PADMASK: one byte per key, 1 = this key's token is <pad>

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  PG_T(7, 0);
  // sequence `seq` = token rows row0 + t*row_step (ESM: contiguous rows of chain b; MSA column attention: the R rows
  // of one column, C token-rows apart)
  int pair = blockIdx.x, qb_first = wave, qb_step = 4;
  if (SPLIT && (int)blockIdx.x >= split_from) {
    const int u = blockIdx.x - split_from;
    pair = split_from + u / split;
    qb_first = u % split + split * wave;                     // blocks part, part + split, ... dealt to the waves in turn
    qb_step = 4 * split;
  }
  const int seq = pair / H, h = pair % H;
  const size_t row0 = (size_t)(seq / sl.inner_count) * sl.outer_rows + (size_t)(seq % sl.inner_count) * sl.inner_rows;
  const size_t ld_qkv = (size_t)ld_qkv_ * sl.row_step, ld_ctx = (size_t)ld_ctx_ * sl.row_step;
  const bf16_t* base = qkv + row0 * ld_qkv_ + h * HD;
  // ESM-1 (add_bias_kv): key T is the learned bias_k / bias_v of this head -- one more key, attended by every query, never masked
  const int Tk = T + (BIASKV ? 1 : 0);
  // All MAXKB key blocks are computed unconditionally: K rows / V^T columns past T are zero-filled and
  // their scores are masked, so no wave-uniform branches (and no dynamic register indexing) are needed.
  constexpr int nkc = MAXKB / 2;

  // ---- stage K and V (swizzled rows)
  stage_kv<MAXKB * 16, 256, BIASKV, HD>(Ks, Vs, tid, base, ld_qkv, k_off, v_off, 0, T, bias_kv + h * HD, bias_kv + (H + h) * HD);
  if (PADMASK) {
    // the <pad> flags of the sequence's keys, once per workgroup (read per key inside the score loop they were 72 dependent global
    // loads per lane and query block: 292 bytes of scratch, a ragged batch's attention 5x the time of a full one)
    for (int key = tid; key < MAXKB * 16; key += 256)
      padf[key] = (key < T && key_tok[row0 + (size_t)key * sl.row_step] == pad_idx) ? 1 : 0;
  }
  PG_T(7, 1);
  __syncthreads();
  PG_T(7, 2);

  const int fr = lane & 15, fq = lane >> 4;
  const int nqb = (T + 15) >> 4;  // query blocks of 16
  // Q fragment (MFMA B operand): query fr, d = kk*32 + fq*8 .. +7; the next block's fragment is prefetched while
  // the current one is computed (a wave has nothing else to cover a global round trip with)
  kf_t qf[NKK], qn[NKK];
  auto load_q = [&](int qb, kf_t (&dst)[NKK]) {
    int qrow = qb * 16 + fr;
    if (qrow >= T) qrow = T - 1;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) dst[kk] = q_frag<HD>(base + (size_t)qrow * ld_qkv, kk, fq);
  };
  if (qb_first < nqb) load_q(qb_first, qf);
  for (int qb = qb_first; qb < nqb; qb += qb_step) {
    if (qb + qb_step < nqb) load_q(qb + qb_step, qn);
    PG_T(qb >> 2, 0);

    // S^T blocks: st[kb][r] = S[query fr][key kb*16 + fq*4 + r]
    f32x4 st[MAXKB];
    {
      // K fragments are fetched one chunk (CH key blocks) ahead of the MFMAs that use them: with 2 waves per SIMD
      // the LDS latency must be covered inside the wave (PMC: 44 % of wave cycles were s_waitcnt before this)
      constexpr int CH = HD == 128 ? 2 : (MAXKB % 6 == 0) ? 6 : (MAXKB % 4 == 0 ? 4 : 2);
      kf_t kbuf[2][CH][NKK];
      auto load_chunk = [&](int ch, kf_t (&dst)[CH][NKK]) {
#pragma unroll
        for (int u = 0; u < CH; ++u) {
#if defined(PG_ATT_PROF) && PG_ATT_ABL == 1      /* ablation: one K fragment read per chunk instead of CH */
          const int krow = (ch * CH + (u > 0 ? 0 : u)) * 16 + fr;
          if (u > 0) { for (int kk = 0; kk < NKK; ++kk) dst[u][kk] = dst[0][kk]; continue; }
#else
          const int krow = (ch * CH + u) * 16 + fr;
#endif
#pragma unroll
          for (int kk = 0; kk < NKK; ++kk) dst[u][kk] = k_frag<HD>(Ks, krow, kk, fq);
        }
      };
      load_chunk(0, kbuf[0]);
#pragma unroll
      for (int ch = 0; ch < MAXKB / CH; ++ch) {
        if (ch + 1 < MAXKB / CH) load_chunk(ch + 1, kbuf[(ch + 1) & 1]);
        __builtin_amdgcn_sched_barrier(0);
        // the two d-halves of a key block as two sweeps over the chunk, so that no MFMA is issued right behind the one
        // producing its accumulator input (hipcc otherwise pairs them through one temporary register); at head 32 one MFMA
        // contracts the whole head and there is a single sweep
#pragma unroll
        for (int u = 0; u < CH; ++u)
          st[ch * CH + u] = score_mfma(kbuf[ch & 1][u][0], qf[0], (f32x4){0.f, 0.f, 0.f, 0.f});
        if constexpr (NKK == 2) {
#pragma unroll
          for (int u = 0; u < CH; ++u)
            st[ch * CH + u] = score_mfma(kbuf[ch & 1][u][1], qf[1], st[ch * CH + u]);
        }
        if constexpr (NKK == 4) {                      // head 128: three more sweeps, one per 32 d
#pragma unroll
          for (int kk = 1; kk < 4; ++kk)
#pragma unroll
            for (int u = 0; u < CH; ++u)
              st[ch * CH + u] = score_mfma(kbuf[ch & 1][u][kk], qf[kk], st[ch * CH + u]);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    PG_T(qb >> 2, 1);
    int tl = Tk - fq * 4;
    asm volatile("" : "+v"(tl));              // keep the compares inside the loop (no hoisted lane masks)
#pragma unroll
    for (int kb = MAXKB > 6 ? MAXKB - 6 : 0; kb < MAXKB; ++kb)
      if ((kb + 1) * 16 > Tk) st[kb] = mask_tail(st[kb], kb, tl);      // wave-uniform: only key blocks that reach past the last key
    float mx = lane_max(st);
    if (PADMASK) {
      // ragged batch (only reachable through the forward entry points; the Gibbs path never holds <pad>): keys that are
      // <pad> tokens are masked.  key_tok = the token buffer; the token of key t of this sequence sits where its qkv row does
      // (row0 + t * row_step).  Chains (ESM: contiguous rows) get -inf like fair-esm's key_padding_mask; the strided sequences
      // of the MSA Transformer's column attention get its finite fill of -10000 (an all-<pad> column then softmaxes to a uniform
      // row instead of NaN, exactly as fair-esm's ColumnSelfAttention does -- and NaN at a padded position would reach the real
      // ones through 0 * NaN in the next tied row attention).
      const float fill = sl.row_step == 1 ? -3.0e38f : -10000.0f;
      mx = -3.0e38f;
#pragma unroll
      for (int kb = 0; kb < MAXKB; ++kb) {
        st[kb] = mask_pad(st[kb], *(const uint32_t*)(padf + kb * 16 + fq * 4), fill);
#pragma unroll
        for (int r = 0; r < 4; ++r) mx = fmaxf(mx, st[kb][r]);
      }
    }
    const float inv = softmax_exact(st, mx);
    PG_T(qb >> 2, 2);

    // O^T[d][q] = sum_key V^T[d][key] * P^T[key][q]
    f32x4 o[NDB];
#pragma unroll
    for (int db = 0; db < NDB; ++db) o[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
    {
      // V^T fragments fetched two 32-key chunks ahead of the PV MFMAs
      VtFrag vbuf[3][NDB];
      auto load_v = [&](int c, VtFrag (&dst)[NDB]) {
#pragma unroll
        for (int db = 0; db < NDB; ++db) {
#if defined(PG_ATT_PROF) && PG_ATT_ABL == 2      /* ablation: one V^T fragment read per chunk instead of 4 */
          if (db > 0) { dst[db] = dst[0]; continue; }
#endif
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) dst[db].h[hh] = vt_half<HD>(Vs, (2 * c + hh) * 16, db, fr, fq);
        }
      };
      load_v(0, vbuf[0]);
      if (nkc > 1) load_v(1, vbuf[1]);
#pragma unroll
      for (int c = 0; c < nkc; ++c) {
        if (c + 2 < nkc) load_v(c + 2, vbuf[(c + 2) % 3]);
        const bf16x8 pf = p_frag(st[2 * c], st[2 * c + 1]);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int db = 0; db < NDB; ++db) o[db] = mfma_op16(vbuf[c % 3][db].v, pf, o[db]);
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    PG_T(qb >> 2, 3);
    // store: lane holds O[q = qb*16 + fr][d = db*16 + fq*4 + r]
    const int q = qb * 16 + fr;
    if (q < T) store_ctx(o, inv, ctx + row0 * ld_ctx_ + (size_t)q * ld_ctx + h * HD + fq * 4);
    qf[0] = qn[0];
    if constexpr (NKK == 2) qf[1] = qn[1];
    if constexpr (NKK == 4) { qf[1] = qn[1]; qf[2] = qn[2]; qf[3] = qn[3]; }
    PG_T(qb >> 2, 4);
  }
  PG_T(7, 3);
}

// ------------------------------------------------------------------------------------------------
// Long sequences (T > 576, up to the 1024-token limit of the learned position table): same MFMA formulation, keys
// processed in tiles of 288 with the online-softmax recurrence (running max m, running sum l, rescaled O).
// One workgroup = (sequence, head, 64 queries); wave w owns one 16-query block for the whole key loop, so the
// per-wave state is just O (16 regs) + m + l; every workgroup streams all K/V tiles of its head (L2-resident).
// ------------------------------------------------------------------------------------------------
// MAXKB = 16-key blocks per tile (even), OCC = workgroups per CU the register / LDS budget is set for: <18, 2> is the long-sequence
// kernel.  <10, 4> (160-key tiles, four workgroups per CU, 117 VGPRs) and <12, 3> were measured at config 2 in round 4 against
// attention_kernel: 9.1 / 11.1 ms per iteration against 7.0 (EXPERIMENTS.md) -- every 64-query workgroup re-stages the head's K / V.
// Head 128: <8, 2> -- 128-key tiles, 64 KB + 128 flag bytes, the tallest even tile of which two fit a CU (attn_frag.h).
template <int MAXKB, int OCC, bool PADMASK, bool BIASKV, int HD = 64>
__global__ __launch_bounds__(256, OCC) void attention_long_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ ctx, int T,
                                                               int H, int ld_qkv_, int ld_ctx_, int k_off, int v_off,
                                                               SeqLayout sl, int n_qchunk, const int32_t* __restrict__ key_tok_,
                                                               int pad_idx, const bf16_t* __restrict__ bias_kv_) {
  // the <pad> mask and ESM-1's bias key as template parameters (as in attention_kernel): as runtime conditions they kept the kernel
  // at 256 VGPRs with 110 dwords of scratch
  const int32_t* __restrict__ key_tok = PADMASK ? key_tok_ : nullptr;
  const bf16_t* __restrict__ bias_kv = BIASKV ? bias_kv_ : nullptr;
  constexpr int tpad = MAXKB * 16, nkc = MAXKB / 2;
  constexpr int ROW = HD * 2, NKK = score_steps(HD), NDB = HD / 16;      // as in attention_kernel
  typedef kfrag_t<HD> kf_t;
  __shared__ __attribute__((aligned(16))) char smem[2 * tpad * ROW + (PADMASK ? tpad : 0)];
  char* Ks = smem;
  char* Vs = smem + tpad * ROW;
  char* padf = smem + 2 * tpad * ROW;             // PADMASK: one byte per key of the tile, 1 = <pad> token (see attention_kernel)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int qc = blockIdx.x % n_qchunk, sh = blockIdx.x / n_qchunk;
  const int seq = sh / H, h = sh % H;
  const size_t row0 = (size_t)(seq / sl.inner_count) * sl.outer_rows + (size_t)(seq % sl.inner_count) * sl.inner_rows;
  const size_t ld_qkv = (size_t)ld_qkv_ * sl.row_step, ld_ctx = (size_t)ld_ctx_ * sl.row_step;
  const bf16_t* base = qkv + row0 * ld_qkv_ + h * HD;
  const int fr = lane & 15, fq = lane >> 4;
  const int q0 = qc * 64 + wave * 16;
  const bool active = q0 < T;                        // wave-uniform
  kf_t qf[NKK];
  {
    int qrow = q0 + fr;
    if (qrow >= T) qrow = T - 1;
#pragma unroll
    for (int kk = 0; kk < NKK; ++kk) qf[kk] = q_frag<HD>(base + (size_t)qrow * ld_qkv, kk, fq);
  }
  f32x4 o[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db) o[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float m = -3.0e38f, l = 0.f;
  constexpr float LOG2E = 1.44269504088896341f;
  const int Tk = T + (bias_kv ? 1 : 0);              // ESM-1: key T = this head's bias_k / bias_v (see attention_kernel)

  for (int k0 = 0; k0 < Tk; k0 += tpad) {
    __syncthreads();
    stage_kv<tpad, 256, BIASKV, HD>(Ks, Vs, tid, base, ld_qkv, k_off, v_off, k0, T, bias_kv + h * HD, bias_kv + (H + h) * HD);
    if (PADMASK) {
      for (int key = tid; key < tpad; key += 256)
        padf[key] = (k0 + key < T && key_tok[row0 + (size_t)(k0 + key) * sl.row_step] == pad_idx) ? 1 : 0;
    }
    __syncthreads();
    if (!active) continue;
    f32x4 st[MAXKB];
#pragma unroll
    for (int kb = 0; kb < MAXKB; ++kb) {
      st[kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < NKK; ++kk) st[kb] = score_mfma(k_frag<HD>(Ks, kb * 16 + fr, kk, fq), qf[kk], st[kb]);
    }
    const int tl = Tk - k0 - fq * 4;
#pragma unroll
    for (int kb = 0; kb < MAXKB; ++kb) st[kb] = mask_tail(st[kb], kb, tl);
    float tmax = lane_max(st);
    if (PADMASK) {                               // <pad> keys of a ragged batch (see attention_kernel)
      const float fill = sl.row_step == 1 ? -3.0e38f : -10000.0f;
      tmax = -3.0e38f;
#pragma unroll
      for (int kb = 0; kb < MAXKB; ++kb) {
        st[kb] = mask_pad(st[kb], *(const uint32_t*)(padf + kb * 16 + fq * 4), fill);
#pragma unroll
        for (int r = 0; r < 4; ++r) tmax = fmaxf(tmax, st[kb][r]);
      }
    }
    const float mn = fmaxf(m, rows4_max(tmax));
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * LOG2E);
    const float mneg = -mn * LOG2E;
    float psum = 0.f;
#pragma unroll
    for (int kb = 0; kb < MAXKB; ++kb)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float e = __builtin_amdgcn_exp2f(fmaf(st[kb][r], LOG2E, mneg));
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
      const bf16x8 pf = p_frag(st[2 * c], st[2 * c + 1]);
#pragma unroll
      for (int db = 0; db < NDB; ++db) {
        VtFrag vf;
#pragma unroll
        for (int hh = 0; hh < 2; ++hh) vf.h[hh] = vt_half<HD>(Vs, (2 * c + hh) * 16, db, fr, fq);
        o[db] = mfma_op16(vf.v, pf, o[db]);
      }
    }
  }
  const int q = q0 + fr;
  if (active && q < T) store_ctx(o, 1.0f / l, ctx + row0 * ld_ctx_ + (size_t)q * ld_ctx + h * HD + fq * 4);
}

// ------------------------------------------------------------------------------------------------
// The dispatch.  plan_attention says which kernel template runs on which grid: a pure function of the shape, the device's CU count
// and the process's PGIBBS_ATTN_SPLIT switch, without a HIP call, so pg_dbg_attention_plan prints its answers on a machine without a GPU
// (tests/test_attention_plan_cpu.py pins them for the shapes the project is measured on).  launch_attention_seq_bf16 is the one
// switch over it.
// ------------------------------------------------------------------------------------------------
struct AttentionPlan {
  std::string error;               // not empty: the call is refused (error code 1)
  bool whole = true;               // attention_kernel on rung kb; false: attention_long_kernel (more than 576 keys)
  int kb = 0, hd = 64;
  bool pad = false, bias = false;  // the kernel's PADMASK / BIASKV form
  int split_from = 0, split = 1;   // split > 1: the SPLIT form, the pairs from split_from on as `split` workgroups each
  unsigned grid = 0;               // workgroups of 256 threads; 0: no sequences, nothing to launch
  int n_qchunk = 0;                // the long kernel's 64-query chunks per (sequence, head) pair
};

static AttentionPlan plan_attention(int64_t n_seq, int T, int H, int head_dim, bool has_pad, bool has_bias, int row_step, int n_cu) {
  AttentionPlan p;
  p.hd = head_dim, p.pad = has_pad, p.bias = has_bias;
  auto refuse = [&](const char* why) { p.error = why; return p; };
  p.error = attention_head_error(head_dim, has_bias);
  if (!p.error.empty() || n_seq == 0) return p;
  const int64_t pairs = n_seq * H;
  if (pairs > 0x7fffffff) return refuse("attention: too many sequences");
  if (T <= 0) return refuse("attention: empty sequence");
  // The rung: the T tokens + ESM-1's bias_k / bias_v key.  The forms without the bias key (the Gibbs path, and ragged batches)
  // take the fine ladder: a chain of 200 residues has 13 key blocks, not 18.
  p.kb = attention_rung(T + (has_bias ? 1 : 0), !has_bias, attention_max_keys(head_dim));
  p.whole = p.kb != 0;
  if (!p.whole) {                                // more than 576 keys: 288-key tiles (at head 32: 36 KB of LDS for K + V);
                                                 // head 128: more than 288 keys, 128-key tiles
    p.n_qchunk = (T + 63) / 64;
    if (pairs * p.n_qchunk > 0x7fffffff) return refuse("attention: too many sequences");
    p.grid = (unsigned)(pairs * p.n_qchunk);
    return p;
  }
  p.grid = (unsigned)pairs;
  // Round 6: split the pairs of a partial last round (see attention_kernel).  Whole-sequence kernels for chains (row_step 1) of at
  // least four query blocks, without <pad> mask / bias key (the Gibbs path), counted in attention_resident workgroups per CU.
  // PGIBBS_ATTN_SPLIT=0 switches it off.
  static const int split_on = env_int("PGIBBS_ATTN_SPLIT", 1);
  if (split_on && !has_pad && !has_bias && row_step == 1 && T >= 64) {
    const long slots = (long)n_cu * attention_resident(p.kb, head_dim);
    const long rem = pairs % slots;
    const int nqb = (T + 15) / 16;
    int sp = rem ? (int)(slots / rem) : 1;
    if (sp > 4) sp = 4;
    if (sp > nqb / 4) sp = nqb / 4;            // every part keeps at least one block per wave
    if (sp >= 2) {
      p.split = sp;
      p.split_from = (int)(pairs - rem);
      p.grid = (unsigned)(p.split_from + rem * sp);
    }
  }
  return p;
}

// the plan in the text a launch records (note_kernel): the kernel template and its grid
static std::string plan_text(const AttentionPlan& p) {
  if (!p.error.empty()) return "error: " + p.error;
  if (!p.grid) return "nothing";
  std::string t = (p.whole ? "whole kb" + std::to_string(p.kb) : std::string(p.hd == 128 ? "long t128" : "long t288")) + " hd" + std::to_string(p.hd);
  if (p.pad) t += " pad";
  if (p.bias) t += " bias";
  if (p.split > 1) return t + " split" + std::to_string(p.split) + " " + std::to_string(p.split_from) + "+" + std::to_string(p.grid - p.split_from) + "wg";
  return t + " " + std::to_string(p.grid) + "wg";
}
void attention_plan_text(int64_t n_seq, int T, int H, int head_dim, bool has_pad, bool has_bias, int row_step, int n_cu, std::string* text) {
  *text = plan_text(plan_attention(n_seq, T, H, head_dim, has_pad, has_bias, row_step, n_cu));
}

// one rung of the key-block ladder: the kernel's <PADMASK, BIASKV, SPLIT> form for this call.  The bias-key forms are built
// on the coarse rungs only (attn_frag.h), and at head dimension 64 only (ESM-1 has heads of 64; the plan refuses the rest).
template <int KB, int HD, class... Args>
static void launch_rung(bool pad, bool bias, bool split, dim3 grid, hipStream_t s, Args... args) {
  auto go = [&](auto* kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, args...); };
  if constexpr (coarse_rung(KB) && HD == 64) {
    if (bias && pad) return go(attention_kernel<KB, true, true, false, HD>);
    if (bias) return go(attention_kernel<KB, false, true, false, HD>);
  }
  if constexpr (KB * 16 <= attention_max_keys(HD)) {      // head 128 above rung 18 is not built, and the plan never asks for it
    if (pad) go(attention_kernel<KB, true, false, false, HD>);
    else if (split) go(attention_kernel<KB, false, false, true, HD>);
    else go(attention_kernel<KB, false, false, false, HD>);
  }
}
// the long kernel's <PADMASK, BIASKV> form; no bias key at head 32 / 128 / 16; 128-key tiles at head 128, else 288
template <int HD, class... Args>
static void launch_long(bool pad, bool bias, dim3 grid, hipStream_t s, Args... args) {
  auto go = [&](auto* kernel) { hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, args...); };
  if constexpr (HD == 64) {
    if (bias && pad) return go(attention_long_kernel<18, 2, true, true, HD>);
    if (bias) return go(attention_long_kernel<18, 2, false, true, HD>);
  }
  constexpr int KB = HD == 128 ? 8 : 18;
  if (pad) go(attention_long_kernel<KB, 2, true, false, HD>);
  else go(attention_long_kernel<KB, 2, false, false, HD>);
}

int launch_attention_seq_bf16(hipStream_t s, const bf16_t* qkv, bf16_t* ctx, int64_t n_seq, int T, int H, int ld_qkv,
                              int ld_ctx, int k_off, int v_off, SeqLayout sl, const int32_t* key_tok, int pad_idx,
                              const bf16_t* bias_kv, int head_dim) {
  const AttentionPlan p = plan_attention(n_seq, T, H, head_dim, key_tok != nullptr, bias_kv != nullptr, sl.row_step, device_cu_count());
  if (!p.error.empty()) return fail(1, p.error);
  if (!p.grid) return 0;
  note_kernel(plan_text(p).c_str());
  auto launch = [&](auto hd) {
    constexpr int HD = decltype(hd)::value;
    if (!p.whole)
      return launch_long<HD>(p.pad, p.bias, dim3(p.grid), s, qkv, ctx, T, H, ld_qkv, ld_ctx, k_off, v_off, sl, p.n_qchunk, key_tok,
                             pad_idx, bias_kv);
    visit_rung(p.kb, [&](auto kb) {
      launch_rung<decltype(kb)::value, HD>(p.pad, p.bias, p.split > 1, dim3(p.grid), s, qkv, ctx, T, H, ld_qkv, ld_ctx, k_off, v_off,
                                           sl, key_tok, pad_idx, bias_kv, p.split_from, p.split);
    });
  };
  visit_head_width(head_dim, launch);
  PG_HIP(hipGetLastError());
  return 0;
}

int launch_attention_bf16(hipStream_t s, const bf16_t* qkv, bf16_t* ctx, int B, int T, int H, int ld_qkv, int ld_ctx,
                          int k_off, int v_off, const int32_t* key_tok, int pad_idx, const bf16_t* bias_kv, int head_dim) {
  SeqLayout sl = {1, T, 0, 1};
  return launch_attention_seq_bf16(s, qkv, ctx, B, T, H, ld_qkv, ld_ctx, k_off, v_off, sl, key_tok, pad_idx, bias_kv, head_dim);
}

PG_OPS_END
