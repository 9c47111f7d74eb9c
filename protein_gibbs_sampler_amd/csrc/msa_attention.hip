// Tied row attention of the MSA Transformer (fair-esm RowSelfAttention), reached by the reference
// through `self.model.model(batch)["logits"]` (/root/reference/src/pgen/esm_msa_sampler.py:136,236):
//   A[h,i,j] = scale * sum_r sum_d q[r,i,h,d] k[r,j,h,d]      (scale = 64^-0.5 / sqrt(R), one map per head for ALL rows)
//   P = softmax_j(A);   ctx[r,i,h,:] = sum_j P[h,i,j] v[r,j,h,:]
// (Column attention is the plain fused attention kernel over strided sequences: attention.hip.)
//
// One workgroup = (msa b, head h, NW*16 queries); wave w owns 16 of them.  Pass 1 streams K_r (C x 64) through LDS for
// r = 0..R-1 and accumulates the S^T blocks of the wave's 16 queries in registers with v_mfma_f32_16x16x32_bf16
// (the lane-local layout of attn_frag.h: a lane holds one query's scores for 4 keys of every 16-key block),
// then one exact softmax; pass 2 streams V_r through LDS the same way (V^T fragments via ds_read_b64_tr_b16) and emits
// ctx for every row with the same P fragments.
// Every workgroup of a (msa, head) re-streams all R tiles, so the workgroup is made as wide as the registers allow:
// NW = 9 waves cover C = 257 columns (bos + 256) in 2 workgroups instead of 5 (the 5th held a single query).
// The tiles alternate between two LDS buffers (one barrier per row) and are fetched into registers two rows ahead
// (one for the widest tiles); measured at 64 MSAs x 32 x 257: 1.79 -> 1.31 ms per layer, of which the strided K / V / Q
// tile loads (128 contiguous bytes per token row) are 0.55 ms and the MFMAs 0.1 ms;
// the query chunks of one (msa, head) are placed on one XCD so the re-streamed tiles hit its L2.
#include "attn_frag.h"

PG_OPS_BEGIN

template <int MAXKB, int NW, int mode>
__global__ __launch_bounds__(NW * 64) void msa_row_attention_kernel(
    const bf16_t* __restrict__ qkv, bf16_t* __restrict__ ctx, int R, int C, int H, int ld_qkv, int ld_ctx, int k_off,
    int v_off, float scale, int n_qblk, int n_bh, int n_rc, float* __restrict__ partial) {
  // mode 0: fused (both passes over all R rows).  Split-R (few (msa, head) pairs, e.g. generate_single with B = 1):
  // mode 1: pass 1 over the row chunk rc only, partial S^T -> partial[bh][rc][query][key];
  // mode 3: (one workgroup per (msa, head, query block)) S = sum of the n_rc partial maps in fixed order, softmax,
  //         P as bf16 MFMA fragments -> pfrag (16 B per lane and fragment, stored behind the partial maps);
  // mode 2: pass 2 over the row chunk rc only with the P fragments of mode 3.
  constexpr int tpad = MAXKB * 16;
  constexpr int NT = NW * 64;                      // threads
  using KRegs = TileRegs<tpad, NT>;                // one row's K (pass 2: V) tile share
  constexpr int NIT = KRegs::NIT;                  // tile items per thread: one uint4 = 8 d of one key
  constexpr int AHEAD = (MAXKB <= 18 && NIT <= 9) ? 2 : 1;   // rows fetched ahead into registers (register budget)
  constexpr int BUF = tpad * 128;                  // one tile buffer: tpad key rows of 128 B (K_r in pass 1, V_r in pass 2)
  __shared__ __attribute__((aligned(16))) char smem[2 * BUF];

  // mode 3 is launched with one wave per workgroup (the reduction has no LDS phase; this spreads it over the chip):
  // blockIdx carries the wave slot
  const int tid = threadIdx.x, lane = tid & 63, wave = mode == 3 ? (int)(blockIdx.x % NW) : tid >> 6;
  const int blk = mode == 3 ? (int)(blockIdx.x / NW) : (int)blockIdx.x;
  // XCD-aware mapping (block b runs on XCD b % 8): the query chunks of one (msa, head) get consecutive slots of ONE
  // XCD, so the K_r / V_r tiles they all stream are served by that XCD's L2 after the first touch.
  int qblk, bh;
  const int per_rc = n_bh * n_qblk;
  const int rc = blk / per_rc;                       // row chunk (0 in fused mode)
  {
    const int bidx = blk - rc * per_rc;
    const int xcd = bidx & 7, slot = bidx >> 3;
    const int full = (n_bh / 8) * 8;                 // (msa, head) pairs covered by the XCD-aligned part of the grid
    if (bidx < full * n_qblk) {
      bh = (slot / n_qblk) * 8 + xcd;
      qblk = slot % n_qblk;
    } else {                                         // remainder: plain order
      const int rest = bidx - full * n_qblk;
      bh = full + rest / n_qblk;
      qblk = rest % n_qblk;
    }
  }
  const int rsz = (R + n_rc - 1) / n_rc;
  const int r_lo = mode == 0 ? 0 : rc * rsz;
  const int r_hi = mode == 0 ? R : ((rc + 1) * rsz < R ? (rc + 1) * rsz : R);
  const int b = bh / H, h = bh % H;
  const bf16_t* base = qkv + (size_t)b * R * C * ld_qkv + h * 64;   // row (r*C + i)
  const int fr = lane & 15, fq = lane >> 4;
  const int q0 = qblk * (NW * 16) + wave * 16;
  const bool active = q0 < C;                                      // wave-uniform
  int qrow = q0 + fr;
  if (qrow >= C) qrow = C - 1;

  f32x4 st[MAXKB];
#pragma unroll
  for (int kb = 0; kb < MAXKB; ++kb) st[kb] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // ---- pass 1: scores summed over rows.  Tile r goes to LDS buffer r & 1; the registers it came from are refilled with
  // row r + 2 right away, so a tile has two rows of MFMAs to arrive.
  KRegs kA, kB;
  auto load_k = [&](KRegs& g, int r, int off) {
    const bf16_t* rb = base + (size_t)r * C * ld_qkv;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + it * NT, row = i >> 3, c = i & 7;
      g.r[it] = make_uint4(0, 0, 0, 0);
      if (i < tpad * 8 && row < C) g.r[it] = *(const uint4*)(rb + (size_t)row * ld_qkv + off + c * 8);
    }
  };
  auto score_row = [&](KRegs& g, int r) {
    char* Ks = smem + (r & 1) * BUF;
    tile_store(g, tid, Ks);
    const bf16_t* qp = base + ((size_t)r * C + qrow) * ld_qkv + fq * 8;     // in flight across the barrier
    const bf16x8 qf0 = *(const bf16x8*)qp, qf1 = *(const bf16x8*)(qp + 32);
    __syncthreads();                                  // tile r visible; everybody is done with tile r - 1 (other buffer)
    if (r + AHEAD < r_hi) load_k(g, r + AHEAD, k_off);
    if (active) {
      // the two k-halves of a key block accumulate into the same registers: keep them MAXKB MFMAs apart
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
        for (int kb = 0; kb < MAXKB; ++kb) st[kb] = mfma_op16(k_frag(Ks, kb * 16 + fr, kk, fq), kk ? qf1 : qf0, st[kb]);
      }
    }
  };
  if (mode < 2) {
    if (r_lo < r_hi) load_k(kA, r_lo, k_off);
    if (AHEAD == 2) {
      if (r_lo + 1 < r_hi) load_k(kB, r_lo + 1, k_off);
      for (int r = r_lo; r < r_hi; r += 2) {
        score_row(kA, r);
        if (r + 1 < r_hi) score_row(kB, r + 1);
      }
    } else {
      for (int r = r_lo; r < r_hi; ++r) score_row(kA, r);
    }
  }

  if (mode == 1) {          // partial score map of this row chunk: lane stores its 4 keys x MAXKB blocks for query q0+fr
    if (active && q0 + fr < C) {
      float* dst = partial + (((size_t)bh * n_rc + rc) * C + (q0 + fr)) * tpad + fq * 4;
#pragma unroll
      for (int kb = 0; kb < MAXKB; ++kb) *(float4*)(dst + kb * 16) = make_float4(st[kb][0], st[kb][1], st[kb][2], st[kb][3]);
    }
    return;
  }
  if (mode == 3 && active) {
    const int qq = (q0 + fr < C) ? q0 + fr : C - 1;
    for (int c2 = 0; c2 < n_rc; ++c2) {
      const float* src = partial + (((size_t)bh * n_rc + c2) * C + qq) * tpad + fq * 4;
#pragma unroll
      for (int kb = 0; kb < MAXKB; ++kb) {
        const float4 v = *(const float4*)(src + kb * 16);
        st[kb][0] += v.x; st[kb][1] += v.y; st[kb][2] += v.z; st[kb][3] += v.w;
      }
    }
  }
  union PF { bf16x8 v; uint32_t u[4]; uint4 q; };
  PF pf[MAXKB / 2];
  // fragment store of this wave: [(bh, qblk, wave)][c][lane]
  uint4* pfrag = (uint4*)(partial + (size_t)n_bh * n_rc * C * tpad) + (((size_t)bh * n_qblk + qblk) * NW + wave) * (MAXKB / 2) * 64 + lane;
  if (mode == 2) {
#pragma unroll
    for (int c = 0; c < MAXKB / 2; ++c) pf[c].q = pfrag[c * 64];
  } else {
    // ---- softmax over keys ---------------------------------------------------------------------
    constexpr float LOG2E = 1.44269504088896341f;
    float mx = -3.0e38f;
    int tl = C - fq * 4;
  #pragma unroll
    for (int kb = 0; kb < MAXKB; ++kb) {
  #pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        st[kb][r4] *= scale;
        if (kb >= MAXKB - 6 && kb * 16 + r4 >= tl) st[kb][r4] = -3.0e38f;
        mx = fmaxf(mx, st[kb][r4]);
      }
    }
    mx = rows4_max(mx);
    const float mneg = -mx * LOG2E;
    float sum = 0.f;
  #pragma unroll
    for (int kb = 0; kb < MAXKB; ++kb) {
  #pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const float e = __builtin_amdgcn_exp2f(fmaf(st[kb][r4], LOG2E, mneg));
        st[kb][r4] = e;
        sum += e;
      }
    }
    sum = rows4_sum(sum);
    const float inv = 1.0f / sum;
  #pragma unroll
    for (int c = 0; c < MAXKB / 2; ++c) {           // P itself, not exp(s - max): pass 2 stores O as it is
      const f32x4 lo = st[2 * c], hi = st[2 * c + 1];
      pf[c].u[0] = pack_op2(lo[0] * inv, lo[1] * inv);
      pf[c].u[1] = pack_op2(lo[2] * inv, lo[3] * inv);
      pf[c].u[2] = pack_op2(hi[0] * inv, hi[1] * inv);
      pf[c].u[3] = pack_op2(hi[2] * inv, hi[3] * inv);
    }
    if (mode == 3) {
#pragma unroll
      for (int c = 0; c < MAXKB / 2; ++c) pfrag[c * 64] = pf[c].q;
      return;
    }
  }

  // ---- pass 2: ctx[r] = P . V_r for every row.  V_r tiles are staged exactly like the K_r tiles (row-major, swizzled,
  // two buffers, fetched AHEAD rows ahead); the V^T fragments of the PV MFMAs come out of them through the transposing
  // LDS read (vt_frag) -- the former transposition pass was most of this kernel's VALU work.
  auto apply_row = [&](KRegs& g, int r, int slot) {
    char* Vs = smem + slot * BUF;
    tile_store(g, tid, Vs);
    __syncthreads();
    if (r + AHEAD < r_hi) load_k(g, r + AHEAD, v_off);
    if (active) {
      f32x4 o[4];
#pragma unroll
      for (int db = 0; db < 4; ++db) o[db] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int c = 0; c < MAXKB / 2; ++c) {
#pragma unroll
        for (int db = 0; db < 4; ++db) {
          VtFrag vf;
#pragma unroll
          for (int hh = 0; hh < 2; ++hh) vf.h[hh] = vt_half(Vs, (2 * c + hh) * 16, db, fr, fq);
          o[db] = mfma_op16(vf.v, pf[c].v, o[db]);
        }
      }
      const int q = q0 + fr;
      if (q < C) store_ctx(o, 1.0f, ctx + ((size_t)(b * R + r) * C + q) * ld_ctx + h * 64 + fq * 4);
    }
  };
  __syncthreads();                                    // pass 1's last tile (either buffer) fully consumed
  if (r_lo < r_hi) load_k(kA, r_lo, v_off);
  if (AHEAD == 2) {
    if (r_lo + 1 < r_hi) load_k(kB, r_lo + 1, v_off);
    for (int r = r_lo; r < r_hi; r += 2) {
      apply_row(kA, r, 0);
      if (r + 1 < r_hi) apply_row(kB, r + 1, 1);
    }
  } else {
    for (int r = r_lo; r < r_hi; ++r) apply_row(kA, r, (r - r_lo) & 1);
  }
}

// ------------------------------------------------------------------------------------------------
// The dispatch, as in attention.hip: plan_msa_row is a pure function of the shape and the scratch on offer
// (pg_dbg_attention_plan prints it, tests/test_attention_plan_cpu.py pins it); the launcher and the engine's scratch sizing share it.
// ------------------------------------------------------------------------------------------------
// Waves per workgroup on rung kb: 4 up to 64 columns, beyond that the widest the register budget of the score fragments allows
// (9 waves up to 288 keys, 8 beyond).  The one definition: the plan's geometry and the kernel template's NW both come from here.
constexpr int row_attention_waves(int kb) { return kb <= 4 ? 4 : (kb <= 18 ? 9 : 8); }
static_assert(row_attention_waves(20) == row_attention_waves(24), "the 20 -> 24 exception below keeps the query blocks it was decided on");

struct RowPlan {
  const char* error = nullptr;     // not null: the call is refused with error_code
  int error_code = 0;
  int kb = 0, nw = 0;              // msa_row_attention_kernel<kb, nw, mode>
  int n_qblk = 0;                  // workgroups (nw * 16 queries each) per (msa, head)
  int n_rc = 1;                    // > 1: the split-R form (modes 1, 3, 2) over n_rc row chunks, else the fused mode 0
  size_t split_bytes = 0;          // fp32 scratch the split-R form of this shape needs (0: the shape does not split)
  unsigned grid = 0;               // workgroups of nw waves (modes 0, 1, 2); 0: nothing to launch
  unsigned grid_reduce = 0;        // mode 3: workgroups of one wave
};
// order_bh: the (msa, head) count the split-R decision is taken on.  The row loop is split over workgroups when the (msa, head,
// query-chunk) grid alone cannot fill the chip; the number of row chunks fixes the order of the sum over alignment rows, so it is
// derived from order_bh -- the (msa, head) count of the JOB, or of ONE template in a batched generate_single -- not from this
// call's share.  scratch_bytes: the fp32 scratch on offer; a split-R form that does not fit runs fused.
static RowPlan plan_msa_row(int B, int R, int C, int H, int order_bh, size_t scratch_bytes) {
  RowPlan p;
  auto refuse = [&](int code, const char* why) { p.error_code = code, p.error = why; return p; };
  if (B == 0 || R == 0) return p;
  if (C <= 0) return refuse(1, "row attention: empty alignment");
  if (C > 576) return refuse(5, "row attention: alignments wider than 576 token columns (<cls> + 575 residues) take the fp32-scores path");
  const int n_bh = B * H, obh = order_bh > 0 ? order_bh : n_bh;
  // a rung for every even block count (round 4)
  p.kb = attention_rung(C, true);
  p.nw = row_attention_waves(p.kb);
  p.n_qblk = ((C + 15) / 16 + p.nw - 1) / p.nw;
  if (obh * ((C + 63) / 64) < 384 && obh * p.n_qblk < 384 && R >= 8) {      // few (msa, head, 64-query) units: the chip would idle
    p.n_rc = 512 / (obh * p.n_qblk);                  // two whole rounds of one workgroup per CU (measured best: 512 vs 768)
    if (p.n_rc > R / 4) p.n_rc = R / 4;
    if (p.n_rc < 1) p.n_rc = 1;
  }
  // One exception, measured (profiles/r04_attention_key_block_ladder_ab.txt): one template of 32 x 301 (288 workgroups, split-R form)
  // takes 0.97 ms on the 20-block rung against 0.88 on the 24-block one, while bigger grids gain 10 %.  (The 20-block rung's 80 KB of
  // LDS lets two workgroups share a CU; whether that is the cause was not established.)  Grids below two rounds stay on 24 blocks.
  if (p.kb == 20 && (long)n_bh * p.n_qblk * p.n_rc < 512) p.kb = 24;
  // fp32 scratch of the split-R form: n_rc partial score maps per (msa, head), then every wave's P fragments (1 KiB each)
  if (p.n_rc > 1) p.split_bytes = (size_t)n_bh * p.n_rc * C * (p.kb * 16) * 4 + (size_t)n_bh * p.n_qblk * p.nw * (p.kb / 2) * 1024;
  if (p.split_bytes > scratch_bytes) p.n_rc = 1;
  p.grid = (unsigned)(n_bh * p.n_qblk * p.n_rc);
  p.grid_reduce = p.n_rc > 1 ? (unsigned)(n_bh * p.n_qblk * p.nw) : 0;
  return p;
}
// bytes of fp32 scratch the split-R form needs for B alignments (0: the shape does not split)
size_t msa_row_split_scratch_bytes(int B, int R, int C, int H, int order_bh) {
  return plan_msa_row(B, R, C, H, order_bh, ~(size_t)0).split_bytes;
}

static std::string plan_text(const RowPlan& p) {
  if (p.error) return std::string("error: ") + p.error;
  if (!p.grid) return "nothing";
  std::string t = "row kb" + std::to_string(p.kb) + " w" + std::to_string(p.nw) + " rc" + std::to_string(p.n_rc) + " " + std::to_string(p.grid) + "wg";
  return p.n_rc > 1 ? t + ", reduce " + std::to_string(p.grid_reduce) + "x1w, " + std::to_string(p.grid) + "wg" : t;
}
// with the scratch msa_row_split_scratch_bytes asks for on offer, as the engine launches it
void msa_row_plan_text(int B, int R, int C, int H, int order_bh, std::string* text) {
  *text = plan_text(plan_msa_row(B, R, C, H, order_bh, ~(size_t)0));
}

int launch_msa_row_attention_bf16(hipStream_t s, const bf16_t* qkv, bf16_t* ctx, int B, int R, int C, int H, int ld_qkv,
                                  int ld_ctx, int k_off, int v_off, float scale, float* partial, size_t partial_bytes,
                                  int order_bh) {
  const RowPlan p = plan_msa_row(B, R, C, H, order_bh, partial ? partial_bytes : 0);
  if (p.error) return fail(p.error_code, p.error);
  if (!p.grid) return 0;
  note_kernel(plan_text(p).c_str());
  visit_rung(p.kb, [&](auto kb) {
    constexpr int KB = decltype(kb)::value, NW = row_attention_waves(KB);
    auto go = [&](auto* kernel, dim3 grid, dim3 block) {
      hipLaunchKernelGGL(kernel, grid, block, 0, s, qkv, ctx, R, C, H, ld_qkv, ld_ctx, k_off, v_off, scale, p.n_qblk, B * H, p.n_rc, partial);
    };
    const dim3 grid(p.grid), block(NW * 64);
    if (p.n_rc == 1) return go(msa_row_attention_kernel<KB, NW, 0>, grid, block);
    go(msa_row_attention_kernel<KB, NW, 1>, grid, block);
    go(msa_row_attention_kernel<KB, NW, 3>, dim3(p.grid_reduce), dim3(64));
    go(msa_row_attention_kernel<KB, NW, 2>, grid, block);
  });
  PG_HIP(hipGetLastError());
  return 0;
}

PG_OPS_END
