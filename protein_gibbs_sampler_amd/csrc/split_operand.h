// The strict precision mode's split operand row (PG_PREC_FP32): the ONLY definition of its arithmetic, its layout and its stores.
//
// A row of d fp32 values v becomes 3 d bf16 values: hi = bf16(v), lo = bf16(v - hi), interleaved in groups of 32 columns.  Group g
// of an ACTIVATION row is [lo(32) | hi(32) | hi(32)] of columns 32 g .. 32 g + 31, group g of a WEIGHT row [hi | lo | hi].  One bf16
// GEMM over K' = 3 d on two such rows sums, per 32 columns and in this order, x_lo.w_hi + x_hi.w_lo + x_hi.w_hi in its fp32
// accumulator -- whichever tile kernel runs it.  The fused 16-wave kernel (gemm_w16.hip; the tail tile of gemm_epilogue.h) reads only
// the first two blocks of each group -- 64 values = one 128-byte K-step at a source stride of kSplitVals * 2 = 192 bytes -- and issues
// the same three products from registers; the producer of an activation row may then leave the third block unwritten (dup = false:
// launch_layernorm_bf16 split3_dup, EPI_SPLIT2_GELU, split_d < 0; the consumer is gemm_split3_fused's to name).
// The pair is bf16 in either operand flavour (pg_common.h): nothing here goes through pack_op2 / op16_to_f32.
// Writers: store_row_bf16 (ln_row.h), split3_bf16_kernel (elementwise.hip), the two split epilogues of gemm_epilogue.h and
// SplitAttn::store_ctx (attention_f32.hip; from this header's pieces, its comment says why).  Readers: every GEMM (as
// plain rows of 3 d), gemm_split3_w16_kernel and gemm_tail_tile64<SPLIT3>, split3_rows_to_host (api_dbg.hip).
// tests/_ln_host.py store_rows_host restates it independently.
#pragma once
#include "pg_common.h"

namespace pg {

// ---- the layout ----------------------------------------------------------------------------------------------------------------
constexpr int kSplitCols = 32;      // columns of a group = values of a block
constexpr int kSplitBlocks = 3;     // blocks of a group: a row of d columns is kSplitBlocks * d values
constexpr int kSplitVals = 96;      // values of a group
static_assert(kSplitVals == kSplitBlocks * kSplitCols, "a group is three blocks");
constexpr int kSplitHi = 32;        // activation row: the hi value of a column, from its lo value
constexpr int kSplitDup = 64;       // ... and the duplicate hi value
// offset, in the row of 3 d values, of the lo value of column `col` of an activation row = of the first block of its group
__host__ __device__ constexpr int split_group_offset(int group, int col_in_group) { return group * kSplitVals + col_in_group; }
__host__ __device__ constexpr int split_lo_offset(int col) { return split_group_offset(col >> 5, col & (kSplitCols - 1)); }

#if defined(__HIPCC__)
// ---- the split ------------------------------------------------------------------------------------------------------------------
typedef __bf16 split_bf16x2_t __attribute__((ext_vector_type(2)));
typedef uint32_t split_u32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t split_pack2(float a, float b) {      // v_cvt_pk_bf16_f32: round to nearest even
  split_bf16x2_t v = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(uint32_t, v);
}
// v - hi, rounded once: never contracted with a multiply that produced v, whatever the translation unit's setting
__device__ __forceinline__ float split_rest(float v, uint32_t hi_bits) {
#pragma clang fp contract(off)
  return v - __uint_as_float(hi_bits);
}
// four fp32 -> four bf16 hi + four bf16 lo = bf16(v - hi); (a, b) in .x, (c, d) in .y, the first of a pair in the low half
__device__ __forceinline__ void split4(float a, float b, float c, float d, uint2& hi, uint2& lo) {
  hi.x = split_pack2(a, b);
  hi.y = split_pack2(c, d);
  lo.x = split_pack2(split_rest(a, hi.x << 16), split_rest(b, hi.x & 0xffff0000u));
  lo.y = split_pack2(split_rest(c, hi.y << 16), split_rest(d, hi.y & 0xffff0000u));
}
// two split4, written with the four packs of hi first: in split4's order the strict attention kernels that split every staged K / V
// tile with this (attention_f32.hip) schedule differently (msa_row_scores_split_kernel<10>: 1499 -> 1510 instructions)
__device__ __forceinline__ void split8(const float4& a, const float4& b, uint4& hi, uint4& lo) {
  hi.x = split_pack2(a.x, a.y); hi.y = split_pack2(a.z, a.w); hi.z = split_pack2(b.x, b.y); hi.w = split_pack2(b.z, b.w);
  lo.x = split_pack2(split_rest(a.x, hi.x << 16), split_rest(a.y, hi.x & 0xffff0000u));
  lo.y = split_pack2(split_rest(a.z, hi.y << 16), split_rest(a.w, hi.y & 0xffff0000u));
  lo.z = split_pack2(split_rest(b.x, hi.z << 16), split_rest(b.y, hi.z & 0xffff0000u));
  lo.w = split_pack2(split_rest(b.z, hi.w << 16), split_rest(b.w, hi.w & 0xffff0000u));
}

// ---- the stores: g = the row + split_lo_offset(first column); 4 consecutive columns (col % 4 == 0) or 8 (col % 8 == 0) ----------
__device__ __forceinline__ void split_store4(bf16_t* g, uint2 hi, uint2 lo, bool dup) {
  *(uint2*)g = lo;
  *(uint2*)(g + kSplitHi) = hi;
  if (dup) *(uint2*)(g + kSplitDup) = hi;
}
__device__ __forceinline__ void split_store4_weight(bf16_t* g, uint2 hi, uint2 lo) {      // [hi | lo | hi]
  *(uint2*)g = hi;
  *(uint2*)(g + kSplitHi) = lo;
  *(uint2*)(g + kSplitDup) = hi;
}
// non-temporal: a GEMM epilogue's rows, read next by another launch.  (gemm_tile.h's PG_NT_STORE is the same builtin; its vector
// types live in the operand-flavoured namespace of the GEMM headers, which the row kernels that include this header do not see)
__device__ __forceinline__ void split_store8_nt(bf16_t* g, uint4 hi, uint4 lo, bool dup) {
  __builtin_nontemporal_store(__builtin_bit_cast(split_u32x4_t, lo), (split_u32x4_t*)g);
  __builtin_nontemporal_store(__builtin_bit_cast(split_u32x4_t, hi), (split_u32x4_t*)(g + kSplitHi));
  if (dup) __builtin_nontemporal_store(__builtin_bit_cast(split_u32x4_t, hi), (split_u32x4_t*)(g + kSplitDup));
}
#endif

}  // namespace pg
