// The per-wave arithmetic of ONE block of 16 queries against keys that sit in LDS, shared by every MFMA attention kernel with
// 16-bit operands (attention.hip, msa_attention.hip, the attention tail of gemm_colattn.hip, chain_trunk.hip's attention unit)
// and, for the tile addressing and the transposing read, by the strict mode's SplitAttn (attention_f32.hip).  Kernels that
// must give the same bits call the same functions here.  Included inside operand-flavoured files: pack_op2 / mfma_op16 resolve
// per flavour (pg_common.h).
//
// The pieces take and return values (a score block, a fragment half) and spell a tile address as pointer + row*128 + swizzle:
// hipcc optimises a __forceinline__ function on its own before it inlines it, and the forms that update a caller's array through
// a reference under a condition, or hand the whole address over as one integer, cost the kernels registers (up to 76 VGPRs on the
// tall rungs of attention_kernel) -- compare the ISA of every user before changing a signature here.
//
// The head dimension is the template parameter HD of everything that touches a tile or the context: 64 (the default: ESM-1b,
// ESM-1, MSA-1b, ESM-2 650M / 3B -- every caller that names no HD is the head-64 form, instruction for instruction what it was
// before HD existed), 32 (ESM-2 150M), 128 (ESM-2 15B) or 16 (ESM-2 8M).  Softmax, masks and p_frag do not depend on it; the
// key-block ladder ends at 18 blocks at 128 (below).
//
// Geometry (head dim 64).  A K or V tile is row-major in LDS, one key per 128-byte row, the row's eight 16-byte chunks
// XOR-swizzled with (row & 7).  fr = lane & 15 is the lane's query (the MFMA column), fq = lane >> 4.
//   * S^T = K.Q^T: a score block st[kb][r] = S[query fr][key kb*16 + fq*4 + r] -- a query's whole score row is lane-local up
//     to a 4-lane (xor 16, 32) reduction, so the softmax runs in registers;
//   * O^T = V^T.P^T: K-slot (fq*8 + j) of 32-key chunk c <-> key (2c + (j>>2))*16 + fq*4 + (j&3), exactly the order the lane
//     holds P in; o[db][r] = O[query fr][d = db*16 + fq*4 + r] -> 8-byte row-major context stores.
//
// Geometry (head dim 32).  One key per 64-byte row of four 16-byte chunks; ONE v_mfma_f32_16x16x32 contracts the whole head
// (k_frag: chunk fq of key row fr), two output blocks o[2].  Two keys share a 128-byte line and four a 256-byte bank row, so
// chunk ^ (row & 7) no longer means anything; the swizzle is  chunk ^ ((row >> 1) & 2)  -- bit 2 of the key row swaps the two
// 32-byte halves of its row.  Why that and nothing more (LDS banks: 64 x 4 bytes = sixteen 16-byte slots per bank row; the slot of
// chunk c of row r is 4 (r & 3) + c before the swizzle):
//   * the score fragment is a ds_read_b128, served in four groups of 16 lanes, {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the
//     same + 32.  Lane = 16 fq + fr reads chunk fq of row fr, so a group holds rows {0-3, 12-15} at one chunk c and rows {4-11} at
//     chunk c ^ 1: for every value of (r & 3) four rows, one from each quarter q2 = (r >> 2) & 3 of the block, that must land on
//     the four different chunks of their slot group.  Unswizzled they land on two (c for q2 = 0, 3; c ^ 1 for q2 = 1, 2): a 2-way
//     conflict on every read.  With g(q2) = 2 (q2 & 1) the physical chunks are c, c ^ 3, c ^ 1, c ^ 2 for q2 = 0, 1, 2, 3: all
//     four, conflict-free.  (chunk ^ q2, the analogue of the head-64 form, gives c, c, c ^ 3, c ^ 3: still 2-way.)
//   * the transposing read ds_read_b64_tr_b16 is served in two halves of 32 lanes; a half reads, for one d block db, 32 contiguous
//     bytes (chunks 2 db, 2 db + 1) of 8 consecutive key rows key0 + 8 (fq >> 1) + 0..7.  Rows r and r + 4 of those eight sit 256
//     bytes apart -- the same banks unless they read opposite 32-byte halves of their rows, which is exactly what flipping bit 1
//     of the chunk by bit 2 of the row does (bit 0 of a swizzle would only swap two chunks inside the same 32 bytes).  The eight
//     rows then cover all 64 banks once.
//   * the staging writes (ds_write_b128, 8 consecutive lanes per group, 32 banks = 128 bytes) put 8 consecutive items = the four
//     chunks of two neighbouring rows = one whole 128-byte line, whatever permutation the swizzle applies inside each row.
// Packing two keys into one 128-byte row and keeping the head-64 swizzle was the alternative; it needs a second row index
// (key >> 1) and chunk base ((key & 1) * 4) in every address and gives the same bank picture, so the 64-byte row was built.
//
// Geometry (head dim 128).  One key per 256-byte row of sixteen 16-byte chunks = exactly one bank row: unswizzled, chunk c of EVERY
// key sits on slot c.  FOUR v_mfma_f32_16x16x32 steps contract the head (k_frag: chunk 4 kk + fq of key row fr), eight output blocks
// o[8].  The swizzle is  chunk ^ ((row & 7) << 1)  -- the low three bits of the key row pick one of the eight 32-byte chunk pairs.
// By the same bank rules:
//   * the score fragment (ds_read_b128): a group of 16 lanes holds rows {0-3, 12-15} at one chunk c and rows {4-11} at chunk c ^ 1 and
//     needs all sixteen slots.  Unswizzled they land on two: an 8-way conflict on every read.  g(r) = (r & 7) << 1 is even, and over
//     either set of eight rows r & 7 takes every value once ({12-15} give 4-7; {4-11} give 4-7, 0-3): the first set covers the eight
//     slots c ^ {0, 2, .. 14}, the second the eight slots c ^ 1 ^ {0, 2, .. 14} -- together all sixteen, conflict-free.  (chunk ^
//     (row & 15), a plain 4-bit analogue of the head-64 form, also serves this read but fails the next one.)
//   * the transposing read (ds_read_b64_tr_b16): a half of 32 lanes reads the 32 contiguous bytes of chunk pair db of 8 consecutive key
//     rows (an aligned group of eight).  The swizzle never touches bit 0 of the chunk, so the pair stays 32 contiguous bytes, and pair
//     db of row r sits in pair slot db ^ (r & 7): eight different slots = all 64 banks once.
//   * the staging writes (ds_write_b128): 8 consecutive lanes write chunks 0-7 or 8-15 of one row; XOR with one constant maps either
//     set onto one whole 128-byte half of the row, each chunk once.
// LDS budget: K + V of MAXKB key blocks are MAXKB * 8 KB, so the whole-sequence kernel ends at rung 18 (288 keys, 144 KB + the pad
// flags: one workgroup per CU; rung 20 would be the CU's whole 160 KB and is not built) and longer sequences take the tiled kernel
// with 128-key tiles: 2 x 32 KB + 128 flag bytes per workgroup, the tallest even block count that leaves room for two workgroups
// per CU (160-key tiles would be 80 KB + flags each: one too many bytes for two).
//
// Geometry (head dim 16).  One key per 32-byte row of two 16-byte chunks; eight keys share a 256-byte bank row.  The score product
// contracts 16 values: ONE v_mfma_f32_16x16x16 (mfma_op16_k16, pg_common.h), whose lane holds the 4 values d = 4 fq .. 4 fq + 3 of
// row fr -- k_frag is a ds_read_b64 of 8-byte piece fq of key row fr, the Q fragment an 8-byte global load; same output layout as the
// 16x16x32, so st[kb][r] means what it means above.  The alternative was the 16x16x32 with d = 16 .. 31 supplied as zeros in both
// operands (lanes fq >= 2 hold zeros and read nothing): twice the contraction depth per score block for the same result, a 16-byte
// fragment (4 VGPRs, not 2) per key block in the K look-ahead, and a select per fragment to keep the upper lanes off the LDS.  The
// microarchitecture guide gives 16 cycles per 16x16x32 on one SIMD and no figure for the 16x16x16; at worst it costs the same MFMA
// cycles, and it halves the fragment registers and issues one plain b64 read per key block with nothing masked, so it was built.
// (Not timed against each other on the device.)  The context product keeps the 16x16x32 -- its K is the keys -- with ONE output
// block o[1]; the transposing read's four key rows x four 8-byte pieces are exactly four whole rows.
// The swizzle is  chunk ^ ((row >> 3) & 1)  -- bit 3 of the key row swaps the two 16-byte chunks of its row.  By the bank rules:
//   * the score fragment (ds_read_b64, served in two halves of 32 lanes, bank = (address / 4) % 64): lane 16 fq + fr reads piece fq
//     of row fr, so a half (fq = 0, 1 or fq = 2, 3) reads ONE 16-byte chunk c of the block's 16 rows = two bank rows.  Unswizzled,
//     rows r and r + 8 put chunk c on the same four banks: 2-way on every read.  Swapping the chunks of rows 8 - 15 sends them to
//     the other 16 bytes of their 32: the sixteen chunks cover all 64 banks once, conflict-free.
//   * the transposing read (ds_read_b64_tr_b16, two halves of 32 lanes): a half reads all 32 bytes of the 8 consecutive key rows
//     key0 + 8 (fq >> 1) + 0 .. 7 -- one whole aligned bank row, every bank once, whatever happens inside a row.
//   * the staging writes (ds_write_b128, groups of 8 consecutive lanes, bank = (address / 4) % 32): 8 consecutive items = both chunks
//     of four neighbouring rows = one whole aligned 128-byte line, each chunk once, whatever happens inside a row.
// All three conflict-free (tools/lds_bank_model.py evaluates it next to no swizzle and chunk ^ (row & 1)).
// LDS budget: K + V are 64 bytes per key, 36 KB at 576 keys: registers, not the LDS, set the occupancy on every rung.
#pragma once
#include <type_traits>

#include "kernels.h"

PG_OPS_BEGIN

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
// the score product's operand fragment: 8 values of a 32-deep step, or at head dimension 16 the 4 values of the one 16-deep step
template <int HD> struct KFrag { typedef bf16x8 type; };
template <> struct KFrag<16> { typedef bf16x4 type; };
template <int HD> using kfrag_t = typename KFrag<HD>::type;
// score MFMAs per key block
constexpr int score_steps(int hd) { return hd == 16 ? 1 : hd / 32; }
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(2))) float f32x2;
typedef short v4s __attribute__((ext_vector_type(4)));

// ---- host: the key-block ladder.  A kernel template computes MAXKB 16-key blocks (even); the blocks beyond the last key are
// zero-filled and masked -- exact zeros in every sum, so the rung changes the wasted work, never the bits.  `fine`: a rung for
// every even block count; otherwise the coarse rungs, the only ones built for ESM-1's bias-key form.  0: more than 576 keys.
constexpr int kCoarseRungs[] = {2, 4, 8, 12, 18, 24, 30, 36};
constexpr bool coarse_rung(int kb) {
  for (int r : kCoarseRungs)
    if (r == kb) return true;
  return false;
}
// max_keys: the tallest rung's keys -- 576, or 288 at head dimension 128 (attention_max_keys)
constexpr int attention_max_keys(int hd) { return hd == 128 ? 288 : 576; }
inline int attention_rung(int n_keys, bool fine, int max_keys = 576) {
  if (n_keys > max_keys) return 0;
  if (fine) return (((n_keys + 15) / 16) + 1) & ~1;
  for (int r : kCoarseRungs)
    if (n_keys <= r * 16) return r;
  return 0;
}
// The launch switch over the ladder: f(std::integral_constant<int, kb>) for an even rung 2 ... 36, so that a launcher names its
// kernel template once, in a generic lambda, and every rung is instantiated.  false: kb is no rung (more than 576 keys).
template <int KB = 2, class F>
inline bool visit_rung(int kb, F&& f) {
  if constexpr (KB > 36) {
    return false;
  } else {
    if (kb != KB) return visit_rung<KB + 2>(kb, f);
    f(std::integral_constant<int, KB>{});
    return true;
  }
}
// what the full-attention plans (attention.hip, attention_f32.hip) refuse before they look at the shape; empty: nothing
inline std::string attention_head_error(int head_dim, bool has_bias) {
  if (!head_width(head_dim)) return "attention: head dimension " + std::to_string(head_dim) + ": the kernels are built for " + head_widths_text(true);
  if (head_dim != 64 && has_bias) return "attention: the bias_k / bias_v key (ESM-1) is built for heads of 64 only";
  return {};
}

// ---- tiles ----------------------------------------------------------------------------------------------------------------
// byte offset of 16-byte chunk `chunk` inside tile row `row`, and from the start of the tile.  The head-64 permutation is also the
// GEMM tile kernels' 128-byte-row layout (gemm_tile.h), which takes it from here, DMA-source side and fragment side:
#define PG_TILE128_CHUNK(row, chunk) ((chunk) ^ ((row) & 7))
template <int HD = 64>
__device__ __forceinline__ int tile_swz(int row, int chunk) {
  static_assert(HD == 64 || HD == 32 || HD == 128 || HD == 16, "head dimension 64, 32, 128 or 16");
  if constexpr (HD == 128) return (chunk ^ ((row & 7) << 1)) << 4;
  if constexpr (HD == 16) return (chunk ^ ((row >> 3) & 1)) << 4;
  return (HD == 64 ? PG_TILE128_CHUNK(row, chunk) : chunk ^ ((row >> 1) & 2)) << 4;
}
template <int HD = 64>
__device__ __forceinline__ int tile_addr(int row, int chunk) { return row * (HD * 2) + tile_swz<HD>(row, chunk); }

// Staging by NT threads: item i = tid + it*NT is chunk (i & (HD/8 - 1)) of tile row (i >> log2(HD/8)).
// One thread's share of one tile of TPAD rows, for kernels that put other work between a tile's loads and its LDS writes
template <int TPAD, int NT, int HD = 64>
struct TileRegs {
  static constexpr int NIT = (TPAD * (HD / 8) + NT - 1) / NT;
  uint4 r[NIT];
};
template <int TPAD, int NT, int HD>
__device__ __forceinline__ void tile_store(const TileRegs<TPAD, NT, HD>& g, int tid, char* dst) {
  constexpr int CPR = HD / 8, CSH = HD == 128 ? 4 : (HD == 64 ? 3 : (HD == 32 ? 2 : 1));                     // 16-byte chunks per key row, and its log2
#pragma unroll
  for (int it = 0; it < TileRegs<TPAD, NT, HD>::NIT; ++it) {
    const int i = tid + it * NT, row = i >> CSH, c = i & (CPR - 1);
    if (i < TPAD * CPR) *(uint4*)(dst + row * (HD * 2) + tile_swz<HD>(row, c)) = g.r[it];
  }
}
// The K and the V tile of one head together, rows row0 .. row0 + TPAD - 1 of the sequence's n_rows: all global loads of both are
// issued before the first LDS write, so a workgroup pays about one memory round trip, not one per item.  bias_k / bias_v (with
// EXTRA: ESM-1's bias key, HD values each) stand in for row n_rows.
template <int TPAD, int NT, bool EXTRA, int HD = 64>
__device__ __forceinline__ void stage_kv(char* Ks, char* Vs, int tid, const bf16_t* src, size_t ld, int k_off, int v_off, int row0,
                                         int n_rows, const bf16_t* bias_k, const bf16_t* bias_v) {
  constexpr int CPR = HD / 8, CSH = HD == 128 ? 4 : (HD == 64 ? 3 : (HD == 32 ? 2 : 1));                     // 16-byte chunks per key row, and its log2
  constexpr int NIT = (TPAD * CPR + NT - 1) / NT;
  uint4 kreg[NIT], vreg[NIT];
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = tid + it * NT, row = row0 + (i >> CSH), c = i & (CPR - 1);       // row of the sequence
    kreg[it] = make_uint4(0, 0, 0, 0);
    vreg[it] = make_uint4(0, 0, 0, 0);
    if (i < TPAD * CPR && row < n_rows) {
      kreg[it] = *(const uint4*)(src + (size_t)row * ld + k_off + c * 8);
      vreg[it] = *(const uint4*)(src + (size_t)row * ld + v_off + c * 8);
    } else if (EXTRA && row == n_rows) {
      kreg[it] = *(const uint4*)(bias_k + c * 8);
      vreg[it] = *(const uint4*)(bias_v + c * 8);
    }
  }
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = tid + it * NT, row = i >> CSH, c = i & (CPR - 1);
    if (i < TPAD * CPR) {
      *(uint4*)(Ks + row * (HD * 2) + tile_swz<HD>(row, c)) = kreg[it];
      *(uint4*)(Vs + row * (HD * 2) + tile_swz<HD>(row, c)) = vreg[it];
    }
  }
}

// ---- fragments ------------------------------------------------------------------------------------------------------------
// One ds_read_b64, kept one: left to itself hipcc pairs the fragment reads of two key blocks (512 bytes apart) into a
// ds_read2st64_b64, which the LDS serves in 8 cycles where two ds_read_b64 take 4, on 32 banks instead of 64 (the head-16 swizzle is
// derived for 64).  A volatile access through an LDS-qualified pointer is not paired and keeps its immediate offset.
__device__ __forceinline__ bf16x4 lds_read_b64(const char* a) {
  return *(const volatile bf16x4 __attribute__((address_space(3)))*)((__attribute__((address_space(3))) char*)a);
}
// K (MFMA A operand of S^T) or Q (B operand) fragment out of a tile: row krow, d = kk*32 + fq*8 .. +7 (kk < HD / 32); at head
// dimension 16 d = fq*4 .. +3, the 8-byte piece fq & 1 of chunk fq >> 1 (kk = 0)
template <int HD = 64>
__device__ __forceinline__ kfrag_t<HD> k_frag(const char* Ks, int krow, int kk, int fq) {
  if constexpr (HD == 16) return lds_read_b64(Ks + krow * (HD * 2) + tile_swz<HD>(krow, fq >> 1) + (fq & 1) * 8);
  else return *(const bf16x8*)(Ks + krow * (HD * 2) + tile_swz<HD>(krow, kk * 4 + fq));
}
// the same fragment of a query straight from its row of 16-bit values in memory (qrow = the head's first value)
template <int HD = 64>
__device__ __forceinline__ kfrag_t<HD> q_frag(const bf16_t* qrow, int kk, int fq) {
  if constexpr (HD == 16) return *(const bf16x4*)(qrow + fq * 4);
  else return *(const bf16x8*)(qrow + kk * 32 + fq * 8);
}
// one step of the score product: the 32-deep MFMA, or the 16-deep one that is the whole product at head dimension 16
__device__ __forceinline__ f32x4 score_mfma(bf16x8 k, bf16x8 q, f32x4 c) { return mfma_op16(k, q, c); }
__device__ __forceinline__ f32x4 score_mfma(bf16x4 k, bf16x4 q, f32x4 c) { return mfma_op16_k16(k, q, c); }

// V^T fragment (A operand of O^T) for d = db*16 .. +15 and a chunk of 32 keys, straight out of the row-major V tile through
// gfx950's transposing LDS read ds_read_b64_tr_b16 (semantics probed on the device): the 16 lanes of a group point at 4 key
// rows x four 8-byte pieces of 16 d (lane s -> row s>>2, piece s&3) and lane fr receives V[key .. key+3][d = db*16 + fr].
// vt_half reads the half of the 16-key block that starts at key0 (a multiple of 16); a chunk is the halves of blocks 2c, 2c + 1.
union VtFrag { bf16x8 v; uint2 h[2]; };
__device__ __forceinline__ uint2 lds_read_tr16(const char* a) {
  const v4s t = __builtin_amdgcn_ds_read_tr16_b64_v4i16((v4s __attribute__((address_space(3)))*)(
      (__attribute__((address_space(3))) char*)a));
  return __builtin_bit_cast(uint2, t);
}
template <int HD = 64>
__device__ __forceinline__ uint2 vt_half(const char* Vs, int key0, int db, int fr, int fq) {
  const int krow = key0 + fq * 4 + (fr >> 2);
  const int dcol = db * 16 + (fr & 3) * 4;                                     // 16-bit index inside the key row
  return lds_read_tr16(Vs + krow * (HD * 2) + tile_swz<HD>(krow, dcol >> 3) + ((dcol >> 2) & 1) * 8);
}

// P fragment (B operand of O^T) of one 32-key chunk from its two score blocks
__device__ __forceinline__ bf16x8 p_frag(const f32x4& lo, const f32x4& hi) {
  union { bf16x8 v; uint32_t u[4]; } pf;
  pf.u[0] = pack_op2(lo[0], lo[1]);
  pf.u[1] = pack_op2(lo[2], lo[3]);
  pf.u[2] = pack_op2(hi[0], hi[1]);
  pf.u[3] = pack_op2(hi[2], hi[3]);
  return pf.v;
}

// ---- masks and softmax ----------------------------------------------------------------------------------------------------
// keys past the last one, one score block: with tl = (keys of this tile) - fq*4, key kb*16 + fq*4 + r is padding iff
// kb*16 + r >= tl.  The caller loops over the blocks that can hold any (a ladder rung has T > 16*(MAXKB-6)).
__device__ __forceinline__ f32x4 mask_tail(f32x4 s, int kb, int tl) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if (kb * 16 + r >= tl) s[r] = -3.0e38f;
  return s;
}
// the lane's share of a query's row maximum (rows4_max of it = the maximum over all KB*16 keys)
template <int KB>
__device__ __forceinline__ float lane_max(const f32x4 (&st)[KB]) {
  float mx = -3.0e38f;
#pragma unroll
  for (int kb = 0; kb < KB; ++kb)
#pragma unroll
    for (int r = 0; r < 4; ++r) mx = fmaxf(mx, st[kb][r]);      // -> v_max3_f32
  return mx;
}
// <pad> keys of a ragged batch: byte r of f4 is set iff the token of the block's key fq*4 + r is <pad>
__device__ __forceinline__ f32x4 mask_pad(f32x4 s, uint32_t f4, float fill) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
    if ((f4 >> (8 * r)) & 0xffu) s[r] = fill;
  return s;
}
// exact (non-online) softmax over a query's KB*16 keys, mx = its lane_max: st <- exp(st - max), returns 1 / sum -- applied to O
// at the end, the lane's query is also its O column.  exp(s - m) = exp2(s*log2e - m*log2e), two scores per instruction
// (v_pk_fma_f32 / v_pk_add_f32): 284 instead of 418 VALU instructions per 16-query block at 18 key blocks, 72 of them
// quarter-rate v_exp_f32
template <int KB>
__device__ __forceinline__ float softmax_exact(f32x4 (&st)[KB], float mx) {
  mx = rows4_max(mx);
  const f32x2 l2e = {1.44269504088896341f, 1.44269504088896341f};
  const float mneg1 = -mx * 1.44269504088896341f;
  const f32x2 mneg = {mneg1, mneg1};
  f32x2 sum2 = {0.f, 0.f};
#pragma unroll
  for (int kb = 0; kb < KB; ++kb) {
    const f32x2 a = __builtin_elementwise_fma((f32x2){st[kb][0], st[kb][1]}, l2e, mneg);
    const f32x2 b = __builtin_elementwise_fma((f32x2){st[kb][2], st[kb][3]}, l2e, mneg);
    const f32x2 ea = {__builtin_amdgcn_exp2f(a[0]), __builtin_amdgcn_exp2f(a[1])};
    const f32x2 eb = {__builtin_amdgcn_exp2f(b[0]), __builtin_amdgcn_exp2f(b[1])};
    st[kb] = (f32x4){ea[0], ea[1], eb[0], eb[1]};
    sum2 += ea;
    sum2 += eb;
  }
  return 1.0f / rows4_sum(sum2[0] + sum2[1]);
}

// ---- context --------------------------------------------------------------------------------------------------------------
// the lane's NDB x 4 context values (NDB = HD / 16), scaled by inv, as 8-byte pieces: store(db, piece) puts d = db*16 + fq*4 .. +3
template <int NDB, class Store>
__device__ __forceinline__ void store_ctx(const f32x4 (&o)[NDB], float inv, Store&& store) {
#pragma unroll
  for (int db = 0; db < NDB; ++db) {
    uint2 p;
    p.x = pack_op2(o[db][0] * inv, o[db][1] * inv);
    p.y = pack_op2(o[db][2] * inv, o[db][3] * inv);
    store(db, p);
  }
}
// dst = the query's context row at column h*HD + fq*4
template <int NDB>
__device__ __forceinline__ void store_ctx(const f32x4 (&o)[NDB], float inv, bf16_t* dst) {
  store_ctx(o, inv, [&](int db, uint2 p) { *(uint2*)(dst + db * 16) = p; });
}

PG_OPS_END
