// The parts the GEMM tile kernels have in common, each defined here once (included through gemm_epilogue.h): vector types, the walk
// from a workgroup id to its tile, the two LDS swizzles with their DMA-source and fragment sides next to each other, row-shaped
// buffer access, the operand DMA of the 16-wave family, and the host-side switch from a runtime value to a template argument.
// Address arithmetic is given as macros, not functions: hipcc optimises a __forceinline__ function on its own before it inlines
// it, and as functions these expressions moved the instruction schedule of default-path kernels (gemm_tail_tile64's callers,
// gemm_bf16_w16_kernel: prologue instructions reordered, registers renamed) -- compare the ISA of every user before changing a form.
// For the same reason the two w16 kernels spell out their (plain) 64 x 64 tail prologue and their 4-piece DMA loop, and the ping-pong
// half-step loop stays in gemm_bf16_pp_kernel: as shared functions they renamed the scalar registers of every
// w16 / split3 instance and moved the schedule of every gemm_bf16_pp_kernel instance.
//   kernel                                            tile walk                      operand layout in LDS
//   gemm_bf16_kernel (lockstep; gemm_bf16.hip)        xcd_contiguous                 128-byte rows
//   gemm_bf16_pp_kernel (gemm_bf16.hip)               xcd_contiguous + grouped_tile  half-K (64-byte rows)
//   gemm_bf16_w16_kernel, gemm_split3_w16_kernel      xcd_contiguous + grouped_tile  128-byte rows
//   gemm_colattn_kernel (gemm_colattn.hip)            xcd_contiguous + grouped_tile  128-byte rows
//   gemm_tail_tile64 (gemm_epilogue.h)                tail_tile (8-wave) / caller's  128-byte rows
#pragma once
#include <type_traits>

#include "attn_frag.h"
#include "kernels.h"

PG_OPS_BEGIN

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef unsigned int u32x4_t __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;

#define PG_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
#define PG_GLB_PTR(p) ((const __attribute__((address_space(1))) void*)(p))
// Row-shaped epilogue stores (and the residual rows an epilogue reads) are streamed with the non-temporal policy: a round of tiles
// writes 4 MB per XCD -- its whole L2 -- which otherwise evicts the X / W k-slices the main loops share through it.  Measured at the
// four ESM-1b shapes: QKV 0.589 -> 0.580 ms, fc1 0.859 -> 0.818, out-proj 0.308 -> 0.285, fc2 0.856 -> 0.818; whole iteration
// 96.1 -> 94.1 ms.  (Non-temporal loads / stores in LayerNorm: no effect.)
#define PG_NT_STORE(p, v) __builtin_nontemporal_store(__builtin_bit_cast(u32x4_t, v), (u32x4_t*)(p))
constexpr int kBufNt = 2;                                        // the same policy as the aux argument of a buffer op

// ---- tile walk ------------------------------------------------------------------------------------------------------------
// Workgroup b of a 1-D grid runs on XCD b % 8, and every XCD has an L2 of its own.  xcd_contiguous is the bijection that gives each
// XCD a contiguous range of the n_tiles tile ids; grouped_tile then walks such a range in groups of GM m-panels x all n-tiles, m
// fastest, so that the ~32 tiles an XCD runs at a time form a GM x (32 / GM) rectangle that shares X and W k-slices through its L2.
__device__ __forceinline__ int xcd_contiguous(int bid, int n_tiles) {
  const int xcd = bid & 7, q = n_tiles >> 3, r = n_tiles & 7;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}
template <int GM>
__device__ __forceinline__ void grouped_tile(int bid, int n_tiles, int tiles_n, int& tile_m, int& tile_n) {
  const int tiles_m = n_tiles / tiles_n;
  const int gsz = GM * tiles_n, g = bid / gsz, within = bid - g * gsz;
  const int rows = (tiles_m - g * GM) < GM ? (tiles_m - g * GM) : GM;
  tile_m = g * GM + within % rows;
  tile_n = within / rows;
}
// The 64 x 64 tail tiles of a 256 x 256 grid (gemm_tail_tile64, gemm_epilogue.h) are n_tail extra workgroups, the FIRST of the
// grid.  tail_tile: is this workgroup one, and of which 64-row block rb and 64-column tile tn.  XCD_ROWS (the ping-pong kernel): all
// column tiles of a row block go to one XCD (they share the block's X rows through its L2) whenever the row blocks divide by 8 (tail rows are multiples of 256: at least by 4);
// otherwise, and without XCD_ROWS (the plain mapping the 16-wave kernels spell out themselves, see above), row blocks in grid order.
template <bool XCD_ROWS>
__device__ __forceinline__ bool tail_tile(int n_tail, int tiles_n, int& rb, int& tn) {
  if ((int)blockIdx.x >= n_tail) return false;
  const int tn64 = tiles_n * 4, bt = blockIdx.x, n_rb = n_tail / tn64;
  if (XCD_ROWS && (n_rb & 7) == 0) { const int j = bt >> 3; rb = (j / tn64) * 8 + (bt & 7); tn = j % tn64; }
  else { rb = bt / tn64; tn = bt % tn64; }
  return true;
}

// ---- LDS layouts ----------------------------------------------------------------------------------------------------------
// Operands reach LDS by direct DMA (16 B per lane, no VGPR round trip).  The LDS image of such a wave-instruction is lane-linear,
// so the 16-byte chunks of a row are XOR-swizzled by permuting the per-lane SOURCE address: the chunk a lane fetches is the
// swizzle of the chunk it fills.  The fragment side applies the same function to the chunk it wants; every ds_read_b128 lane
// group then touches 16 distinct 16-byte slots (conflict-free).
//
// 128-byte rows (a K-step of 64 values per row): attn_frag.h's head-64 tile, permutation PG_TILE128_CHUNK (defined there, once).
//   fragment side: chunk kk * 4 + fq of row fr inside a 16-row block of 2 KiB (= tile_addr, spelled as a macro for the schedule);
//   source side: a wave-instruction fills 8 rows = 1 KiB, lane l chunk (l & 7) of row (l >> 3): byte offset of the source chunk
//   from the piece's first row, rows of ld values.
#define PG_ROW128_SRC(lane, ld) ((((lane) >> 3) * (ld) + PG_TILE128_CHUNK((lane) >> 3, (lane) & 7) * 8) * 2)
#define PG_ROW128_FRAG(fr, chunk) ((fr) * 128 + (PG_TILE128_CHUNK(fr, chunk) << 4))

// Half-K layout, 64-byte rows (32 values: one MFMA k-step per row; the ping-pong ring of half-K buffers): four rows share a
// 256-byte bank row, so the chunk is swizzled with pi[(row >> 2) & 3], pi = {0, 3, 2, 1} = (-g) & 3.
//   PG_HALFK_FRAG: the fragment side, byte offset of chunk fq of row fr inside a 16-row piece of 1 KiB;
//   PG_HALFK_SRC_CHUNK: the source side -- a wave-instruction fills 16 rows, lane l chunk (l & 3) of row (l >> 2) -- the source chunk,
//   in units of 8 values.
#define PG_HALFK_FRAG(fr, fq) ((fr) * 64 + (((fq) ^ ((0 - ((fr) >> 2)) & 3)) << 4))
#define PG_HALFK_SRC_CHUNK(lane) (((lane) & 3) ^ ((0 - ((lane) >> 4)) & 3))      /* row = lane >> 2: (row >> 2) = lane >> 4 */

// ---- buffer access --------------------------------------------------------------------------------------------------------
// `bytes` from base on are in range; a load beyond them returns zeros without touching memory
__device__ __forceinline__ rsrc_t buf_rsrc(const void* base, int bytes = 0x7fffffff) { return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, bytes, 0x00020000); }
// Whole output rows as buffer ops: wave-uniform row base in the resource, one VGPR (lane * 16) for all accesses of a wave -- 64-bit
// per-row VGPR addresses would not leave room for 32 rows in flight.
__device__ __forceinline__ rsrc_t row_rsrc(void* base) { return buf_rsrc(base); }
__device__ __forceinline__ f32x4 buf_load_f32x4(rsrc_t rs, int voff, int soff) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, kBufNt));
}
// Stores keep the row step in the VGPR offset: with an SGPR soffset the compiler's hazard recogniser assumes a 128-bit
// store's data registers may be overwritten by the very next VALU instruction, and on gfx950 that corrupted the last
// dword of the stored row (seen as wrong .w components in lanes 12-15 of each 16) -- with soffset = 0 it pads the hazard.
__device__ __forceinline__ void buf_store_f32x4(f32x4 v, rsrc_t rs, int voff, int row_off) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4_t, v), rs, voff + row_off, 0, kBufNt);
}

// ---- operand DMA in 8-row pieces (band_rsrc: gemm_bf16_w16_kernel, gemm_colattn_kernel; dma_pieces: gemm_colattn_kernel) ----
// A wave stages a band of consecutive operand rows in pieces of 8 rows x 128 B (PG_ROW128_SRC).  Buffer form: one lane offset, the
// piece and k offsets in the scalar offset; the resource ends with the band's last row, so a step past the end of K (PG_KSTEP_SOFF)
// reads zeros without touching memory.
__device__ __forceinline__ rsrc_t band_rsrc(const bf16_t* band, int rows, int ld, int row_values) {
  return buf_rsrc(band, ((rows - 1) * ld + row_values) * 2);
}
#define PG_KSTEP_SOFF(t, nk, step_bytes) ((t) < (nk) ? (t) * (step_bytes) : 0x7f000000)
// pieces G0 .. G1 - 1 of the band to dst + 1 KiB per piece; soff = the K-step's byte offset inside a row
template <int G0, int G1>
__device__ __forceinline__ void dma_pieces(rsrc_t rs, char* dst, int voff, int soff, int piece_bytes) {
#pragma unroll
  for (int g = G0; g < G1; ++g)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs, PG_LDS_PTR(dst + g * 1024), 16, voff, soff + g * piece_bytes, 0, 0);
}
// element e of a wave's 4 x 4 accumulators for tile256_epilogue: acc[i][j] is D[n = wn*64 + i*16 + fq*4 + r][m = wm*64 + j*16 + fr]
__device__ __forceinline__ f32x4 w16_elem(const f32x4 (&acc)[4][4], int e, int wm, int wn, int fr, int fq, int& m_loc, int& n_loc) {
  m_loc = wm * 64 + (e & 3) * 16 + fr;
  n_loc = wn * 64 + (e >> 2) * 16 + fq * 4;
  return acc[e >> 2][e & 3];
}

// ---- host: runtime value -> template argument ------------------------------------------------------------------------------
// f(std::integral_constant<int, V>) for the V of the list that equals v, in the manner of visit_rung (attn_frag.h): a launcher
// names its kernel template once, in a generic lambda, and instantiates exactly the listed values.  false: v is not in the list, or
// f itself returned false (a nested visit_int that found nothing) -- so a launcher's nest fails as a whole.
template <int... Vs, class F>
inline bool visit_int(int v, F&& f) {
  auto call = [&](auto c) {
    if constexpr (std::is_void_v<decltype(f(c))>) { f(c); return true; }
    else return (bool)f(c);
  };
  return ((v == Vs ? call(std::integral_constant<int, Vs>{}) : false) || ...);
}

PG_OPS_END
