// Rotary position embedding (ESM-2): the q and k thirds of a [q | k | v] row buffer rotated in place, one launch per layer between
// the QKV projection and the attention kernel.
//
// fair-esm's RotaryEmbedding, "rotate-half" form, written here for head dimension 64 (heads of 32: below): with ang[t][i] = float(t) * inv_freq[i] (i = 0..31, t = the
// token's index along the sequence axis, padding or not) a head vector u[0..63] of q or k becomes
//   u'[i]      = u[i]      * cos(ang[t][i]) - u[i + 32] * sin(ang[t][i])
//   u'[i + 32] = u[i + 32] * cos(ang[t][i]) + u[i]      * sin(ang[t][i])
// cos / sin come from a host-built table [positions][64] fp32 ([t][0..31] cos, [t][32..63] sin; 256 B per position, L2-resident):
// no trigonometry on the device.  v is not touched.
//
// Arithmetic: the two products and the add / subtract of every output are separately rounded fp32 operations, in every precision
// mode: contraction to FMA is OFF -- the Makefile compiles this file with -ffp-contract=off, as it does sample.hip (under hipcc's
// default the __f*_rn intrinsics are ordinary operators and some of the pairs were fused, others not).  The 16-bit modes widen
// their operands exactly, rotate in fp32 and round once (nearest-even) back to the buffer's type.  A host loop that
// evaluates the formula in fp32 therefore reproduces the strict mode bit for bit and the 16-bit modes up to that one rounding.
//
// Layout rule (elementwise.hip): a pure HBM-bandwidth pass -- one 64-lane wave per token row, 16-byte accesses per lane, nothing
// through LDS, no cross-lane traffic.  q and k are the first 2 d_model columns of a row, i.e. 2 H heads of 64 values side by side.
// A lane owns 16 bytes of a head's low half AND the 16 bytes 32 values higher, so both members of every pair are lane-local:
// 16-bit buffers 8 + 8 values, 4 lanes per head, 8 H lane-slots per row (160 at d = 1280); fp32 buffers 4 + 4 values, 8 lanes per
// head, 16 H lane-slots.  Slot s = lane + 64 * pass: the lane's place inside the head (s mod 4 or 8) is the same in every pass, so
// its cos / sin values are loaded once per row.  A row's loads are all issued before the first rotation.
// Heads of 32 (ESM-2 150M, template parameter HD): pairs (i, i + 16), the same rule with half the head -- 16-bit buffers 8 + 8 values =
// the lane's 16 bytes and the 16 bytes 32 bytes higher, 2 lanes per head, 4 H lane-slots per row (80 at d = 640: two passes); fp32
// buffers 4 + 4 values, 4 lanes per head, 8 H lane-slots (three passes at d = 640); the table row is [16 cos | 16 sin].
// Heads of 128 (ESM-2 15B): pairs (i, i + 64), the same rule with twice the head -- 16-bit buffers 8 + 8 values = the lane's 16 bytes and
// the 16 bytes 128 bytes higher, 8 lanes per head, 16 H lane-slots per row (640 at d = 5120: ten passes); fp32 buffers 4 + 4 values, 16
// lanes per head, 32 H lane-slots (twenty passes at d = 5120, ten in flight at a time); the table row is [64 cos | 64 sin].
// Heads of 16 (ESM-2 8M): pairs (i, i + 8), the same rule with a quarter of the head -- 16-bit buffers 8 + 8 values = the lane's 16
// bytes (the head's whole low half) and the next 16 bytes, ONE lane per head, 2 H lane-slots per row (40 at d = 320: one pass, up to
// 32 heads); fp32 buffers 4 + 4 values, 2 lanes per head, 4 H lane-slots (two passes); the table row is [8 cos | 8 sin].
// Grid: at most one resident round of workgroups (the kernel's occupancy x CUs), every wave walking rows row, row + waves, ... -- a mid-size
// batch has no nearly empty last round (the reason layernorm_bf16_stride_kernel exists), and stores retire behind the next row's
// loads.  Rows >= M (the 256-row padding of the activation buffers) are not touched.
#include "kernels.h"

PG_OPS_BEGIN

__device__ __forceinline__ void rope_pair(float& lo, float& hi, float c, float s) {
  const float a = lo, b = hi;
  lo = __fsub_rn(__fmul_rn(a, c), __fmul_rn(b, s));
  hi = __fadd_rn(__fmul_rn(b, c), __fmul_rn(a, s));
}

// two packed 16-bit values of the low half with their partners of the high half
__device__ __forceinline__ void rope_word16(uint32_t& wl, uint32_t& wh, float c0, float s0, float c1, float s1) {
  float l0 = op16_to_f32((bf16_t)(wl & 0xffff)), l1 = op16_to_f32((bf16_t)(wl >> 16));
  float h0 = op16_to_f32((bf16_t)(wh & 0xffff)), h1 = op16_to_f32((bf16_t)(wh >> 16));
  rope_pair(l0, h0, c0, s0);
  rope_pair(l1, h1, c1, s1);
  wl = pack_op2(l0, l1);
  wh = pack_op2(h0, h1);
}

template <int NP, int HD = 64>
__global__ __launch_bounds__(256) void rope16_kernel(bf16_t* __restrict__ qkv, const float* __restrict__ tab, int M, int T, int H,
                                                    int ld) {
  constexpr int LPH = HD / 16;                                  // lanes per head = uint4 in a head's half
  const int lane = threadIdx.x & 63;
  const int stride = (int)gridDim.x * 4;
  const int slots = 2 * LPH * H;
  const int c = lane & (LPH - 1);                               // values 8 c .. 8 c + 7 of the head's low half
  for (int row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6); row < M; row += stride) {
    const float4* tr = (const float4*)(tab + (size_t)(row % T) * HD);
    uint4* base = (uint4*)(qkv + (size_t)row * ld);             // 2 LPH uint4 per head
    uint4 lo[NP], hi[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int s = lane + 64 * i;
      if (s < slots) {
        const uint4* p = base + (s / LPH) * (2 * LPH) + c;
        lo[i] = p[0];
        hi[i] = p[LPH];
      }
    }
    const float4 ca = tr[2 * c], cb = tr[2 * c + 1], sa = tr[HD / 8 + 2 * c], sb = tr[HD / 8 + 2 * c + 1];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const int s = lane + 64 * i;
      if (s < slots) {
        rope_word16(lo[i].x, hi[i].x, ca.x, sa.x, ca.y, sa.y);
        rope_word16(lo[i].y, hi[i].y, ca.z, sa.z, ca.w, sa.w);
        rope_word16(lo[i].z, hi[i].z, cb.x, sb.x, cb.y, sb.y);
        rope_word16(lo[i].w, hi[i].w, cb.z, sb.z, cb.w, sb.w);
        uint4* p = base + (s / LPH) * (2 * LPH) + c;
        p[0] = lo[i];
        p[LPH] = hi[i];
      }
    }
  }
}

// strict precision mode: the same rotation on an fp32 buffer
template <int NP, int HD = 64>
__global__ __launch_bounds__(256) void rope32_kernel(float* __restrict__ qkv, const float* __restrict__ tab, int M, int T, int H,
                                                    int ld) {
  constexpr int LPH = HD / 8;                                   // lanes per head = float4 in a head's half
  const int lane = threadIdx.x & 63;
  const int stride = (int)gridDim.x * 4;
  const int slots = 2 * LPH * H;
  const int c = lane & (LPH - 1);                               // values 4 c .. 4 c + 3 of the head's low half
  for (int row = (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6); row < M; row += stride) {
    const float4* tr = (const float4*)(tab + (size_t)(row % T) * HD);
    float4* base = (float4*)(qkv + (size_t)row * ld);           // 2 LPH float4 per head
    if constexpr (NP <= 10) {
      float4 lo[NP], hi[NP];
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int s = lane + 64 * i;
        if (s < slots) {
          const float4* p = base + (s / LPH) * (2 * LPH) + c;
          lo[i] = p[0];
          hi[i] = p[LPH];
        }
      }
      const float4 cs = tr[c], sn = tr[LPH + c];
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        const int s = lane + 64 * i;
        if (s < slots) {
          rope_pair(lo[i].x, hi[i].x, cs.x, sn.x);
          rope_pair(lo[i].y, hi[i].y, cs.y, sn.y);
          rope_pair(lo[i].z, hi[i].z, cs.z, sn.z);
          rope_pair(lo[i].w, hi[i].w, cs.w, sn.w);
          float4* p = base + (s / LPH) * (2 * LPH) + c;
          p[0] = lo[i];
          p[LPH] = hi[i];
        }
      }
    } else {
      // 40 heads of 128: twenty passes would be 160 VGPRs of row (256 + AGPR copies as compiled, one wave per SIMD); two groups of ten
      // passes, each loaded whole before its first rotation -- the same per-element arithmetic
      constexpr int G = 10;
      static_assert(NP % G == 0, "whole groups of passes");
      const float4 cs = tr[c], sn = tr[LPH + c];
#pragma unroll
      for (int g = 0; g < NP; g += G) {
        float4 lo[G], hi[G];
#pragma unroll
        for (int i = 0; i < G; ++i) {
          const int s = lane + 64 * (g + i);
          if (s < slots) {
            const float4* p = base + (s / LPH) * (2 * LPH) + c;
            lo[i] = p[0];
            hi[i] = p[LPH];
          }
        }
#pragma unroll
        for (int i = 0; i < G; ++i) {
          const int s = lane + 64 * (g + i);
          if (s < slots) {
            rope_pair(lo[i].x, hi[i].x, cs.x, sn.x);
            rope_pair(lo[i].y, hi[i].y, cs.y, sn.y);
            rope_pair(lo[i].z, hi[i].z, cs.z, sn.z);
            rope_pair(lo[i].w, hi[i].w, cs.w, sn.w);
            float4* p = base + (s / LPH) * (2 * LPH) + c;
            p[0] = lo[i];
            p[LPH] = hi[i];
          }
        }
      }
    }
  }
}

template <typename Kern>
static int rope_occupancy(Kern kern) {
  int v = 0;
  return hipOccupancyMaxActiveBlocksPerMultiprocessor(&v, kern, 256, 0) == hipSuccess && v > 0 ? v : 4;
}

struct RopePlan {
  std::string error;      // not empty: the call is refused (error code 1)
  int hd = 0, passes = 0; // the kernel's <NP, HD>
};
// which instantiation rotates rows of H heads of head_dim: the narrow one up to the width's rope_narrow heads, else the wide one
static RopePlan plan_rope(bool f32, int H, int head_dim) {
  RopePlan p;
  const HeadWidth* w = head_width(head_dim);
  if (!w) p.error = "rope: head dimension " + std::to_string(head_dim) + ": the kernels are built for " + head_widths_text(true);
  else if (H < 1 || H > w->max_heads)
    p.error = "rope: 1.." + std::to_string(w->max_heads) + " heads of " + std::to_string(head_dim) + " (d_model <= " + std::to_string(w->max_heads * head_dim) + ")";
  else p.hd = head_dim, p.passes = rope_passes(head_dim, H <= w->rope_narrow ? w->rope_narrow : w->max_heads, f32);
  return p;
}

// the <NP, HD> kernel of a buffer type
template <int NP, int HD> static auto rope_kernel(bf16_t*) { return rope16_kernel<NP, HD>; }
template <int NP, int HD> static auto rope_kernel(float*) { return rope32_kernel<NP, HD>; }

// the grid = what is resident at once (occupancy of the kernel x CUs), or fewer workgroups when the rows need fewer
template <int NP, int HD, typename Buf>
static void rope_launch(hipStream_t s, Buf* qkv, const float* table, int64_t M, int T, int H, int ld) {
  // asked once per instantiation (function-local static: initialised thread-safely)
  static const int occ = rope_occupancy(rope_kernel<NP, HD>(qkv));
  const int64_t need = (M + 3) / 4, resident = (int64_t)device_cu_count() * occ;
  hipLaunchKernelGGL((rope_kernel<NP, HD>(qkv)), dim3((unsigned)(need < resident ? need : resident)), dim3(256), 0, s, qkv, table, (int)M, T, H, ld);
}

int launch_rope(hipStream_t s, void* qkv, bool f32, const float* table, int table_rows, int64_t M, int T, int H, int ld,
                int head_dim) {
  const RopePlan p = plan_rope(f32, H, head_dim);
  if (!p.error.empty()) return fail(1, p.error);
  if (T < 1 || T > table_rows) return fail(1, "rope: sequence longer than the cos / sin table");
  if (ld < 3 * H * head_dim || ld % (f32 ? 4 : 8)) return fail(1, "rope: rows must hold [q | k | v] and keep 16-byte alignment");
  if (M == 0) return 0;
  if (M > 0x7fffffff - 4 * 8 * 1024) return fail(1, "rope: too many rows");     // 32-bit row arithmetic in the kernels
  // width x {narrow, wide} x {16-bit, fp32}: a width whose narrow row is its widest has no wide form
  visit_head_width(p.hd, [&](auto hd) {
    constexpr int HD = decltype(hd)::value;
    constexpr HeadWidth w = *head_width(HD);
    auto go = [&](auto heads) {
      constexpr int HEADS = decltype(heads)::value;
      if (f32) rope_launch<rope_passes(HD, HEADS, true), HD>(s, (float*)qkv, table, M, T, H, ld);
      else rope_launch<rope_passes(HD, HEADS, false), HD>(s, (bf16_t*)qkv, table, M, T, H, ld);
    };
    if constexpr (w.rope_narrow < w.max_heads)
      if (p.passes > rope_passes(HD, w.rope_narrow, f32)) return go(std::integral_constant<int, w.max_heads>{});
    go(std::integral_constant<int, w.rope_narrow>{});
  });
  PG_HIP(hipGetLastError());
  return 0;
}

PG_OPS_END
