// Head widths: the one table of what the attention and rotary kernels are built for.  Everything that admits, refuses, scales or
// dispatches by head width reads it -- the engine's configuration check and its folded q scale (engine.hip), the rotary launcher
// (rope.hip), the attention plans (attn_frag.h) and launch switch (attention.hip), the debug entries (api_dbg.hip).  weights.py
// mirrors the rows as HEAD_WIDTHS; tests/test_head_widths_cpu.py holds the two sides together.
#pragma once
#include <string>
#include <type_traits>

namespace pg {

struct HeadWidth {
  int width;
  bool esm2_only;      // false: every architecture
  // heads per row of the rotary kernels: up to rope_narrow the narrow instantiation, up to max_heads the wide one (equal: one form).
  // max_heads is also the engine's cap: max_heads * width features are what the row kernels hold at this width (ln_row.h)
  int rope_narrow, max_heads;
  float q_scale;       // width^-0.5 as fp32, folded into W_q and b_q
  const char* model;   // the released model that needs the row at its widest
};
constexpr HeadWidth kHeadWidths[] = {
    {64, false, 32, 40, 0.125f, "esm2_t36_3B_UR50D"},
    {32, true, 32, 32, 0.17677669529663687f, "esm2_t30_150M_UR50D"},
    {128, true, 20, 40, 0.08838834764831845f, "esm2_t48_15B_UR50D"},
    {16, true, 32, 32, 0.25f, "esm2_t6_8M_UR50D"},
};
constexpr int kNumHeadWidths = sizeof(kHeadWidths) / sizeof(kHeadWidths[0]);

// the row of a width, null when no kernel is built for it
constexpr const HeadWidth* head_width(int hd) {
  for (const HeadWidth& r : kHeadWidths)
    if (r.width == hd) return &r;
  return nullptr;
}

// "64 or 32, 128, 16"; with notes "64 (every architecture) or 32, 128, 16 (ESM-2 only)": what a refusal of another width names
inline std::string head_widths_text(bool notes) {
  std::string any, esm2;
  for (const HeadWidth& r : kHeadWidths) {
    std::string& t = r.esm2_only ? esm2 : any;
    t += (t.empty() ? "" : ", ") + std::to_string(r.width);
  }
  return any + (notes ? " (every architecture) or " : " or ") + esm2 + (notes ? " (ESM-2 only)" : "");
}

// The launch switch over the widths: f(std::integral_constant<int, HD>) for the row of hd, so that a launcher names its kernel
// template once, in a generic lambda, and every width is instantiated (visit_rung of attn_frag.h).  false: hd is not built.
template <int I = 0, class F>
inline bool visit_head_width(int hd, F&& f) {
  if constexpr (I >= kNumHeadWidths) {
    return false;
  } else {
    if (hd != kHeadWidths[I].width) return visit_head_width<I + 1>(hd, f);
    f(std::integral_constant<int, kHeadWidths[I].width>{});
    return true;
  }
}

// Passes per row of the rotary kernels = lane-slots / 64 lanes, rounded up.  A lane owns 16 bytes of a head's low half and their
// partners of the high half: hd / 16 lanes per head of a 16-bit buffer, hd / 8 of an fp32 one, q and k side by side (rope.hip)
constexpr int rope_passes(int hd, int heads, bool f32) { return (2 * (hd / (f32 ? 8 : 16)) * heads + 63) / 64; }
static_assert(rope_passes(64, 32, false) == 4 && rope_passes(64, 40, false) == 5 && rope_passes(64, 32, true) == 8 && rope_passes(64, 40, true) == 10, "heads of 64");
static_assert(rope_passes(32, 32, false) == 2 && rope_passes(32, 32, true) == 4, "heads of 32");
static_assert(rope_passes(128, 20, false) == 5 && rope_passes(128, 40, false) == 10 && rope_passes(128, 20, true) == 10 && rope_passes(128, 40, true) == 20, "heads of 128");
static_assert(rope_passes(16, 32, false) == 1 && rope_passes(16, 32, true) == 2, "heads of 16");

}  // namespace pg
