// Launchers of the gfx950 kernels (one translation unit per kernel family).
#pragma once
#include "pg_common.h"
#include "head_width.h"

#include "../../include/pgibbs.h"

namespace pg {

// a "sequence" for the attention kernels: sequence s covers token rows
//   (s / inner_count) * outer_rows + (s % inner_count) * inner_rows + t * row_step,  t = 0..T-1
// (defined at global scope and aliased: argument-dependent lookup on a pg:: type would make calls inside pg::opf16 ambiguous
// with the inline default flavour)
}  // namespace pg
// launch_chain_trunk's answer when the persistent grid cannot be co-resident on the device (occupancy): take the per-layer launches
constexpr int kChainTrunkUnfit = -1;
struct PgSeqLayout { int inner_count, outer_rows, inner_rows, row_step; };
// the persistent single-chain trunk (chain_trunk.hip): one layer's weights as device pointers, and the launch's arguments
struct PgChainLayerW {
  const float *ln1_g, *ln1_b;
  const unsigned short* qkv_w; const float* qkv_b;     // [3 d][d] 16-bit operands (q rows pre-scaled), fp32 bias
  const unsigned short* out_w; const float* out_b;
  const float *ln2_g, *ln2_b;
  const unsigned short* fc1_w; const float* fc1_b;
  const unsigned short* fc2_w; const float* fc2_b;
};
struct PgChainTrunkArgs {
  const PgChainLayerW* layers;   // device array [n_layers]
  int n_layers;                  // layers to run, from layers[0]
  int partial_last;              // 1: the last of them stops after its attention (the pruned tail runs on the selected rows elsewhere)
  int B, T;                      // chains x tokens, B * T <= 32 token rows
  float* x;                      // [M][d] fp32 residual stream, in / out
  unsigned short* qkv;           // [M][3 d]
  unsigned short* ctx;           // [M][d]
  unsigned short* ffn;           // [M][4 d]
  float* part;                   // [4][M][d] fp32: fc2's K-split partial products
  unsigned* sync;                // chain_trunk_sync_bytes() of zeroed device memory
  unsigned* err;                 // host-visible word, set to 1 when a device-wide barrier timed out (results are then invalid)
  float eps;
};
namespace pg {
using SeqLayout = ::PgSeqLayout;

enum { EPI_BF16 = 0, EPI_BF16_GELU = 1, EPI_F32_RESID = 2, EPI_F32 = 3, EPI_F32_GELU = 4,
       EPI_F32_PARTIAL = 5 /* internal: split-K partial sums, no bias */,
       EPI_SPLIT3_GELU = 6 /* strict mode fc1: erf-GELU, then the bf16 operand rows [lo | hi | hi] (ldo = 3 N) that fc2 reads; 16-wave kernel only */,
       EPI_SPLIT2_GELU = 7 /* the same rows without the duplicate hi block ([lo | hi | --], same ldo): for an fc2 that runs on the fused
                              three-product kernel, which never reads it (gemm_split3_fused) -- a third less epilogue traffic */ };

// launch_layernorm_bf16's kernels, as layernorm_bf16_choice names them (pg_dbg_layernorm_rows reports the value)
enum { LN_KERNEL_PLAIN = 0, LN_KERNEL_STRIDE = 1, LN_KERNEL_COLMAJOR = 2 };

// ---- the operand-flavoured kernel families (pg_common.h): declared in both namespaces, defined once per flavour ----
inline namespace opbf16 {
#include "kernels_ops.inc"
}
namespace opf16 {
#include "kernels_ops.inc"
}

// ---- flavour-independent launchers (sample.hip) ----
int launch_iter_counter(hipStream_t st, int32_t* d_iter, bool set, int value);
// graph state block (graph_state_bytes() bytes): d_iter[0] = iteration, then the call's sampling parameters -- the kernels of a
// captured iteration read both from the device, so ONE graph serves every iteration of every call of the same shape
size_t graph_state_bytes();
// A draw guide on the device (pg_draw v2): what pg_engine_set_draw_guide uploaded, or a plug-in caller's own
// device tables.  check_draw_guide is the run-time refusal every entry makes before it launches with one.
struct DrawGuideDev {
  const float* bias = nullptr;      // [bias_rows][width][n_valid], -inf = forbidden
  int64_t bias_rows = 0;            // 1 = shared, else the call's token rows
  int width = 0, n_valid = 0;
  const float* temps = nullptr;     // [n_temps]
  int n_temps = 0;
  float top_p = __builtin_nanf(""); // NaN = off
  bool active() const;              // anything set: the launch takes the v2 kernel
};
int check_draw_guide_tables(const pg_draw_guide* g, const char* who);      // what the host tables hold (set time); touches no device
int check_draw_guide(const DrawGuideDev* g, const char* who, int width, int n_valid, int64_t token_rows, int64_t n_iters);
int launch_graph_state(hipStream_t st, int32_t* d_iter, int iteration, const pg_sample_params* p, const DrawGuideDev* guide = nullptr);
int launch_logprob_gather(hipStream_t st, const float* logits, int V, int compact, int width, const int32_t* idx,
                          const int32_t* row_map, const int32_t* targets, int64_t n_sel, int P, float* out,
                          unsigned* nonfinite = nullptr);     // nonfinite: device-visible word set to 1 when a logit row holds NaN / inf
// the table form of the gather: out[n_sel][P][n_cols], entropy[n_sel][P] (may be null); cols[n_cols] is device-resident.
// check_logprob_table_args is the launcher's own host-side refusal, for callers that have work to queue before the launch
int check_logprob_table_args(int V, int n_cols, int norm, int64_t n_sel, int P);
int launch_logprob_table(hipStream_t st, const float* logits, int V, int compact, int width, const int32_t* idx,
                         const int32_t* row_map, const int32_t* cols, int n_cols, int norm, int64_t n_sel, int P, float* out,
                         float* entropy, unsigned* nonfinite = nullptr);
int launch_mask_scatter(hipStream_t st, int32_t* tokens, int width, const int32_t* idx, const int32_t* row_map,
                        int64_t n_sel, int P, int mask_idx, const int32_t* d_iter = nullptr);
int launch_sample_writeback(hipStream_t st, int32_t* tokens, int width, const float* logits, int V, int compact,
                            const int32_t* idx, const int32_t* row_map, int64_t n_sel, int P, const pg_sample_params* p,
                            int iteration, int32_t* sampled_tokens, const int32_t* d_iter = nullptr, unsigned* nonfinite = nullptr,
                            const DrawGuideDev* guide = nullptr);      // guide: null or inactive = pg_draw v1's kernel

// ---- sequence representations (repr.hip): fp32 in and out, one flavour ----
// out[M][d_live] = the live columns of x[M][d], through LayerNorm (ln_row.h: launch_layernorm_f32's bits) when gamma / beta are
// given; a row whose token equals pad_idx is written as zeros (tokens may be null: no such rows).  d_live 0 = d
int launch_repr_rows(hipStream_t s, const float* x, const float* gamma, const float* beta, const int32_t* tokens, int pad_idx, float* out,
                     int64_t M, int d, int d_live, float eps);
// out[n_pools][B][d_live] = the mean of in[b][begin .. begin + count - 1] for (begin, count) = ranges[pool][b] (device-resident, checked
// by repr_pools_check on the host): a sequential fp32 sum in ascending row order divided by float(count); count 0 -> zeros
int launch_repr_pool(hipStream_t s, const float* in, const int32_t* ranges, float* out, int n_pools, int B, int T, int d_live);
int repr_pools_check(const char* who, const int32_t* pools, int n_pools, int B, int T);      // host ranges: 0 <= begin, 0 <= count, begin + count <= T

// ---- contact prediction (contact.hip): fp32, one flavour ----
// One layer folded into the running contact logits: logits[B][T-2][T-2] (+)= sum_h w[h] * APC(P[b][h]) for P[B][H][T][T] (launch_attn_probs),
// the arithmetic contract and its reduction order at the top of contact.hip.  first: the logits start from 0, not from the stored
// values; last: bias is added and, with a contacts buffer, contacts = sigmoid(logits).  sums: scratch of contact_sums_floats floats.
// T >= 3.  w: the H weights of this layer (device)
size_t contact_sums_floats(int B, int H, int T);
int launch_contact_accumulate(hipStream_t s, const float* P, const int32_t* tokens, int eos_idx, int pad_idx, const float* w, float bias,
                              bool first, bool last, float* sums, float* logits, float* contacts, int B, int T, int H);
// The window form: W = T - 1 - tail positions 1 .. T - 1 - tail (tail 1: the form above; tail 0: no trailing position is cut -- the MSA
// Transformer), the tokens of item b at tokens + b * tok_stride (R * C: row 0 of tokens[B][R][C]).  logits / contacts [B][W][W], sums of
// contact_window_sums_floats floats.  The same kernels and arithmetic
size_t contact_window_sums_floats(int B, int H, int T, int tail);
int launch_contact_accumulate_window(hipStream_t s, const float* P, const int32_t* tokens, int eos_idx, int pad_idx, const float* w, float bias,
                                     bool first, bool last, float* sums, float* logits, float* contacts, int B, int T, int H, int tail,
                                     size_t tok_stride);

// ---- MSA Transformer contacts (msa_contact.hip): P[n_rows][C] fp32 dense = softmax over the first C of each S row of ldS floats
// (launch_msa_row_scores[_f32]); one wave per row.  A row with a non-finite score is written as NaN
int launch_row_softmax_probs(hipStream_t s, const float* S, float* P, int64_t n_rows, int C, int ldS);

}  // namespace pg
