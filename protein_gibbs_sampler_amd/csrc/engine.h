// Engine: weights of one masked protein LM resident on one MI355X + the Gibbs hot loop.
#pragma once
#include <map>
#include <string>
#include <vector>

#include "kernels.h"

namespace pg {

// the operand-flavoured launchers (pg_common.h) by the `precision` in scope (an Engine's, the Uploader's, a debug entry's argument):
// fp16 operands in PG_PREC_F16, bf16 otherwise (the strict mode's split operands are bf16 pairs)
#define OPS(fn, ...) (precision == PG_PREC_F16 ? opf16::fn(__VA_ARGS__) : opbf16::fn(__VA_ARGS__))

struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  // grow-only; new storage is zero-filled (pad rows must hold finite values)
  int ensure(size_t need, hipStream_t s);
  void release();
  template <typename T> T* as() const { return (T*)p; }
};

struct Prof {
  struct Rec { int cls; hipEvent_t a, b; std::string kernels; };   // kernels: what the GEMM / attention dispatch noted (pg::note_kernel)
  bool on = false;
  std::vector<Rec> recs;
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  hipEvent_t get();
  void reset();
  void destroy();
};

// PC_GEMM_*: the four per-layer projections of a full-batch forward, timed apart (bench.py's per-kernel roofline); "gemm" = all five.
// PC_NONE: an op inside a timed() block of its caller's (the LM head's one record) -- no record of its own
enum ProfClass { PC_NONE = -1, PC_GEMM = 0, PC_ATTN, PC_LN, PC_EMBED, PC_HEAD, PC_SAMPLE, PC_GEMM_QKV, PC_GEMM_OUT, PC_GEMM_FC1, PC_GEMM_FC2,
                 PC_ROPE /* ESM-2: the rotation of q and k, one launch per layer */,
                 PC_REPR_ROWS, PC_REPR_POOL /* representations: the row copy / LayerNorm and the pooled means (repr.hip) */,
                 PC_ATTN_PROBS, PC_CONTACT /* contact prediction: the attention probabilities and the APC / regression fold (contact.hip) */, PC_COUNT };

struct DenseW {   // y = x W^T + b ; W bf16 [N][K], b fp32 [N].  Strict precision mode: w is [N][3K], each row the
  bf16_t* w = nullptr;   // K-concatenated split-bf16 operand [hi | lo | hi] (hi = bf16(W), lo = bf16(W - hi))
  float* b = nullptr;
  int N = 0, K = 0;
};
struct LnW { float* g = nullptr; float* b = nullptr; };

struct FfnW { LnW ln; DenseW fc1, fc2; };   // x += fc2(gelu(fc1(LayerNorm(x))))

struct EsmLayer {
  LnW ln1;
  DenseW qkv, out;
  FfnW ffn;
  bf16_t* bias_kv16 = nullptr;   // ESM-1 (add_bias_kv): [bias_k | bias_v] as 16-bit operands of the engine's flavour ...
  float* bias_kv32 = nullptr;    // ... and fp32 (strict mode)
};
struct MsaLayer {
  LnW ln_row, ln_col;
  DenseW row_qkv, row_out, col_qkv, col_out;
  FfnW ffn;
  DenseW col_qkv_hm;      // col_qkv with its rows grouped per head ([q_h | k_h | v_h]): operand of the fused column kernel (gemm_colattn.hip)
};

// What a captured Gibbs iteration depends on besides the device-side state block: a graph is replayed only under an equal key
struct GraphKey {
  int32_t mask = 0, mask_idx = 0;                 // baked into the captured launches (the scatter and its argument)
  const void *tok = nullptr, *idx = nullptr;      // the caller's buffers: the graph holds raw pointers
  int64_t B = 0, T = 0, P = 0;
  hipStream_t stream = nullptr;
  uint64_t epoch_pad = 0;                         // 2 x the allocation epoch (a workspace buffer that moved) + <pad> in the batch
  int64_t job_items = 0;                          // picks kernels (sel_gemm_rows, splitk_ws): no replay under another job size
  bool guided = false;                            // which draw kernel was captured (v1 or v2); the guide's tables are in the state block
  bool operator==(const GraphKey& o) const {
    return mask == o.mask && mask_idx == o.mask_idx && tok == o.tok && idx == o.idx && B == o.B && T == o.T && P == o.P &&
           stream == o.stream && epoch_pad == o.epoch_pad && job_items == o.job_items && guided == o.guided;
  }
  void reset() { *this = GraphKey(); }            // equals no call's key (tok == nullptr)
};

// What a representations call (pg_esm_forward_representations) asks of the forward: while Engine::tap points at one, esm_trunk hands
// the residual stream of every listed layer to tap_layer, which stages its compact rows and, with pools, their means
struct ReprTap {
  std::vector<int> layers;           // strictly ascending, each in 0 .. n_layers
  const int32_t* d_tok = nullptr;    // the call's tokens: rows at <pad> are written as zeros
  int B = 0, T = 0;
  const int32_t* d_pools = nullptr;  // [n_pools][B][2] = (begin, count), device-resident
  int n_pools = 0;
  float* rows = nullptr;             // staging [layers.size()][B * T][d_live]
  float* pooled = nullptr;           // [layers.size()][n_pools][B][d_live], or null
  size_t next = 0;                   // index of the next layer to stage
  bool wants_inner(int n_layers) const {      // a layer only the per-layer launches can show
    for (int l : layers)
      if (l >= 1 && l < n_layers) return true;
    return false;
  }
};

// What a contacts call (pg_esm_forward_contacts) asks of the forward: while Engine::ctap points at one, esm_trunk hands every block's
// qkv buffer -- after the rotary kernel, next to the fused attention launch, which does not modify it -- to tap_attention.  The
// probabilities of ONE layer are staged at a time (contact_P: B H T T fp32, so memory does not grow with depth) and folded into the
// contact logits; a layer whose map the caller asked for is written to its slot of attn_out instead and folded from there
// pg_msa_forward_contacts: msa_trunk hands every block's ROW qkv buffer to tap_row_attention, which runs its own scores launch into
// tap-owned staging (contact_S: one layer's B H C rows of scaled fp32 scores) and the softmax over it; T is the column count C, the
// window cuts <cls> only ([B][C-1][C-1]) and the live mask is row 0 of each MSA
struct ContactTap {
  const int32_t* d_tok = nullptr;    // the call's tokens [B][T] ([B][R][T] for the MSA engine)
  int B = 0, T = 0;
  int R = 1;                         // alignment depth (MSA engine)
  bool fold = false;                 // contacts or logits wanted: the engine's head is folded over every layer into `logits`
  float* logits = nullptr;           // [B][T-2][T-2]
  float* contacts = nullptr;         // the same shape, or null
  std::vector<int> attn_layers;      // 0-based block indices, strictly ascending
  float* attn_out = nullptr;         // [attn_layers.size()][B][H][T][T]
  size_t next_attn = 0;              // index of the next requested layer
  int folded = 0;                    // layers seen
};

struct Engine {
  pg_model_config cfg;
  int device = 0;
  int precision = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  bool strict() const { return precision == PG_PREC_FP32; }
  bool esm1() const { return cfg.arch == PG_ARCH_ESM1; }      // ESM-1 differences: see pgibbs.h PG_ARCH_ESM1
  bool esm2() const { return cfg.arch == PG_ARCH_ESM2; }      // ESM-2 differences: see pgibbs.h PG_ARCH_ESM2
  bool esm_family() const { return cfg.arch == PG_ARCH_ESM1B || cfg.arch == PG_ARCH_ESM1 || cfg.arch == PG_ARCH_ESM2; }   // the pg_esm_* entry points

  ~Engine();
  // live_head > 0 (init_embedded): c is the run shape, the tensors are the natural ones of a model with heads of live_head
  int init(const pg_model_config* c, const pg_tensor* tensors, int n_tensors, int device_ordinal, int precision, int live_head = 0);
  // An embedded model: heads of a width no kernel is built for, each in a slot of a built width (head_slot), the other features of
  // the slot structurally zero.  c carries the model's own sizes and the tensors are its natural fair-esm ones; the engine runs the
  // shape d_model = n_heads * head_slot with every tensor scattered into its run-shape image (embedded_image), which computes the
  // same function but in LayerNorm -- the row launchers are given d_live
  int init_embedded(const pg_model_config* c, int head_slot, const pg_tensor* tensors, int n_tensors, int device_ordinal, int precision);

  // ---- weights ----
  std::vector<void*> owned;   // every hipMalloc'd weight block
  float *embed = nullptr, *pos = nullptr, *msa_pos = nullptr, *embed_out = nullptr;
  float embed_scale() const { return cfg.arch == PG_ARCH_ESM1 ? sqrtf((float)cfg.d_model) : 1.0f; }
  LnW ln_before, ln_after, head_ln;
  DenseW head_dense;
  float* head_bias = nullptr;
  std::vector<EsmLayer> esm_layers;
  std::vector<MsaLayer> msa_layers;
  int d_live = 0;             // the model's own features per row: cfg.d_model, less for an embedded model (what the row launchers normalise over)
  bool embedded() const { return d_live != cfg.d_model; }
  int head_dim = 64;          // d_model / n_heads, a width of head_width.h's table -- what every attention and rotation launch of the ESM path is given
  // ESM-2 rotary embedding: cos / sin table [rope_rows][head_dim] fp32 built at init (rope.hip)
  float* rope_tab = nullptr;
  int rope_rows = 0;
  // persistent single-chain trunk (chain_trunk.hip): device table of the layers' weight pointers
  PgChainLayerW* chain_layers = nullptr;

  // ---- workspace (grow-only) ----
  DevBuf x, h, qkv, ctx, ffn, sel_h, sel_g, logits, d_tokens, d_idx, d_samp_tok, d_samp_logits, d_rowmap, scratch;
  DevBuf x_sel, ctx_sel, h_sel, ffn_sel;   // last-layer pruning (compact rows)
  DevBuf tmp_idx, tmp_out;                 // batched generate_single on small MSAs: one template's step table / outputs
  DevBuf splitk;                           // fp32 partial maps of split-K fc2 GEMMs (small batches)
  // strict precision mode (PG_PREC_FP32): h, ctx, ffn, sel_h hold [lo | hi | hi] rows (3x wide); fp32 fc1 output;
  // row-attention scores (also the bf16 mode's wide-alignment fallback)
  DevBuf ffn_f32, scores;
  DevBuf chain_sync, chain_part;           // persistent single-chain trunk: barrier block, fc2 partials
  DevBuf repr_rows, repr_pooled, repr_ranges;   // representations: staged rows of the requested layers, their means, the pool ranges
  int size_activations(int64_t Mp);        // x, h, qkv, ctx, ffn for Mp padded token rows
  float* splitk_ws(int rows, int n, int K, int64_t batch_rows);

  // ---- representations tap ----
  // null (every call but pg_esm_forward_representations): tap_layer is a no-op and the forward issues the launches it always did
  ReprTap* tap = nullptr;
  // x now holds layer l (0: the embedding output; l: the stream after block l): if the tap lists it, stage its rows -- through
  // emb_layer_norm_after for l = n_layers where the architecture has one -- and pool them
  int tap_layer(int l);
  // ---- contacts tap (pg_esm_forward_contacts) ----
  // null (every other call): tap_attention returns at once and the forward issues the launches it always did.  With a tap the call
  // carries no selection and never takes the persistent single-chain launch, which hides the per-layer qkv
  ContactTap* ctap = nullptr;
  int tap_attention(int l, const void* qkv_rows);      // block l's qkv (the engine's 16-bit type; fp32 in strict mode) is ready
  // the MSA trunk's form (pg_msa_forward_contacts): block l's row qkv is ready, right before its row-attention launch.  The maps come
  // from the tap's own scores launch, never from the forward's scratch: they do not depend on the batch or on the split-R decision
  int tap_row_attention(int l, const void* qkv_rows);
  DevBuf contact_S;                                    // one layer's scaled row scores [B*H*C][msa_row_scores_ld(C)]
  // the regression head (pg_engine_set_contact_head): n_layers * n_heads weights on the device (channel l * n_heads + h), null = none
  float* contact_w = nullptr;
  float contact_bias = 0.f;
  int set_contact_head(const float* weight, int n_weights, float bias);
  DevBuf contact_P, contact_sums, contact_logits, contact_probs, contact_attn;   // one layer's maps, a1 / a12, the outputs, the requested maps

  // ---- job-order knobs: what keeps a shard's arithmetic that of the whole job ----
  bool esm_pad_in_batch = false;           // set by the host-token entry points: some token is <pad> -> key-padding mask
  int64_t job_items = 0;                   // pg_engine_set_job_items: batch items of the whole (multi-GPU) job, 0 = this call
  int64_t order_items = 0;                 // > 0: order-changing kernel choices as for a job of this many items (batched generate_single: 1)
  int64_t job_batch(int64_t B) const { return order_items > 0 ? order_items : (job_items > B ? job_items : B); }
  int64_t batch_rows_for(int64_t B, int64_t rows_per_item) const { return job_batch(B) * rows_per_item; }
  int64_t batch_rows = 0;                  // token rows of the JOB's forward (batch_rows_for; set by the trunks)
  int sel_gemm_rows(int64_t n_sel, int64_t Np) const;

  // ---- persistent-trunk recovery ----
  // a host-pinned error word the kernel sets when a device-wide barrier timed out
  unsigned* chain_err = nullptr;
  // after a stream synchronisation: PG_ERR_HIP if chain_err is set.  The kernel is then switched off for the rest of this engine's
  // life (the device is evidently shared with another persistent grid) and chain_retry tells the host-buffer entry points, whose
  // inputs are intact, to run the call again on the per-layer launches
  int chain_check();
  bool chain_disabled = false, chain_retry = false;
  // Device-pointer Gibbs calls (pg_esm_gibbs_run_device) are asynchronous and overwrite the caller's tokens in place, so a barrier
  // timeout is only seen after the damage.  Every such call that may take the persistent launch is therefore logged with a
  // snapshot of its (<= 32) token rows; when a later synchronisation finds the error word set, chain_check() switches the kernel
  // off, restores the first snapshot of every token buffer and runs the logged calls again, in order, on the per-layer launches.
  struct ChainCall {
    int32_t* d_tok; int B, T; const int32_t* d_idx; int n_iters, P; pg_sample_params sp; float* lg; int32_t* st; size_t snap_off;
  };
  std::vector<ChainCall> chain_log;
  bool chain_replay_ok = false;                              // set by chain_check(): the logged calls were run again successfully
  DevBuf chain_snap;
  static constexpr size_t kChainSnapBytes = 128, kChainLogMax = 64;
  bool chain_may_run(int B, int T) const;                    // would a forward of this shape take the persistent launch?
  int chain_log_call(int32_t* d_tok, int B, int T, const int32_t* d_idx, int n_iters, int P, const pg_sample_params* sp, float* lg,
                     int32_t* st);
  // host-pinned word the draw / log-probability kernels set when a logit row is not finite (an fp16 operand that overflowed
  // upstream, or broken weights).  After a stream synchronisation: PG_ERR_RANGE once, the word cleared.
  unsigned* range_err = nullptr;
  int range_check();
  int finish_check() { int rc = chain_check(); return rc ? rc : range_check(); }      // right after a stream synchronisation

  // ---- draw guide (pg_engine_set_draw_guide; pg_draw v2) ----
  // Device copies of the guide's tables: allocations of their own, not DevBufs -- a new guide must not move the allocation epoch a
  // captured iteration is keyed on (its pointers reach the kernel through the state block, not through the graph)
  DrawGuideDev guide;
  float *guide_bias_dev = nullptr, *guide_temps_dev = nullptr;
  int set_draw_guide(const pg_draw_guide* g);
  const DrawGuideDev* draw_guide() const { return guide.active() ? &guide : nullptr; }

  // ---- graph ----
  // launch-bound (small) Gibbs loops: one iteration captured as a hipGraph and replayed; the iteration number lives in
  // d_iter on the device, so the same graph serves every iteration
  DevBuf d_iter;
  hipGraphExec_t graph_exec = nullptr;
  GraphKey graph_key;                                          // of graph_exec
  int64_t stat_graph_captures = 0, stat_graph_replays = 0;     // pg_engine_get_stat

  // ---- strict mode (PG_PREC_FP32) ----
  // out[Mp][N] fp32 (=|+=) X.W^T + b with X = xh + xl, W = wh + wl as ONE bf16 GEMM over K' = 3K:
  // [xl | xh | xh] . [wh | wl | wh]^T = xl.wh + xh.wl + xh.wh  (the dropped xl.wl term is ~2^-17 relative)
  int dense3(const bf16_t* x3, const DenseW& W, float* out, int Mp, bool accumulate);
  int dense3_gelu(const bf16_t* x3, const DenseW& W, int Mp, const DenseW* next = nullptr);   // fc1: ffn (operand rows) = split3(gelu(.)); next = the projection that reads them
  bool dense3_wants_dup(const DenseW& W, int Mp, bool gelu = false) const;   // does this projection read the duplicate hi block of its operand rows?
  // the attention sub-block of a strict layer on x: h = LN(x) -> qkv (fp32) = qkv_w(h) -> ctx = attn(split_d) -> x += out_w(ctx).
  // attn launches the attention (ESM-2: after the rotation) on qkv given ctx's form, split_d = +-d_model (launch_attention_f32):
  // without the duplicate hi block when out_w never reads it
  template <typename Attn> int strict_attention(const LnW& ln, const DenseW& qkv_w, const DenseW& out_w, int Mi, int64_t M, Attn&& attn);
  int ffn_strict(const FfnW& F, int Mi, int64_t M);           // the FFN of a strict layer on x

  // ---- forward ops (all on `stream`, device pointers; each a record of its profiling class) ----
  Prof prof;
  template <typename F> int timed(int cls, F&& f);
  // x = the embedded tokens (+ h = first_ln(x), the first projection's operand rows); rows_per_msa > 0: an alignment batch
  int embed_rows(const int32_t* d_tok, int64_t M, int T, int rows_per_msa, const LnW* first_ln);
  // out[rows][W.N] (+)= a[rows][W.K] W^T + b through the epilogue epi: the flavour's GEMM dispatch with every leading dimension W's
  // own.  m_live: the real token rows among `rows` (0: not said -- launch_gemm_bf16).  splitk: offer the split-K scratch (splitk_ws)
  int dense(int cls, const bf16_t* a, const DenseW& W, void* out, int rows, int epi, int m_live = 0, bool splitk = false);
  // out (16-bit) = LayerNorm(x; ln) W^T + b: the weight-streaming GEMM with the LayerNorm in its operand load (gemm_ln_skinny_ok)
  int dense_ln(const float* x, const LnW& ln, const DenseW& W, bf16_t* out, int rows, int epi);
  // h = LayerNorm(x; ln) on M rows, as operand rows of the projection that reads them: 16-bit, or in strict mode split rows whose
  // duplicate hi block is written only if that projection looks at it (dup = its dense3_wants_dup).  colmajor: launch_layernorm_bf16
  int layer_norm(const float* x, const LnW& ln, bf16_t* h, int64_t M, bool dup = true, int colmajor_R = 0, int colmajor_C = 0);
  // x (+)= a W^T + b as dense(cls, ..., m_live = M_real), then h = LayerNorm(x; ln): residual GEMM + LayerNorm kernel
  int resid_gemm_ln(int cls, const bf16_t* a, const DenseW& W, float* x, int rows, int64_t M_real, const LnW& ln, bf16_t* h,
                    bool splitk = false, int colmajor_R = 0, int colmajor_C = 0);
  // rope() rotates the q and k thirds of a freshly projected qkv buffer (the engine's 16-bit type, fp32 in strict mode) of M token
  // rows, T per sequence.  A no-op for every architecture but ESM-2
  int rope(void* qkv_rows, int64_t M, int T);
  // the end of a 16-bit layer on all Mi token rows (M real), both trunks, from the attention's ctx on.  Tile regime: x += out(ctx);
  // h = LN(x); x += fc2(gelu(fc1(h))); h = next_ln(x) when a layer follows.  folded (single chains): the same with both LayerNorms
  // inside the weight-streaming GEMMs that read them -- fc1 here, the next layer's QKV projection in the trunk -- so h is not written
  int ffn_block(const DenseW& out, const FfnW& F, const LnW* next_ln, int Mi, int64_t M, bool folded = false);
  // finish the last layer on the n_draws selected rows only?  (PGIBBS_PRUNE_LAST=0: never) ... and that tail: the selected rows of
  // x and ctx -> x_sel / ctx_sel, then ffn_block's steps on GEMMs of height Ni.  ln_in_gemm: the trunk folds LayerNorm into the
  // weight-streaming GEMMs (fc1's too when Ni allows)
  bool prune_last(int64_t n_draws, int64_t token_rows) const;
  int pruned_tail(const DenseW& out, const FfnW& F, const int32_t* sel_idx, const int32_t* sel_row_map, int P, int width, int64_t n_sel,
                  const int32_t* d_iter, int Ni, bool ln_in_gemm);
  // every layer of a single short chain in ONE persistent launch, when the shape and this engine's state allow: *ran says how far
  // the forward got.  stop_at_last_attention: the caller finishes the last layer on selected rows (pruned_tail)
  enum ChainRan { CHAIN_NOT_RUN, CHAIN_TO_LAST_ATTENTION, CHAIN_WHOLE_FORWARD };
  int chain_forward(int B, int T, int Mi, bool stop_at_last_attention, ChainRan* ran);
  // tokens -> x (before ln_after).  With a selection (sel_idx != nullptr, bf16 mode) the LAST layer's out-proj, LN2 and
  // FFN run only on the selected rows and x_sel [n_sel][d] holds their residual stream (exact: nothing else reads
  // the last layer's output); head() then reads x_sel (masked_logits).
  int esm_trunk(const int32_t* d_tok, int B, int T, const int32_t* sel_idx, int P, int64_t n_sel, const int32_t* d_iter);
  // tokens[B][R][C] -> x; with a selection the LAST layer's column out-projection and FFN run on the selected rows only
  // (x_sel), as in esm_trunk
  int msa_trunk(const int32_t* d_tok, int B, int R, int C, const int32_t* sel_idx, const int32_t* sel_row_map, int P, int64_t n_sel);
  // the trunk of this engine's architecture on tokens[B][R][C]; R = 1 for the ESM family (d_iter: its captured iteration only)
  int trunk(const int32_t* d_tok, int B, int R, int C, const int32_t* sel_idx = nullptr, const int32_t* sel_row_map = nullptr, int P = 0,
            int64_t n_sel = 0, const int32_t* d_iter = nullptr);
  int head(const int32_t* d_idx, const int32_t* d_row_map, int P, int width, int64_t n_sel, float* d_logits,
           const float* x_src = nullptr);

  // ---- entry points ----
  // Can this engine run a call on tokens[B][R][C]?  Answered from cfg and the call's scalars alone, one message per condition, in this
  // order: the architecture (msa: the call came through a pg_msa_* entry or method; else a pg_esm_* one, R = 1), B >= 0 and R, C >= 1,
  // R within msa_position_embedding, C within the position table, then the call's two counts (P / n_iters, P_max / n_steps,
  // n_sel / P) >= 0 and its two row indices (generate_single's mask_row / target_row) within R.  The one such check: every C entry
  // that takes tokens makes it before anything is allocated or copied, and so do the *_device methods below.
  int check_call(bool msa, int B, int R, int C, int count0 = 0, int count1 = 0, int row0 = 0, int row1 = 0) const;
  // A per-row bias table of the draw guide is indexed by the token row of the WHOLE call: while this lives, a call on a block of its
  // alignments (generate_single batches) that begins at token row row0 reads its own rows of the table
  struct GuideRowShift {
    DrawGuideDev& g;
    const float* bias;
    GuideRowShift(Engine& e, int64_t row0, int C) : g(e.guide), bias(e.guide.bias) {
      if (g.bias && g.bias_rows > 1) g.bias += (size_t)row0 * C * g.n_valid;
    }
    ~GuideRowShift() { g.bias = bias; }
  };
  // One Gibbs iteration up to its logits: mask_idx scattered (if mask) to idx[n_rows][P] of the token rows mask_map, the trunk
  // (pruned when prune_last says so), the LM head at idx[n_rows][P] of the token rows sel_map -> lg[n_rows * P][V].  A null map:
  // row i is token row i.  dit: the device-side iteration counter of a captured iteration (pruned only)
  int masked_logits(int32_t* d_tok, int B, int R, int C, const int32_t* idx, const int32_t* mask_map, const int32_t* sel_map,
                    int64_t n_rows, int P, bool mask, int mask_idx, float* lg, const int32_t* dit = nullptr);
  int esm_gibbs_device(int32_t* d_tok, int B, int T, const int32_t* d_idx, int n_iters, int P, const pg_sample_params* sp,
                       float* d_samp_logits, int32_t* d_samp_tok);
  int msa_gibbs_device(int32_t* d_tok, int B, int R, int C, const int32_t* d_idx, int n_iters, int P,
                       const pg_sample_params* sp, float* d_samp_logits, int32_t* d_samp_tok);
  // generate_single on B templates of equal shape: step s masks row mask_row of every template and samples row target_row of
  // template b at d_step_idx[s][b][P_max] with sp[b]
  int msa_single_device(int32_t* d_tok, int B, int R, int C, int mask_row, int target_row, const int32_t* d_step_idx,
                        const int32_t* step_sample_flag_host, int n_steps, int P_max, const pg_sample_params* sp,
                        float* d_samp_logits, int32_t* d_samp_tok);
};

// Templates [b0, b0 + nb) of a generate_single batch as a call of their own: their rows of a [n_steps][B][row] table (step positions,
// sampled logits, sampled tokens) <-> a contiguous [n_steps][nb][row] block, one copy(block part, table part, values) per step.  The
// copy picks the direction and the memory: memcpy on host tables (api.hip), hipMemcpyAsync on the stream on device ones (engine.hip)
template <typename Tb, typename Tt, typename Copy>
int template_block_rows(Tb* block, Tt* table, int n_steps, int B, int b0, int nb, size_t row, Copy&& copy) {
  for (int s = 0; s < n_steps && row > 0; ++s)
    if (int rc = copy(block + (size_t)s * nb * row, table + ((size_t)s * B + b0) * row, (size_t)nb * row)) return rc;
  return PG_OK;
}

// host side of the ESM-2 rotary embedding: the cos / sin table the rotation kernel reads (engine.hip)
// live > 0: heads of `live` in slots of hd -- the frequencies of a head of `live`, cos 1 and sin 0 in a half's pad columns
std::vector<float> rope_table(int rows, int hd = 64, int live = 0);
// An embedded model's tensors (Engine::init_embedded).  A tensor's role is read from its fair-esm name; *rows x *cols is its natural
// shape (a vector: cols 1) and the result its run-shape image, live values at their run positions and 0.0 everywhere else:
// residual-stream features keep their index, feature j of head h goes to h * slot + j (j < width / 2) or h * slot + j + (slot - width) / 2.
// false: the name is none of an ESM-2 model's tensors
struct EmbedShape { int n_heads, width, slot, d_ffn, vocab; };
bool embedded_image(const std::string& name, const EmbedShape& es, const float* src, int64_t* rows, int64_t* cols, std::vector<float>* image);
// the embedded entry's own refusals, in the order pgibbs.h states (PG_OK: init's checks of the run shape follow)
int embedded_check(const pg_model_config* c, int head_slot);

// state-dict lookup used by init
struct TensorMap {
  std::map<std::string, const pg_tensor*> m;
  const float* get(const std::string& name, int64_t numel, std::string& err) const;
};

}  // namespace pg

struct pg_engine {
  pg::Engine e;
};
