// Launchers of the operand-flavoured translation units; included by kernels.h once per flavour namespace (no include guard).
// out[M][N] (+)= X[M][K] . W[N][K]^T + bias.  M a multiple of 16 up to 256 rows, of 128 beyond; N a multiple of 64; K of 64
// (activation buffers are padded to 256 rows: kernels may touch the padding rows of the last tile).
// ws (optional, fp32 scratch): lets a residual GEMM with few tiles and a deep K (fc2 of a small batch) run as parallel
// K-splits into ws followed by one fixed-order reduction into out -- bit-reproducible, no atomics.
// m_live (optional): the rows of X / out that hold real tokens (M counts the padded rows).  No kernel choice reads it today: every
// tile kernel works on the padded rows
int launch_gemm_bf16(hipStream_t s, const bf16_t* X, const bf16_t* W, const float* bias, void* out, int M, int N, int K,
                     int ldx, int ldw, int ldo, int epi, float* ws = nullptr, size_t ws_bytes = 0, int m_live = 0);
// The K-splits a residual GEMM of depth K runs as when it is given scratch and has few tiles (1: never split), and the scratch that
// form needs for M token rows -- whoever hands `ws` to launch_gemm_bf16 sizes it with this, so that split or unsplit is decided by
// the shape alone, never by how large a buffer happens to be
int gemm_splitk_splits(int K);
size_t gemm_splitk_ws_bytes(int M, int N, int K);
// The micro-benchmark entry (pg_dbg_gemm_bench, tools/).  variant:
//    2        the production dispatch (what launch_gemm_bf16 runs unless PGIBBS_GEMM says otherwise; 3 ... 5 are the same)
//    1        lockstep tiles only: 256^2, 128^2 or 64^2 by divisibility; no weight streaming, no K-splits
//    6 / 7    64^2 / 128^2 lockstep tiles on every row
//    8        192 x 256 ping-pong tiles + tail tiles (residual epilogue)
//    20       the 8-wave ping-pong kernel on all rows, no tail tiles
//    80       the 16-wave kernel on all rows, no tail tiles
//    90       pg_dbg_gemm_bench only (api_dbg.hip): the strict mode's fused three-product kernel
// A variant that names a kernel takes it where the shape allows (6 - 8: divisibility; 20, 80: more than 256 rows, M and N
// multiples of 256) and is the production dispatch without K-splits elsewhere.  Any other variant is an error ("gemm: unknown variant").
int launch_gemm_bf16_variant(hipStream_t s, const bf16_t* X, const bf16_t* W, const float* bias, void* out, int M, int N,
                             int K, int ldx, int ldw, int ldo, int epi, int variant, float* ws = nullptr, size_t ws_bytes = 0,
                             int m_live = 0);

// weight-streaming GEMM with the preceding LayerNorm folded into its operand load (single chains; gemm_bf16.hip):
// out bf16 = LayerNorm(x fp32 [M][K]; gamma, beta) . W^T + bias (+ GELU); M = 16 or 32 rows, K = 256 .. 1280 in steps of 256
bool gemm_ln_skinny_ok(int M, int N, int K);
// nb_force: 16-feature blocks per workgroup, 1 or 2 (2: N a multiple of 32); 0 = PGIBBS_LN_SKINNY_NB, else 2 when N / 16 workgroups
// exceed the CU count
int launch_gemm_ln_skinny(hipStream_t s, const float* X, int ldx, const float* gamma, const float* beta, float eps, const bf16_t* W,
                          const float* bias, void* out, int M, int N, int K, int ldw, int ldo, int epi, int nb_force = 0);
// every layer of a single short chain (<= 32 token rows) as ONE persistent launch with device-wide barriers (chain_trunk.hip);
// bit-identical with the per-layer launches it replaces.  M = padded token rows (16 / 32)
bool chain_trunk_ok(int M, int d_model, int d_ffn, int n_heads);
size_t chain_trunk_sync_bytes();
size_t chain_trunk_part_bytes(int M, int d_model);
int launch_chain_trunk(hipStream_t s, const PgChainTrunkArgs& a, int M, int d_model);
// the big-batch GEMM: whole rounds of 256 x 256 tiles + 64 x 64 tail tiles in one grid (gemm_bf16.hip); M, N multiples of 256
int launch_gemm_big(hipStream_t s, const bf16_t* X, const bf16_t* W, const float* bias, void* out, int M, int N, int K, int ldx,
                    int ldw, int ldo, int epi, int m_live = 0);
// what launch_gemm_bf16_variant would record for a shape (note_kernel's text; "error: ..." for a shape it refuses) on a device of
// n_cu compute units, offered split-K scratch or not -- the dispatch decision alone, no HIP call (pg_dbg_gemm_plan)
void gemm_plan_text(int M, int N, int K, int epi, int variant, bool have_ws, int m_live, int n_cu, std::string* text);
// its split of the rows: m-panels of 256 x 256 tiles (whole rounds of one tile per CU) + rows of 64 x 64 tail tiles
void gemm_big_geometry(int M, int N, int K, int* m_main_panels, int* tail_rows);
// the 16-wave 256x256 tile kernel (gemm_w16.hip): M (may be 0 with tail_rows > 0), N multiples of 256, K a multiple of 64;
// tail_rows rows of 64 x 64 tail tiles from row M on
int launch_gemm_w16(hipStream_t s, const bf16_t* X, const bf16_t* W, const float* bias, void* out, int M, int N, int K, int ldx,
                    int ldw, int ldo, int epi, int tail_rows = 0);
// strict mode: the three split-bf16 products of a projection in one pass (gemm_w16.hip); X3 / W3 in the split operand layout,
// K = logical depth; bit-identical with launch_gemm_bf16 over K' = 3K on the same operands
int launch_gemm_split3(hipStream_t s, const bf16_t* X3, const bf16_t* W3, const float* bias, void* out, int M, int N, int K, int ldo,
                       int epi);      // dispatcher: fused kernel or the plain GEMM over K' = 3K (gemm_bf16.hip)
// its choice for a shape: true = the fused kernel, which reads only the [lo | hi] blocks of the activation rows' groups -- the
// producer of X3 may then leave the duplicate hi block unwritten (launch_layernorm_bf16 split3_dup = false, EPI_SPLIT2_GELU)
bool gemm_split3_fused(int M, int N, int K, int epi);
int launch_gemm_split3_w16(hipStream_t s, const bf16_t* X3, const bf16_t* W3, const float* bias, void* out, int M, int N, int K,
                           int ldo, int epi);

// fused attention, one (sequence, head) per workgroup; qkv rows are [q | k | v] with head h at h*head_dim; head_dim 64, or 32
// (ESM-2 150M; without bias_kv)
// key_tok (optional): the int32 token buffer [n_seq][T]; keys whose token is pad_idx are masked (ragged batches)
// bias_kv (optional, ESM-1's add_bias_kv): [bias_k | bias_v], d_model 16-bit values each -- ONE extra key / value per sequence,
// appended behind the T token keys, never masked
int launch_attention_bf16(hipStream_t s, const bf16_t* qkv, bf16_t* ctx, int B, int T, int H, int ld_qkv, int ld_ctx,
                          int k_off, int v_off, const int32_t* key_tok = nullptr, int pad_idx = -1, const bf16_t* bias_kv = nullptr,
                          int head_dim = 64);
int launch_attention_seq_bf16(hipStream_t s, const bf16_t* qkv, bf16_t* ctx, int64_t n_seq, int T, int H, int ld_qkv,
                              int ld_ctx, int k_off, int v_off, SeqLayout sl, const int32_t* key_tok = nullptr,
                              int pad_idx = -1, const bf16_t* bias_kv = nullptr, int head_dim = 64);
// MSA tied row attention (SURVEY.md A.3): one C x C map per (msa, head) from scores summed over the R rows
// `partial` (optional fp32 scratch of partial_bytes) enables the split-R mode used when B*H is small
// order_bh (0 = B * H): the (msa, head) count the split-R decision is taken on (job-level, so that shards agree);
// msa_row_split_scratch_bytes: the fp32 scratch `partial` must offer for the split form (0 = this shape does not split)
size_t msa_row_split_scratch_bytes(int B, int R, int C, int H, int order_bh);
// What the attention launchers would record for a shape (note_kernel's text: kernel template and grid; "error: ..." for a shape they
// refuse) -- the dispatch decision alone, no HIP call (pg_dbg_attention_plan).  attention_plan_text: launch_attention_seq_bf16 on a
// device of n_cu compute units (row_step: SeqLayout's, 1 = contiguous chains); msa_row_plan_text: launch_msa_row_attention_bf16
// with the scratch of msa_row_split_scratch_bytes on offer; the _f32 pair: the strict launchers (attention_f32.hip)
void attention_plan_text(int64_t n_seq, int T, int H, int head_dim, bool has_pad, bool has_bias, int row_step, int n_cu, std::string* text);
void attention_f32_plan_text(int64_t n_seq, int T, int H, int head_dim, bool has_pad, bool has_bias, std::string* text);
void msa_row_plan_text(int B, int R, int C, int H, int order_bh, std::string* text);
void msa_row_f32_plan_text(int B, int R, int C, int H, std::string* text);
// attention probabilities for contact prediction (contact.hip): P[n_seq][H][T][T] fp32 = softmax over the keys of q . k, from one
// layer's qkv buffer read as that layer's fused attention launch reads it (after the rotary kernel, q pre-scaled; v is not looked at).
// Keys whose token (key_tok, optional) is pad_idx get exactly 0.  Every T: two sweeps over 64-key tiles, no T-dependent branch.
// The _f32 pair is the strict mode's (fp32 qkv, split-bf16 three-product scores; bf16 flavour only).  *_plan_text: note_kernel's text
// for a shape ("error: ..." for one they refuse), no HIP call
int launch_attn_probs(hipStream_t s, const bf16_t* qkv, float* P, int64_t n_seq, int T, int H, int ld_qkv, int k_off, SeqLayout sl,
                      const int32_t* key_tok = nullptr, int pad_idx = -1, int head_dim = 64);
int launch_attn_probs_f32(hipStream_t s, const float* qkv, float* P, int64_t n_seq, int T, int H, int ld_qkv, int k_off, SeqLayout sl,
                          const int32_t* key_tok = nullptr, int pad_idx = -1, int head_dim = 64);
void attn_probs_plan_text(int64_t n_seq, int T, int H, int head_dim, bool has_pad, std::string* text);
void attn_probs_f32_plan_text(int64_t n_seq, int T, int H, int head_dim, bool has_pad, std::string* text);
int launch_msa_row_attention_bf16(hipStream_t s, const bf16_t* qkv, bf16_t* ctx, int B, int R, int C, int H, int ld_qkv,
                                  int ld_ctx, int k_off, int v_off, float scale, float* partial = nullptr,
                                  size_t partial_bytes = 0, int order_bh = 0);

int launch_embed_ln(hipStream_t s, const int32_t* tokens, const float* embed, const float* pos, const float* msa_pos,
                    const float* gamma, const float* beta, float* x, int64_t n_tok, int T, int d, int pad_idx,
                    int mask_idx, int token_dropout, int rows_per_msa, float eps,
                    const float* gamma2 = nullptr, const float* beta2 = nullptr, bf16_t* h2 = nullptr,   // h2: also the first layer's LayerNorm of x
                    float embed_scale = 1.0f,    // gamma == nullptr: no emb_layer_norm_before; embed_scale = sqrt(d) (both: ESM-1);
                                                 // pos == nullptr: no position table either (ESM-2)
                    int d_live = 0);             // the live width of the row launchers, here of h2's LayerNorm (below)
// d_live (0 = d) of the row launchers: the rows are d wide in memory and their first d_live features are the model's own (an embedded
// model, engine.h): statistics, affine and the decoder's dot products run over d_live features -- on them, bit for bit what the same
// kernel gives for rows of d = d_live -- and the pad features of every output row are written as zeros (ln_row.h)
// ESM-2 rotary position embedding (rope.hip): the q and k thirds of qkv[M][ld] (rows [q | k | v], H heads of head_dim each, 64 or 32)
// rotated in place, row r at position r % T; table = [table_rows][head_dim] fp32 ([t][0 .. head_dim/2 - 1] cos, then as many sin, of
// float(t) * inv_freq[i]: rope_table); f32: the buffer is fp32 (strict mode), else the flavour's 16-bit type.  Rows >= M are not touched
int launch_rope(hipStream_t s, void* qkv, bool f32, const float* table, int table_rows, int64_t M, int T, int H, int ld,
                int head_dim = 64);
int launch_layernorm_bf16(hipStream_t s, const float* x, const float* gamma, const float* beta, bf16_t* h, int64_t M,
                          int d, float eps, bool split3 = false,   // split3: h rows are [lo | hi | hi], 3 d wide
                          int colmajor_R = 0, int colmajor_C = 0,  // > 0: token row (b*R + r)*C + c is written as row (b*C + c)*R + r
                          bool split3_dup = true,                  // false: the duplicate hi block is not written (fused consumer)
                          int d_live = 0);                         // no column-major form, never the stride kernel
// its argument refusals alone (0 = fine; no HIP call), and the kernel it picks for M > 0 rows on the current device (LN_KERNEL_*;
// *stride_grid = the stride kernel's workgroup count): one definition for the launcher and for the debug entry that reports it
int layernorm_bf16_check(int64_t M, int d, bool split3, int colmajor_R, int colmajor_C, int d_live = 0);
int layernorm_bf16_choice(int64_t M, int d, int colmajor_R, unsigned* stride_grid, int d_live = 0);
// ESM-MSA-1b column attention fused into its QKV projection (gemm_colattn.hip): X = LayerNorm rows in column-major token order,
// W / bias = the projection's rows grouped per head (launch_headmajor_qkv); ctx rows in ordinary token order.  R in {32,64,128,256}
bool colattn_ok(int R, int d_model, int n_heads);
int launch_gemm_colattn(hipStream_t s, const bf16_t* X, const bf16_t* W, const float* bias, bf16_t* ctx, int B, int R, int C, int H,
                        int d, int ld_ctx);
int launch_headmajor_qkv(hipStream_t s, const bf16_t* w, const float* b, bf16_t* w2, float* b2, int H, int K);
int launch_layernorm_f32(hipStream_t s, const float* x, const float* gamma, const float* beta, float* y, int64_t M, int d,
                         float eps, int d_live = 0);
int launch_gather_ln_bf16(hipStream_t s, const float* x, const int32_t* idx, const int32_t* row_map, int P, int width,
                          const float* gamma, const float* beta, bf16_t* h, int64_t n_sel, int d, float eps,
                          bool split3 = false, int d_live = 0);
// strict precision mode: fp32 [rows][K] -> K-concatenated split-bf16 operand bf16 [rows][3K], [lo | hi | hi] for an
// activation (optionally through erf-GELU), [hi | lo | hi] for a weight; fp32 GELU in place
int launch_split3_bf16(hipStream_t s, const float* src, bf16_t* dst, int64_t rows, int K, float scale, bool gelu, bool weight);
int launch_gelu_f32(hipStream_t s, float* p, int64_t n);
// strict precision mode attention: fp32 qkv in, softmax and accumulation in fp32 (VALU); ctx out as bf16 rows of ld_ctx
// values, or with split_d = d_model as the [lo | hi | hi] operand rows (ld_ctx = 3 d); split_d = -d_model: the same rows without the
// duplicate hi block (for an out-projection on the fused three-product kernel, gemm_split3_fused)
int launch_attention_f32(hipStream_t s, const float* qkv, bf16_t* ctx, int split_d, int64_t n_seq, int T, int H,
                         int ld_qkv, int ld_ctx, int k_off, int v_off, SeqLayout sl, const int32_t* key_tok = nullptr,
                         int pad_idx = -1, const float* bias_kv = nullptr,      // bias_kv: fp32 [bias_k | bias_v] (ESM-1)
                         int head_dim = 64);                                    // 64, or 32 (split kernel only, without bias_kv)
// strict tied row attention; `scores` is an fp32 scratch of B*H*C rows of msa_row_scores_ld(C) floats
static inline int msa_row_scores_ld(int C) { return (C + 3) & ~3; }
// tok (optional): the int32 token buffer [B][R][C] of a batch that holds <pad> (ragged MSA lists): fair-esm's padding semantics
int launch_msa_row_attention_f32(hipStream_t s, const float* qkv, float* scores, bf16_t* ctx, int split_d, int B, int R,
                                 int C, int H, int ld_qkv, int ld_ctx, int k_off, int v_off, float scale,
                                 const int32_t* tok = nullptr, int pad_idx = -1);
// Its first launch alone (msa_row_scores_split_kernel): the scaled fp32 scores S[B*H*C][msa_row_scores_ld(C)] of the strict mode, for
// the contacts tap.  launch_msa_row_scores (msa_contact.hip) writes the same buffer from 16-bit q and k.  *_plan_text: no HIP call
int launch_msa_row_scores_f32(hipStream_t s, const float* qkv, float* scores, int B, int R, int C, int H, int ld_qkv, int k_off, float scale,
                              const int32_t* tok = nullptr, int pad_idx = -1);
int launch_msa_row_scores(hipStream_t s, const bf16_t* qkv, float* scores, int B, int R, int C, int H, int ld_qkv, int k_off, float scale,
                          const int32_t* tok = nullptr, int pad_idx = -1);
void msa_row_scores_plan_text(int B, int R, int C, int H, bool has_pad, std::string* text);
void msa_row_scores_f32_plan_text(int B, int R, int C, int H, bool has_pad, std::string* text);
// d_iter (optional): device-side iteration counter; idx is then the base of a [n_iters][...] table (hipGraph replay)
int launch_gather_rows(hipStream_t s, const void* src, void* dst, const int32_t* idx, const int32_t* row_map, int P, int width,
                       int64_t n_sel, int row_bytes, const int32_t* d_iter = nullptr);
int launch_lm_tail(hipStream_t s, const float* g, const float* gamma, const float* beta, const float* embed,
                   const float* out_bias, float* logits, int64_t n, int d, int V, float eps, int d_live = 0);
bool lm_tail_small(int64_t n, int d);      // launch_lm_tail's choice: the workgroup-per-row kernel (n <= PGIBBS_LM_TAIL_SMALL, 1024, and d <= 2560)
int launch_f32_to_bf16(hipStream_t s, const float* src, bf16_t* dst, int64_t n, float scale);
int launch_bf16_to_f32(hipStream_t s, const bf16_t* src, float* dst, int64_t n);
int launch_scale_f32(hipStream_t s, float* p, int64_t n, float scale);

