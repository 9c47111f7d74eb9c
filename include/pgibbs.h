/* pgibbs.h -- C ABI of the MI355X-native Gibbs-sampling engine for masked protein LMs.
 *
 * Plain pointers and sizes only (no torch / C++ types), so any FFI (ctypes, cffi, cgo, JNI ...)
 * can bind it.  Every entry point names the reference interface it replaces; paths are relative
 * to the reference tree (seanrjohnson/protein_gibbs_sampler, `pgen` 0.2.3).
 *
 * Conventions
 *   - every function returning int returns PG_OK (0) or a PG_ERR_* code; pg_last_error() gives the
 *     message of the last failure on the calling thread;
 *   - the caller owns every host buffer; the engine owns its device memory; one engine per device;
 *     calls on one engine are serialized by the caller (the reference is single-threaded too);
 *   - no callbacks; safe to call with the Python GIL released (ctypes default);
 *   - token buffers are int32 row-major; logits are fp32 row-major;
 *   - "*_device" entry points take pointers that are already resident in HBM on the engine's
 *     device and run on the engine's stream (pg_engine_set_stream).
 */
#ifndef PGIBBS_H
#define PGIBBS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Every entry point below is marked PG_API: the shared library exports these symbols and nothing else. */
#ifndef PG_API
#if defined(__GNUC__) || defined(__clang__)
#define PG_API __attribute__((visibility("default")))
#else
#define PG_API
#endif
#endif

#define PG_OK 0
#define PG_ERR_INVALID 1   /* bad argument / shape */
#define PG_ERR_HIP 2       /* HIP runtime failure (message has hipGetErrorString) */
#define PG_ERR_NO_DEVICE 3 /* no MI355X visible -- the product never falls back to a CPU path */
#define PG_ERR_WEIGHTS 4   /* missing / mis-shaped tensor in the state dict */
#define PG_ERR_UNSUPPORTED 5
#define PG_ERR_RANGE 6     /* non-finite logits reached the draw / log-probability / output stage: a 16-bit tensor of the forward left
                              the fp16 range in PG_PREC_F16 (or the weights hold NaN / inf).  Host-buffer entry points report it
                              BEFORE they overwrite the caller's buffers, so the call can be repeated on a PG_PREC_BF16 engine;
                              device-pointer entry points report it at pg_engine_synchronize */

PG_API const char* pg_version(void);
PG_API const char* pg_last_error(void);
/* number of HIP devices visible (0 when there is none or the runtime cannot initialise) */
PG_API int pg_device_count(void);

/* ------------------------------------------------------------------------------------------
 * Host: CPython-exact Mersenne Twister.
 * Replaces the reference's use of the *global* Python RNG on the hot path:
 *   random.sample(indexes, num_positions)   src/pgen/esm_sampler.py:245, esm_msa_sampler.py:277
 *   random.choices(seed_seq, k=batch_size)  src/pgen/esm_sampler.py:112
 *   random.shuffle(positions)               src/pgen/esm_msa_sampler.py:129
 * The Python layer moves random.getstate() in, generates the whole position table natively, and
 * moves the advanced state back with random.setstate(), so position selection is bit-exact and
 * the interpreter's RNG is left exactly where the reference would have left it.
 * ------------------------------------------------------------------------------------------ */
typedef struct pg_pyrandom pg_pyrandom;
PG_API pg_pyrandom* pg_pyrandom_create(void);
PG_API void pg_pyrandom_destroy(pg_pyrandom*);
/* random.seed(int): key = little-endian 32-bit words of abs(n) (at least one word) */
PG_API int pg_pyrandom_seed(pg_pyrandom*, const uint32_t* key_words, int n_words);
PG_API int pg_pyrandom_setstate(pg_pyrandom*, const uint32_t* mt624, int index);
PG_API int pg_pyrandom_getstate(const pg_pyrandom*, uint32_t* mt624, int* index);
PG_API uint32_t pg_pyrandom_getrandbits32(pg_pyrandom*, int k /* 1..32 */);
PG_API double pg_pyrandom_random(pg_pyrandom*);
/* random.sample(population, k): out[k] = chosen population values */
PG_API int pg_pyrandom_sample(pg_pyrandom*, const int32_t* population, int n, int k, int32_t* out);
/* n_rows successive random.sample calls (one per chain / MSA row), out[n_rows][k] */
PG_API int pg_pyrandom_sample_table(pg_pyrandom*, const int32_t* population, int n, int k, int64_t n_rows, int32_t* out);
PG_API int pg_pyrandom_shuffle(pg_pyrandom*, int32_t* x, int n);
/* random.choices(range(n), k=k) (no weights): out[k] = chosen indices */
PG_API int pg_pyrandom_choices(pg_pyrandom*, int n, int k, int32_t* out);

/* ------------------------------------------------------------------------------------------
 * Engine: holds the weights of one masked LM on one MI355X and runs the Gibbs hot path.
 * Replaces the `model.model` attribute of the reference's plug-in object
 * (src/pgen/models.py:59-88; call sites esm_sampler.py:223, esm_msa_sampler.py:136,236) plus the
 * per-position Python loop around it (esm_sampler.py:209-234, esm_msa_sampler.py:128-145,221-248).
 * ------------------------------------------------------------------------------------------ */
typedef struct pg_engine pg_engine;

#define PG_ARCH_ESM1B 1 /* fair-esm ProteinBertModel, "ESM-1b" architecture (ESM-1b, ESM-1v) */
#define PG_ARCH_MSA1B 2 /* fair-esm MSATransformer (esm_msa1b_t12_100M_UR50S) */
#define PG_ARCH_ESM1 3  /* fair-esm ProteinBertModel, "ESM-1" architecture (esm1_t6_43M / t12_85M / t34_670M_UR50S: the models behind
                           pgen.models.ESM6 / ESM12 / ESM34, /root/reference/src/pgen/models.py:69-82): embed_scale sqrt(d), sinusoidal
                           positions (supplied as the `embed_positions.weight` table), no emb_layer_norm_before / after, one extra
                           attention key / value per layer (`layers.i.self_attn.bias_k` / `bias_v`, d_model values each), untied output
                           projection `embed_out.weight` [V][d] + `embed_out.bias` [V], no LM-head dense / LayerNorm, no token
                           dropout; vocabulary of 35 (<cls> = 32, <mask> = 33).  Runs through the ESM-1b entry points. */
#define PG_ARCH_ESM2 4  /* fair-esm ESM2 (esm2_t33_650M_UR50D, esm2_t36_3B_UR50D: any ESM-2 size with heads of 64 and d_model <= 2560 = 40 heads;
                           esm2_t30_150M_UR50D: heads of 32, at most 32 of them = d_model <= 1024, this architecture only;
                           esm2_t48_15B_UR50D: heads of 128, at most 40 of them = d_model <= 5120 (a multiple of 512 above 2560), this
                           architecture only;
                           esm2_t6_8M_UR50D: heads of 16, at most 32 of them = d_model <= 512, this architecture only (d_model 320);
                           pg_engine_create answers PG_ERR_INVALID for any other head width or a wider model;
                           esm2_t12_35M_UR50D, heads of 24, runs through pg_engine_create_embedded below).  The ESM-1b block
                           stack, token dropout, emb_layer_norm_after and tied RoBERTa LM head, with three differences: no position
                           table (`embed_positions.weight` is neither required nor read) -- positions enter through ROTARY embeddings
                           applied to q and k of every attention layer ("rotate-half" pairs (i, i + 32) of each 64-wide head, angle
                           float(t) * 10000^(-2i/64) -- (i, i + 16) and 10000^(-2i/32) for heads of 32, (i, i + 64) and 10000^(-2i/128) for heads of 128, (i, i + 8) and 10000^(-2i/16) for heads of 16 --, t = the token's index along the sequence axis whether or not it is <pad>; one
                           extra launch per layer between the QKV projection and the attention kernel, all three precision modes;
                           the cos / sin table of max_positions + 2 rows is built when the engine is created); no
                           emb_layer_norm_before (not required); vocabulary of 33 as ESM-1b.  Tensors read: `embed_tokens.weight`,
                           `layers.i.*` as ESM-1b, `emb_layer_norm_after.*`, `lm_head.dense.*`, `lm_head.layer_norm.*`, `lm_head.bias`;
                           `layers.i.self_attn.rot_emb.inv_freq` and `contact_head.*` are ignored when handed in (the contact regression
                           is set apart, pg_engine_set_contact_head).  Runs through the
                           pg_esm_* entry points (the pg_msa_* ones answer PG_ERR_INVALID); max_positions bounds T as for ESM-1b
                           (default 1024).  The persistent single-chain trunk is ESM-1b-only: ESM-2 chains of <= 32 token rows take
                           the per-layer launches (weight-streaming GEMMs, hipGraph replay); at d_model > 1280 their LayerNorm is a
                           launch of its own (the LayerNorm-folding GEMM takes K <= 1280). */

#define PG_PREC_BF16 0 /* bf16 MFMA operands, fp32 accumulate, fp32 residual stream (throughput mode) */
#define PG_PREC_F16 2  /* the throughput mode with IEEE fp16 operands instead of bf16 (same kernels, same MFMA rate; 3 more mantissa
                          bits: logit error 8x smaller, profiles/r04_rounding_ablation.txt).  No saturation: a 16-bit tensor of the
                          forward beyond +-65504 becomes inf, the next LayerNorm / softmax turns it into NaN logits, and the call
                          returns PG_ERR_RANGE instead of drawing from them -- use PG_PREC_BF16 for such checkpoints (the Python
                          layer's precision="auto" does that by itself: weights.py / engine.py). */
#define PG_PREC_FP32 1 /* strict parity mode: every matrix product (projections, q.k^T, P.v) as three bf16 MFMA products on
                          (hi, lo) splits of both operands (lo.hi + hi.lo + hi.hi, fp32 accumulate); fp32 softmax, LayerNorm
                          and residual stream; ~3x slower, logits within 1e-3 of the fp32 oracle.  The FFN's GELU is
                          evaluated as relu(x) - |x| 2^p(|x|) with a degree-5 fit p of log2 Phi(-t) (max abs error 3.2e-6,
                          below the split products' own ~2^-17 relative error) when d_ffn is a multiple of 256 -- both
                          models -- and with erff otherwise */

typedef struct {
  int32_t arch;
  int32_t vocab;         /* 33 */
  int32_t d_model;       /* 1280 (ESM-1b) / 768 (MSA-1b); multiple of 128 -- of 64 for PG_ARCH_ESM2 (esm2_t6_8M_UR50D: 320) */
  int32_t n_layers;      /* 33 / 12 */
  int32_t n_heads;       /* d_model / 64: head dim is 64 in every model but ESM-2 150M / 15B / 8M; PG_ARCH_ESM2 also takes d_model / 32 (heads of
                            32, n_heads <= 32), d_model / 128 (heads of 128, n_heads <= 40) and d_model / 16 (heads of 16, n_heads <= 32); the head dim is derived as d_model / n_heads and anything else is PG_ERR_INVALID */
  int32_t d_ffn;         /* 5120 / 3072; multiple of 128 */
  int32_t max_positions; /* learned position table has max_positions + pad_idx + 1 rows (ESM-2: longest T; sizes the rotary table) */
  int32_t pad_idx, mask_idx, cls_idx, eos_idx;
  int32_t token_dropout; /* 1 for ESM-1b, 0 for MSA-1b */
  int32_t max_msa_rows;  /* rows of msa_position_embedding (1024), 0 for ESM-1b */
  float layer_norm_eps;  /* 1e-5 */
} pg_model_config;

/* one fp32 tensor of a fair-esm state dict, by its fair-esm key.
 * The decoder is tied: logits = LN(gelu(dense(x))) . embed_tokens^T + lm_head.bias.  fair-esm zeroes the <mask> row of
 * embed_tokens when it loads an ESM-1b checkpoint (token dropout), and the Python loader (weights.load_fair_esm_checkpoint) does
 * the same -- so after a real ESM-1b checkpoint load logit[<mask>] = lm_head.bias[<mask>] only.  The samplers never draw <mask>
 * (not in valid_idx); log-likelihoods normalise over all V logits including that bias-only term, as fair-esm does.  Tensors
 * handed to pg_engine_create directly are used as given. */
typedef struct {
  const char* name;
  const float* data;
  int64_t numel;
} pg_tensor;

PG_API int pg_engine_create(const pg_model_config* cfg, const pg_tensor* tensors, int n_tensors, int device_ordinal,
                     int precision, pg_engine** out);
/* An EMBEDDED model: a PG_ARCH_ESM2 model whose head width no kernel is built for (esm2_t12_35M_UR50D: d_model 480, 20 heads of 24),
 * run with every head in a slot of a built width, head_slot (32 for heads of 24).  cfg carries the model's OWN sizes (480 / 20 / 1920)
 * and the tensors are its natural fair-esm ones.  The engine runs the shape d_model = n_heads * head_slot (640: the kernels of
 * esm2_t30_150M_UR50D) on zero-padded weights: residual-stream feature c stays column c, columns d_model .. of every row stay 0;
 * feature j of head h goes to column h * head_slot + j for j < width / 2 and to h * head_slot + j + (head_slot - width) / 2 above, so
 * that rotate-half partners stay half a slot apart; q is scaled by float(width^-0.5); the rotary table carries the frequencies of a
 * head of `width` (cos 1, sin 0 in the pad columns).  A zero-padded transformer computes the same function except in LayerNorm, whose
 * kernels normalise over the live features and write zeros behind them.  Refused with PG_ERR_INVALID, in this order: an architecture
 * other than PG_ARCH_ESM2; a slot that is no built head width; a width that is not a multiple of 4 or not smaller than the slot; more
 * heads than the slot's width allows per row; then pg_engine_create's own rules on the run shape.  Every entry point, precision mode and
 * knob works on such an engine as on any other.  pg_engine_create itself keeps refusing such a configuration. */
PG_API int pg_engine_create_embedded(const pg_model_config* cfg, int head_slot, const pg_tensor* tensors, int n_tensors, int device_ordinal,
                              int precision, pg_engine** out);
PG_API void pg_engine_destroy(pg_engine*);
/* run on a caller-provided hipStream_t (NULL = the engine's own stream) */
PG_API int pg_engine_set_stream(pg_engine*, void* hip_stream);
PG_API int pg_engine_synchronize(pg_engine*);
PG_API int pg_engine_device(const pg_engine*);
/* Multi-GPU jobs (contiguous blocks of chains / MSAs per GPU): the number of batch items (chains, MSAs) of the
 * WHOLE job this engine's calls are a shard of; 0 (default) = every call is a whole job.  Kernel choices that change the
 * order of a floating-point sum (K-split GEMMs and the weight-streaming GEMM of the few-chain regime, the row-split form of
 * the tied row attention) are then taken on the job's size instead of the shard's, so that every shard computes bit for bit
 * what a single engine computes on the whole batch (jobs with more than 2048 token rows; smaller jobs run in the few-chain
 * regime whose kernels are picked by the local shape).  No effect on results of a call that is a whole job. */
PG_API int pg_engine_set_job_items(pg_engine*, int64_t job_items);
/* engine counters: "graph_captures" / "graph_replays" = hipGraph captures and replayed iterations of the launch-bound
 * (few-token) Gibbs loop, which replays ONE captured iteration for every call of the same shape (tests assert the path taken) */
PG_API int pg_engine_get_stat(pg_engine*, const char* name, int64_t* value);

/* Sampling parameters == the kwargs of generate() that reach generate_step
 * (src/pgen/esm_sampler.py:8-45, 227-232). */
typedef struct {
  int32_t mask;        /* scatter <mask> at the targets before the forward (esm_sampler.py:220-221) */
  int32_t mask_idx;    /* alphabet.mask_idx */
  int32_t top_k;       /* as passed by the caller; the sample/top_k rule of :32-38 is applied inside */
  int32_t burnin;      /* iterations ii < burnin draw from the full distribution; INT32_MAX = inf */
  float temperature;   /* NaN == None (no division) */
  int32_t n_valid;     /* <= 32 */
  int32_t valid_idx[32]; /* sampler.valid_aa_idx (esm_sampler.py:82, esm_msa_sampler.py:65) */
  uint64_t rng_seed;   /* pg_draw v1 Philox key */
  uint32_t rng_stream; /* Philox counter word 3 */
  uint32_t row_id_base;/* global id of row 0 (Philox counter word 0 = row_id_base + row): results are
                          identical for any sharding of the chains over GPUs */
  int32_t iter_base;   /* Philox counter word 1 = iter_base + iteration */
} pg_sample_params;

/* ---- what the engine entries refuse, and in which order -----------------------------------------
 * The 13 entries below that take tokens (pg_esm_* / pg_msa_*: forward_logits, gibbs_run[_device], gibbs_single[_batch]_run,
 * forward_logprobs, forward_logprob_table) answer PG_ERR_INVALID on the host, before anything is allocated, copied or launched and
 * with the caller's buffers untouched, for the first of these that applies:
 *   1. a null pointer among the required arguments                       "<entry>: null argument"
 *   2. sample parameters: n_valid outside 1..32, a valid_idx outside the vocabulary
 *   3. the call itself, one check for every entry: an engine of the other architecture ("engine was not built for ..."); B < 0,
 *      R < 1, C (T) < 1 ("bad shape"); R > max_msa_rows ("MSA has more rows than msa_position_embedding"); C or T > max_positions
 *      ("alignment / sequence longer than the learned position table") -- the embedding reads one row of those tables per token
 *   4. counts: P, n_iters, n_steps, P_max, n_sel < 0 ("bad shape"); mask_row / target_row outside 0..R-1; the table entries' V,
 *      n_cols, norm and columns
 *   5. nothing to do (B == 0, no iterations or steps, no scored entries): PG_OK, nothing further is looked at
 *   6. the draw guide against the call (pg_engine_set_draw_guide's run-time refusals)
 *   7. index tables on the host: a target position >= the row's width, a scoring target outside the vocabulary, a row_of entry
 *      outside the token rows
 *   8. tokens on the host: the first id outside 0..vocab-1, by entry, flat index and value
 *      ("<entry>: token 33 at flat index 11 is outside the vocabulary of 33")
 * No test of the suite pins another order for any pair.  The *_device entries take device pointers and cannot look into their index
 * table or tokens (7, 8): the caller guarantees 0 <= token < vocab; positions outside the row are skipped by the kernels.
 * pg_msa_gibbs_single_run names itself in 1 and is pg_msa_gibbs_single_batch_run with B = 1 from there on. */

/* ---- ESM-1b -------------------------------------------------------------------------------
 * pg_esm_forward_logits: model.model(tokens)["logits"] (esm_sampler.py:223): tokens[B,T] -> logits[B,T,V].
 * pg_esm_gibbs_run: the whole `for ii in range(num_iters)` loop of ESM_sampler.generate
 *   (esm_sampler.py:209-234) for one batch: per iteration mask scatter -> forward -> restrict /
 *   temperature / top-k / categorical -> write-back, all on the device with no host round trip.
 *   target_idx[n_iters][B][P] are the (1-based token) positions chosen on the host; entries < 0 are
 *   skipped (ragged lists); positions >= T are PG_ERR_INVALID (the *_device variants skip them); bit 30 set = position already written by a later duplicate in the same
 *   row (sampled but not written back: keeps the reference's sequential last-write-wins result).
 *   Optional outputs (NULL to skip): sampled_logits[n_iters][B][P][V], sampled_tokens[n_iters][B][P].
 */
PG_API int pg_esm_forward_logits(pg_engine*, const int32_t* tokens, int B, int T, float* logits_out);
PG_API int pg_esm_gibbs_run(pg_engine*, int32_t* tokens_inout, int B, int T, const int32_t* target_idx, int n_iters, int P,
                     const pg_sample_params* params, float* sampled_logits, int32_t* sampled_tokens);
/* same, every pointer device-resident (tokens stay in HBM; used by bench.py and multi-GPU drivers).  Asynchronous: returns after
 * enqueueing on the engine's stream; every buffer (incl. d_target_idx) must stay valid until pg_engine_synchronize.  The tokens are
 * device-resident, so their range is NOT checked: the caller guarantees 0 <= token < vocab (pg_msa_gibbs_run_device too).  Single short
 * chains (<= 32 token rows) may run on a persistent launch whose device-wide barriers can time out when the GPU is shared; such
 * calls are logged with a snapshot of their token rows, and the next pg_esm_gibbs_run_device / pg_engine_synchronize that sees
 * the timeout restores the rows and runs the logged calls again on the per-layer launches (same results, one warning).
 * Consequence for the caller: between two synchronisations nothing but pg_*_device calls of this engine may write a token buffer
 * that was handed to such a call -- the replay restores the snapshot taken at the first logged call and re-runs only those. */
PG_API int pg_esm_gibbs_run_device(pg_engine*, int32_t* d_tokens_inout, int B, int T, const int32_t* d_target_idx,
                            int n_iters, int P, const pg_sample_params* params, float* d_sampled_logits,
                            int32_t* d_sampled_tokens);

/* ---- sequence representations (embeddings) --------------------------------------------------------
 * fair-esm's model(tokens, repr_layers=[...])["representations"] / scripts/extract.py, HuggingFace's output_hidden_states=True, for
 * the single-sequence engines (PG_ARCH_ESM1B, PG_ARCH_ESM1, PG_ARCH_ESM2, embedded models included).  Layers of an n-layer model are
 * numbered 0 .. n: 0 = the embedding output (after emb_layer_norm_before where there is one and the token-dropout rescale), l = the
 * residual stream after block l, n = the stream after block n through emb_layer_norm_after (PG_ARCH_ESM1: the raw stream, that
 * architecture has no final LayerNorm).  Values are fp32 and d_model wide -- the model's OWN d_model (480 for esm2_t12_35M_UR50D, not
 * the 640 of its run shape); rows at <pad> are zeros.
 *   layers[n_req]            strictly ascending, each in 0 .. n_layers
 *   pools[n_pools][B][2]     (begin, count): token range begin .. begin + count - 1 of sequence b, inside [0, T]; may be NULL / 0
 *   per_token_out            [n_req][B][T][d_model] or NULL
 *   pooled_out               [n_req][n_pools][B][d_model] or NULL: the mean over each range, computed as acc = 0.0f; acc = acc + row[t]
 *                            for t ascending (fp32, round to nearest); acc / float(count); a count of 0 gives zeros
 * PG_ERR_INVALID, before a device is touched and in this order: null tokens or layers; n_req < 1; a negative layer; layers not strictly
 * ascending; both outputs NULL; pooled_out without pools; a range that leaves [0, T]; a negative count; a null engine; an MSA engine;
 * the call check of the other entries (shape, position table); a layer above n_layers; tokens outside the vocabulary.
 * PG_ERR_RANGE when a copied-back value is not finite (PG_PREC_F16 overflow: run the call on a PG_PREC_BF16 engine).
 * A request that names a layer in 1 .. n-1 does not take the persistent single-chain launch; the per-layer launches it takes instead
 * give the same bits. */
PG_API int pg_esm_forward_representations(pg_engine*, const int32_t* tokens, int B, int T, const int32_t* layers, int n_req,
                                          const int32_t* pools, int n_pools, float* per_token_out, float* pooled_out);
/* The two kernels of that entry alone, on host fp32 buffers (kernel-level tests): rows_out[M][d_live] = the live columns of x[M][d],
 * through LayerNorm when gamma / beta [d_live] are given (both or neither), zeros where tokens[M] (optional) equals pad_idx; with
 * pools[n_pools][B][2] (then M = B * T) also pooled_out[n_pools][B][d_live] = the means of those rows as above. */
PG_API int pg_repr_dbg_rows(int device, const float* x, int64_t M, int d, int d_live, const float* gamma, const float* beta, float eps,
                            const int32_t* tokens, int pad_idx, float* rows_out, int B, int T, const int32_t* pools, int n_pools,
                            float* pooled_out);

/* ---- contact prediction --------------------------------------------------------------------------
 * fair-esm's model.predict_contacts(tokens) / return_contacts=True and need_head_weights=True, HuggingFace's predict_contacts and
 * output_attentions=True, for PG_ARCH_ESM1B and PG_ARCH_ESM2 engines (embedded models included: channel l * n_heads + h with the
 * model's own head count).  PG_ARCH_ESM1 (its bias key changes the softmax and the map shape) is refused; the MSA engine has an entry
 * of its own, pg_msa_forward_contacts (below), and is refused by pg_esm_forward_contacts.
 * With A[b][l][h][i][j] = block l's softmax probability of query i over key j (<pad> keys masked, as in the forward):
 *   live[b][t]  = tokens[b][t] != eos_idx && tokens[b][t] != pad_idx; A is zeroed wherever i or j is not live, then the first and the
 *                 last row and column are cut off: the window t = 1 .. T-2 of W = T - 2 positions;
 *   S = A + A^T per channel c = l * n_heads + h;  a1[i] = sum_j S[i][j], a12 = sum_i a1[i];  N[i][j] = S[i][j] - a1[i] * a1[j] / a12;
 *   logit[b][i][j] = bias + sum_c w[c] * N_c[i][j], c ascending;  contact = 1 / (1 + exp(-logit)).
 * All in fp32; the order of every add, the place of the division and the reduction order of the sums are fixed and written down in
 * csrc/contact.hip (tests/_contact_reference.py restates them).  Where this engine's own convention applies:
 *   - a channel with a12 == 0 (no live residue in the window) contributes 0 -- fair-esm divides by zero there and yields NaN;
 *   - a window entry whose row or column is not live (<pad>, or an <eos> before the row's end) gets logit = bias exactly.
 * The attention probabilities come from a kernel of their own (the fused attention kernels never hold them): same operands, same
 * masks, fp32 softmax; deterministic, and a sequence's result does not depend on the other sequences of the call.
 *
 * pg_engine_set_contact_head: weight[n_weights] with n_weights == n_layers * n_heads, uploaded once; weight NULL clears the head.
 * PG_ERR_INVALID: null engine; an ESM-1 engine (the message names the architecture); a wrong count; a non-finite value.  An MSA engine
 * takes a head too: it is the one pg_msa_forward_contacts folds (below).
 *
 * pg_esm_forward_contacts:
 *   contacts_out / logits_out   [B][T-2][T-2] or NULL
 *   attn_layers[n_attn]         0-based block indices, strictly ascending; may be NULL / 0
 *   attn_out                    [n_attn][B][n_heads][T][T] or NULL; given exactly when layers are.  Needs no head: attn_out alone works
 *                               on an engine without one (fair-esm's need_head_weights)
 * PG_ERR_INVALID, before a device is touched and in this order: null tokens; all three outputs NULL; attn_out without layers or layers
 * without attn_out; a negative layer or layers not strictly ascending; T < 3; a null engine; an MSA or ESM-1 engine; contacts or logits
 * wanted with no head set; the call check of the other entries (shape, position table); a layer >= n_layers; tokens outside the
 * vocabulary.  PG_ERR_RANGE when a copied-back value is not finite (PG_PREC_F16 overflow: run the call on a PG_PREC_BF16 engine).
 * The call never takes the persistent single-chain launch; one layer's maps (B * n_heads * T * T fp32) are staged at a time. */
PG_API int pg_engine_set_contact_head(pg_engine*, const float* weight, int n_weights, float bias);
PG_API int pg_esm_forward_contacts(pg_engine*, const int32_t* tokens, int B, int T, float* contacts_out, float* logits_out,
                                   const int32_t* attn_layers, int n_attn, float* attn_out);
/* The two launchers of that entry alone, on host buffers (kernel-level tests).  pg_contact_dbg_probs: probs_out[n_seq][H][T][T] from
 * qkv[n_seq * T][3 * H * head_dim] fp32 (rows [q | k | v], q already scaled), rounded to the 16-bit type of `precision` first or kept
 * fp32 for PG_PREC_FP32; key_tok[n_seq][T] optional: keys whose token is pad_idx are masked; plan / plan_bytes optional: the launcher's
 * plan text -- with probs_out NULL only that, without a device.  pg_contact_dbg_accumulate: one layer's P[B][H][T][T] folded with
 * w[H] into logits_inout[B][T-2][T-2] (started from 0 when `first`, else from the values handed in); `last` adds bias and writes
 * contacts_out (optional). */
PG_API int pg_contact_dbg_probs(int device, int precision, const float* qkv, int n_seq, int T, int H, int head_dim, const int32_t* key_tok,
                                int pad_idx, float* probs_out, char* plan, int plan_bytes);
PG_API int pg_contact_dbg_accumulate(int device, const float* P, const int32_t* tokens, int eos_idx, int pad_idx, const float* w, float bias,
                                     int first, int last, float* logits_inout, float* contacts_out, int B, int T, int H);

/* ---- MSA Transformer contacts (fair-esm's return_contacts=True on esm_msa1b_t12_100M_UR50S) ------------
 * tokens[B][R][C], row 0 the query sequence, column 0 <cls>; the MSA alphabet appends no <eos>.  Per block l and head h the TIED row
 * attention map
 *   S[b][h][i][j] = (64^-0.5 / sqrt(R)) * sum_r sum_d q[b,r,i,h,d] k[b,r,j,h,d],   P = softmax_j S        [B][n_heads][C][C]
 * with the forward's semantics for a batch that holds <pad>: q zeroed at <pad> positions of any row, the scores of key columns that are
 * <pad> in ROW 0 set to -10000 (finite, as in fair-esm), R the padded depth.  The head is the one above with prepend_bos = True,
 * append_eos = False: only the <cls> row and column are cut (window t = 1 .. C-1, W = C - 1), nothing is masked for <eos>, channel
 * c = l * n_heads + h, "live" = row 0's token at that column is not <pad>; same fp32 arithmetic, order and conventions (a12 == 0
 * contributes 0; a not-live row or column gets logit = bias exactly).  Column-attention maps and MSA representations are not offered.
 * The maps come from launches of their own into staging of their own (csrc/msa_contact.hip; one block's S and P at a time): an MSA's
 * result does not depend on the other MSAs of the call nor on how the forward splits its row loop.
 *
 * pg_engine_set_contact_head takes PG_ARCH_MSA1B engines too (n_layers * n_heads weights).
 * pg_msa_forward_contacts:
 *   contacts_out / logits_out   [B][C-1][C-1] or NULL
 *   attn_layers[n_attn]         0-based block indices, strictly ascending; may be NULL / 0
 *   row_attn_out                [B][n_attn][n_heads][C][C] or NULL; given exactly when layers are; needs no head
 * PG_ERR_INVALID, before a device is touched and in this order: null tokens; all three outputs NULL; row_attn_out without layers or
 * layers without row_attn_out; a negative layer or layers not strictly ascending; C < 2; a null engine; an engine that is not MSA-1b;
 * contacts or logits wanted with no head set; the call check of the other MSA entries; a layer >= n_layers; one block's maps beyond
 * 2^31 - 1 values; tokens outside the vocabulary.  What the forward refuses the call refuses with the forward's message
 * (PG_ERR_UNSUPPORTED: PG_PREC_F16 with <pad> or with C > 576).  PG_ERR_RANGE when a copied-back value is not finite.
 *
 * Kernel-level entries: pg_msa_contact_dbg_probs -- probs_out[B][H][C][C] from qkv[B * R * C][3 * H * 64] fp32 (rows [q | k | v]; rounded
 * to the 16-bit type of `precision`, or kept fp32 for PG_PREC_FP32: the strict scores kernel), scores scaled by `scale`, tok[B][R][C]
 * optional (the ragged semantics with pad_idx); plan: the scores launcher's plan text, with probs_out NULL only that, without a device.
 * pg_contact_dbg_accumulate_window -- pg_contact_dbg_accumulate with a window of W = T - 1 - tail positions (tail 0 or 1) and the
 * tokens of item b at tokens + b * tok_stride (>= T); logits_inout / contacts_out [B][W][W]. */
PG_API int pg_msa_forward_contacts(pg_engine*, const int32_t* tokens, int B, int R, int C, float* contacts_out, float* logits_out,
                                   const int32_t* attn_layers, int n_attn, float* row_attn_out);
PG_API int pg_msa_contact_dbg_probs(int device, int precision, const float* qkv, int B, int R, int C, int H, float scale, const int32_t* tok,
                                    int pad_idx, float* probs_out, char* plan, int plan_bytes);
PG_API int pg_contact_dbg_accumulate_window(int device, const float* P, const int32_t* tokens, int eos_idx, int pad_idx, const float* w,
                                            float bias, int first, int last, float* logits_inout, float* contacts_out, int B, int T, int H,
                                            int tail, int64_t tok_stride);

/* ---- ESM-MSA-1b ---------------------------------------------------------------------------
 * tokens[B][R][C] (C = L + 1: <cls> then L columns, no <eos>).
 * pg_msa_gibbs_run: loop of ESM_MSA_sampler.generate (esm_msa_sampler.py:221-248):
 *   target_idx[n_iters][B][R][P].
 * pg_msa_gibbs_single_run: loop of ESM_MSA_sampler.generate_single (esm_msa_sampler.py:128-145), B = 1:
 *   n_steps forwards; step s masks row `mask_row` and samples row `target_row` at
 *   step_idx[s][P_max] (entries < 0 = padding of the shorter partitions); sample flag per step.
 */
PG_API int pg_msa_forward_logits(pg_engine*, const int32_t* tokens, int B, int R, int C, float* logits_out);
PG_API int pg_msa_gibbs_run(pg_engine*, int32_t* tokens_inout, int B, int R, int C, const int32_t* target_idx, int n_iters,
                     int P, const pg_sample_params* params, float* sampled_logits, int32_t* sampled_tokens);
PG_API int pg_msa_gibbs_run_device(pg_engine*, int32_t* d_tokens_inout, int B, int R, int C, const int32_t* d_target_idx,
                            int n_iters, int P, const pg_sample_params* params, float* d_sampled_logits,
                            int32_t* d_sampled_tokens);
PG_API int pg_msa_gibbs_single_run(pg_engine*, int32_t* tokens_inout, int R, int C, int mask_row, int target_row,
                            const int32_t* step_idx, const int32_t* step_sample_flag, int n_steps, int P_max,
                            const pg_sample_params* params, float* sampled_logits, int32_t* sampled_tokens);
/* pg_msa_gibbs_single_batch_run: B calls of generate_single on B MSAs ("templates") of equal shape R x C in ONE pass -- the inner
 *   loop of pgen_msa_revised (src/pgen/pgen_msa_revised.py:107-115: one generate_single per template and per requested sequence;
 *   BASELINE config 5 "batch=32 templates").  tokens[B][R][C]; step_idx[n_steps][B][P_max] (template b's partition of ITS OWN
 *   shuffled positions, < 0 = padding); step_sample_flag[n_steps] (shared: same passes / burn_in); params[B] -- template b draws
 *   with params[b] (the reference draws one torch seed per call), Philox row id = params[b].row_id_base.
 *   sampled_logits[n_steps][B][P_max][V], sampled_tokens[n_steps][B][P_max] optional.
 *   Template b's result is bit-identical with pg_msa_gibbs_single_run on it alone (kernel choices that change a summation order
 *   are taken per template), hence independent of how templates are batched or sharded over GPUs. */
PG_API int pg_msa_gibbs_single_batch_run(pg_engine*, int32_t* tokens_inout, int B, int R, int C, int mask_row, int target_row,
                                  const int32_t* step_idx, const int32_t* step_sample_flag, int n_steps, int P_max,
                                  const pg_sample_params* params, float* sampled_logits, int32_t* sampled_tokens);

/* ---- masked log-likelihood scoring ----------------------------------------------------------------
 * The forward + log_softmax + gather of log_likelihood_batch (src/pgen/esm_sampler.py:336-348,355-362;
 * src/pgen/esm_msa_sampler.py:398-410,421-431).  Sample s scores token row row_of[s] (ESM: the chain index;
 * MSA: b*R + target_index) at positions idx[s][P] (entries < 0 are skipped and yield 0) against targets[s][P];
 * out[s][P] = log_softmax(logits[row, pos, :])[target].  The LM head runs only at the scored rows.
 * pg_*_forward_logprobs writes nothing to `out` when it returns an error (PG_ERR_RANGE included: the results wait on the device
 * until the range check has passed).
 * pg_logprob_gather_device: the same gather on a caller's device-resident full logits[n_rows][width][V]. */
PG_API int pg_esm_forward_logprobs(pg_engine*, const int32_t* tokens, int B, int T, const int32_t* row_of, const int32_t* idx,
                            const int32_t* targets, int n_sel, int P, float* out);
PG_API int pg_msa_forward_logprobs(pg_engine*, const int32_t* tokens, int B, int R, int C, const int32_t* row_of,
                            const int32_t* idx, const int32_t* targets, int n_sel, int P, float* out);
PG_API int pg_logprob_gather_device(void* stream, const float* d_logits, int64_t n_rows, int width, int V, const int32_t* d_idx,
                             const int32_t* d_row_map, const int32_t* d_targets, int64_t n_sel, int P, float* d_out);

/* ---- masked-marginal substitution tables -------------------------------------------------------------
 * The same forward, with the whole row kept instead of one entry of it: for every scored entry (s, p) -- addressed exactly as
 * above: row_of / row_map, idx, entries < 0 skipped -- out[s][p][c] = log-probability of vocabulary token cols[c], c < n_cols, and
 * optionally entropy[s][p] = -sum p log p in nats over the normalisation set.  Skipped entries yield zeros in both.
 * Replaces ESM_MSA_sampler.probs_single as src/pgen/pgen_msa_seq_probs.py:31-45 calls it (the reference class no longer has that
 * method) and the log_softmax of src/pgen/esm_sampler.py:340-345 before its gather.
 *   norm PG_TABLE_NORM_VOCAB    log_softmax over all V logits, then the columns are picked (esm_sampler.py:340-345): the value at
 *                               column c is bit-identical with what pg_*_forward_logprobs / pg_logprob_gather_device return for
 *                               target cols[c] (one device function computes the maximum and the log-sum for both kernels)
 *   norm PG_TABLE_NORM_COLUMNS  log_softmax over the n_cols selected logits only: the distribution generate_step draws from when
 *                               temperature is None and top-k is off (Categorical(logits = valid logits), esm_sampler.py:8-45)
 * V in 1..64, n_cols in 1..V, every column in 0..V-1, counts >= 0: anything else is PG_ERR_INVALID before a device is touched.
 * The engine entries take cols as a HOST pointer and check its contents; pg_logprob_table_device takes a DEVICE pointer whose
 * contents it cannot check -- the caller guarantees 0 <= d_cols[c] < V (a column outside reads as NaN, never out of bounds).
 * pg_esm_forward_logprob_table / pg_msa_forward_logprob_table: the twins of pg_*_forward_logprobs (same checks, same forward, LM head
 * at the scored rows only, PG_ERR_RANGE on non-finite logits before `out` is written).
 * pg_logprob_table_device: the table kernel on a caller's device-resident full logits[n_rows][width][V] (plug-in models). */
#define PG_TABLE_NORM_VOCAB 0
#define PG_TABLE_NORM_COLUMNS 1
PG_API int pg_logprob_table_device(void* stream, const float* d_logits, int64_t n_rows, int width, int V, const int32_t* d_idx,
                            const int32_t* d_row_map, int64_t n_sel, int P, const int32_t* d_cols, int n_cols, int norm,
                            float* d_out /* [n_sel][P][n_cols] */, float* d_entropy /* [n_sel][P] or NULL */);
PG_API int pg_esm_forward_logprob_table(pg_engine*, const int32_t* tokens, int B, int T, const int32_t* row_of, const int32_t* idx,
                                 int n_sel, int P, const int32_t* cols, int n_cols, int norm, float* out, float* entropy_or_null);
PG_API int pg_msa_forward_logprob_table(pg_engine*, const int32_t* tokens, int B, int R, int C, const int32_t* row_of,
                                 const int32_t* idx, int n_sel, int P, const int32_t* cols, int n_cols, int norm, float* out,
                                 float* entropy_or_null);

/* ---- stand-alone data-parallel ends of the iteration --------------------------------------
 * For plug-in models whose forward is not this engine (the reference accepts any object with
 * .model/.alphabet/.batch_converter, esm_sampler.py:54-58): logits come from the caller's model,
 * mask scatter and the draw run here.  All pointers device-resident; `stream` is a hipStream_t.
 *   tokens[n_rows][width] int32; idx[n_sel][P]; row_map[n_sel] (NULL: row r = r) maps a selected row to
 *   its token row; logits[n_rows][width][V] fp32 (full model output).
 * pg_mask_scatter_device  == mask_target_indexes      (esm_sampler.py:259-262, esm_msa_sampler.py:255-264)
 * pg_sample_writeback_device == generate_step + write (esm_sampler.py:225-234)
 */
PG_API int pg_mask_scatter_device(void* stream, int32_t* d_tokens, int64_t n_rows, int width, const int32_t* d_idx,
                           const int32_t* d_row_map, int64_t n_sel, int P, int mask_idx);
PG_API int pg_sample_writeback_device(void* stream, int32_t* d_tokens, int64_t n_rows, int width, const float* d_logits,
                               int V, const int32_t* d_idx, const int32_t* d_row_map, int64_t n_sel, int P,
                               const pg_sample_params* params, int iteration, int32_t* d_sampled_tokens);

/* ---- guided draws: "pg_draw v2" (not in the reference) ------------------------------------------------
 * Three ways to steer the draw, each optional; with none of them every bit is pg_draw v1's.  For one draw at token row `trow`,
 * position `pos`, call-local iteration `it`, over the valid list j = 0 .. n_valid-1:
 *   x_j = logits[valid_idx[j]]                      (the non-finite check applies to these raw logits)
 *   x_j = fl32(x_j + bias[brow][pos][j])            brow = 0 when bias_rows == 1, else trow; -inf = residue j forbidden here
 *   x_j = fl32(x_j / T)                             T = temperatures[it] with a schedule -- pg_sample_params.temperature is then not
 *                                                   read --, else as v1
 *   stable descending rank and k as v1, then k = min(k, number of x_j > -inf): the forbidden entries sort last and are cut
 *   e_r, c_j as v1;  top-p (set, < 1, not in burn-in -- as top_k): q = fl32(top_p c_{k-1}), k' = min(k, 1 + #{j < k : c_j < q})
 *   t = fl32(u c_{k'-1}); the first j < k' with c_j > t, else k' - 1.  Philox counter, key and u are v1's.
 * pg_draw_guide holds HOST pointers: bias fp32 [bias_rows][width][n_valid] indexed by valid-list position (NULL: none; width and
 * n_valid are then not read), temperatures fp32 [n_temperatures] (NULL: none), top_p (NaN = off; 1 = the whole list).
 * pg_engine_set_draw_guide checks the tables, uploads them once and makes every later Gibbs entry of the engine -- pg_esm_gibbs_run[_device],
 * pg_msa_gibbs_run[_device], pg_msa_gibbs_single_run, pg_msa_gibbs_single_batch_run (these two: it = the step number; a per-row table has
 * B * R rows) -- draw v2 until it is set again; NULL, or a guide with nothing set, clears it.  The guide is read when a call's launches
 * run, so it stays set until the calls made under it have been synchronised.  PG_ERR_INVALID at set time, each with its own message, the
 * first five before a device is touched: n_valid outside 1..32 or width / bias_rows < 1 (with a bias), a NaN or +inf bias entry, a (row,
 * position) with no entry > -inf, a temperature that is not finite and > 0, top_p outside (0, 1].  PG_ERR_INVALID at run time, before
 * the call launches anything: bias width != T (or C), bias n_valid != params->n_valid, bias_rows neither 1 nor the call's token rows
 * (B, or B * R), n_temperatures < n_iters (or n_steps).  The device pointers travel in the graph state block: the captured iteration
 * of the few-token ESM loop is replayed across guided calls with different tables (one capture for guided calls, one for unguided). */
typedef struct {
  const float* bias;
  int64_t bias_rows;
  int width;
  int n_valid;
  const float* temperatures;
  int n_temperatures;
  float top_p;
} pg_draw_guide;
PG_API int pg_engine_set_draw_guide(pg_engine*, const pg_draw_guide* guide_or_null);
/* pg_sample_writeback_device with a guide whose tables are DEVICE pointers (plug-in models): d_bias [bias_rows][width][n_valid of params]
 * or NULL, bias_rows 1 or n_rows; d_temperatures [n_temperatures] or NULL, read at `iteration`, which must be < n_temperatures; top_p NaN =
 * off, else in (0, 1].  It cannot check what the tables hold: the caller guarantees bias entries finite or -inf with one > -inf per
 * (row, position), and temperatures finite and > 0 (a cell with nothing allowed yields its first entry; nothing is read out of bounds). */
PG_API int pg_sample_writeback_guided_device(void* stream, int32_t* d_tokens, int64_t n_rows, int width, const float* d_logits, int V,
                                      const int32_t* d_idx, const int32_t* d_row_map, int64_t n_sel, int P,
                                      const pg_sample_params* params, int iteration, int32_t* d_sampled_tokens, const float* d_bias,
                                      int64_t bias_rows, const float* d_temperatures, int n_temperatures, float top_p);

/* ---- multi-GPU tail: the one collective of a sharded job -------------------------------------------
 * Chains / MSAs / templates are independent, so a job shards as contiguous blocks over the GPUs of a node with NO data-path
 * collective; what the reference untokenises at the end of a batch -- the token buffer of ALL chains,
 * src/pgen/esm_sampler.py:236-239, esm_msa_sampler.py:250-253 -- is rebuilt from the shards by one RCCL all-gather over xGMI.
 * One process per GPU, one communicator per process.  librccl.so is opened at run time (PG_ERR_UNSUPPORTED when absent).
 *   pg_comm_unique_id   rank 0 fills id_out[PG_COMM_ID_BYTES] (ncclGetUniqueId) and hands it to the other ranks out of band
 *                       (environment, file, MPI, a torch.distributed store ...)
 *   pg_comm_create      every rank, same id: joins the communicator on `device_ordinal` (ncclCommInitRank; collective)
 *   pg_gather_tokens    d_local[rows][width] int32 of every rank -> d_out[sum(counts)][width] on every rank, rank-major (= chain
 *                       order of contiguous shards).  counts[world] = rows of each rank (NULL: every rank has `rows`); equal
 *                       counts gather straight into d_out, ragged ones through padded blocks.  Runs on `hip_stream` (a
 *                       hipStream_t, NULL = the null stream), asynchronously: synchronise the stream before reading d_out on
 *                       the host.  Order it after the engine's work (pg_engine_synchronize, or pass the engine's stream). */
#define PG_COMM_ID_BYTES 128
typedef struct pg_comm pg_comm;
PG_API int pg_comm_unique_id(void* id_out);
PG_API int pg_comm_create(int rank, int world, const void* unique_id, int device_ordinal, pg_comm** out);
PG_API void pg_comm_destroy(pg_comm*);
PG_API int pg_comm_rank(const pg_comm*);
PG_API int pg_comm_world(const pg_comm*);
PG_API int pg_gather_tokens(pg_comm*, void* hip_stream, const int32_t* d_local, int64_t rows, int width, const int64_t* counts,
                     int32_t* d_out);
/* Rehearsal of pg_gather_tokens without GPUs (tests only): the SAME bookkeeping -- which form, block size, scratch layout, per-rank
 * pack offsets -- on HOST buffers, with the all-gather injected by the caller: allgather(ctx, send, recv, n) must fill recv with
 * the `world` ranks' n int32 values in rank order and return 0.  One call per simulated rank (e.g. one thread each); world sizes
 * 2 ... 8 with ragged and empty shards run in the CPU suite this way (tests/test_gather_rehearsal.py).  pg_dbg_gather_plan reports
 * the plan itself: out7 = {equal form?, nothing to move?, rows of a padded block, bytes per row, bytes per block, scratch bytes,
 * bytes of the gathered output}, out_off_bytes[world] = byte offset of every rank's rows in the output (may be NULL). */
typedef int (*pg_allgather_fn)(void* ctx, const void* send, void* recv, size_t n_int32);
PG_API int pg_dbg_gather_tokens_host(int rank, int world, const int32_t* local, int64_t rows, int width, const int64_t* counts,
                              int force_padded, pg_allgather_fn allgather, void* ctx, int32_t* out);
PG_API int pg_dbg_gather_plan(int rank, int world, int64_t rows, int width, const int64_t* counts, int force_padded, int64_t* out7,
                       int64_t* out_off_bytes);

/* ---- measurement ---------------------------------------------------------------------------
 * HIP-event timing of kernel classes on the engine's stream (bench.py's roofline figure).
 * class names: "gemm", "attention", "layernorm", "embed", "head", "sample", and "rope": ESM-2's rotation of q and k, timed under
 * its own class (not under "attention"; no launch of the other architectures falls into it); "repr_rows" and "repr_pool": the two
 * kernels of pg_esm_forward_representations (no other call has a launch in them); "attn_probs" and "contact": the attention
 * probabilities and the APC / regression fold of pg_esm_forward_contacts and pg_msa_forward_contacts (likewise; for the latter the
 * tied row scores and their softmax are "attn_probs").  */
PG_API int pg_prof_enable(pg_engine*, int on);
PG_API int pg_prof_reset(pg_engine*);
PG_API int pg_prof_get(pg_engine*, const char* kernel_class, double* total_ms, int64_t* launches);
/* the kernels the GEMM dispatch picked for the profiled launches of a class ("gemm_qkv", "gemm_out", "gemm_fc1", "gemm_fc2",
 * "gemm_other", "head"): distinct labels such as "pp192 220t" (220 tiles of 192 x 256) or "tile64 400t x4k" (64 x 64 tiles,
 * 4 K-splits), separated by " | ", into buf. */
PG_API int pg_prof_get_kernels(pg_engine*, const char* kernel_class, char* buf, int buf_bytes);

/* ---- kernel-level debug entry points (parity tests call individual kernels through these) --- */
/* out[M][N] = x[M][K] @ w[N][K]^T + bias (fp32 host buffers; computed in `precision`); epi: 0 none, 1 gelu,
 * 2 residual (out is read too: out += x w^T + bias), 3 bf16 output, 4 bf16 output + gelu.  PG_PREC_FP32 (the engine's
 * strict-mode projection: one GEMM over K-concatenated split-bf16 operands) takes epi 0, 2 and 5 = fc1's fused epilogue
 * (GELU, then the split operand rows fc2 reads; N a multiple of 256; out = hi + lo of those rows); PG_PREC_F16 = the bf16
 * path's kernels with fp16 operands (epi 0-4) */
PG_API int pg_dbg_gemm(int device, int precision, const float* x, const float* w, const float* bias, float* out, int M, int N,
                int K, int epi);
/* pg_dbg_gemm with the kernel named and reported (pg_dbg_gemm is this with variant -1, have_ws -1, m_live M, no plan).
 * variant: -1 = the process's dispatch (launch_gemm_bf16, PGIBBS_GEMM), else one of the variants of pg_dbg_gemm_bench that compute a
 * whole result -- 1 lockstep tiles, 2 production dispatch, 6 / 7 64^2 / 128^2 tiles, 8 192 x 256 tiles + tail tiles (residual), 20 the
 * 8-wave ping-pong kernel, 80 the 16-wave kernel; every other value, the ablation ids included, is PG_ERR_INVALID.  PG_PREC_FP32 takes
 * variant -1 only (PG_ERR_UNSUPPORTED otherwise).  have_ws: 0 = no split-K scratch, 1 = scratch on offer whatever the epilogue (the
 * dispatch takes it for the residual epilogue only), -1 = on offer to the residual epilogue.  m_live: rows that hold tokens, 0 = all.
 * plan (NULL: not wanted): the text the GEMM launch alone recorded, as pg_dbg_gemm_plan words it; the strict mode's fused kernel
 * records "gemm_split3_w16 <tiles>t".  All refusals precede the device lookup; a shape the dispatch refuses is the launcher's error. */
PG_API int pg_dbg_gemm_v(int device, int precision, const float* x, const float* w, const float* bias, float* out, int M, int N, int K, int epi,
                  int variant, int have_ws, int m_live, char* plan, int plan_bytes);
/* The single-chain GEMM that computes the preceding LayerNorm in its operand load (gemm_ln_skinny_kernel), alone:
 * out = LayerNorm(x; gamma, beta, eps) . w^T + bias, through GELU when gelu = 1, in the 16-bit type of `precision` (PG_PREC_BF16 or
 * PG_PREC_F16).  x[M][K] fp32: the live rows, M in 1 ... 32; the kernel runs on Mi = 16 or 32 rows, and x_pad[Mi - M][K] (NULL: zeros)
 * is what the rows behind the live ones hold.  gamma[K], beta[K], bias[N] fp32; w[N][K] fp32, converted to the 16-bit type on the
 * device.  N a multiple of 16; K = 256, 512, 768, 1024 or 1280.  out[out_rows][N], out_rows >= Mi: its contents are converted to the
 * 16-bit type and uploaded first, the kernel writes its Mi rows, and all out_rows rows are returned widened -- whatever the kernel does
 * not write keeps the caller's (16-bit representable) pattern.  nb: 16-feature blocks per workgroup, 1 or 2 (2: N a multiple of 32),
 * 0 = the launcher's choice (PGIBBS_LN_SKINNY_NB, else 2 when N / 16 exceeds the CU count).  plan (NULL: not wanted): the text the
 * launch recorded, "ln+skinny8w <N / (16 nb)>t".  All refusals are PG_ERR_INVALID and precede the device lookup. */
PG_API int pg_dbg_gemm_ln(int device, int precision, const float* x, const float* x_pad, const float* gamma, const float* beta, float eps,
                   const float* w, const float* bias, float* out, int out_rows, int M, int N, int K, int gelu, int nb, char* plan,
                   int plan_bytes);
/* times `iters` back-to-back launches of the GEMM on device-resident random bf16 operands (HIP events; M a multiple of 16,
 * of 64 above 256); variant 1 =
 * lockstep kernel, 2 = ping-pong kernel; epi: 0 bf16 out, 1 bf16+gelu, 2 fp32 residual, 3 fp32, 4 fp32+gelu */
PG_API int pg_dbg_gemm_bench(int device, int M, int N, int K, int epi, int variant, int iters, double* avg_ms);
/* which kernel the GEMM dispatch picks for a shape on a device of n_cu compute units, as the text pg_prof_get_kernels reports for
 * that launch ("pp192x256 250t + tail64 40t", "skinny8w 80t x4k"; empty for an ablation variant; "error: ..." for a refused shape).
 * have_ws: split-K scratch is on offer (residual GEMMs of an engine); m_live: rows that hold tokens, 0 = all.  Touches no device. */
PG_API int pg_dbg_gemm_plan(int M, int N, int K, int epi, int variant, int have_ws, int m_live, int n_cu, char* buf, int buf_bytes);
/* which kernel template an attention launcher picks for a shape, and on which grid, as the text pg_prof_get_kernels reports for that
 * launch under "attention" ("whole kb18 hd64 split4 512+512wg", "split-f32 kb6 nqb5 hd64 5120wg", "row kb18 w9 rc1 2560wg"; "error:
 * ..." for a shape the launcher refuses).  kind 0: full attention over n_seq sequences of T tokens (row_step 1: contiguous chains;
 * else the strided sequences of the MSA column attention), has_pad / has_bias: with a <pad> key mask / ESM-1's bias key; kind 1:
 * tied row attention of B alignments of R rows x C columns (head_dim, has_pad, has_bias, row_step unused; order_bh: the (msa, head) count the
 * split of the row loop is decided on, 0 = B * H).  precision PG_PREC_FP32: the strict launchers, else the 16-bit ones (both operand
 * flavours share one plan).  A sequence length or column count < 1 is answered by the launcher's own refusal.  Touches no device. */
PG_API int pg_dbg_attention_plan(int kind, int precision, int64_t n_seq_or_B, int T_or_C, int R, int H, int head_dim, int has_pad, int has_bias,
                          int row_step, int order_bh, int n_cu, char* buf, int buf_bytes);
/* round-5 ablation: QKV projection + attention of B sequences of T in {32, 64, 128, 256} tokens as ONE launch (the fused
 * projection-attention kernel of the MSA column block, one head per 256 x 192 tile) against the two launches of the ESM-1b path;
 * ms[0] fused, ms[1] projection, ms[2] attention (HIP events, `iters` launches each); max_diff = max |fused - unfused| context */
PG_API int pg_dbg_qkv_attention_bench(int device, int B, int T, int H, int iters, double* ms, double* max_diff);
/* The fused column QKV + attention kernel of the MSA column block (csrc/gemm_colattn.hip) in one launch of its own, or the two launches
 * it replaces, on the same operands: x[B*R*C][d] fp32 in token order (row (b*R + r)*C + c), d = H*64; w[3 d][d] with the q rows first
 * and bias[3 d] (the engine's col_qkv); R in {32, 64, 128, 256}; precision PG_PREC_BF16 or PG_PREC_F16 (the strict mode never runs
 * this kernel).  x and w are rounded to the 16-bit type on the device.
 *   fused 1: the operand rows are permuted on the host to column-major order (row (b*C + c)*R + r) into round_up(B*C*R, 256) rows,
 *            the rows behind the live ones holding pad_fill (finite) in every feature; launch_headmajor_qkv regroups weights and bias
 *            per head; launch_gemm_colattn.  PGIBBS_MSA_COLFUSE=0 is answered with the launcher's error, never with the other path;
 *   fused 0: launch_gemm_bf16 (bf16 q, k, v rows) on the token-order rows padded to 256, then launch_attention_seq_bf16 over the
 *            B*C strided sequences of R tokens -- the engine's unfused branch.
 * ctx_inout[ctx_rows][d], ctx_rows >= B*R*C: the caller's pattern is uploaded in the 16-bit type, the launch writes its context rows
 * (token order) into it, and all ctx_rows rows come back widened -- what the kernel does not write keeps the pattern.  plan (NULL: not
 * wanted): the text the launches recorded.  All refusals (null pointer; B, C, H < 1; R; fused; pad_fill; ctx_rows; more than
 * 2^31 - 1 values; precision) are PG_ERR_INVALID with their own message and precede the device lookup. */
PG_API int pg_dbg_colattn(int device, int precision, const float* x, const float* w, const float* bias, float* ctx_inout, int64_t ctx_rows,
                   int B, int R, int C, int H, int fused, float pad_fill, char* plan, int plan_bytes);
/* y = LayerNorm(x[M][d]) * gamma + beta */
PG_API int pg_dbg_layernorm(int device, const float* x, const float* gamma, const float* beta, float* y, int M, int d,
                     float eps);
/* the same LayerNorm as the GEMMs read it (d a multiple of 32, <= 2560, or a multiple of 512 up to 5120): the operand rows written in `precision` and widened to fp32
 * -- bf16 (PG_PREC_BF16) or fp16 (PG_PREC_F16) rows, or the strict mode's split rows (PG_PREC_FP32) returned as hi + lo */
PG_API int pg_dbg_layernorm_operand(int device, int precision, const float* x, const float* gamma, const float* beta, float* y, int M,
                             int d, float eps);
/* softmax(q k^T) v per (b, h); q already scaled; qkv[B][T][3*H*64] fp32 -> ctx[B][T][H*64]; PG_PREC_BF16 or PG_PREC_FP32
 * (split-bf16 MFMA kernel, output = hi + lo of the operand rows it writes) or PG_PREC_F16 (the bf16 kernel with fp16 operands) */
PG_API int pg_dbg_attention(int device, int precision, const float* qkv, float* ctx, int B, int T, int H);
/* ESM-2's rotary embedding: the q and k thirds of qkv_inout[B*T][3*H*64] (fp32 host buffer) rotated in place, row r at position
 * r % T, in `precision` (16-bit modes: through a device buffer of that type, the result widened back); the v third is left alone */
PG_API int pg_dbg_rope(int device, int precision, float* qkv_inout, int B, int T, int H);      /* H <= 40 */
/* the same two with the head dimension as an argument: head_dim 64 (what pg_dbg_attention / pg_dbg_rope run), 32 (ESM-2 150M;
 * pg_dbg_rope_hd: H <= 32), 128 (ESM-2 15B; pg_dbg_rope_hd: H <= 40) or 16 (ESM-2 8M; pg_dbg_rope_hd: H <= 32), buffers [..][3*H*head_dim] and [..][H*head_dim].  key_tok (NULL: none): int32 tokens [B][T] of the keys;
 * a key whose token equals pad_idx is masked, as the <pad> keys of a ragged batch are */
PG_API int pg_dbg_attention_hd(int device, int precision, const float* qkv, float* ctx, int B, int T, int H, int head_dim,
                        const int32_t* key_tok, int pad_idx);
PG_API int pg_dbg_rope_hd(int device, int precision, float* qkv_inout, int B, int T, int H, int head_dim);
/* pg_dbg_attention_hd with ESM-1's bias key (add_bias_kv): bias_k / bias_v [H][head_dim] fp32, both or neither -- one more key behind
 * the T token keys, attended by every query, never masked.  The entry lays the two out as the engine does ([bias_k | bias_v], k of
 * head h at h*head_dim, v at (H + h)*head_dim), in the 16-bit type of `precision` or fp32 for PG_PREC_FP32.  Every argument is checked
 * on the host before a device is looked for (null / non-null pairs, the head dimension, the bias key at head 32 -- the plan's own
 * refusal text --, sizes): PG_ERR_INVALID with a message, never a launch.  plan (NULL: not wanted): receives the text the launch
 * recorded, as pg_dbg_attention_plan words it.  The two entries above are calls of this one */
PG_API int pg_dbg_attention_kv(int device, int precision, const float* qkv, float* ctx, int B, int T, int H, int head_dim,
                        const int32_t* key_tok, int pad_idx, const float* bias_k, const float* bias_v, char* plan, int plan_bytes);

/* MSA attention blocks: qkv[B][R][C][3*H*64] fp32 -> ctx[B][R][C][H*64]; which = 0 tied row attention (scores * scale),
 * 1 column attention (q pre-scaled); 2 / 3 = the same two with the strict precision mode's kernels; 4 / 5 = 0 / 1 with fp16
 * operands */
PG_API int pg_dbg_msa_attention(int device, int which, const float* qkv, float* ctx, int B, int R, int C, int H, float scale);
/* the same with the tokens tok[B][R][C] of a batch that holds <pad> (NULL: none; pg_dbg_msa_attention is a call of this).  Column
 * attention (which 1, 3, 5): the key rows that are pad_idx at a column get fair-esm's fill of -10000.  Tied row attention with tokens
 * takes the engine's route for a ragged batch: which 0 widens the 16-bit q, k, v to fp32 and runs the fp32-scores kernels with 16-bit
 * context rows, which 2 is the strict mode, which 4 (fp16) is refused with the engine's message (PG_ERR_UNSUPPORTED).  Arguments are
 * checked on the host before a device is looked for.  plan (NULL: not wanted): the text the launches recorded */
PG_API int pg_dbg_msa_attention_tok(int device, int which, const float* qkv, float* ctx, int B, int R, int C, int H, float scale,
                             const int32_t* tok, int pad_idx, char* plan, int plan_bytes);


/* ---- the memory-bound row kernels (csrc/elementwise.hip), each through its launcher ----
 * All five check on the host, before they look for a device, that no token, position row, row_map entry or gathered row the kernel
 * would read lies outside the buffers as the caller sized them: PG_ERR_INVALID with a message, never a GPU fault.  16-bit rows are
 * returned as raw bits in `precision` = PG_PREC_BF16 or PG_PREC_F16; buffers named _inout are copied to the device before the launch,
 * so whatever the kernel leaves unwritten comes back holding the caller's pattern. */
/* embed_ln_kernel: tokens[n_seq][T] (each in 0 .. V-1), embed[V][d] -> x[n_seq*T][d] fp32.  pos (NULL: no position table, ESM-2) has
 * pos_rows rows; msa_pos (rows_per_msa > 0) has rows_per_msa rows; gamma / beta (both or neither): emb_layer_norm_before; gamma2 /
 * beta2 / h2 (all or none): the first layer's LayerNorm of x as operand rows h2[n_seq*T][d]; h2 is _inout like the other 16-bit row
 * buffers: copied to the device before the launch (the kernel writes every row of it) */
PG_API int pg_dbg_embed(int device, int precision, const int32_t* tokens, int n_seq, int T, const float* embed, int V, int d, const float* pos,
                 int pos_rows, const float* msa_pos, int rows_per_msa, const float* gamma, const float* beta, const float* gamma2,
                 const float* beta2, int pad_idx, int mask_idx, int token_dropout, float eps, float embed_scale, float* x, uint16_t* h2);
/* launch_layernorm_bf16 on x[M][d]: form 0 = plain rows of d values, 1 = the strict mode's split rows of 3 d values (per 32 columns
 * [lo | hi | hi]; bf16 only), 2 = the same without the duplicate block; colmajor_R / colmajor_C > 0: token row (b*R + r)*C + c is
 * written as row (b*C + c)*R + r (form 0, d <= 2048, M a multiple of R*C).  h_inout holds h_rows >= M rows.  *kernel (may be NULL):
 * the kernel the launcher chose -- 0 plain, 1 the stride kernel (d = 1280 / 768, ~8 k .. 33 k rows, PGIBBS_LN_STRIDE), 2 column-major */
PG_API int pg_dbg_layernorm_rows(int device, int precision, const float* x, const float* gamma, const float* beta, uint16_t* h_inout,
                          int64_t h_rows, int M, int d, float eps, int form, int colmajor_R, int colmajor_C, int* kernel);
/* gather_ln_bf16_kernel: selected row r = LayerNorm of token row row_of(r / P) * width + (idx[r] & 0x3fffffff) of x[x_rows][d], zeros
 * when idx[r] < 0 or the position is >= width; row_of = row_map[n_map] (NULL: the identity); idx == NULL: selected row r = token row r.
 * split: 1 = [lo | hi | hi] rows (bf16).  h_inout holds h_rows >= n_sel rows */
PG_API int pg_dbg_gather_ln(int device, int precision, const float* x, int64_t x_rows, const int32_t* idx, const int32_t* row_map, int64_t n_map,
                     int P, int width, const float* gamma, const float* beta, uint16_t* h_inout, int64_t h_rows, int64_t n_sel, int d,
                     float eps, int split);
/* gather_rows_kernel: dst[r] = src[row_of(r / P) * width + pos] for rows of row_bytes (a multiple of 16) bytes; pos = idx[r] without
 * bit 30, 0 when that is negative or >= width.  n_iters = 0: idx[n_sel]; n_iters > 0: idx[n_iters][n_sel] and the kernel reads row
 * `iter` of it through a device-side iteration counter.  dst_inout holds dst_rows >= n_sel rows */
PG_API int pg_dbg_gather_rows(int device, const void* src, int64_t src_rows, void* dst_inout, int64_t dst_rows, const int32_t* idx, int n_iters,
                       int iter, const int32_t* row_map, int64_t n_map, int P, int width, int64_t n_sel, int row_bytes);
/* launch_split3_bf16 on x[rows][K] fp32 (K a multiple of 32): the strict mode's split operand rows of scale * x, 3 K bf16 words per row
 * (csrc/split_operand.h), into h_inout[h_rows >= rows][3 K].  form = weight (1) + through GELU (2): 0 an activation row [lo | hi | hi]
 * per 32 columns, 1 a weight row [hi | lo | hi], 2 an activation row of erf-GELU(x), which takes scale 1 and also returns
 * gelu_out[rows][K] = launch_gelu_f32 of the same x; 3 (GELU on a weight) and every other value are refused.  All refusals are
 * PG_ERR_INVALID on the host, before a device is looked for */
PG_API int pg_dbg_split_rows(int device, const float* x, uint16_t* h_inout, int64_t h_rows, int rows, int K, float scale, int form,
                      float* gelu_out);
/* launch_lm_tail: logits[n][V] = LayerNorm(g[n][d]; gamma, beta) . embed[V][d]^T + out_bias (gamma == beta == NULL: no LayerNorm,
 * ESM-1); V <= 64.  *small_kernel (may be NULL): 1 = the workgroup-per-row kernel ran (n <= PGIBBS_LM_TAIL_SMALL, default 1024) */
PG_API int pg_dbg_lm_tail(int device, const float* g, const float* gamma, const float* beta, const float* embed, const float* out_bias,
                   float* logits, int64_t n, int d, int V, float eps, int* small_kernel);

/* ---- the draw and the mask scatter (csrc/sample.hip), in every form the engine launches ----
 * n_steps steps; step s is iteration it = first_iter + s: launch_mask_scatter (mask_idx >= 0), then launch_sample_writeback, both on
 * the null stream, everything downloaded after each step.
 *   tokens_inout[n_rows][width]    the token rows before, and after the last step
 *   logits, V, compact             compact 1: [n_tables][n_sel*P][V], step s reads table it (the engine's LM head at the sampled rows);
 *                                  compact 0: [n_rows][width][V], shared by all steps (pg_sample_writeback_device's addressing)
 *   idx[n_tables][n_sel][P]        entries < 0 are padding, bit 30 marks a shadowed duplicate (drawn, not written); step s reads table it
 *   row_map[n_sel] (NULL: s)       the token row of selected row s
 *   params                         mask / mask_idx of it are not read (mask_idx below is)
 *   device_iter 0                  the step's table (idx + it * n_sel * P) and iteration = it are host arguments, d_iter = NULL
 *   device_iter 1                  what Engine captures, without a graph: launch_graph_state(first_iter, params) once; every step passes
 *                                  the table base, iteration 0 and the state block as d_iter; launch_iter_counter after each step
 *   mask_idx                       < 0: no mask step
 *   permit_out_of_range 1          positions >= width are let through to the kernels' own guards (pos >= width: -1, nothing read or
 *                                  written); 0: they are refused
 *   sampled_out[n_steps][n_sel][P] copied to the device before each step, so an entry the kernel leaves unwritten keeps the caller's
 *                                  pattern; -1 for padding and out-of-range entries
 *   masked_tokens_out[n_steps][n_rows][width] (NULL: not wanted)   the token rows after each step's mask scatter
 *   nonfinite_out (NULL: not wanted)   the word the draw kernel sets when a logit it reads is NaN or inf
 * Refused on the host before a device is looked for, each with its own message: null required pointers, counts < 1, flags other than
 * 0 / 1, masked_tokens_out without a mask step, n_tables < first_iter + n_steps, n_valid outside 1..32, a valid_idx outside 0..V-1, an
 * array of more than 2^31 - 1 values, n_sel > n_rows without a row_map, a row_map entry outside 0..n_rows-1, and (without the permit)
 * a position & 0x3fffffff >= width in any table. */
PG_API int pg_dbg_sample(int device, int32_t* tokens_inout, int64_t n_rows, int width, const float* logits, int V, int compact, const int32_t* idx,
                  int n_tables, const int32_t* row_map, int64_t n_sel, int P, const pg_sample_params* params, int first_iter, int n_steps,
                  int device_iter, int mask_idx, int permit_out_of_range, int32_t* sampled_out, int32_t* masked_tokens_out,
                  unsigned* nonfinite_out);
/* pg_dbg_sample with a draw guide (host pointers, as pg_engine_set_draw_guide takes them; NULL or nothing set: pg_dbg_sample's bits): the
 * same addressing forms, device_iter modes and outputs.  Step s draws at call-local iteration first_iter + s, so a schedule needs
 * n_temperatures >= first_iter + n_steps; a per-row bias table has n_rows rows.  With device_iter 1 the iteration AND the guide's device
 * pointers are read from the state block.  Refusals: pg_dbg_sample's, then the guide's set-time and run-time ones, all on the host
 * before a device is looked for.  pg_guided_sizeof_draw_guide: sizeof(pg_draw_guide), for bindings that mirror the struct. */
PG_API int pg_guided_dbg_sample(int device, int32_t* tokens_inout, int64_t n_rows, int width, const float* logits, int V, int compact,
                         const int32_t* idx, int n_tables, const int32_t* row_map, int64_t n_sel, int P, const pg_sample_params* params,
                         int first_iter, int n_steps, int device_iter, int mask_idx, int permit_out_of_range, int32_t* sampled_out,
                         int32_t* masked_tokens_out, unsigned* nonfinite_out, const pg_draw_guide* guide);
PG_API int pg_guided_sizeof_draw_guide(void);

/* ---- the live-width forms of pg_dbg_embed, pg_dbg_layernorm_rows, pg_dbg_gather_ln and pg_dbg_lm_tail (an embedded model's rows) ----
 * Every table, row and vector is d wide in memory; its first d_live features (a multiple of 4, at most d) are the model's own.
 * Statistics, affine and the decoder's dot products run over d_live features -- on them, bit for bit what the same entry gives for
 * rows of d = d_live -- and the d - d_live pad features of every 16-bit output row are written as zeros, in the split forms too.
 * d_live = d is the entry above; each entry names itself in its error messages.  No live form: emb_layer_norm_before (gamma / beta of pg_dbg_embed), column-major rows, the stride kernel */
PG_API int pg_embedded_embed_rows(int device, int precision, const int32_t* tokens, int n_seq, int T, const float* embed, int V, int d,
                           const float* pos, int pos_rows, const float* msa_pos, int rows_per_msa, const float* gamma, const float* beta,
                           const float* gamma2, const float* beta2, int pad_idx, int mask_idx, int token_dropout, float eps, float embed_scale,
                           float* x, uint16_t* h2, int d_live);
PG_API int pg_embedded_layernorm_rows(int device, int precision, const float* x, const float* gamma, const float* beta, uint16_t* h_inout,
                               int64_t h_rows, int M, int d, float eps, int form, int colmajor_R, int colmajor_C, int* kernel, int d_live);
PG_API int pg_embedded_gather_ln(int device, int precision, const float* x, int64_t x_rows, const int32_t* idx, const int32_t* row_map, int64_t n_map,
                          int P, int width, const float* gamma, const float* beta, uint16_t* h_inout, int64_t h_rows, int64_t n_sel, int d,
                          float eps, int split, int d_live);
PG_API int pg_embedded_lm_tail(int device, const float* g, const float* gamma, const float* beta, const float* embed, const float* out_bias,
                        float* logits, int64_t n, int d, int V, float eps, int* small_kernel, int d_live);
/* Host only (no device is looked for): the run-shape image pg_engine_create_embedded uploads for the natural tensor `name` (its role is
 * read from the fair-esm key: embed_tokens.weight, layers.i.self_attn.{q,k,v,out}_proj.*, layers.i.fc1.* / fc2.*, every *layer_norm*,
 * lm_head.dense.*, lm_head.bias) of a model of n_heads heads of head_width in slots of head_slot: live values at their run positions,
 * 0.0 everywhere else.  numel / image_numel must be the natural and the run size */
PG_API int pg_embedded_image(const char* name, const float* src, int64_t numel, int n_heads, int head_width, int head_slot, int d_ffn, int vocab,
                      float* image, int64_t image_numel);
/* Host only: the rotary table [rows][head_slot] of such an engine: row t = [cos(t f_i), i < head_width / 2, then 1 ... | sin(t f_i),
 * then 0 ...], f_i = 10000^(-2i / head_width) as fp32 (head_width == head_slot: the table of a built width) */
PG_API int pg_embedded_rope_table(int rows, int head_width, int head_slot, float* table);

#ifdef __cplusplus
}
#endif
#endif /* PGIBBS_H */
