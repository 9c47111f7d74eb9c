// extern "C" surface declared in include/pgibbs.h.
#include <math.h>
#include <string.h>

#include <vector>

#include <algorithm>

#include "engine.h"
#include "gemm_epilogue.h"

namespace pg {
const char* last_error_cstr();
}
using namespace pg;

namespace {
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    (void)hipGetDevice(&prev);
    if (dev >= 0 && dev != prev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// vocab > 0: also that every valid_idx entry indexes a logit row of that width.  The engine entry points pass the model's
// vocabulary: a replayed hipGraph copies the parameters into its device-side state block without going through
// launch_sample_writeback's own host-side check.
int check_params(const pg_sample_params* p, int vocab = 0) {
  if (!p) return fail(PG_ERR_INVALID, "null pg_sample_params");
  if (p->n_valid < 1 || p->n_valid > 32) return fail(PG_ERR_INVALID, "n_valid must be in 1..32");
  if (vocab > 0)
    for (int j = 0; j < p->n_valid; ++j)
      if (p->valid_idx[j] < 0 || p->valid_idx[j] >= vocab) return fail(PG_ERR_INVALID, "sample: valid_idx out of range");
  return PG_OK;
}

// host-side index tables: entries < 0 are padding; bit 30 marks a shadowed duplicate; the position itself must lie inside the
// token row (the reference raises IndexError there: batch[b][kk] = ..., esm_sampler.py:234,262)
int check_idx_table(const int32_t* idx, size_t n, int width, const char* who) {
  for (size_t i = 0; i < n; ++i) {
    const int32_t v = idx[i];
    if (v >= 0 && (v & 0x3fffffff) >= width)
      return fail(PG_ERR_INVALID, std::string(who) + ": target position " + std::to_string(v & 0x3fffffff) +
                                      " is out of range for a token row of width " + std::to_string(width));
  }
  return PG_OK;
}
// full-logit entry points: the rows just copied to the host are scanned there (a few MB; the Gibbs and log-probability entry
// points are covered by their kernels, Engine::range_err)
int check_finite(Engine& e, const float* v, size_t n) {
  float worst = 0.f;
  for (size_t i = 0; i < n; ++i) worst = fmaxf(worst, fabsf(v[i]) <= 3.0e38f ? 0.f : 1.f);
  if (worst == 0.f) return PG_OK;
  *e.range_err = 1;
  return e.range_check();
}
bool has_token(const int32_t* tokens, size_t n, int32_t id) {
  for (size_t i = 0; i < n; ++i)
    if (tokens[i] == id) return true;
  return false;
}
// A ragged batch (<pad> in some row; for the MSA model a ragged list of MSAs padded to one tensor, esm_msa_sampler.py:341): while
// this lives the trunks mask keys at <pad> in attention, as fair-esm's key_padding_mask does
struct PadFlag {
  Engine& e;
  PadFlag(Engine& e_, const int32_t* tokens, size_t n) : e(e_) { e.esm_pad_in_batch = has_token(tokens, n, e.cfg.pad_idx); }
  ~PadFlag() { e.esm_pad_in_batch = false; }
};

// tokens[B][R][C] in (R = 1 for the ESM family), logits of every position out
int forward_logits(Engine& e, const int32_t* tokens, int B, int R, int C, float* logits_out) {
  DeviceGuard g(e.device);
  const int64_t M = (int64_t)B * R * C;
  int rc;
  if ((rc = e.d_tokens.ensure((size_t)M * 4, e.stream))) return rc;
  if ((rc = e.logits.ensure((size_t)M * e.cfg.vocab * 4, e.stream))) return rc;
  PG_HIP(hipMemcpyAsync(e.d_tokens.p, tokens, (size_t)M * 4, hipMemcpyHostToDevice, e.stream));
  {
    PadFlag pad(e, tokens, (size_t)M);
    rc = e.trunk(e.d_tokens.as<int32_t>(), B, R, C);
  }
  if (rc) return rc;
  if ((rc = e.head(nullptr, nullptr, 1, C, M, e.logits.as<float>()))) return rc;
  PG_HIP(hipMemcpyAsync(logits_out, e.logits.p, (size_t)M * e.cfg.vocab * 4, hipMemcpyDeviceToHost, e.stream));
  PG_HIP(hipStreamSynchronize(e.stream));
  if ((rc = e.chain_check())) return rc;
  return check_finite(e, logits_out, (size_t)M * e.cfg.vocab);
}

// A Gibbs call on host buffers: tokens and the index table go to the device, run(d_tokens, d_idx, d_sampled_logits, d_sampled_tokens)
// queues the loop (an output the caller did not ask for is null), and tokens and outputs come back.
template <typename Run>
int stage_gibbs(Engine& e, int32_t* tokens_inout, size_t n_tokens, const int32_t* idx, size_t n_draws, float* sampled_logits,
                int32_t* sampled_tokens, Run&& run) {
  const size_t tok_bytes = n_tokens * 4, n1 = n_draws ? n_draws : 1;
  int rc;
  if ((rc = e.d_tokens.ensure(tok_bytes, e.stream))) return rc;
  if ((rc = e.d_idx.ensure(n1 * 4, e.stream))) return rc;
  if (sampled_logits && (rc = e.d_samp_logits.ensure(n1 * e.cfg.vocab * 4, e.stream))) return rc;
  if (sampled_tokens && (rc = e.d_samp_tok.ensure(n1 * 4, e.stream))) return rc;
  PG_HIP(hipMemcpyAsync(e.d_tokens.p, tokens_inout, tok_bytes, hipMemcpyHostToDevice, e.stream));
  if (n_draws) PG_HIP(hipMemcpyAsync(e.d_idx.p, idx, n_draws * 4, hipMemcpyHostToDevice, e.stream));
  if ((rc = run(e.d_tokens.as<int32_t>(), e.d_idx.as<int32_t>(), sampled_logits ? e.d_samp_logits.as<float>() : nullptr,
                sampled_tokens ? e.d_samp_tok.as<int32_t>() : nullptr))) return rc;
  // before the caller's token buffer (input AND output) is overwritten: a timed-out persistent launch is re-run by the caller
  // macro, non-finite logits (PG_ERR_RANGE) leave the input intact for a caller that retries in another precision
  PG_HIP(hipStreamSynchronize(e.stream));
  if ((rc = e.finish_check())) return rc;
  PG_HIP(hipMemcpyAsync(tokens_inout, e.d_tokens.p, tok_bytes, hipMemcpyDeviceToHost, e.stream));
  if (sampled_logits && n_draws)
    PG_HIP(hipMemcpyAsync(sampled_logits, e.d_samp_logits.p, n_draws * e.cfg.vocab * 4, hipMemcpyDeviceToHost, e.stream));
  if (sampled_tokens && n_draws)
    PG_HIP(hipMemcpyAsync(sampled_tokens, e.d_samp_tok.p, n_draws * 4, hipMemcpyDeviceToHost, e.stream));
  PG_HIP(hipStreamSynchronize(e.stream));
  return PG_OK;
}
}  // namespace

extern "C" {

const char* pg_version(void) { return "pgibbs 0.1 (gfx950)"; }
const char* pg_last_error(void) { return last_error_cstr(); }

int pg_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int pg_engine_create(const pg_model_config* cfg, const pg_tensor* tensors, int n_tensors, int device_ordinal,
                     int precision, pg_engine** out) {
  if (!cfg || !out || (n_tensors > 0 && !tensors)) return fail(PG_ERR_INVALID, "pg_engine_create: null argument");
  *out = nullptr;
  int prev = -1;
  (void)hipGetDevice(&prev);
  pg_engine* h = new pg_engine;
  int rc = h->e.init(cfg, tensors, n_tensors, device_ordinal, precision);
  if (prev >= 0) (void)hipSetDevice(prev);
  if (rc != PG_OK) {
    std::string keep = pg_last_error();
    delete h;
    set_error(keep);
    return rc;
  }
  *out = h;
  return PG_OK;
}

void pg_engine_destroy(pg_engine* h) { delete h; }

int pg_engine_set_stream(pg_engine* h, void* hip_stream) {
  if (!h) return fail(PG_ERR_INVALID, "null engine");
  h->e.stream = hip_stream ? (hipStream_t)hip_stream : h->e.own_stream;
  return PG_OK;
}
int pg_engine_synchronize(pg_engine* h) {
  if (!h) return fail(PG_ERR_INVALID, "null engine");
  Engine& e = h->e;
  DeviceGuard g(e.device);
  PG_HIP(hipStreamSynchronize(e.stream));
  // a barrier timeout of the persistent trunk inside asynchronous device-pointer calls: they were logged with their token rows and
  // chain_check() has just run them again on the per-layer launches -- nothing for the caller to repair
  int rc = e.chain_check();
  if (rc && e.chain_replay_ok) {
    e.chain_retry = false;
    rc = PG_OK;
  }
  return rc ? rc : e.range_check();
}
int pg_engine_device(const pg_engine* h) { return h ? h->e.device : -1; }
int pg_engine_set_job_items(pg_engine* h, int64_t job_items) {
  if (!h) return fail(PG_ERR_INVALID, "null engine");
  if (job_items < 0) return fail(PG_ERR_INVALID, "pg_engine_set_job_items: negative count");
  h->e.job_items = job_items;
  return PG_OK;
}

int pg_engine_get_stat(pg_engine* h, const char* name, int64_t* value) {
  if (!h || !name || !value) return fail(PG_ERR_INVALID, "pg_engine_get_stat: null argument");
  if (!strcmp(name, "graph_captures")) *value = h->e.stat_graph_captures;
  else if (!strcmp(name, "graph_replays")) *value = h->e.stat_graph_replays;
  else return fail(PG_ERR_INVALID, std::string("unknown stat ") + name);
  return PG_OK;
}

// ---- ESM-1b ---------------------------------------------------------------------------------
static int esm_forward_logits_once(pg_engine* h, const int32_t* tokens, int B, int T, float* logits_out) {
  if (!h || !tokens || !logits_out) return fail(PG_ERR_INVALID, "pg_esm_forward_logits: null argument");
  Engine& e = h->e;
  if (!e.esm_family()) return fail(PG_ERR_INVALID, "engine was not built for an ESM-1b / ESM-1 / ESM-2 architecture");
  if (B < 0 || T < 1) return fail(PG_ERR_INVALID, "bad shape");
  if (T > e.cfg.max_positions) return fail(PG_ERR_INVALID, "sequence longer than the learned position table");
  if (B == 0) return PG_OK;
  return forward_logits(e, tokens, B, 1, T, logits_out);
}
// The persistent single-chain trunk is an optimistic fast path: when one of its barriers timed out (Engine::chain_check) the
// call's inputs are still intact in the caller's buffers, so it runs once more, now on the per-layer launches.
#define PG_RETRY_WITHOUT_CHAIN_TRUNK(h, call)                          \
  do {                                                                \
    int rc_ = (call);                                                 \
    if (rc_ && (h) && (h)->e.chain_retry) {                           \
      (h)->e.chain_retry = false;                                     \
      rc_ = (call);                                                   \
    }                                                                 \
    return rc_;                                                       \
  } while (0)
int pg_esm_forward_logits(pg_engine* h, const int32_t* tokens, int B, int T, float* logits_out) {
  PG_RETRY_WITHOUT_CHAIN_TRUNK(h, esm_forward_logits_once(h, tokens, B, T, logits_out));
}

int pg_esm_gibbs_run_device(pg_engine* h, int32_t* d_tokens_inout, int B, int T, const int32_t* d_target_idx, int n_iters,
                            int P, const pg_sample_params* params, float* d_sampled_logits, int32_t* d_sampled_tokens) {
  if (!h || !d_tokens_inout || (!d_target_idx && P > 0 && n_iters > 0))
    return fail(PG_ERR_INVALID, "pg_esm_gibbs_run_device: null argument");
  int rc = check_params(params, h->e.cfg.vocab);
  if (rc) return rc;
  Engine& e = h->e;
  DeviceGuard g(e.device);
  // An earlier asynchronous call has reported a barrier timeout of the persistent trunk: repair (restore the logged token rows,
  // run the logged calls again on the per-layer launches) BEFORE this call is queued on top of those tokens -- whatever this
  // call's own shape is (round 6, ADVICE r05: a following call with B*T > 32 on the same tokens used to be enqueued on the
  // corrupted rows, and the later replay then re-ran only the logged calls).  Contract (pgibbs.h): between synchronisations no work
  // other than pg_*_device calls of this engine may touch a token buffer that such a call has been given -- the replay restores
  // the snapshot taken at the first logged call.
  if (!e.chain_log.empty() && e.chain_err && *e.chain_err) {
    PG_HIP(hipStreamSynchronize(e.stream));
    rc = e.chain_check();
    if (rc && !e.chain_replay_ok) return rc;
    e.chain_retry = false;
  }
  if (B > 0 && n_iters > 0 && T >= 1 && e.chain_may_run(B, T) &&
      (rc = e.chain_log_call(d_tokens_inout, B, T, d_target_idx, n_iters, P, params, d_sampled_logits, d_sampled_tokens)))
    return rc;
  return e.esm_gibbs_device(d_tokens_inout, B, T, d_target_idx, n_iters, P, params, d_sampled_logits, d_sampled_tokens);
}

static int esm_gibbs_run_once(pg_engine* h, int32_t* tokens_inout, int B, int T, const int32_t* target_idx, int n_iters, int P,
                              const pg_sample_params* params, float* sampled_logits, int32_t* sampled_tokens) {
  if (!h || !tokens_inout || (!target_idx && P > 0 && n_iters > 0)) return fail(PG_ERR_INVALID, "pg_esm_gibbs_run: null argument");
  int rc = check_params(params, h->e.cfg.vocab);
  if (rc) return rc;
  if (B < 0 || T < 1 || P < 0 || n_iters < 0) return fail(PG_ERR_INVALID, "bad shape");
  if (B == 0) return PG_OK;
  Engine& e = h->e;
  DeviceGuard g(e.device);
  const size_t n_draws = (size_t)B * P * n_iters;
  if (n_draws && (rc = check_idx_table(target_idx, n_draws, T, "pg_esm_gibbs_run"))) return rc;
  PadFlag pad(e, tokens_inout, (size_t)B * T);
  return stage_gibbs(e, tokens_inout, (size_t)B * T, target_idx, n_draws, sampled_logits, sampled_tokens,
                     [&](int32_t* d_tok, const int32_t* d_idx, float* d_lg, int32_t* d_st) {
                       return e.esm_gibbs_device(d_tok, B, T, d_idx, n_iters, P, params, d_lg, d_st);
                     });
}
int pg_esm_gibbs_run(pg_engine* h, int32_t* tokens_inout, int B, int T, const int32_t* target_idx, int n_iters, int P,
                     const pg_sample_params* params, float* sampled_logits, int32_t* sampled_tokens) {
  PG_RETRY_WITHOUT_CHAIN_TRUNK(h, esm_gibbs_run_once(h, tokens_inout, B, T, target_idx, n_iters, P, params, sampled_logits, sampled_tokens));
}

// ---- ESM-MSA-1b -----------------------------------------------------------------------------
int pg_msa_forward_logits(pg_engine* h, const int32_t* tokens, int B, int R, int C, float* logits_out) {
  if (!h || !tokens || !logits_out) return fail(PG_ERR_INVALID, "pg_msa_forward_logits: null argument");
  Engine& e = h->e;
  if (e.cfg.arch != PG_ARCH_MSA1B) return fail(PG_ERR_INVALID, "engine was not built for the MSA-1b architecture");
  if (B < 0 || R < 1 || C < 1) return fail(PG_ERR_INVALID, "bad shape");
  if (B == 0) return PG_OK;
  return forward_logits(e, tokens, B, R, C, logits_out);
}

int pg_msa_gibbs_run(pg_engine* h, int32_t* tokens_inout, int B, int R, int C, const int32_t* target_idx, int n_iters,
                     int P, const pg_sample_params* params, float* sampled_logits, int32_t* sampled_tokens) {
  if (!h || !tokens_inout || (!target_idx && P > 0 && n_iters > 0)) return fail(PG_ERR_INVALID, "pg_msa_gibbs_run: null argument");
  int rc = check_params(params, h->e.cfg.vocab);
  if (rc) return rc;
  if (B < 0 || R < 1 || C < 1 || P < 0 || n_iters < 0) return fail(PG_ERR_INVALID, "bad shape");
  if (B == 0) return PG_OK;
  Engine& e = h->e;
  DeviceGuard g(e.device);
  const size_t n_draws = (size_t)B * R * P * n_iters;
  if (n_draws && (rc = check_idx_table(target_idx, n_draws, C, "pg_msa_gibbs_run"))) return rc;
  return stage_gibbs(e, tokens_inout, (size_t)B * R * C, target_idx, n_draws, sampled_logits, sampled_tokens,
                     [&](int32_t* d_tok, const int32_t* d_idx, float* d_lg, int32_t* d_st) {
                       return e.msa_gibbs_device(d_tok, B, R, C, d_idx, n_iters, P, params, d_lg, d_st);
                     });
}

int pg_msa_gibbs_single_batch_run(pg_engine* h, int32_t* tokens_inout, int B, int R, int C, int mask_row, int target_row,
                                  const int32_t* step_idx, const int32_t* step_sample_flag, int n_steps, int P_max,
                                  const pg_sample_params* params, float* sampled_logits, int32_t* sampled_tokens) {
  if (!h || !tokens_inout || (n_steps > 0 && (!step_sample_flag || (!step_idx && P_max > 0))))
    return fail(PG_ERR_INVALID, "pg_msa_gibbs_single_batch_run: null argument");
  if (B < 0 || R < 1 || C < 1 || P_max < 0 || n_steps < 0) return fail(PG_ERR_INVALID, "bad shape");
  if (B == 0) return PG_OK;
  int rc;
  if (!params) return fail(PG_ERR_INVALID, "null pg_sample_params");
  for (int b = 0; b < B; ++b)
    if ((rc = check_params(params + b, h->e.cfg.vocab))) return rc;
  Engine& e = h->e;
  DeviceGuard g(e.device);
  {
    // The tied row attention of a template batch runs in its split-R form (every template as if alone), whose
    // fp32 scratch grows with B: 0.5 GB for 4 templates of 128 x 513, past 2 GB from about B = 9 at C = 576 or B = 32 at C = 300.
    // Templates are independent, so a larger batch is simply run in chunks that fit (same logits and tokens; ADVICE r03:
    // `--template_batch 32`, BASELINE config 5's "32 templates", used to fail with PG_ERR_INVALID).
    static const size_t limit = (size_t)env_int("PGIBBS_SPLIT_SCRATCH_MB", 1024) << 20;
    const size_t need1 = msa_row_split_scratch_bytes(1, R, C, e.cfg.n_heads, e.cfg.n_heads);
    const int bc = need1 ? (int)std::max<size_t>(1, std::min<size_t>((size_t)B, limit / need1)) : B;
    if (bc < B) {
      std::vector<int32_t> idx_c, tok_c;
      std::vector<float> lg_c;
      const int V = e.cfg.vocab;
      for (int b0 = 0; b0 < B; b0 += bc) {
        const int nb = std::min(bc, B - b0);
        idx_c.assign((size_t)n_steps * nb * P_max + 1, -1);
        for (int s2 = 0; s2 < n_steps && P_max > 0; ++s2)
          memcpy(idx_c.data() + (size_t)s2 * nb * P_max, step_idx + ((size_t)s2 * B + b0) * P_max, (size_t)nb * P_max * 4);
        if (sampled_logits) lg_c.assign((size_t)n_steps * nb * P_max * V + 1, 0.f);
        if (sampled_tokens) tok_c.assign((size_t)n_steps * nb * P_max + 1, 0);
        if ((rc = pg_msa_gibbs_single_batch_run(h, tokens_inout + (size_t)b0 * R * C, nb, R, C, mask_row, target_row, idx_c.data(),
                                                step_sample_flag, n_steps, P_max, params + b0, sampled_logits ? lg_c.data() : nullptr,
                                                sampled_tokens ? tok_c.data() : nullptr))) return rc;
        for (int s2 = 0; s2 < n_steps && P_max > 0; ++s2) {
          if (sampled_logits) memcpy(sampled_logits + ((size_t)s2 * B + b0) * P_max * V, lg_c.data() + (size_t)s2 * nb * P_max * V, (size_t)nb * P_max * V * 4);
          if (sampled_tokens) memcpy(sampled_tokens + ((size_t)s2 * B + b0) * P_max, tok_c.data() + (size_t)s2 * nb * P_max, (size_t)nb * P_max * 4);
        }
      }
      return PG_OK;
    }
  }
  const size_t n_draws = (size_t)B * P_max * n_steps;
  if (n_draws && (rc = check_idx_table(step_idx, n_draws, C, "pg_msa_gibbs_single_batch_run"))) return rc;
  return stage_gibbs(e, tokens_inout, (size_t)B * R * C, step_idx, n_draws, sampled_logits, sampled_tokens,
                     [&](int32_t* d_tok, const int32_t* d_idx, float* d_lg, int32_t* d_st) {
                       return e.msa_single_device(d_tok, B, R, C, mask_row, target_row, d_idx, step_sample_flag, n_steps, P_max, params, d_lg, d_st);
                     });
}

// generate_single == the batched form with one template
int pg_msa_gibbs_single_run(pg_engine* h, int32_t* tokens_inout, int R, int C, int mask_row, int target_row,
                            const int32_t* step_idx, const int32_t* step_sample_flag, int n_steps, int P_max,
                            const pg_sample_params* params, float* sampled_logits, int32_t* sampled_tokens) {
  if (!h || !tokens_inout || (n_steps > 0 && (!step_sample_flag || (!step_idx && P_max > 0))))
    return fail(PG_ERR_INVALID, "pg_msa_gibbs_single_run: null argument");
  return pg_msa_gibbs_single_batch_run(h, tokens_inout, 1, R, C, mask_row, target_row, step_idx, step_sample_flag, n_steps, P_max,
                                       params, sampled_logits, sampled_tokens);
}

int pg_msa_gibbs_run_device(pg_engine* h, int32_t* d_tokens_inout, int B, int R, int C, const int32_t* d_target_idx,
                            int n_iters, int P, const pg_sample_params* params, float* d_sampled_logits,
                            int32_t* d_sampled_tokens) {
  if (!h || !d_tokens_inout || (!d_target_idx && P > 0 && n_iters > 0))
    return fail(PG_ERR_INVALID, "pg_msa_gibbs_run_device: null argument");
  int rc = check_params(params, h->e.cfg.vocab);
  if (rc) return rc;
  DeviceGuard g(h->e.device);
  return h->e.msa_gibbs_device(d_tokens_inout, B, R, C, d_target_idx, n_iters, P, params, d_sampled_logits, d_sampled_tokens);
}

// ---- masked log-likelihood scoring (next-tier path: log_likelihood_batch) ---------------------------
// rows: tokens[n_rows][width]; sample s scores token row row_of[s] at positions idx[s][P] (entries < 0 skipped, out = 0)
// against targets[s][P]; out[s][P] = log_softmax(logits)[target].
static int forward_logprobs(Engine& e, const int32_t* tokens, int B, int R, int C, const int32_t* row_of,
                            const int32_t* idx, const int32_t* targets, int n_sel, int P, float* out) {
  DeviceGuard g(e.device);
  const int64_t M = (int64_t)B * R * C;
  const int64_t n = (int64_t)n_sel * P;
  int rc;
  if (n == 0 || B == 0) return PG_OK;
  if ((rc = e.d_tokens.ensure((size_t)M * 4, e.stream))) return rc;
  if ((rc = e.d_idx.ensure((size_t)n * 4, e.stream)) || (rc = e.d_samp_tok.ensure((size_t)n * 4, e.stream))) return rc;
  if ((rc = e.d_rowmap.ensure((size_t)n_sel * 4, e.stream))) return rc;
  if ((rc = e.logits.ensure((size_t)n * e.cfg.vocab * 4, e.stream)) || (rc = e.d_samp_logits.ensure((size_t)n * 4, e.stream))) return rc;
  for (int64_t i = 0; i < n; ++i)
    if (idx[i] >= C || (idx[i] >= 0 && (targets[i] < 0 || targets[i] >= e.cfg.vocab))) return fail(PG_ERR_INVALID, "logprobs: index out of range");
  for (int i = 0; i < n_sel; ++i)
    if (row_of[i] < 0 || row_of[i] >= B * R) return fail(PG_ERR_INVALID, "logprobs: row out of range");
  PG_HIP(hipMemcpyAsync(e.d_tokens.p, tokens, (size_t)M * 4, hipMemcpyHostToDevice, e.stream));
  PG_HIP(hipMemcpyAsync(e.d_idx.p, idx, (size_t)n * 4, hipMemcpyHostToDevice, e.stream));
  PG_HIP(hipMemcpyAsync(e.d_samp_tok.p, targets, (size_t)n * 4, hipMemcpyHostToDevice, e.stream));
  PG_HIP(hipMemcpyAsync(e.d_rowmap.p, row_of, (size_t)n_sel * 4, hipMemcpyHostToDevice, e.stream));
  {
    PadFlag pad(e, tokens, (size_t)M);
    rc = e.trunk(e.d_tokens.as<int32_t>(), B, R, C);
  }
  if (rc) return rc;
  if ((rc = e.head(e.d_idx.as<int32_t>(), e.d_rowmap.as<int32_t>(), P, C, n, e.logits.as<float>()))) return rc;
  if ((rc = launch_logprob_gather(e.stream, e.logits.as<float>(), e.cfg.vocab, 1, C, e.d_idx.as<int32_t>(), e.d_rowmap.as<int32_t>(),
                                  e.d_samp_tok.as<int32_t>(), n_sel, P, e.d_samp_logits.as<float>(), e.range_err))) return rc;
  PG_HIP(hipMemcpyAsync(out, e.d_samp_logits.p, (size_t)n * 4, hipMemcpyDeviceToHost, e.stream));
  PG_HIP(hipStreamSynchronize(e.stream));
  return e.finish_check();
}

int pg_esm_forward_logprobs(pg_engine* h, const int32_t* tokens, int B, int T, const int32_t* row_of, const int32_t* idx,
                            const int32_t* targets, int n_sel, int P, float* out) {
  if (!h || !tokens || !row_of || !idx || !targets || !out) return fail(PG_ERR_INVALID, "pg_esm_forward_logprobs: null argument");
  if (!h->e.esm_family()) return fail(PG_ERR_INVALID, "engine was not built for an ESM-1b / ESM-1 / ESM-2 architecture");
  if (B < 0 || T < 1 || n_sel < 0 || P < 0) return fail(PG_ERR_INVALID, "bad shape");
  if (T > h->e.cfg.max_positions) return fail(PG_ERR_INVALID, "sequence longer than the learned position table");
  PG_RETRY_WITHOUT_CHAIN_TRUNK(h, forward_logprobs(h->e, tokens, B, 1, T, row_of, idx, targets, n_sel, P, out));
}

int pg_msa_forward_logprobs(pg_engine* h, const int32_t* tokens, int B, int R, int C, const int32_t* row_of,
                            const int32_t* idx, const int32_t* targets, int n_sel, int P, float* out) {
  if (!h || !tokens || !row_of || !idx || !targets || !out) return fail(PG_ERR_INVALID, "pg_msa_forward_logprobs: null argument");
  if (h->e.cfg.arch != PG_ARCH_MSA1B) return fail(PG_ERR_INVALID, "engine was not built for the MSA-1b architecture");
  if (B < 0 || R < 1 || C < 1 || n_sel < 0 || P < 0) return fail(PG_ERR_INVALID, "bad shape");
  return forward_logprobs(h->e, tokens, B, R, C, row_of, idx, targets, n_sel, P, out);
}

int pg_logprob_gather_device(void* stream, const float* d_logits, int64_t n_rows, int width, int V, const int32_t* d_idx,
                             const int32_t* d_row_map, const int32_t* d_targets, int64_t n_sel, int P, float* d_out) {
  if (!d_logits || !d_idx || !d_targets || !d_out) return fail(PG_ERR_INVALID, "pg_logprob_gather_device: null argument");
  if (n_rows < 0 || width < 1 || V < 1 || n_sel < 0 || P < 0) return fail(PG_ERR_INVALID, "bad shape");
  return launch_logprob_gather((hipStream_t)stream, d_logits, V, 0, width, d_idx, d_row_map, d_targets, n_sel, P, d_out);
}

// ---- stand-alone ends of the iteration ---------------------------------------------------------
int pg_mask_scatter_device(void* stream, int32_t* d_tokens, int64_t n_rows, int width, const int32_t* d_idx,
                           const int32_t* d_row_map, int64_t n_sel, int P, int mask_idx) {
  if (!d_tokens || (!d_idx && n_sel * P > 0)) return fail(PG_ERR_INVALID, "pg_mask_scatter_device: null argument");
  if (n_rows < 0 || width < 1 || n_sel < 0 || P < 0) return fail(PG_ERR_INVALID, "bad shape");
  return launch_mask_scatter((hipStream_t)stream, d_tokens, width, d_idx, d_row_map, n_sel, P, mask_idx);
}

int pg_sample_writeback_device(void* stream, int32_t* d_tokens, int64_t n_rows, int width, const float* d_logits, int V,
                               const int32_t* d_idx, const int32_t* d_row_map, int64_t n_sel, int P,
                               const pg_sample_params* params, int iteration, int32_t* d_sampled_tokens) {
  if (!d_tokens || !d_logits || (!d_idx && n_sel * P > 0)) return fail(PG_ERR_INVALID, "pg_sample_writeback_device: null argument");
  int rc = check_params(params, V);
  if (rc) return rc;
  if (n_rows < 0 || width < 1 || n_sel < 0 || P < 0 || V < 1) return fail(PG_ERR_INVALID, "bad shape");
  return launch_sample_writeback((hipStream_t)stream, d_tokens, width, d_logits, V, 0, d_idx, d_row_map, n_sel, P, params,
                                 iteration, d_sampled_tokens);
}

// ---- measurement ----------------------------------------------------------------------------
int pg_prof_enable(pg_engine* h, int on) {
  if (!h) return fail(PG_ERR_INVALID, "null engine");
  h->e.prof.on = on != 0;
  return PG_OK;
}
int pg_prof_reset(pg_engine* h) {
  if (!h) return fail(PG_ERR_INVALID, "null engine");
  DeviceGuard g(h->e.device);
  PG_HIP(hipStreamSynchronize(h->e.stream));
  h->e.prof.reset();
  return PG_OK;
}
int pg_prof_get(pg_engine* h, const char* kernel_class, double* total_ms, int64_t* launches) {
  if (!h || !kernel_class || !total_ms || !launches) return fail(PG_ERR_INVALID, "pg_prof_get: null argument");
  static const char* names[PC_COUNT] = {"gemm_other", "attention", "layernorm", "embed", "head", "sample", "gemm_qkv", "gemm_out", "gemm_fc1", "gemm_fc2", "rope"};
  int cls = -1;
  const bool all_gemm = !strcmp(kernel_class, "gemm");       // the whole family: the four per-layer projections + the rest
  for (int i = 0; i < PC_COUNT; ++i)
    if (!strcmp(names[i], kernel_class)) cls = i;
  if (cls < 0 && !all_gemm) return fail(PG_ERR_INVALID, std::string("unknown kernel class ") + kernel_class);
  DeviceGuard g(h->e.device);
  PG_HIP(hipStreamSynchronize(h->e.stream));
  double ms = 0;
  int64_t n = 0;
  for (auto& r : h->e.prof.recs)
    if (r.cls == cls || (all_gemm && (r.cls == PC_GEMM || (r.cls >= PC_GEMM_QKV && r.cls <= PC_GEMM_FC2)))) {
      float t = 0;
      PG_HIP(hipEventElapsedTime(&t, r.a, r.b));
      ms += t;
      ++n;
    }
  *total_ms = ms;
  *launches = n;
  return PG_OK;
}

int pg_prof_get_kernels(pg_engine* h, const char* kernel_class, char* buf, int buf_bytes) {
  if (!h || !kernel_class || !buf || buf_bytes < 2) return fail(PG_ERR_INVALID, "pg_prof_get_kernels: null argument");
  static const char* names[PC_COUNT] = {"gemm_other", "attention", "layernorm", "embed", "head", "sample", "gemm_qkv", "gemm_out", "gemm_fc1", "gemm_fc2", "rope"};
  int cls = -1;
  for (int i = 0; i < PC_COUNT; ++i)
    if (!strcmp(names[i], kernel_class)) cls = i;
  if (cls < 0) return fail(PG_ERR_INVALID, std::string("unknown kernel class ") + kernel_class);
  std::vector<std::string> seen;
  for (auto& r : h->e.prof.recs)
    if (r.cls == cls && !r.kernels.empty() && std::find(seen.begin(), seen.end(), r.kernels) == seen.end()) seen.push_back(r.kernels);
  std::string out;
  for (auto& k : seen) out += (out.empty() ? "" : " | ") + k;
  snprintf(buf, (size_t)buf_bytes, "%s", out.c_str());
  return PG_OK;
}

// ---- kernel-level debug entry points ------------------------------------------------------------
namespace {
struct Tmp {
  std::vector<void*> v;
  ~Tmp() { for (void* p : v) (void)hipFree(p); }
  void* get(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 4) != hipSuccess) return nullptr;
    (void)hipMemset(p, 0, bytes ? bytes : 4);
    v.push_back(p);
    return p;
  }
};
int dbg_device(int device) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(PG_ERR_NO_DEVICE, "no HIP device visible");
  if (device < 0 || device >= n) return fail(PG_ERR_INVALID, "bad device ordinal");
  PG_HIP(hipSetDevice(device));
  return PG_OK;
}
// device rows in the strict mode's split operand layout (3 d bf16: per group of 32 columns [lo | hi | hi]) -> host fp32 rows
// hi + lo; also checks that the two hi copies agree
int split3_rows_to_host(const bf16_t* c3, float* dst, int64_t M, int d) {
  PG_HIP(hipDeviceSynchronize());
  std::vector<bf16_t> h((size_t)M * 3 * d);
  PG_HIP(hipMemcpy(h.data(), c3, h.size() * 2, hipMemcpyDeviceToHost));
  for (int64_t r = 0; r < M; ++r)
    for (int c = 0; c < d; ++c) {
      const size_t g = (size_t)r * 3 * d + (size_t)(c >> 5) * 96 + (c & 31);
      const bf16_t lo = h[g], hi = h[g + 32], hi2 = h[g + 64];
      if (hi != hi2) return fail(PG_ERR_HIP, "split operand row: the two hi copies differ");
      dst[(size_t)r * d + c] = bf16_to_f32(hi) + bf16_to_f32(lo);
    }
  return PG_OK;
}
}  // namespace

int pg_dbg_gemm(int device, int precision, const float* x, const float* w, const float* bias, float* out, int M, int N,
                int K, int epi) {
  if (precision != PG_PREC_BF16 && precision != PG_PREC_FP32 && precision != PG_PREC_F16) return fail(PG_ERR_INVALID, "unknown precision mode");
  if (!x || !w || !bias || !out || M < 1 || N % 64 || K % 64) return fail(PG_ERR_INVALID, "pg_dbg_gemm: bad argument");
  DeviceGuard g(-1);
  int rc = dbg_device(device);
  if (rc) return rc;
  const int Mp = round_up(M, kRowPad);
  const int ks = precision == PG_PREC_FP32 ? 3 : 1;      // strict mode: K-concatenated split-bf16 operands (engine.h dense3)
  Tmp t;
  float* dx = (float*)t.get((size_t)Mp * K * 4);
  float* dw = (float*)t.get((size_t)N * K * 4);
  float* db = (float*)t.get((size_t)N * 4);
  float* dout = (float*)t.get((size_t)Mp * N * 4);
  bf16_t* bx = (bf16_t*)t.get((size_t)Mp * K * 2 * ks);
  bf16_t* bw = (bf16_t*)t.get((size_t)N * K * 2 * ks);
  if (!dx || !dw || !db || !dout || !bx || !bw) return fail(PG_ERR_HIP, "hipMalloc failed");
  PG_HIP(hipMemcpy(dx, x, (size_t)M * K * 4, hipMemcpyHostToDevice));
  PG_HIP(hipMemcpy(dw, w, (size_t)N * K * 4, hipMemcpyHostToDevice));
  PG_HIP(hipMemcpy(db, bias, (size_t)N * 4, hipMemcpyHostToDevice));
  if (precision == PG_PREC_FP32) {
    if (epi == 5) {      // fc1's fused epilogue: operand rows [lo | hi | hi] of gelu(x w^T + b); returned as hi + lo
      if (N % 256) return fail(PG_ERR_INVALID, "pg_dbg_gemm: the fused GELU-and-split epilogue needs N a multiple of 256");
      bf16_t* o3 = (bf16_t*)t.get((size_t)Mp * 3 * N * 2);
      if (!o3) return fail(PG_ERR_HIP, "hipMalloc failed");
      if ((rc = launch_split3_bf16(nullptr, dx, bx, Mp, K, 1.f, false, false))) return rc;
      if ((rc = launch_split3_bf16(nullptr, dw, bw, N, K, 1.f, false, true))) return rc;
      if ((rc = launch_gemm_split3(nullptr, bx, bw, db, o3, Mp, N, K, 3 * N, EPI_SPLIT3_GELU))) return rc;
      return split3_rows_to_host(o3, out, M, N);
    }
    if (epi != 0 && epi != 2) return fail(PG_ERR_UNSUPPORTED, "strict mode: plain (0), residual (2) and fused GELU-split (5) epilogues only");
    if ((rc = launch_split3_bf16(nullptr, dx, bx, Mp, K, 1.f, false, false))) return rc;
    if ((rc = launch_split3_bf16(nullptr, dw, bw, N, K, 1.f, false, true))) return rc;
    if (epi == 2) PG_HIP(hipMemcpy(dout, out, (size_t)M * N * 4, hipMemcpyHostToDevice));
    if ((rc = launch_gemm_split3(nullptr, bx, bw, db, dout, Mp, N, K, N, epi == 2 ? EPI_F32_RESID : EPI_F32))) return rc;
    PG_HIP(hipDeviceSynchronize());
    PG_HIP(hipMemcpy(out, dout, (size_t)M * N * 4, hipMemcpyDeviceToHost));
    return PG_OK;
  }
  if ((rc = OPS(launch_f32_to_bf16, nullptr, dx, bx, (int64_t)Mp * K, 1.f))) return rc;
  if ((rc = OPS(launch_f32_to_bf16, nullptr, dw, bw, (int64_t)N * K, 1.f))) return rc;
  if (epi == 2) PG_HIP(hipMemcpy(dout, out, (size_t)M * N * 4, hipMemcpyHostToDevice));     // residual variant: out += x w^T + b
  if (epi == 3 || epi == 4) {                       // bf16 outputs (the QKV / fc1 epilogues), widened to fp32 for the caller
    bf16_t* bout = (bf16_t*)t.get((size_t)Mp * N * 2);
    if (!bout) return fail(PG_ERR_HIP, "hipMalloc failed");
    if ((rc = OPS(launch_gemm_bf16, nullptr, bx, bw, db, bout, M <= 256 ? round_up(M, 16) : Mp, N, K, K, K, N,
                      epi == 4 ? EPI_BF16_GELU : EPI_BF16, nullptr, 0, M))) return rc;
    if ((rc = OPS(launch_bf16_to_f32, nullptr, bout, dout, (int64_t)M * N))) return rc;
  } else {
    // the residual variant gets split-K scratch, as the engine gives its fc2 GEMMs (taken for deep K and few tiles)
    const size_t ws_bytes = epi == 2 ? OPS(gemm_splitk_ws_bytes, Mp, N, K) : 0;
    float* ws = ws_bytes && ws_bytes <= ((size_t)1 << 30) ? (float*)t.get(ws_bytes) : nullptr;
    if ((rc = OPS(launch_gemm_bf16, nullptr, bx, bw, db, dout, M <= 256 ? round_up(M, 16) : Mp, N, K, K, K, N,
                      epi == 2 ? EPI_F32_RESID : (epi ? EPI_F32_GELU : EPI_F32), ws, ws ? ws_bytes : 0, M))) return rc;
  }
  PG_HIP(hipDeviceSynchronize());
  PG_HIP(hipMemcpy(out, dout, (size_t)M * N * 4, hipMemcpyDeviceToHost));
  return PG_OK;
}

int pg_dbg_gemm_bench(int device, int M, int N, int K, int epi, int variant, int iters, double* avg_ms) {
  if (!avg_ms || M % 16 || (M > 256 && M % 64) || N % 64 || K % 64 || iters < 1) return fail(PG_ERR_INVALID, "pg_dbg_gemm_bench: bad argument");
  DeviceGuard g(-1);
  int rc = dbg_device(device);
  if (rc) return rc;
  Tmp t;
  float* f = (float*)t.get((size_t)(M > N ? M : N) * K * 4);
  bf16_t* bx = (bf16_t*)t.get((size_t)round_up(M, kRowPad) * K * 2);   // kernels may touch the padding rows of the last tile
  bf16_t* bw = (bf16_t*)t.get((size_t)N * K * 2);
  float* db = (float*)t.get((size_t)N * 4);
  void* dout = t.get((size_t)round_up(M, kRowPad) * N * 4);
  if (!f || !bx || !bw || !db || !dout) return fail(PG_ERR_HIP, "hipMalloc failed");
  const size_t ws_bytes = (epi == EPI_F32_RESID && M <= 8192) ? gemm_splitk_ws_bytes(M, N, K) : 0;
  float* ws = ws_bytes ? (float*)t.get(ws_bytes) : nullptr;
  std::vector<float> h((size_t)(M > N ? M : N) * K);
  uint32_t st = 12345u;
  for (auto& v : h) { st = st * 1664525u + 1013904223u; v = ((st >> 8) * (1.0f / 8388608.0f) - 1.0f); }   // uniform [-1,1)
  PG_HIP(hipMemcpy(f, h.data(), h.size() * 4, hipMemcpyHostToDevice));
  if ((rc = launch_f32_to_bf16(nullptr, f, bx, (int64_t)M * K, 1.f))) return rc;
  if ((rc = launch_f32_to_bf16(nullptr, f, bw, (int64_t)N * K, 0.05f))) return rc;
  hipEvent_t a, b;
  PG_HIP(hipEventCreate(&a));
  PG_HIP(hipEventCreate(&b));
  // variant 90: the strict mode's fused three-product kernel on operands of logical depth K / 3 (K = 3 x depth, as the plain
  // kernels see them), so that "variant 2, K" and "variant 90, K" time the same arithmetic
  auto launch = [&]() {
    if (variant == 90) return launch_gemm_split3_w16(nullptr, bx, bw, db, dout, M, N, K / 3, N, epi);
    return launch_gemm_bf16_variant(nullptr, bx, bw, db, dout, M, N, K, K, K, N, epi, variant, ws, ws ? ws_bytes : 0);
  };
  if (variant == 90 && (K % 96 || (epi != EPI_F32 && epi != EPI_F32_RESID))) return fail(PG_ERR_INVALID, "variant 90: K = 3 x depth, fp32 epilogues");
  for (int i = 0; i < 2; ++i)
    if ((rc = launch())) return rc;
  PG_HIP(hipEventRecord(a, nullptr));
  for (int i = 0; i < iters; ++i)
    if ((rc = launch())) return rc;
  PG_HIP(hipEventRecord(b, nullptr));
  PG_HIP(hipEventSynchronize(b));
  float ms = 0;
  PG_HIP(hipEventElapsedTime(&ms, a, b));
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  *avg_ms = ms / iters;
  return PG_OK;
}

int pg_dbg_gemm_plan(int M, int N, int K, int epi, int variant, int have_ws, int m_live, int n_cu, char* buf, int buf_bytes) {
  if (!buf || buf_bytes < 2 || M < 1 || N < 1 || K < 1 || n_cu < 1) return fail(PG_ERR_INVALID, "pg_dbg_gemm_plan: bad argument");
  std::string text;
  gemm_plan_text(M, N, K, epi, variant, have_ws != 0, m_live, n_cu, &text);
  snprintf(buf, (size_t)buf_bytes, "%s", text.c_str());
  return PG_OK;
}

int pg_dbg_attention_plan(int kind, int precision, int64_t n_seq_or_B, int T_or_C, int R, int H, int head_dim, int has_pad, int has_bias,
                          int row_step, int order_bh, int n_cu, char* buf, int buf_bytes) {
  if (precision != PG_PREC_BF16 && precision != PG_PREC_FP32 && precision != PG_PREC_F16) return fail(PG_ERR_INVALID, "unknown precision mode");
  if (!buf || buf_bytes < 2 || (kind != 0 && kind != 1) || n_seq_or_B < 1 || H < 1 || n_cu < 1 || (kind == 1 && (R < 1 || n_seq_or_B > 0x7fffffff)))
    return fail(PG_ERR_INVALID, "pg_dbg_attention_plan: bad argument");
  const bool strict = precision == PG_PREC_FP32;
  std::string text;
  if (kind == 0 && strict) attention_f32_plan_text(n_seq_or_B, T_or_C, H, head_dim, has_pad != 0, has_bias != 0, row_step, &text);
  else if (kind == 0) attention_plan_text(n_seq_or_B, T_or_C, H, head_dim, has_pad != 0, has_bias != 0, row_step, n_cu, &text);
  else if (strict) msa_row_f32_plan_text((int)n_seq_or_B, R, T_or_C, H, has_pad != 0, &text);
  else msa_row_plan_text((int)n_seq_or_B, R, T_or_C, H, order_bh, &text);
  snprintf(buf, (size_t)buf_bytes, "%s", text.c_str());
  return PG_OK;
}

// round 6: the full-row out-projection + LayerNorm kernel (gemm_rowln.hip) against the two launches it replaces, on synthetic operands
// of d_model = 768: ms[0] fused kernel, ms[1] its main loop alone, ms[2] four half-steps + its epilogue, ms[3] residual GEMM on
// 256-column tiles (default dispatch), ms[4] LayerNorm kernel; max_diff = max |h fused - h unfused| over the 16-bit rows (0: bit-identical).
int pg_dbg_rowln_bench(int device, int M, int K, int iters, double* ms, double* max_diff) {
  if (!ms || M < 256 || K % 64 || K < 128 || iters < 1) return fail(PG_ERR_INVALID, "pg_dbg_rowln_bench: bad argument");
  DeviceGuard g(-1);
  int rc = dbg_device(device);
  if (rc) return rc;
  const int N = 768, Mp = round_up(M, kRowPad);
  Tmp t;
  float* f = (float*)t.get((size_t)std::max(Mp, N) * std::max(K, N) * 4);
  bf16_t* ba = (bf16_t*)t.get((size_t)Mp * K * 2);
  bf16_t* bw = (bf16_t*)t.get((size_t)N * K * 2);
  float* db = (float*)t.get((size_t)N * 4 * 3);
  float* x0 = (float*)t.get((size_t)Mp * N * 4);
  float* x1 = (float*)t.get((size_t)Mp * N * 4);
  float* x2 = (float*)t.get((size_t)Mp * N * 4);
  bf16_t* h1 = (bf16_t*)t.get((size_t)Mp * N * 2);
  bf16_t* h2 = (bf16_t*)t.get((size_t)Mp * N * 2);
  if (!f || !ba || !bw || !db || !x0 || !x1 || !x2 || !h1 || !h2) return fail(PG_ERR_HIP, "hipMalloc failed");
  std::vector<float> hbuf((size_t)std::max(Mp, N) * std::max(K, N));
  uint32_t st = 4242u;
  for (auto& v : hbuf) { st = st * 1664525u + 1013904223u; v = ((st >> 8) * (1.0f / 8388608.0f) - 1.0f); }
  PG_HIP(hipMemcpy(f, hbuf.data(), hbuf.size() * 4, hipMemcpyHostToDevice));
  if ((rc = launch_f32_to_bf16(nullptr, f, ba, (int64_t)Mp * K, 1.f))) return rc;
  if ((rc = launch_f32_to_bf16(nullptr, f + 977, bw, (int64_t)N * K, 0.05f))) return rc;
  PG_HIP(hipMemcpy(db, hbuf.data() + 31, (size_t)N * 4 * 3, hipMemcpyHostToDevice));       // bias | gamma | beta
  PG_HIP(hipMemcpy(x0, hbuf.data() + 5, (size_t)Mp * N * 4, hipMemcpyHostToDevice));
  const float *gam = db + N, *bet = db + 2 * N;
  hipEvent_t a, b;
  PG_HIP(hipEventCreate(&a));
  PG_HIP(hipEventCreate(&b));
  auto timeit = [&](auto&& fn, double* out) -> int {
    int r;
    for (int i = 0; i < 2; ++i) if ((r = fn())) return r;
    PG_HIP(hipEventRecord(a, nullptr));
    for (int i = 0; i < iters; ++i) if ((r = fn())) return r;
    PG_HIP(hipEventRecord(b, nullptr));
    PG_HIP(hipEventSynchronize(b));
    float e = 0;
    PG_HIP(hipEventElapsedTime(&e, a, b));
    *out = e / iters;
    return 0;
  };
  // correctness first: one application of each path to the same x
  PG_HIP(hipMemcpy(x1, x0, (size_t)Mp * N * 4, hipMemcpyDeviceToDevice));
  PG_HIP(hipMemcpy(x2, x0, (size_t)Mp * N * 4, hipMemcpyDeviceToDevice));
  if ((rc = launch_gemm_rowln(nullptr, ba, bw, db, x1, gam, bet, h1, M, Mp, K, K, K, 1e-5f))) return rc;
  if ((rc = launch_gemm_bf16(nullptr, ba, bw, db, x2, Mp, N, K, K, K, N, EPI_F32_RESID, nullptr, 0, M))) return rc;
  if ((rc = launch_layernorm_bf16(nullptr, x2, gam, bet, h2, M, N, 1e-5f))) return rc;
  PG_HIP(hipDeviceSynchronize());
  if (max_diff) {
    std::vector<uint16_t> c1((size_t)M * N), c2((size_t)M * N);
    std::vector<float> y1((size_t)M * N), y2((size_t)M * N);
    PG_HIP(hipMemcpy(c1.data(), h1, c1.size() * 2, hipMemcpyDeviceToHost));
    PG_HIP(hipMemcpy(c2.data(), h2, c2.size() * 2, hipMemcpyDeviceToHost));
    PG_HIP(hipMemcpy(y1.data(), x1, y1.size() * 4, hipMemcpyDeviceToHost));
    PG_HIP(hipMemcpy(y2.data(), x2, y2.size() * 4, hipMemcpyDeviceToHost));
    double md = 0;
    for (size_t i = 0; i < c1.size(); ++i) {
      if (c1[i] != c2[i]) md = std::max(md, 1.0 + std::fabs((double)bf16_to_f32(c1[i]) - (double)bf16_to_f32(c2[i])));
      if (memcmp(&y1[i], &y2[i], 4)) md = std::max(md, 2.0 + std::fabs((double)y1[i] - (double)y2[i]));
    }
    *max_diff = md;
  }
  if ((rc = timeit([&] { return launch_gemm_rowln(nullptr, ba, bw, db, x1, gam, bet, h1, M, Mp, K, K, K, 1e-5f); }, ms + 0))) return rc;
  if ((rc = timeit([&] { return launch_gemm_rowln(nullptr, ba, bw, db, x1, gam, bet, h1, M, Mp, K, K, K, 1e-5f, 0, 0, 1); }, ms + 1))) return rc;
  if ((rc = timeit([&] { return launch_gemm_rowln(nullptr, ba, bw, db, x1, gam, bet, h1, M, Mp, K, K, K, 1e-5f, 0, 0, 2); }, ms + 2))) return rc;
  if (const char* e = getenv("PGIBBS_ROWLN_BENCH_ABL")) {      // timing ablation of the epilogue in place of ms[2]
    const int abl = atoi(e);
    if ((rc = timeit([&] { return launch_gemm_rowln(nullptr, ba, bw, db, x1, gam, bet, h1, M, Mp, K, K, K, 1e-5f, 0, 0, abl); }, ms + 2))) return rc;
  }
  if ((rc = timeit([&] { return launch_gemm_bf16(nullptr, ba, bw, db, x2, Mp, N, K, K, K, N, EPI_F32_RESID, nullptr, 0, M); }, ms + 3))) return rc;
  if ((rc = timeit([&] { return launch_layernorm_bf16(nullptr, x2, gam, bet, h2, M, N, 1e-5f); }, ms + 4))) return rc;
  (void)hipEventDestroy(a);
  (void)hipEventDestroy(b);
  return PG_OK;
}

// round 5 ablation ("QKV projection fused with attention for ESM-1b"): the fused kernel that exists --
// gemm_colattn_kernel<16> with one "column" per chain IS projection + attention of whole sequences of T = 256 tokens, one head per
// 256 x 192 tile, the fusion's best case (16 query blocks on 16 waves, no 17th block, no padded rows) -- against the two launches it
// would replace (QKV projection with 256 x 256 tiles, attention_kernel) on the same operands.  ms[0] fused, ms[1] projection,
// ms[2] attention; max_diff = max |ctx fused - ctx unfused| (0: the paths are bit-identical).
int pg_dbg_qkv_attention_bench(int device, int B, int T, int H, int iters, double* ms, double* max_diff) {
  if (!ms || B < 1 || H < 1 || iters < 1 || !(T == 32 || T == 64 || T == 128 || T == 256))
    return fail(PG_ERR_INVALID, "pg_dbg_qkv_attention_bench: T must be 32, 64, 128 or 256");
  DeviceGuard g(-1);
  int rc = dbg_device(device);
  if (rc) return rc;
  const int d = H * 64;
  const int64_t M = (int64_t)B * T, Mp = round_up64(M, kRowPad);
  Tmp t;
  float* f = (float*)t.get((size_t)Mp * d * 4);
  bf16_t* bx = (bf16_t*)t.get((size_t)Mp * d * 2);
  bf16_t* bw = (bf16_t*)t.get((size_t)3 * d * d * 2);
  bf16_t* bwh = (bf16_t*)t.get((size_t)3 * d * d * 2);
  float* db = (float*)t.get((size_t)3 * d * 4);
  float* dbh = (float*)t.get((size_t)3 * d * 4);
  bf16_t* qkv = (bf16_t*)t.get((size_t)Mp * 3 * d * 2);
  bf16_t* c1 = (bf16_t*)t.get((size_t)Mp * d * 2);
  bf16_t* c2 = (bf16_t*)t.get((size_t)Mp * d * 2);
  if (!f || !bx || !bw || !bwh || !db || !dbh || !qkv || !c1 || !c2) return fail(PG_ERR_HIP, "hipMalloc failed");
  std::vector<float> h((size_t)std::max<int64_t>(Mp, 3 * d) * d);
  uint32_t st = 777u;
  for (auto& v : h) { st = st * 1664525u + 1013904223u; v = ((st >> 8) * (1.0f / 8388608.0f) - 1.0f); }
  PG_HIP(hipMemcpy(f, h.data(), (size_t)Mp * d * 4, hipMemcpyHostToDevice));
  if ((rc = launch_f32_to_bf16(nullptr, f, bx, Mp * d, 1.f))) return rc;
  PG_HIP(hipMemcpy(f, h.data(), (size_t)3 * d * d * 4, hipMemcpyHostToDevice));
  if ((rc = launch_f32_to_bf16(nullptr, f, bw, (int64_t)3 * d * d, 0.03f))) return rc;
  PG_HIP(hipMemcpy(db, h.data(), (size_t)3 * d * 4, hipMemcpyHostToDevice));
  if ((rc = launch_headmajor_qkv(nullptr, bw, db, bwh, dbh, H, d))) return rc;
  PG_HIP(hipMemset(c1, 0, (size_t)Mp * d * 2));
  PG_HIP(hipMemset(c2, 0, (size_t)Mp * d * 2));
  hipEvent_t ev[2];
  PG_HIP(hipEventCreate(&ev[0]));
  PG_HIP(hipEventCreate(&ev[1]));
  auto fused = [&] { return launch_gemm_colattn(nullptr, bx, bwh, dbh, c1, B, T, 1, H, d, d); };
  auto proj = [&] { return launch_gemm_bf16(nullptr, bx, bw, db, qkv, (int)Mp, 3 * d, d, d, d, 3 * d, EPI_BF16); };
  auto attn = [&] { return launch_attention_bf16(nullptr, qkv, c2, B, T, H, 3 * d, d, d, 2 * d); };
  auto time_it = [&](auto&& fn, double* out) -> int {
    int r;
    for (int i = 0; i < 2; ++i)
      if ((r = fn())) return r;
    PG_HIP(hipEventRecord(ev[0], nullptr));
    for (int i = 0; i < iters; ++i)
      if ((r = fn())) return r;
    PG_HIP(hipEventRecord(ev[1], nullptr));
    PG_HIP(hipEventSynchronize(ev[1]));
    float e = 0;
    PG_HIP(hipEventElapsedTime(&e, ev[0], ev[1]));
    *out = e / iters;
    return PG_OK;
  };
  if ((rc = time_it(fused, ms + 0)) || (rc = time_it(proj, ms + 1)) || (rc = time_it(attn, ms + 2))) return rc;
  (void)hipEventDestroy(ev[0]);
  (void)hipEventDestroy(ev[1]);
  if (max_diff) {
    std::vector<uint16_t> a((size_t)M * d), b((size_t)M * d);
    PG_HIP(hipMemcpy(a.data(), c1, a.size() * 2, hipMemcpyDeviceToHost));
    PG_HIP(hipMemcpy(b.data(), c2, b.size() * 2, hipMemcpyDeviceToHost));
    double worst = 0;
    for (size_t i = 0; i < a.size(); ++i) {
      uint32_t ua = (uint32_t)a[i] << 16, ub = (uint32_t)b[i] << 16;
      float fa, fb;
      memcpy(&fa, &ua, 4);
      memcpy(&fb, &ub, 4);
      worst = std::max(worst, (double)fabsf(fa - fb));
    }
    *max_diff = worst;
  }
  return PG_OK;
}

int pg_dbg_layernorm(int device, const float* x, const float* gamma, const float* beta, float* y, int M, int d, float eps) {
  if (!x || !gamma || !beta || !y || M < 1 || d < 4) return fail(PG_ERR_INVALID, "pg_dbg_layernorm: bad argument");
  DeviceGuard g(-1);
  int rc = dbg_device(device);
  if (rc) return rc;
  Tmp t;
  float* dx = (float*)t.get((size_t)M * d * 4);
  float* dg = (float*)t.get((size_t)d * 4);
  float* dbt = (float*)t.get((size_t)d * 4);
  float* dy = (float*)t.get((size_t)M * d * 4);
  if (!dx || !dg || !dbt || !dy) return fail(PG_ERR_HIP, "hipMalloc failed");
  PG_HIP(hipMemcpy(dx, x, (size_t)M * d * 4, hipMemcpyHostToDevice));
  PG_HIP(hipMemcpy(dg, gamma, (size_t)d * 4, hipMemcpyHostToDevice));
  PG_HIP(hipMemcpy(dbt, beta, (size_t)d * 4, hipMemcpyHostToDevice));
  if ((rc = launch_layernorm_f32(nullptr, dx, dg, dbt, dy, M, d, eps))) return rc;
  PG_HIP(hipDeviceSynchronize());
  PG_HIP(hipMemcpy(y, dy, (size_t)M * d * 4, hipMemcpyDeviceToHost));
  return PG_OK;
}

int pg_dbg_attention(int device, int precision, const float* qkv, float* ctx, int B, int T, int H) {
  return pg_dbg_attention_hd(device, precision, qkv, ctx, B, T, H, 64, nullptr, -1);
}

/* pg_dbg_attention with the head dimension (64 or 32) and, optionally, the tokens of the keys: key_tok[B][T], keys whose token is
 * pad_idx are masked as in a ragged batch (NULL: none) */
int pg_dbg_attention_hd(int device, int precision, const float* qkv, float* ctx, int B, int T, int H, int head_dim,
                        const int32_t* key_tok, int pad_idx) {
  return pg_dbg_attention_kv(device, precision, qkv, ctx, B, T, H, head_dim, key_tok, pad_idx, nullptr, nullptr, nullptr, 0);
}

namespace {
// what a debug entry's launches recorded (note_kernel), into the caller's buffer
void dbg_noted_text(char* plan, int plan_bytes) {
  if (plan && plan_bytes > 0) snprintf(plan, (size_t)plan_bytes, "%s", noted_kernels().c_str());
}
}  // namespace

/* pg_dbg_attention_hd with ESM-1's bias key: bias_k / bias_v [H][head_dim] fp32 (both or neither), laid out as the engine lays them
 * out -- [bias_k | bias_v], k of head h at h*HD, v at (H + h)*HD -- in the operand type of `precision` (fp32 for the strict
 * kernels).  Everything is checked on the host before a device is looked for.  plan (may be NULL): the text the launch recorded */
int pg_dbg_attention_kv(int device, int precision, const float* qkv, float* ctx, int B, int T, int H, int head_dim,
                        const int32_t* key_tok, int pad_idx, const float* bias_k, const float* bias_v, char* plan, int plan_bytes) {
  if (plan && plan_bytes > 0) plan[0] = 0;
  if (precision != PG_PREC_BF16 && precision != PG_PREC_FP32 && precision != PG_PREC_F16) return fail(PG_ERR_INVALID, "unknown precision mode");
  if (!qkv || !ctx || B < 1 || T < 1 || H < 1 || (plan && plan_bytes < 1)) return fail(PG_ERR_INVALID, "pg_dbg_attention: bad argument");
  if (head_dim != 64 && head_dim != 32) return fail(PG_ERR_INVALID, "pg_dbg_attention_hd: head_dim must be 64 or 32");
  if (!bias_k != !bias_v) return fail(PG_ERR_INVALID, "pg_dbg_attention_kv: bias_k and bias_v come together or not at all");
  const std::string head_err = attention_head_error(head_dim, bias_k != nullptr);      // the plans' own refusal of a bias key at head 32
  if (!head_err.empty()) return fail(PG_ERR_INVALID, head_err);
  if ((double)B * T * 3 * H * head_dim > 2147483647.0) return fail(PG_ERR_INVALID, "pg_dbg_attention: more than 2^31 - 1 qkv values");
  DeviceGuard g(-1);
  int rc = dbg_device(device);
  if (rc) return rc;
  const int d = H * head_dim;
  const int64_t M = (int64_t)B * T;
  Tmp t;
  float* dq = (float*)t.get((size_t)M * 3 * d * 4);
  int32_t* dtok = nullptr;
  if (key_tok) {
    dtok = (int32_t*)t.get((size_t)M * 4);
    if (!dtok) return fail(PG_ERR_HIP, "hipMalloc failed");
    PG_HIP(hipMemcpy(dtok, key_tok, (size_t)M * 4, hipMemcpyHostToDevice));
  }
  float* bias32 = nullptr;      // [bias_k | bias_v], d fp32 each
  if (bias_k) {
    bias32 = (float*)t.get((size_t)2 * d * 4);
    if (!bias32) return fail(PG_ERR_HIP, "hipMalloc failed");
    PG_HIP(hipMemcpy(bias32, bias_k, (size_t)d * 4, hipMemcpyHostToDevice));
    PG_HIP(hipMemcpy(bias32 + d, bias_v, (size_t)d * 4, hipMemcpyHostToDevice));
  }
  clear_noted_kernels();
  if (precision == PG_PREC_FP32) {
    bf16_t* c3 = (bf16_t*)t.get((size_t)M * 3 * d * 2);
    if (!dq || !c3) return fail(PG_ERR_HIP, "hipMalloc failed");
    PG_HIP(hipMemcpy(dq, qkv, (size_t)M * 3 * d * 4, hipMemcpyHostToDevice));
    const SeqLayout chain = {1, T, 0, 1};
    if ((rc = launch_attention_f32(nullptr, dq, c3, d, B, T, H, 3 * d, 3 * d, d, 2 * d, chain, dtok, pad_idx, bias32, head_dim))) return rc;
    dbg_noted_text(plan, plan_bytes);
    return split3_rows_to_host(c3, ctx, M, d);
  }
  bf16_t* bq = (bf16_t*)t.get((size_t)M * 3 * d * 2);
  bf16_t* bc = (bf16_t*)t.get((size_t)M * d * 2);
  float* dc = (float*)t.get((size_t)M * d * 4);
  bf16_t* bias16 = bias_k ? (bf16_t*)t.get((size_t)2 * d * 2) : nullptr;
  if (!dq || !bq || !bc || !dc || (bias_k && !bias16)) return fail(PG_ERR_HIP, "hipMalloc failed");
  PG_HIP(hipMemcpy(dq, qkv, (size_t)M * 3 * d * 4, hipMemcpyHostToDevice));
  if ((rc = OPS(launch_f32_to_bf16, nullptr, dq, bq, M * 3 * d, 1.f))) return rc;
  if (bias_k && (rc = OPS(launch_f32_to_bf16, nullptr, bias32, bias16, 2 * d, 1.f))) return rc;
  if ((rc = OPS(launch_attention_bf16, nullptr, bq, bc, B, T, H, 3 * d, d, d, 2 * d, dtok, pad_idx, bias16, head_dim))) return rc;
  dbg_noted_text(plan, plan_bytes);
  if ((rc = OPS(launch_bf16_to_f32, nullptr, bc, dc, M * d))) return rc;
  PG_HIP(hipDeviceSynchronize());
  PG_HIP(hipMemcpy(ctx, dc, (size_t)M * d * 4, hipMemcpyDeviceToHost));
  return PG_OK;
}

/* LayerNorm as the engine's GEMMs read it: the operand rows launch_layernorm_bf16 writes in `precision`, widened to fp32 --
 * bf16 or fp16 rows, or (PG_PREC_FP32) the strict mode's split rows [lo | hi | hi] returned as hi + lo, the two hi copies checked */
int pg_dbg_layernorm_operand(int device, int precision, const float* x, const float* gamma, const float* beta, float* y, int M, int d,
                             float eps) {
  if (precision != PG_PREC_BF16 && precision != PG_PREC_FP32 && precision != PG_PREC_F16) return fail(PG_ERR_INVALID, "unknown precision mode");
  if (!x || !gamma || !beta || !y || M < 1 || d < 32 || d % 32) return fail(PG_ERR_INVALID, "pg_dbg_layernorm_operand: bad argument");
  DeviceGuard g(-1);
  int rc = dbg_device(device);
  if (rc) return rc;
  const bool split = precision == PG_PREC_FP32;
  Tmp t;
  float* dx = (float*)t.get((size_t)M * d * 4);
  float* dg = (float*)t.get((size_t)d * 4);
  float* dbt = (float*)t.get((size_t)d * 4);
  float* dy = (float*)t.get((size_t)M * d * 4);
  bf16_t* h = (bf16_t*)t.get((size_t)M * d * 2 * (split ? 3 : 1));
  if (!dx || !dg || !dbt || !dy || !h) return fail(PG_ERR_HIP, "hipMalloc failed");
  PG_HIP(hipMemcpy(dx, x, (size_t)M * d * 4, hipMemcpyHostToDevice));
  PG_HIP(hipMemcpy(dg, gamma, (size_t)d * 4, hipMemcpyHostToDevice));
  PG_HIP(hipMemcpy(dbt, beta, (size_t)d * 4, hipMemcpyHostToDevice));
  if ((rc = OPS(launch_layernorm_bf16, nullptr, dx, dg, dbt, h, M, d, eps, split, 0, 0, true))) return rc;
  if (split) return split3_rows_to_host(h, y, M, d);
  if ((rc = OPS(launch_bf16_to_f32, nullptr, h, dy, (int64_t)M * d))) return rc;
  PG_HIP(hipDeviceSynchronize());
  PG_HIP(hipMemcpy(y, dy, (size_t)M * d * 4, hipMemcpyDeviceToHost));
  return PG_OK;
}

/* ESM-2's rotary embedding on a host fp32 buffer qkv[B*T][3*H*64]: the q and k thirds rotated in place (row r at position r % T),
 * v left alone.  16-bit modes: through a device buffer of that type, the result widened back */
int pg_dbg_rope(int device, int precision, float* qkv, int B, int T, int H) {
  return pg_dbg_rope_hd(device, precision, qkv, B, T, H, 64);
}

/* pg_dbg_rope with the head dimension: 64 (H <= 40) or 32 (H <= 32) */
int pg_dbg_rope_hd(int device, int precision, float* qkv, int B, int T, int H, int head_dim) {
  if (precision != PG_PREC_BF16 && precision != PG_PREC_FP32 && precision != PG_PREC_F16) return fail(PG_ERR_INVALID, "unknown precision mode");
  if (head_dim != 64 && head_dim != 32) return fail(PG_ERR_INVALID, "pg_dbg_rope_hd: head_dim must be 64 or 32");
  if (!qkv || B < 1 || T < 1 || H < 1 || H > (head_dim == 64 ? 40 : 32)) return fail(PG_ERR_INVALID, "pg_dbg_rope: bad argument");
  DeviceGuard g(-1);
  int rc = dbg_device(device);
  if (rc) return rc;
  const int d = H * head_dim;
  const int64_t M = (int64_t)B * T, n = M * 3 * d;
  const std::vector<float> tab = rope_table(T, head_dim);
  Tmp t;
  float* dq = (float*)t.get((size_t)n * 4);
  float* dtab = (float*)t.get(tab.size() * 4);
  bf16_t* bq = precision == PG_PREC_FP32 ? nullptr : (bf16_t*)t.get((size_t)n * 2);
  if (!dq || !dtab || (precision != PG_PREC_FP32 && !bq)) return fail(PG_ERR_HIP, "hipMalloc failed");
  PG_HIP(hipMemcpy(dq, qkv, (size_t)n * 4, hipMemcpyHostToDevice));
  PG_HIP(hipMemcpy(dtab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  if (precision == PG_PREC_FP32) {
    if ((rc = launch_rope(nullptr, dq, true, dtab, T, M, T, H, 3 * d, head_dim))) return rc;
  } else {
    if ((rc = OPS(launch_f32_to_bf16, nullptr, dq, bq, n, 1.f))) return rc;
    if ((rc = OPS(launch_rope, nullptr, bq, false, dtab, T, M, T, H, 3 * d, head_dim))) return rc;
    if ((rc = OPS(launch_bf16_to_f32, nullptr, bq, dq, n))) return rc;
  }
  PG_HIP(hipDeviceSynchronize());
  PG_HIP(hipMemcpy(qkv, dq, (size_t)n * 4, hipMemcpyDeviceToHost));
  return PG_OK;
}

/* MSA attention blocks on fp32 host buffers qkv[B][R][C][3*H*64] -> ctx[B][R][C][H*64]; which: 0 = tied row attention
 * (scores scaled by `scale`), 1 = column attention (q already scaled); 2 / 3 = the same two in the strict precision mode */
int pg_dbg_msa_attention(int device, int which, const float* qkv, float* ctx, int B, int R, int C, int H, float scale) {
  return pg_dbg_msa_attention_tok(device, which, qkv, ctx, B, R, C, H, scale, nullptr, -1, nullptr, 0);
}

/* pg_dbg_msa_attention with the tokens tok[B][R][C] of a batch that holds <pad> (NULL: none, pg_dbg_msa_attention itself).  Column
 * attention (which 1, 3, 5) hands them to its launcher.  Tied row attention with tokens takes the engine's route for a ragged batch:
 * which 0 widens the bf16 q, k, v to fp32 and runs launch_msa_row_attention_f32 with 16-bit context rows, which 2 is the strict
 * kernel, which 4 (fp16) is refused as the engine refuses it.  Everything is checked on the host before a device is looked for.
 * plan (may be NULL): the text the launches recorded */
int pg_dbg_msa_attention_tok(int device, int which, const float* qkv, float* ctx, int B, int R, int C, int H, float scale,
                             const int32_t* tok, int pad_idx, char* plan, int plan_bytes) {
  if (plan && plan_bytes > 0) plan[0] = 0;
  if (!qkv || !ctx || B < 1 || R < 1 || C < 1 || H < 1 || (plan && plan_bytes < 1)) return fail(PG_ERR_INVALID, "pg_dbg_msa_attention: bad argument");
  if (which < 0 || which > 5) return fail(PG_ERR_INVALID, "pg_dbg_msa_attention: which must be 0 ... 5");
  if ((double)B * R * C * 3 * H * 64 > 2147483647.0) return fail(PG_ERR_INVALID, "pg_dbg_msa_attention: more than 2^31 - 1 qkv values");
  if (tok && which == 4)
    return fail(PG_ERR_UNSUPPORTED, "fp16 precision mode: alignments wider than 576 columns take the split-bf16 row attention, "
                                    "which exists for bf16 operands only -- use precision bf16 or fp32");
  if ((which == 2 || (which == 0 && tok)) && (double)B * H * C * msa_row_scores_ld(C) > 1073741823.0)
    return fail(PG_ERR_INVALID, "pg_dbg_msa_attention: the fp32 score maps of this shape exceed 4 GiB");
  const int precision = (which == 4 || which == 5) ? PG_PREC_F16 : PG_PREC_BF16;      // 4 / 5: which 0 / 1 with fp16 operands
  if (which == 4 || which == 5) which -= 4;
  DeviceGuard g(-1);
  int rc = dbg_device(device);
  if (rc) return rc;
  const int d = H * 64;
  const int64_t M = (int64_t)B * R * C;
  Tmp t;
  float* dq = (float*)t.get((size_t)M * 3 * d * 4);
  int32_t* dtok = nullptr;
  if (tok) {
    dtok = (int32_t*)t.get((size_t)M * 4);
    if (!dtok) return fail(PG_ERR_HIP, "hipMalloc failed");
    PG_HIP(hipMemcpy(dtok, tok, (size_t)M * 4, hipMemcpyHostToDevice));
  }
  clear_noted_kernels();
  if (which == 2 || which == 3) {      // strict precision mode kernels: fp32 in, [lo | hi | hi] operand rows out
    bf16_t* c3 = (bf16_t*)t.get((size_t)M * 3 * d * 2);
    float* sc = which == 2 ? (float*)t.get((size_t)B * H * C * msa_row_scores_ld(C) * 4) : nullptr;
    if (!dq || !c3 || (which == 2 && !sc)) return fail(PG_ERR_HIP, "hipMalloc failed");
    PG_HIP(hipMemcpy(dq, qkv, (size_t)M * 3 * d * 4, hipMemcpyHostToDevice));
    const SeqLayout col = {C, R * C, 1, C};
    if (which == 2) rc = launch_msa_row_attention_f32(nullptr, dq, sc, c3, d, B, R, C, H, 3 * d, 3 * d, d, 2 * d, scale, dtok, pad_idx);
    else rc = launch_attention_f32(nullptr, dq, c3, d, (int64_t)B * C, R, H, 3 * d, 3 * d, d, 2 * d, col, dtok, pad_idx);
    if (rc) return rc;
    dbg_noted_text(plan, plan_bytes);
    return split3_rows_to_host(c3, ctx, M, d);
  }
  bf16_t* bq = (bf16_t*)t.get((size_t)M * 3 * d * 2);
  bf16_t* bc = (bf16_t*)t.get((size_t)M * d * 2);
  float* dc = (float*)t.get((size_t)M * d * 4);
  if (!dq || !bq || !bc || !dc) return fail(PG_ERR_HIP, "hipMalloc failed");
  PG_HIP(hipMemcpy(dq, qkv, (size_t)M * 3 * d * 4, hipMemcpyHostToDevice));
  if ((rc = OPS(launch_f32_to_bf16, nullptr, dq, bq, M * 3 * d, 1.f))) return rc;
  if (which == 0 && tok) {
    // a ragged batch, as Engine::msa_trunk runs it: the 16-bit q, k, v widened to fp32, fp32 scores through a scratch buffer
    float* wide = (float*)t.get((size_t)M * 3 * d * 4);
    float* sc = (float*)t.get((size_t)B * H * C * msa_row_scores_ld(C) * 4);
    if (!wide || !sc) return fail(PG_ERR_HIP, "hipMalloc failed");
    if ((rc = launch_bf16_to_f32(nullptr, bq, wide, M * 3 * d))) return rc;
    if ((rc = launch_msa_row_attention_f32(nullptr, wide, sc, bc, 0, B, R, C, H, 3 * d, d, d, 2 * d, scale, dtok, pad_idx))) return rc;
  } else if (which == 0) {
    // scratch for the split-R mode (taken when B*H*ceil(C/64) < 384 and R >= 8), so the tests exercise both modes
    const size_t pbytes = (size_t)B * H * 16 * C * 576 * 4 + (size_t)B * H * (C / 16 + 9) * 18 * 1024;
    float* part = pbytes <= ((size_t)1 << 30) ? (float*)t.get(pbytes) : nullptr;
    if ((rc = OPS(launch_msa_row_attention_bf16, nullptr, bq, bc, B, R, C, H, 3 * d, d, d, 2 * d, scale, part, part ? pbytes : 0, 0))) return rc;
  } else {
    SeqLayout col = {C, R * C, 1, C};
    if ((rc = OPS(launch_attention_seq_bf16, nullptr, bq, bc, (int64_t)B * C, R, H, 3 * d, d, d, 2 * d, col, dtok, pad_idx))) return rc;
  }
  dbg_noted_text(plan, plan_bytes);
  if ((rc = OPS(launch_bf16_to_f32, nullptr, bc, dc, M * d))) return rc;
  PG_HIP(hipDeviceSynchronize());
  PG_HIP(hipMemcpy(ctx, dc, (size_t)M * d * 4, hipMemcpyDeviceToHost));
  return PG_OK;
}

// ---- the row kernels of elementwise.hip ---------------------------------------------------------------------------------------------
// Every entry below checks its arguments on the host first -- shapes, then every token, position row, row_map entry and gathered
// row the kernel would read against the sizes the caller states -- and only then looks for a device: a wrong array is
// PG_ERR_INVALID with a message, never a GPU fault, and the refusals can be tested without a GPU.
extern "C++" {
namespace {
int dbg_row_width(const char* who, int d) {
  if (d < 4 || d % 4 || d > 2560) return      // row_d_ok of elementwise.hip
    fail(PG_ERR_INVALID, std::string(who) + ": d must be a multiple of 4 and <= 2560");
  return PG_OK;
}
int dbg_prec16(const char* who, int precision) {
  if (precision != PG_PREC_BF16 && precision != PG_PREC_F16) return fail(PG_ERR_INVALID, std::string(who) + ": precision must be PG_PREC_BF16 or PG_PREC_F16");
  return PG_OK;
}
// the token row a gather reads for selected row r (what gather_ln_bf16_kernel / gather_rows_kernel compute), -1 = none (zeros);
// -2 = outside the source (error set)
int64_t dbg_gather_src(const char* who, int64_t r, int32_t pos, bool zero_fill, const int32_t* row_map, int64_t n_map, int P, int width,
                       int64_t src_rows) {
  if (pos < 0 || (pos & 0x3fffffff) >= width) {
    if (zero_fill) return -1;
    pos = 0;
  }
  pos &= 0x3fffffff;
  const int64_t s = r / P;
  if (row_map && s >= n_map) { fail(PG_ERR_INVALID, std::string(who) + ": row_map is shorter than the selected rows need"); return -2; }
  const int64_t row = (row_map ? (int64_t)row_map[s] : s) * width + pos;
  if (row < 0 || row >= src_rows) {
    fail(PG_ERR_INVALID, std::string(who) + ": selected row " + std::to_string(r) + " reads source row " + std::to_string(row) + " of " + std::to_string(src_rows));
    return -2;
  }
  return row;
}
template <typename T>
T* to_device(Tmp& t, const T* host, size_t n) {
  T* p = (T*)t.get(n * sizeof(T));
  if (p && n && hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
  return p;
}
}  // namespace
}  // extern "C++"

int pg_dbg_embed(int device, int precision, const int32_t* tokens, int n_seq, int T, const float* embed, int V, int d, const float* pos,
                 int pos_rows, const float* msa_pos, int rows_per_msa, const float* gamma, const float* beta, const float* gamma2,
                 const float* beta2, int pad_idx, int mask_idx, int token_dropout, float eps, float embed_scale, float* x, uint16_t* h2) {
  int rc = dbg_prec16("pg_dbg_embed", precision);
  if (rc) return rc;
  if (!tokens || !embed || !x || n_seq < 1 || T < 1 || V < 1 || (pos && pos_rows < 1) || rows_per_msa < 0 || (rows_per_msa > 0 && !msa_pos) ||
      !gamma != !beta || !gamma2 != !beta2 || !gamma2 != !h2)
    return fail(PG_ERR_INVALID, "pg_dbg_embed: bad argument");
  if ((rc = dbg_row_width("pg_dbg_embed", d))) return rc;
  const int64_t n_tok = (int64_t)n_seq * T;
  for (int64_t sq = 0; sq < n_seq; ++sq) {
    int n_before = 0;
    for (int t = 0; t < T; ++t) {
      const int32_t tok = tokens[sq * T + t];
      if (tok < 0 || tok >= V)
        return fail(PG_ERR_INVALID, "pg_dbg_embed: token " + std::to_string(tok) + " is outside the embedding table of " + std::to_string(V) + " rows");
      n_before += tok != pad_idx;
      const int p = tok == pad_idx ? pad_idx : n_before + pad_idx;      // embed_ln_kernel's position row
      if (pos && (p < 0 || p >= pos_rows))
        return fail(PG_ERR_INVALID, "pg_dbg_embed: position row " + std::to_string(p) + " is outside the position table of " + std::to_string(pos_rows) + " rows");
    }
  }
  DeviceGuard g(-1);
  if ((rc = dbg_device(device))) return rc;
  Tmp t;
  const int32_t* dtok = to_device(t, tokens, (size_t)n_tok);
  const float* de = to_device(t, embed, (size_t)V * d);
  const float* dp = pos ? to_device(t, pos, (size_t)pos_rows * d) : nullptr;
  const float* dm = rows_per_msa > 0 ? to_device(t, msa_pos, (size_t)rows_per_msa * d) : nullptr;
  const float* dg = gamma ? to_device(t, gamma, (size_t)d) : nullptr;
  const float* db = gamma ? to_device(t, beta, (size_t)d) : nullptr;
  const float* dg2 = gamma2 ? to_device(t, gamma2, (size_t)d) : nullptr;
  const float* db2 = gamma2 ? to_device(t, beta2, (size_t)d) : nullptr;
  float* dx = (float*)t.get((size_t)n_tok * d * 4);
  bf16_t* dh = h2 ? (bf16_t*)t.get((size_t)n_tok * d * 2) : nullptr;
  if (!dtok || !de || (pos && !dp) || (rows_per_msa > 0 && !dm) || (gamma && (!dg || !db)) || (gamma2 && (!dg2 || !db2 || !dh)) || !dx)
    return fail(PG_ERR_HIP, "hipMalloc / copy failed");
  if ((rc = OPS(launch_embed_ln, nullptr, dtok, de, dp, dm, dg, db, dx, n_tok, T, d, pad_idx, mask_idx, token_dropout, rows_per_msa, eps, dg2,
                db2, dh, embed_scale)))
    return rc;
  PG_HIP(hipDeviceSynchronize());
  PG_HIP(hipMemcpy(x, dx, (size_t)n_tok * d * 4, hipMemcpyDeviceToHost));
  if (h2) PG_HIP(hipMemcpy(h2, dh, (size_t)n_tok * d * 2, hipMemcpyDeviceToHost));
  return PG_OK;
}

int pg_dbg_layernorm_rows(int device, int precision, const float* x, const float* gamma, const float* beta, uint16_t* h_inout,
                          int64_t h_rows, int M, int d, float eps, int form, int colmajor_R, int colmajor_C, int* kernel) {
  int rc = dbg_prec16("pg_dbg_layernorm_rows", precision);
  if (rc) return rc;
  if (!x || !gamma || !beta || !h_inout || M < 1 || h_rows < M || form < 0 || form > 2 || colmajor_R < 0 || (colmajor_R > 0 && colmajor_C < 1))
    return fail(PG_ERR_INVALID, "pg_dbg_layernorm_rows: bad argument");
  if (form && (precision != PG_PREC_BF16 || d % 32))
    return fail(PG_ERR_INVALID, "pg_dbg_layernorm_rows: split rows are bf16 pairs in groups of 32 columns");
  if ((rc = OPS(layernorm_bf16_check, M, d, form != 0, colmajor_R, colmajor_C))) return rc;
  DeviceGuard g(-1);
  if ((rc = dbg_device(device))) return rc;
  const size_t h_n = (size_t)h_rows * d * (form ? 3 : 1);
  Tmp t;
  const float* dx = to_device(t, x, (size_t)M * d);
  const float* dg = to_device(t, gamma, (size_t)d);
  const float* db = to_device(t, beta, (size_t)d);
  bf16_t* dh = to_device(t, h_inout, h_n);      // the caller's pattern: what the kernel leaves unwritten keeps it
  if (!dx || !dg || !db || !dh) return fail(PG_ERR_HIP, "hipMalloc / copy failed");
  unsigned stride_grid = 0;
  if (kernel) *kernel = OPS(layernorm_bf16_choice, M, d, colmajor_R, &stride_grid);
  if ((rc = OPS(launch_layernorm_bf16, nullptr, dx, dg, db, dh, M, d, eps, form != 0, colmajor_R, colmajor_C, form != 2))) return rc;
  PG_HIP(hipDeviceSynchronize());
  PG_HIP(hipMemcpy(h_inout, dh, h_n * 2, hipMemcpyDeviceToHost));
  return PG_OK;
}

int pg_dbg_gather_ln(int device, int precision, const float* x, int64_t x_rows, const int32_t* idx, const int32_t* row_map, int64_t n_map,
                     int P, int width, const float* gamma, const float* beta, uint16_t* h_inout, int64_t h_rows, int64_t n_sel, int d,
                     float eps, int split) {
  int rc = dbg_prec16("pg_dbg_gather_ln", precision);
  if (rc) return rc;
  if (!x || !gamma || !beta || !h_inout || x_rows < 1 || n_sel < 1 || h_rows < n_sel || P < 1 || width < 1 || (row_map && n_map < 1) ||
      split < 0 || split > 1)
    return fail(PG_ERR_INVALID, "pg_dbg_gather_ln: bad argument");
  if ((rc = dbg_row_width("pg_dbg_gather_ln", d))) return rc;
  if (split && (precision != PG_PREC_BF16 || d % 32))
    return fail(PG_ERR_INVALID, "pg_dbg_gather_ln: split rows are bf16 pairs in groups of 32 columns");
  if (!idx) {      // identity: selected row r = token row r
    if (n_sel > x_rows) return fail(PG_ERR_INVALID, "pg_dbg_gather_ln: more selected rows than source rows");
  } else {
    for (int64_t r = 0; r < n_sel; ++r)
      if (dbg_gather_src("pg_dbg_gather_ln", r, idx[r], true, row_map, n_map, P, width, x_rows) == -2) return PG_ERR_INVALID;
  }
  DeviceGuard g(-1);
  if ((rc = dbg_device(device))) return rc;
  const size_t h_n = (size_t)h_rows * d * (split ? 3 : 1);
  Tmp t;
  const float* dx = to_device(t, x, (size_t)x_rows * d);
  const int32_t* di = idx ? to_device(t, idx, (size_t)n_sel) : nullptr;
  const int32_t* dm = row_map ? to_device(t, row_map, (size_t)n_map) : nullptr;
  const float* dg = to_device(t, gamma, (size_t)d);
  const float* db = to_device(t, beta, (size_t)d);
  bf16_t* dh = to_device(t, h_inout, h_n);
  if (!dx || (idx && !di) || (row_map && !dm) || !dg || !db || !dh) return fail(PG_ERR_HIP, "hipMalloc / copy failed");
  if ((rc = OPS(launch_gather_ln_bf16, nullptr, dx, di, dm, P, width, dg, db, dh, n_sel, d, eps, split != 0))) return rc;
  PG_HIP(hipDeviceSynchronize());
  PG_HIP(hipMemcpy(h_inout, dh, h_n * 2, hipMemcpyDeviceToHost));
  return PG_OK;
}

int pg_dbg_gather_rows(int device, const void* src, int64_t src_rows, void* dst_inout, int64_t dst_rows, const int32_t* idx, int n_iters,
                       int iter, const int32_t* row_map, int64_t n_map, int P, int width, int64_t n_sel, int row_bytes) {
  if (!src || !dst_inout || !idx || src_rows < 1 || n_sel < 1 || dst_rows < n_sel || P < 1 || width < 1 || (row_map && n_map < 1) ||
      n_iters < 0 || (n_iters > 0 && (iter < 0 || iter >= n_iters)) || row_bytes < 16)
    return fail(PG_ERR_INVALID, "pg_dbg_gather_rows: bad argument");
  if (row_bytes % 16) return fail(PG_ERR_INVALID, "pg_dbg_gather_rows: rows must be multiples of 16 bytes");
  const int32_t* now = idx + (n_iters > 0 ? (size_t)iter * n_sel : 0);      // the table row the kernel reads through d_iter
  for (int64_t r = 0; r < n_sel; ++r)
    if (dbg_gather_src("pg_dbg_gather_rows", r, now[r], false, row_map, n_map, P, width, src_rows) == -2) return PG_ERR_INVALID;
  DeviceGuard g(-1);
  int rc = dbg_device(device);
  if (rc) return rc;
  Tmp t;
  const char* ds = to_device(t, (const char*)src, (size_t)src_rows * row_bytes);
  char* dd = to_device(t, (const char*)dst_inout, (size_t)dst_rows * row_bytes);
  const int32_t* di = to_device(t, idx, (size_t)(n_iters > 0 ? n_iters : 1) * n_sel);
  const int32_t* dm = row_map ? to_device(t, row_map, (size_t)n_map) : nullptr;
  const int32_t it32 = iter;
  const int32_t* dit = n_iters > 0 ? to_device(t, &it32, 1) : nullptr;
  if (!ds || !dd || !di || (row_map && !dm) || (n_iters > 0 && !dit)) return fail(PG_ERR_HIP, "hipMalloc / copy failed");
  if ((rc = launch_gather_rows(nullptr, ds, dd, di, dm, P, width, n_sel, row_bytes, dit))) return rc;
  PG_HIP(hipDeviceSynchronize());
  PG_HIP(hipMemcpy(dst_inout, dd, (size_t)dst_rows * row_bytes, hipMemcpyDeviceToHost));
  return PG_OK;
}

int pg_dbg_lm_tail(int device, const float* g, const float* gamma, const float* beta, const float* embed, const float* out_bias,
                   float* logits, int64_t n, int d, int V, float eps, int* small_kernel) {
  if (!g || !embed || !out_bias || !logits || n < 1 || !gamma != !beta) return fail(PG_ERR_INVALID, "pg_dbg_lm_tail: bad argument");
  if (V < 1 || V > 64) return fail(PG_ERR_INVALID, "pg_dbg_lm_tail: vocab must be in 1..64");
  int rc = dbg_row_width("pg_dbg_lm_tail", d);
  if (rc) return rc;
  DeviceGuard guard(-1);
  if ((rc = dbg_device(device))) return rc;
  Tmp t;
  const float* dg = to_device(t, g, (size_t)n * d);
  const float* dga = gamma ? to_device(t, gamma, (size_t)d) : nullptr;
  const float* dbe = gamma ? to_device(t, beta, (size_t)d) : nullptr;
  const float* de = to_device(t, embed, (size_t)V * d);
  const float* dob = to_device(t, out_bias, (size_t)V);
  float* dl = to_device(t, logits, (size_t)n * V);      // the caller's pattern
  if (!dg || (gamma && (!dga || !dbe)) || !de || !dob || !dl) return fail(PG_ERR_HIP, "hipMalloc / copy failed");
  if (small_kernel) *small_kernel = lm_tail_small(n) ? 1 : 0;
  if ((rc = launch_lm_tail(nullptr, dg, dga, dbe, de, dob, dl, n, d, V, eps))) return rc;
  PG_HIP(hipDeviceSynchronize());
  PG_HIP(hipMemcpy(logits, dl, (size_t)n * V * 4, hipMemcpyDeviceToHost));
  return PG_OK;
}

}  // extern "C"
