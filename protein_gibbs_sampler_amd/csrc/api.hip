// extern "C" surface declared in include/pgibbs.h: engine, Gibbs runs, log-probabilities, profiling.  The pg_dbg_* entries are in
// api_dbg.hip (and comm.cpp).
#include <math.h>
#include <string.h>

#include <vector>

#include <algorithm>

#include "engine.h"

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
// The one pass over the tokens of a host-buffer call.  The first id outside the vocabulary is refused by entry, flat index and value:
// embed_ln_kernel reads embed + tok * d with whatever it is handed (device-pointer entries cannot look).  *has_pad: <pad> occurs
int scan_tokens(const Engine& e, const char* who, const int32_t* tokens, size_t n, bool* has_pad) {
  bool pad = false;
  for (size_t i = 0; i < n; ++i) {
    const int32_t t = tokens[i];
    if (t < 0 || t >= e.cfg.vocab)
      return fail(PG_ERR_INVALID, std::string(who) + ": token " + std::to_string(t) + " at flat index " + std::to_string(i) +
                                      " is outside the vocabulary of " + std::to_string(e.cfg.vocab));
    pad |= t == e.cfg.pad_idx;
  }
  *has_pad = pad;
  return PG_OK;
}
// A ragged batch (<pad> in some row; for the MSA model a ragged list of MSAs padded to one tensor, esm_msa_sampler.py:341): while
// this lives the trunks mask keys at <pad> in attention, as fair-esm's key_padding_mask does
struct PadFlag {
  Engine& e;
  PadFlag(Engine& e_, bool pad) : e(e_) { e.esm_pad_in_batch = pad; }
  ~PadFlag() { e.esm_pad_in_batch = false; }
};

// tokens[B][R][C] in (R = 1 for the ESM family), logits of every position out
int forward_logits(pg_engine* h, const char* who, bool msa, const int32_t* tokens, int B, int R, int C, float* logits_out) {
  if (!h || !tokens || !logits_out) return fail(PG_ERR_INVALID, std::string(who) + ": null argument");
  Engine& e = h->e;
  const int64_t M = (int64_t)B * R * C;
  int rc;
  bool has_pad;
  if ((rc = e.check_call(msa, B, R, C))) return rc;
  if (B == 0) return PG_OK;
  if ((rc = scan_tokens(e, who, tokens, (size_t)M, &has_pad))) return rc;
  DeviceGuard g(e.device);
  if ((rc = e.d_tokens.ensure((size_t)M * 4, e.stream))) return rc;
  if ((rc = e.logits.ensure((size_t)M * e.cfg.vocab * 4, e.stream))) return rc;
  PG_HIP(hipMemcpyAsync(e.d_tokens.p, tokens, (size_t)M * 4, hipMemcpyHostToDevice, e.stream));
  {
    PadFlag pad(e, has_pad);
    rc = e.trunk(e.d_tokens.as<int32_t>(), B, R, C);
  }
  if (rc) return rc;
  if ((rc = e.head(nullptr, nullptr, 1, C, M, e.logits.as<float>()))) return rc;
  PG_HIP(hipMemcpyAsync(logits_out, e.logits.p, (size_t)M * e.cfg.vocab * 4, hipMemcpyDeviceToHost, e.stream));
  PG_HIP(hipStreamSynchronize(e.stream));
  if ((rc = e.chain_check())) return rc;
  return check_finite(e, logits_out, (size_t)M * e.cfg.vocab);
}

// While this lives the ESM trunk stages the layers the tap lists (Engine::tap_layer)
struct TapScope {
  Engine& e;
  TapScope(Engine& e_, ReprTap* t) : e(e_) { e.tap = t; }
  ~TapScope() { e.tap = nullptr; }
};

// tokens[B][T] in, the residual stream of the requested layers out: per token and / or as means over per-sequence token ranges.
// forward_logits' shape with the tap in place of the LM head.  Everything in the argument list is refused before a device is touched
int forward_representations(pg_engine* h, const int32_t* tokens, int B, int T, const int32_t* layers, int n_req, const int32_t* pools,
                            int n_pools, float* per_token_out, float* pooled_out) {
  const char* who = "pg_esm_forward_representations";
  // what the request itself says is refused first: it needs neither a device nor, for that matter, an engine
  if (!tokens || !layers) return fail(PG_ERR_INVALID, std::string(who) + ": null argument");
  if (n_req < 1) return fail(PG_ERR_INVALID, std::string(who) + ": no layer requested");
  for (int i = 0; i < n_req; ++i) {
    if (layers[i] < 0) return fail(PG_ERR_INVALID, std::string(who) + ": layer " + std::to_string(layers[i]) + " is outside 0 .. n_layers");
    if (i && layers[i] <= layers[i - 1]) return fail(PG_ERR_INVALID, std::string(who) + ": layers must be strictly ascending");
  }
  if (!per_token_out && !pooled_out) return fail(PG_ERR_INVALID, std::string(who) + ": neither per-token nor pooled output requested");
  if (pooled_out && (!pools || n_pools < 1)) return fail(PG_ERR_INVALID, std::string(who) + ": pooled output requested without pools");
  if (!pooled_out) n_pools = 0;
  int rc;
  if (n_pools && B > 0 && T > 0 && (rc = repr_pools_check(who, pools, n_pools, B, T))) return rc;
  if (!h) return fail(PG_ERR_INVALID, std::string(who) + ": null engine");
  Engine& e = h->e;
  if (e.cfg.arch == PG_ARCH_MSA1B) return fail(PG_ERR_INVALID, std::string(who) + ": the MSA engine has no representations entry");
  if ((rc = e.check_call(false, B, 1, T))) return rc;
  if (layers[n_req - 1] > e.cfg.n_layers)
    return fail(PG_ERR_INVALID, std::string(who) + ": layer " + std::to_string(layers[n_req - 1]) + " is outside 0 .. " + std::to_string(e.cfg.n_layers));
  if (B == 0) return PG_OK;
  const int64_t M = (int64_t)B * T;
  bool has_pad;
  if ((rc = scan_tokens(e, who, tokens, (size_t)M, &has_pad))) return rc;
  DeviceGuard g(e.device);
  const size_t n_rows = (size_t)n_req * M * e.d_live, n_means = (size_t)n_req * n_pools * B * e.d_live, n_ranges = (size_t)n_pools * B * 2;
  if ((rc = e.d_tokens.ensure((size_t)M * 4, e.stream)) || (rc = e.repr_rows.ensure(n_rows * 4, e.stream))) return rc;
  if (n_pools && ((rc = e.repr_pooled.ensure(n_means * 4, e.stream)) || (rc = e.repr_ranges.ensure(n_ranges * 4, e.stream)))) return rc;
  PG_HIP(hipMemcpyAsync(e.d_tokens.p, tokens, (size_t)M * 4, hipMemcpyHostToDevice, e.stream));
  if (n_pools) PG_HIP(hipMemcpyAsync(e.repr_ranges.p, pools, n_ranges * 4, hipMemcpyHostToDevice, e.stream));
  ReprTap tap;
  tap.layers.assign(layers, layers + n_req);
  tap.d_tok = e.d_tokens.as<int32_t>();
  tap.B = B;
  tap.T = T;
  tap.d_pools = n_pools ? e.repr_ranges.as<int32_t>() : nullptr;
  tap.n_pools = n_pools;
  tap.rows = e.repr_rows.as<float>();
  tap.pooled = n_pools ? e.repr_pooled.as<float>() : nullptr;
  {
    PadFlag pad(e, has_pad);
    TapScope scope(e, &tap);
    rc = e.trunk(e.d_tokens.as<int32_t>(), B, 1, T);
  }
  if (rc) return rc;
  if (tap.next != tap.layers.size()) return fail(PG_ERR_HIP, std::string(who) + ": the forward did not reach every requested layer");
  if (per_token_out) PG_HIP(hipMemcpyAsync(per_token_out, e.repr_rows.p, n_rows * 4, hipMemcpyDeviceToHost, e.stream));
  if (n_pools) PG_HIP(hipMemcpyAsync(pooled_out, e.repr_pooled.p, n_means * 4, hipMemcpyDeviceToHost, e.stream));
  PG_HIP(hipStreamSynchronize(e.stream));
  if ((rc = e.chain_check())) return rc;
  if (per_token_out && (rc = check_finite(e, per_token_out, n_rows))) return rc;
  return n_pools ? check_finite(e, pooled_out, n_means) : PG_OK;
}

// While this lives the ESM trunk hands every block's qkv to Engine::tap_attention
struct ContactScope {
  Engine& e;
  ContactScope(Engine& e_, ContactTap* t) : e(e_) { e.ctap = t; }
  ~ContactScope() { e.ctap = nullptr; }
};
const char* arch_name(int arch) {
  return arch == PG_ARCH_MSA1B ? "MSA-1b" : arch == PG_ARCH_ESM1 ? "ESM-1" : arch == PG_ARCH_ESM2 ? "ESM-2" : "ESM-1b";
}
// the architectures with a contacts entry: ESM-1b and ESM-2 (<cls> ... <eos>, no bias key) through pg_esm_forward_contacts, MSA-1b
// (row-attention maps) through pg_msa_forward_contacts; msa_ok: the caller serves the MSA engine too (the head setter).  0 = fine
int contact_arch_check(const char* who, const Engine& e, bool msa_ok = false) {
  if (e.cfg.arch == PG_ARCH_MSA1B && !msa_ok)
    return fail(PG_ERR_INVALID, std::string(who) + ": the MSA-1b architecture has no contact head behind this entry (ESM-1b and ESM-2 only; "
                                                   "row-attention contacts: pg_msa_forward_contacts)");
  if (e.cfg.arch == PG_ARCH_ESM1)
    return fail(PG_ERR_INVALID, std::string(who) + ": the ESM-1 architecture has no contact head in this engine (ESM-1b, ESM-2 and MSA-1b only)");
  return PG_OK;
}

// tokens[B][T] in; contact probabilities and / or logits [B][T-2][T-2] and / or the attention maps of the listed blocks out.
// Everything in the argument list is refused before a device is touched, in the order pgibbs.h states
int forward_contacts(pg_engine* h, const int32_t* tokens, int B, int T, float* contacts_out, float* logits_out, const int32_t* attn_layers,
                     int n_attn, float* attn_out) {
  const std::string who = "pg_esm_forward_contacts";
  if (!tokens) return fail(PG_ERR_INVALID, who + ": null tokens");
  if (!contacts_out && !logits_out && !attn_out) return fail(PG_ERR_INVALID, who + ": no output requested");
  const bool want_layers = attn_layers && n_attn > 0;
  if (n_attn < 0 || (attn_out != nullptr) != want_layers || (!attn_layers && n_attn > 0))
    return fail(PG_ERR_INVALID, who + ": attention layers and attn_out come together or not at all");
  for (int i = 0; i < n_attn; ++i) {
    if (attn_layers[i] < 0) return fail(PG_ERR_INVALID, who + ": attention layer " + std::to_string(attn_layers[i]) + " is negative");
    if (i && attn_layers[i] <= attn_layers[i - 1]) return fail(PG_ERR_INVALID, who + ": attention layers must be strictly ascending");
  }
  if (T < 3) return fail(PG_ERR_INVALID, who + ": T = " + std::to_string(T) + ": a contact map needs <cls>, at least one position and <eos>");
  if (!h) return fail(PG_ERR_INVALID, who + ": null engine");
  Engine& e = h->e;
  int rc;
  if ((rc = contact_arch_check(who.c_str(), e))) return rc;
  const bool fold = contacts_out || logits_out;
  if (fold && !e.contact_w) return fail(PG_ERR_INVALID, who + ": no contact head set (pg_engine_set_contact_head); attention maps alone need none");
  if ((rc = e.check_call(false, B, 1, T))) return rc;
  if (n_attn && attn_layers[n_attn - 1] >= e.cfg.n_layers)
    return fail(PG_ERR_INVALID, who + ": attention layer " + std::to_string(attn_layers[n_attn - 1]) + " is outside 0 .. " + std::to_string(e.cfg.n_layers - 1));
  if (B == 0) return PG_OK;
  const int64_t M = (int64_t)B * T;
  bool has_pad;
  if ((rc = scan_tokens(e, who.c_str(), tokens, (size_t)M, &has_pad))) return rc;
  DeviceGuard g(e.device);
  const int W = T - 2, H = e.cfg.n_heads;
  const size_t n_map = (size_t)B * H * T * T, n_win = (size_t)B * W * W;
  if ((rc = e.d_tokens.ensure((size_t)M * 4, e.stream)) || (rc = e.contact_P.ensure(n_map * 4, e.stream))) return rc;
  if (n_attn && (rc = e.contact_attn.ensure(n_map * n_attn * 4, e.stream))) return rc;
  if (fold && ((rc = e.contact_logits.ensure(n_win * 4, e.stream)) || (rc = e.contact_probs.ensure(n_win * 4, e.stream)) ||
               (rc = e.contact_sums.ensure(contact_sums_floats(B, H, T) * 4, e.stream)))) return rc;
  PG_HIP(hipMemcpyAsync(e.d_tokens.p, tokens, (size_t)M * 4, hipMemcpyHostToDevice, e.stream));
  ContactTap tap;
  tap.d_tok = e.d_tokens.as<int32_t>();
  tap.B = B;
  tap.T = T;
  tap.fold = fold;
  tap.logits = fold ? e.contact_logits.as<float>() : nullptr;
  tap.contacts = contacts_out ? e.contact_probs.as<float>() : nullptr;
  if (n_attn) tap.attn_layers.assign(attn_layers, attn_layers + n_attn);
  tap.attn_out = n_attn ? e.contact_attn.as<float>() : nullptr;
  {
    PadFlag pad(e, has_pad);
    ContactScope scope(e, &tap);
    rc = e.trunk(e.d_tokens.as<int32_t>(), B, 1, T);
  }
  if (rc) return rc;
  if (tap.folded != e.cfg.n_layers || tap.next_attn != tap.attn_layers.size())
    return fail(PG_ERR_HIP, who + ": the forward did not show every layer's attention");
  if (contacts_out) PG_HIP(hipMemcpyAsync(contacts_out, e.contact_probs.p, n_win * 4, hipMemcpyDeviceToHost, e.stream));
  if (logits_out) PG_HIP(hipMemcpyAsync(logits_out, e.contact_logits.p, n_win * 4, hipMemcpyDeviceToHost, e.stream));
  if (n_attn) PG_HIP(hipMemcpyAsync(attn_out, e.contact_attn.p, n_map * n_attn * 4, hipMemcpyDeviceToHost, e.stream));
  PG_HIP(hipStreamSynchronize(e.stream));
  if ((rc = e.chain_check())) return rc;
  if (contacts_out && (rc = check_finite(e, contacts_out, n_win))) return rc;
  if (logits_out && (rc = check_finite(e, logits_out, n_win))) return rc;
  return n_attn ? check_finite(e, attn_out, n_map * n_attn) : PG_OK;
}

// tokens[B][R][C] in; contact probabilities and / or logits [B][C-1][C-1] and / or the tied row-attention maps [B][n_attn][H][C][C] of
// the listed blocks out: forward_contacts' shape on the MSA trunk (Engine::tap_row_attention).  Everything in the argument list is
// refused before a device is touched, in the order pgibbs.h states
int msa_forward_contacts(pg_engine* h, const int32_t* tokens, int B, int R, int C, float* contacts_out, float* logits_out,
                         const int32_t* attn_layers, int n_attn, float* row_attn_out) {
  const std::string who = "pg_msa_forward_contacts";
  if (!tokens) return fail(PG_ERR_INVALID, who + ": null tokens");
  if (!contacts_out && !logits_out && !row_attn_out) return fail(PG_ERR_INVALID, who + ": no output requested");
  const bool want_layers = attn_layers && n_attn > 0;
  if (n_attn < 0 || (row_attn_out != nullptr) != want_layers || (!attn_layers && n_attn > 0))
    return fail(PG_ERR_INVALID, who + ": attention layers and row_attn_out come together or not at all");
  for (int i = 0; i < n_attn; ++i) {
    if (attn_layers[i] < 0) return fail(PG_ERR_INVALID, who + ": attention layer " + std::to_string(attn_layers[i]) + " is negative");
    if (i && attn_layers[i] <= attn_layers[i - 1]) return fail(PG_ERR_INVALID, who + ": attention layers must be strictly ascending");
  }
  if (C < 2) return fail(PG_ERR_INVALID, who + ": C = " + std::to_string(C) + ": a contact map needs <cls> and at least one position");
  if (!h) return fail(PG_ERR_INVALID, who + ": null engine");
  Engine& e = h->e;
  int rc;
  if (e.cfg.arch != PG_ARCH_MSA1B)
    return fail(PG_ERR_INVALID, who + ": the " + arch_name(e.cfg.arch) + " architecture has no row attention (MSA-1b only; pg_esm_forward_contacts)");
  const bool fold = contacts_out || logits_out;
  if (fold && !e.contact_w) return fail(PG_ERR_INVALID, who + ": no contact head set (pg_engine_set_contact_head); attention maps alone need none");
  if ((rc = e.check_call(true, B, R, C))) return rc;
  if (n_attn && attn_layers[n_attn - 1] >= e.cfg.n_layers)
    return fail(PG_ERR_INVALID, who + ": attention layer " + std::to_string(attn_layers[n_attn - 1]) + " is outside 0 .. " + std::to_string(e.cfg.n_layers - 1));
  if (B == 0) return PG_OK;
  const int64_t M = (int64_t)B * R * C;
  const int W = C - 1, H = e.cfg.n_heads;
  if ((double)B * H * C * msa_row_scores_ld(C) > 2147483647.0)
    return fail(PG_ERR_INVALID, who + ": the row-attention maps of one block exceed 2^31 - 1 values: use smaller batches");
  bool has_pad;
  if ((rc = scan_tokens(e, who.c_str(), tokens, (size_t)M, &has_pad))) return rc;
  DeviceGuard g(e.device);
  const size_t n_map = (size_t)B * H * C * C, n_win = (size_t)B * W * W;
  if ((rc = e.d_tokens.ensure((size_t)M * 4, e.stream)) || (rc = e.contact_P.ensure(n_map * 4, e.stream)) ||
      (rc = e.contact_S.ensure((size_t)B * H * C * msa_row_scores_ld(C) * 4, e.stream))) return rc;
  if (n_attn && (rc = e.contact_attn.ensure(n_map * n_attn * 4, e.stream))) return rc;
  if (fold && ((rc = e.contact_logits.ensure(n_win * 4, e.stream)) || (rc = e.contact_probs.ensure(n_win * 4, e.stream)) ||
               (rc = e.contact_sums.ensure(contact_window_sums_floats(B, H, C, 0) * 4, e.stream)))) return rc;
  PG_HIP(hipMemcpyAsync(e.d_tokens.p, tokens, (size_t)M * 4, hipMemcpyHostToDevice, e.stream));
  ContactTap tap;
  tap.d_tok = e.d_tokens.as<int32_t>();
  tap.B = B;
  tap.R = R;
  tap.T = C;
  tap.fold = fold;
  tap.logits = fold ? e.contact_logits.as<float>() : nullptr;
  tap.contacts = contacts_out ? e.contact_probs.as<float>() : nullptr;
  if (n_attn) tap.attn_layers.assign(attn_layers, attn_layers + n_attn);
  tap.attn_out = n_attn ? e.contact_attn.as<float>() : nullptr;
  {
    PadFlag pad(e, has_pad);
    ContactScope scope(e, &tap);
    rc = e.trunk(e.d_tokens.as<int32_t>(), B, R, C);
  }
  if (rc) return rc;
  if (tap.folded != e.cfg.n_layers || tap.next_attn != tap.attn_layers.size())
    return fail(PG_ERR_HIP, who + ": the forward did not show every layer's row attention");
  // the engine stages the requested maps as [n_attn][B][H][C][C]; the caller's layout is [B][n_attn][H][C][C]
  if (contacts_out) PG_HIP(hipMemcpyAsync(contacts_out, e.contact_probs.p, n_win * 4, hipMemcpyDeviceToHost, e.stream));
  if (logits_out) PG_HIP(hipMemcpyAsync(logits_out, e.contact_logits.p, n_win * 4, hipMemcpyDeviceToHost, e.stream));
  const size_t one = (size_t)H * C * C;
  for (int i = 0; i < n_attn; ++i)
    for (int b = 0; b < B; ++b)
      PG_HIP(hipMemcpyAsync(row_attn_out + ((size_t)b * n_attn + i) * one, e.contact_attn.as<float>() + ((size_t)i * B + b) * one, one * 4,
                            hipMemcpyDeviceToHost, e.stream));
  PG_HIP(hipStreamSynchronize(e.stream));
  if ((rc = e.chain_check())) return rc;
  if (contacts_out && (rc = check_finite(e, contacts_out, n_win))) return rc;
  if (logits_out && (rc = check_finite(e, logits_out, n_win))) return rc;
  return n_attn ? check_finite(e, row_attn_out, n_map * n_attn) : PG_OK;
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

// What every Gibbs entry refuses before it touches a device, in the order pgibbs.h states: null pointers (other_null: a pointer only this
// entry has), the n_params sample parameters, the call check with its counts and row indices, and -- unless there is nothing to do --
// the draw guide against the WHOLE call and, for an entry on host buffers, its index table idx[n_iters][idx_rows][P] and its tokens
int gibbs_prologue(pg_engine* h, const char* who, bool msa, bool host, const int32_t* tokens, int B, int R, int C, const int32_t* idx,
                   int64_t idx_rows, int n_iters, int P, const pg_sample_params* params, int n_params = 1, bool* has_pad = nullptr,
                   bool other_null = false, int mask_row = 0, int target_row = 0) {
  if (!h || !tokens || other_null || (!idx && P > 0 && n_iters > 0)) return fail(PG_ERR_INVALID, std::string(who) + ": null argument");
  Engine& e = h->e;
  int rc;
  for (int b = 0; b < n_params; ++b)
    if ((rc = check_params(params ? params + b : nullptr, e.cfg.vocab))) return rc;
  if ((rc = e.check_call(msa, B, R, C, n_iters, P, mask_row, target_row))) return rc;
  if (B == 0 || n_iters == 0) return PG_OK;
  for (int b = 0; b < n_params; ++b)
    if ((rc = check_draw_guide(e.draw_guide(), who, C, params[b].n_valid, (int64_t)B * R, n_iters))) return rc;
  if (!host) return PG_OK;
  const size_t n_draws = (size_t)idx_rows * P * n_iters;
  if (n_draws && (rc = check_idx_table(idx, n_draws, C, who))) return rc;
  bool pad;
  if ((rc = scan_tokens(e, who, tokens, (size_t)B * R * C, &pad))) return rc;
  if (has_pad) *has_pad = pad;
  return PG_OK;
}

// The scoring entries below their own argument checks.  Sample s scores token row row_of[s] of tokens[B][R][C] at idx[s][P]: those
// three and aux[n_aux], the int32 array of the entry's own kernel (targets, or columns), go to the device; the trunk and the LM head at
// the scored rows run; launch(d_aux, d_res) queues the kernel that fills d_res[n_res].  The results wait on the device until the range
// check has passed -- a PG_ERR_RANGE call leaves the caller's buffers alone --, then n_out floats go to out and the n_out2 behind them
// to out2 (may be null).  what: the entry's name in the index messages
template <typename Launch>
int score_rows(Engine& e, const char* who, const std::string& what, const int32_t* tokens, int B, int R, int C, const int32_t* row_of,
               const int32_t* idx, int n_sel, int P, const int32_t* aux, size_t n_aux, size_t n_res, Launch&& launch, float* out,
               size_t n_out, float* out2, size_t n_out2) {
  const int64_t M = (int64_t)B * R * C;
  const int64_t n = (int64_t)n_sel * P;
  int rc;
  bool has_pad;
  for (int64_t i = 0; i < n; ++i)
    if (idx[i] >= C) return fail(PG_ERR_INVALID, what + ": index out of range");
  for (int i = 0; i < n_sel; ++i)
    if (row_of[i] < 0 || row_of[i] >= B * R) return fail(PG_ERR_INVALID, what + ": row out of range");
  if ((rc = scan_tokens(e, who, tokens, (size_t)M, &has_pad))) return rc;
  DeviceGuard g(e.device);
  if ((rc = e.d_tokens.ensure((size_t)M * 4, e.stream))) return rc;
  if ((rc = e.d_idx.ensure((size_t)n * 4, e.stream)) || (rc = e.d_samp_tok.ensure(n_aux * 4, e.stream))) return rc;
  if ((rc = e.d_rowmap.ensure((size_t)n_sel * 4, e.stream))) return rc;
  if ((rc = e.logits.ensure((size_t)n * e.cfg.vocab * 4, e.stream)) || (rc = e.d_samp_logits.ensure(n_res * 4, e.stream))) return rc;
  PG_HIP(hipMemcpyAsync(e.d_tokens.p, tokens, (size_t)M * 4, hipMemcpyHostToDevice, e.stream));
  PG_HIP(hipMemcpyAsync(e.d_idx.p, idx, (size_t)n * 4, hipMemcpyHostToDevice, e.stream));
  PG_HIP(hipMemcpyAsync(e.d_samp_tok.p, aux, n_aux * 4, hipMemcpyHostToDevice, e.stream));
  PG_HIP(hipMemcpyAsync(e.d_rowmap.p, row_of, (size_t)n_sel * 4, hipMemcpyHostToDevice, e.stream));
  {
    PadFlag pad(e, has_pad);
    rc = e.trunk(e.d_tokens.as<int32_t>(), B, R, C);
  }
  if (rc) return rc;
  if ((rc = e.head(e.d_idx.as<int32_t>(), e.d_rowmap.as<int32_t>(), P, C, n, e.logits.as<float>()))) return rc;
  float* d_res = e.d_samp_logits.as<float>();
  if ((rc = launch(e.d_samp_tok.as<int32_t>(), d_res))) return rc;
  PG_HIP(hipStreamSynchronize(e.stream));
  if ((rc = e.finish_check())) return rc;
  PG_HIP(hipMemcpyAsync(out, d_res, n_out * 4, hipMemcpyDeviceToHost, e.stream));
  if (out2) PG_HIP(hipMemcpyAsync(out2, d_res + n_out, n_out2 * 4, hipMemcpyDeviceToHost, e.stream));
  PG_HIP(hipStreamSynchronize(e.stream));
  return PG_OK;
}

// pg_engine_create / pg_engine_create_embedded around their init(Engine&); the caller's current device is put back
template <typename Init>
int create_engine(const char* who, const pg_model_config* cfg, const pg_tensor* tensors, int n_tensors, pg_engine** out, Init&& init) {
  if (!cfg || !out || (n_tensors > 0 && !tensors)) return fail(PG_ERR_INVALID, std::string(who) + ": null argument");
  *out = nullptr;
  int prev = -1;
  (void)hipGetDevice(&prev);
  pg_engine* h = new pg_engine;
  int rc = init(h->e);
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
// the profiling classes by name (pg_prof_get, pg_prof_get_kernels): the PC_* index, -1 = no such class
int prof_class(const char* name) {
  static const char* const names[PC_COUNT] = {"gemm_other", "attention", "layernorm", "embed",    "head", "sample",
                                              "gemm_qkv",   "gemm_out",  "gemm_fc1",  "gemm_fc2", "rope",     "repr_rows", "repr_pool",
                                              "attn_probs", "contact"};
  for (int i = 0; i < PC_COUNT; ++i)
    if (!strcmp(names[i], name)) return i;
  return -1;
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
  return create_engine("pg_engine_create", cfg, tensors, n_tensors, out,
                       [&](Engine& e) { return e.init(cfg, tensors, n_tensors, device_ordinal, precision); });
}

int pg_engine_create_embedded(const pg_model_config* cfg, int head_slot, const pg_tensor* tensors, int n_tensors, int device_ordinal,
                              int precision, pg_engine** out) {
  return create_engine("pg_engine_create_embedded", cfg, tensors, n_tensors, out,
                       [&](Engine& e) { return e.init_embedded(cfg, head_slot, tensors, n_tensors, device_ordinal, precision); });
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

int pg_engine_set_draw_guide(pg_engine* h, const pg_draw_guide* guide) {
  // what the tables hold is refused first: it needs neither a device nor, for that matter, an engine
  if (guide)
    if (int rc = check_draw_guide_tables(guide, "pg_engine_set_draw_guide")) return rc;
  if (!h) return fail(PG_ERR_INVALID, "null engine");
  DeviceGuard g(h->e.device);
  return h->e.set_draw_guide(guide);
}

int pg_engine_get_stat(pg_engine* h, const char* name, int64_t* value) {
  if (!h || !name || !value) return fail(PG_ERR_INVALID, "pg_engine_get_stat: null argument");
  if (!strcmp(name, "graph_captures")) *value = h->e.stat_graph_captures;
  else if (!strcmp(name, "graph_replays")) *value = h->e.stat_graph_replays;
  else return fail(PG_ERR_INVALID, std::string("unknown stat ") + name);
  return PG_OK;
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

// ---- ESM-1b ---------------------------------------------------------------------------------
int pg_esm_forward_logits(pg_engine* h, const int32_t* tokens, int B, int T, float* logits_out) {
  PG_RETRY_WITHOUT_CHAIN_TRUNK(h, forward_logits(h, "pg_esm_forward_logits", false, tokens, B, 1, T, logits_out));
}

int pg_esm_forward_representations(pg_engine* h, const int32_t* tokens, int B, int T, const int32_t* layers, int n_req, const int32_t* pools,
                                   int n_pools, float* per_token_out, float* pooled_out) {
  PG_RETRY_WITHOUT_CHAIN_TRUNK(h, forward_representations(h, tokens, B, T, layers, n_req, pools, n_pools, per_token_out, pooled_out));
}

int pg_esm_forward_contacts(pg_engine* h, const int32_t* tokens, int B, int T, float* contacts_out, float* logits_out, const int32_t* attn_layers,
                            int n_attn, float* attn_out) {
  PG_RETRY_WITHOUT_CHAIN_TRUNK(h, forward_contacts(h, tokens, B, T, contacts_out, logits_out, attn_layers, n_attn, attn_out));
}

int pg_msa_forward_contacts(pg_engine* h, const int32_t* tokens, int B, int R, int C, float* contacts_out, float* logits_out,
                            const int32_t* attn_layers, int n_attn, float* row_attn_out) {
  return msa_forward_contacts(h, tokens, B, R, C, contacts_out, logits_out, attn_layers, n_attn, row_attn_out);
}

int pg_engine_set_contact_head(pg_engine* h, const float* weight, int n_weights, float bias) {
  const char* who = "pg_engine_set_contact_head";
  if (!h) return fail(PG_ERR_INVALID, std::string(who) + ": null engine");
  Engine& e = h->e;
  if (int rc = contact_arch_check(who, e, true)) return rc;
  if (weight) {
    const int want = e.cfg.n_layers * e.cfg.n_heads;
    if (n_weights != want)
      return fail(PG_ERR_INVALID, std::string(who) + ": " + std::to_string(n_weights) + " weights for a model of " + std::to_string(e.cfg.n_layers) + " layers x " +
                                      std::to_string(e.cfg.n_heads) + " heads = " + std::to_string(want) + " channels");
    for (int i = 0; i < n_weights; ++i)
      if (!(fabsf(weight[i]) <= 3.0e38f)) return fail(PG_ERR_INVALID, std::string(who) + ": weight " + std::to_string(i) + " is not finite");
    if (!(fabsf(bias) <= 3.0e38f)) return fail(PG_ERR_INVALID, std::string(who) + ": the bias is not finite");
  }
  DeviceGuard g(e.device);
  return e.set_contact_head(weight, n_weights, bias);
}

int pg_esm_gibbs_run_device(pg_engine* h, int32_t* d_tokens_inout, int B, int T, const int32_t* d_target_idx, int n_iters,
                            int P, const pg_sample_params* params, float* d_sampled_logits, int32_t* d_sampled_tokens) {
  int rc = gibbs_prologue(h, "pg_esm_gibbs_run_device", false, false, d_tokens_inout, B, 1, T, d_target_idx, B, n_iters, P, params);
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
  bool has_pad = false;
  int rc = gibbs_prologue(h, "pg_esm_gibbs_run", false, true, tokens_inout, B, 1, T, target_idx, B, n_iters, P, params, 1, &has_pad);
  if (rc || B == 0 || n_iters == 0) return rc;
  Engine& e = h->e;
  DeviceGuard g(e.device);
  PadFlag pad(e, has_pad);
  return stage_gibbs(e, tokens_inout, (size_t)B * T, target_idx, (size_t)B * P * n_iters, sampled_logits, sampled_tokens,
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
  return forward_logits(h, "pg_msa_forward_logits", true, tokens, B, R, C, logits_out);
}

int pg_msa_gibbs_run(pg_engine* h, int32_t* tokens_inout, int B, int R, int C, const int32_t* target_idx, int n_iters,
                     int P, const pg_sample_params* params, float* sampled_logits, int32_t* sampled_tokens) {
  int rc = gibbs_prologue(h, "pg_msa_gibbs_run", true, true, tokens_inout, B, R, C, target_idx, (int64_t)B * R, n_iters, P, params);
  if (rc || B == 0 || n_iters == 0) return rc;
  Engine& e = h->e;
  DeviceGuard g(e.device);
  return stage_gibbs(e, tokens_inout, (size_t)B * R * C, target_idx, (size_t)B * R * P * n_iters, sampled_logits, sampled_tokens,
                     [&](int32_t* d_tok, const int32_t* d_idx, float* d_lg, int32_t* d_st) {
                       return e.msa_gibbs_device(d_tok, B, R, C, d_idx, n_iters, P, params, d_lg, d_st);
                     });
}

int pg_msa_gibbs_single_batch_run(pg_engine* h, int32_t* tokens_inout, int B, int R, int C, int mask_row, int target_row,
                                  const int32_t* step_idx, const int32_t* step_sample_flag, int n_steps, int P_max,
                                  const pg_sample_params* params, float* sampled_logits, int32_t* sampled_tokens) {
  // every check is of the WHOLE call: a block of it (below) has fewer token rows than a per-row bias table
  int rc = gibbs_prologue(h, "pg_msa_gibbs_single_batch_run", true, true, tokens_inout, B, R, C, step_idx, B, n_steps, P_max, params, B,
                          nullptr, n_steps > 0 && !step_sample_flag, mask_row, target_row);
  if (rc || B == 0 || n_steps == 0) return rc;
  Engine& e = h->e;
  DeviceGuard g(e.device);
  const int V = e.cfg.vocab;
  // templates [b0, b0 + nb) as one staged call: their tokens, their step table idx[n_steps][nb][P_max], their parameters and outputs
  auto run = [&](int b0, int nb, const int32_t* idx, float* lg, int32_t* st) {
    return stage_gibbs(e, tokens_inout + (size_t)b0 * R * C, (size_t)nb * R * C, idx, (size_t)nb * P_max * n_steps, lg, st,
                       [&](int32_t* d_tok, const int32_t* d_idx, float* d_lg, int32_t* d_st) {
                         return e.msa_single_device(d_tok, nb, R, C, mask_row, target_row, d_idx, step_sample_flag, n_steps, P_max,
                                                    params + b0, d_lg, d_st);
                       });
  };
  // The tied row attention of a template batch runs in its split-R form (every template as if alone), whose
  // fp32 scratch grows with B: 0.5 GB for 4 templates of 128 x 513, past 2 GB from about B = 9 at C = 576 or B = 32 at C = 300.
  // Templates are independent, so a larger batch is simply run in blocks that fit (same logits and tokens; ADVICE r03:
  // `--template_batch 32`, BASELINE config 5's "32 templates", used to fail with PG_ERR_INVALID).
  static const size_t limit = (size_t)env_int("PGIBBS_SPLIT_SCRATCH_MB", 1024) << 20;
  const size_t need1 = msa_row_split_scratch_bytes(1, R, C, e.cfg.n_heads, e.cfg.n_heads);
  const int bc = need1 ? (int)std::max<size_t>(1, std::min<size_t>((size_t)B, limit / need1)) : B;
  if (bc >= B) return run(0, B, step_idx, sampled_logits, sampled_tokens);
  std::vector<int32_t> idx_c, tok_c;
  std::vector<float> lg_c;
  auto to_block = [](auto* block, const auto* table, size_t n) { memcpy(block, table, n * sizeof(*block)); return PG_OK; };
  auto to_table = [](const auto* block, auto* table, size_t n) { memcpy(table, block, n * sizeof(*block)); return PG_OK; };
  for (int b0 = 0; b0 < B; b0 += bc) {
    const int nb = std::min(bc, B - b0);
    const size_t n1 = (size_t)n_steps * nb * P_max;
    idx_c.assign(n1 + 1, -1);
    (void)template_block_rows(idx_c.data(), step_idx, n_steps, B, b0, nb, P_max, to_block);
    if (sampled_logits) lg_c.assign(n1 * V + 1, 0.f);
    if (sampled_tokens) tok_c.assign(n1 + 1, 0);
    {
      Engine::GuideRowShift rows(e, (int64_t)b0 * R, C);
      rc = run(b0, nb, idx_c.data(), sampled_logits ? lg_c.data() : nullptr, sampled_tokens ? tok_c.data() : nullptr);
    }
    if (rc) return rc;
    if (sampled_logits) (void)template_block_rows(lg_c.data(), sampled_logits, n_steps, B, b0, nb, (size_t)P_max * V, to_table);
    if (sampled_tokens) (void)template_block_rows(tok_c.data(), sampled_tokens, n_steps, B, b0, nb, P_max, to_table);
  }
  return PG_OK;
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
  int rc = gibbs_prologue(h, "pg_msa_gibbs_run_device", true, false, d_tokens_inout, B, R, C, d_target_idx, (int64_t)B * R, n_iters, P, params);
  if (rc) return rc;
  DeviceGuard g(h->e.device);
  return h->e.msa_gibbs_device(d_tokens_inout, B, R, C, d_target_idx, n_iters, P, params, d_sampled_logits, d_sampled_tokens);
}

// ---- masked log-likelihood scoring (next-tier path: log_likelihood_batch) ---------------------------
// rows: tokens[n_rows][width]; sample s scores token row row_of[s] at positions idx[s][P] (entries < 0 skipped, out = 0)
// against targets[s][P]; out[s][P] = log_softmax(logits)[target].
static int forward_logprobs(pg_engine* h, const char* who, bool msa, const int32_t* tokens, int B, int R, int C, const int32_t* row_of,
                            const int32_t* idx, const int32_t* targets, int n_sel, int P, float* out) {
  if (!h || !tokens || !row_of || !idx || !targets || !out) return fail(PG_ERR_INVALID, std::string(who) + ": null argument");
  Engine& e = h->e;
  if (int rc = e.check_call(msa, B, R, C, n_sel, P)) return rc;
  const size_t n = (size_t)n_sel * P;
  if (n == 0 || B == 0) return PG_OK;
  for (size_t i = 0; i < n; ++i)
    if (idx[i] >= 0 && (targets[i] < 0 || targets[i] >= e.cfg.vocab)) return fail(PG_ERR_INVALID, "logprobs: index out of range");
  return score_rows(e, who, "logprobs", tokens, B, R, C, row_of, idx, n_sel, P, targets, n, n,
                    [&](const int32_t* d_targets, float* d_out) {
                      return launch_logprob_gather(e.stream, e.logits.as<float>(), e.cfg.vocab, 1, C, e.d_idx.as<int32_t>(),
                                                   e.d_rowmap.as<int32_t>(), d_targets, n_sel, P, d_out, e.range_err);
                    },
                    out, n, nullptr, 0);
}

int pg_esm_forward_logprobs(pg_engine* h, const int32_t* tokens, int B, int T, const int32_t* row_of, const int32_t* idx,
                            const int32_t* targets, int n_sel, int P, float* out) {
  PG_RETRY_WITHOUT_CHAIN_TRUNK(h, forward_logprobs(h, "pg_esm_forward_logprobs", false, tokens, B, 1, T, row_of, idx, targets, n_sel, P, out));
}

int pg_msa_forward_logprobs(pg_engine* h, const int32_t* tokens, int B, int R, int C, const int32_t* row_of,
                            const int32_t* idx, const int32_t* targets, int n_sel, int P, float* out) {
  return forward_logprobs(h, "pg_msa_forward_logprobs", true, tokens, B, R, C, row_of, idx, targets, n_sel, P, out);
}

int pg_logprob_gather_device(void* stream, const float* d_logits, int64_t n_rows, int width, int V, const int32_t* d_idx,
                             const int32_t* d_row_map, const int32_t* d_targets, int64_t n_sel, int P, float* d_out) {
  if (!d_logits || !d_idx || !d_targets || !d_out) return fail(PG_ERR_INVALID, "pg_logprob_gather_device: null argument");
  if (n_rows < 0 || width < 1 || V < 1 || n_sel < 0 || P < 0) return fail(PG_ERR_INVALID, "bad shape");
  return launch_logprob_gather((hipStream_t)stream, d_logits, V, 0, width, d_idx, d_row_map, d_targets, n_sel, P, d_out);
}

// ---- masked-marginal substitution tables: forward_logprobs with the table kernel in the gather's place ----------------------
// out[s][P][n_cols] = log-probability of token cols[c] at (token row row_of[s], position idx[s][p]), entropy[s][P] optional
static int check_table_cols(const int32_t* cols, int n_cols, int V) {
  for (int c = 0; c < n_cols; ++c)
    if (cols[c] < 0 || cols[c] >= V)
      return fail(PG_ERR_INVALID, "logprob table: column " + std::to_string(cols[c]) + " is outside the vocabulary of " + std::to_string(V));
  return PG_OK;
}

static int forward_logprob_table(pg_engine* h, const char* who, bool msa, const int32_t* tokens, int B, int R, int C, const int32_t* row_of,
                                 const int32_t* idx, int n_sel, int P, const int32_t* cols, int n_cols, int norm, float* out, float* entropy) {
  if (!h || !tokens || !row_of || !idx || !cols || !out) return fail(PG_ERR_INVALID, std::string(who) + ": null argument");
  Engine& e = h->e;
  const int V = e.cfg.vocab;
  int rc;
  if ((rc = e.check_call(msa, B, R, C, n_sel, P))) return rc;
  if ((rc = check_logprob_table_args(V, n_cols, norm, n_sel, P)) || (rc = check_table_cols(cols, n_cols, V))) return rc;
  const size_t n = (size_t)n_sel * P;
  if (n == 0 || B == 0) return PG_OK;
  // the device holds the table, then the entropies
  return score_rows(e, who, "logprob table", tokens, B, R, C, row_of, idx, n_sel, P, cols, (size_t)n_cols, n * (n_cols + 1),
                    [&](const int32_t* d_cols, float* d_out) {
                      return launch_logprob_table(e.stream, e.logits.as<float>(), V, 1, C, e.d_idx.as<int32_t>(), e.d_rowmap.as<int32_t>(),
                                                  d_cols, n_cols, norm, n_sel, P, d_out, entropy ? d_out + n * n_cols : nullptr, e.range_err);
                    },
                    out, n * n_cols, entropy, n);
}

int pg_esm_forward_logprob_table(pg_engine* h, const int32_t* tokens, int B, int T, const int32_t* row_of, const int32_t* idx,
                                 int n_sel, int P, const int32_t* cols, int n_cols, int norm, float* out, float* entropy) {
  PG_RETRY_WITHOUT_CHAIN_TRUNK(h, forward_logprob_table(h, "pg_esm_forward_logprob_table", false, tokens, B, 1, T, row_of, idx, n_sel, P, cols,
                                                        n_cols, norm, out, entropy));
}

int pg_msa_forward_logprob_table(pg_engine* h, const int32_t* tokens, int B, int R, int C, const int32_t* row_of,
                                 const int32_t* idx, int n_sel, int P, const int32_t* cols, int n_cols, int norm, float* out,
                                 float* entropy) {
  return forward_logprob_table(h, "pg_msa_forward_logprob_table", true, tokens, B, R, C, row_of, idx, n_sel, P, cols, n_cols, norm, out, entropy);
}

int pg_logprob_table_device(void* stream, const float* d_logits, int64_t n_rows, int width, int V, const int32_t* d_idx,
                            const int32_t* d_row_map, int64_t n_sel, int P, const int32_t* d_cols, int n_cols, int norm,
                            float* d_out, float* d_entropy) {
  if (!d_logits || !d_idx || !d_cols || !d_out) return fail(PG_ERR_INVALID, "pg_logprob_table_device: null argument");
  if (int rc = check_logprob_table_args(V, n_cols, norm, n_sel, P)) return rc;
  if (n_rows < 0 || width < 1) return fail(PG_ERR_INVALID, "bad shape");
  return launch_logprob_table((hipStream_t)stream, d_logits, V, 0, width, d_idx, d_row_map, d_cols, n_cols, norm, n_sel, P, d_out,
                              d_entropy);
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

int pg_sample_writeback_guided_device(void* stream, int32_t* d_tokens, int64_t n_rows, int width, const float* d_logits, int V,
                                      const int32_t* d_idx, const int32_t* d_row_map, int64_t n_sel, int P,
                                      const pg_sample_params* params, int iteration, int32_t* d_sampled_tokens, const float* d_bias,
                                      int64_t bias_rows, const float* d_temperatures, int n_temperatures, float top_p) {
  if (!d_tokens || !d_logits || (!d_idx && n_sel * P > 0)) return fail(PG_ERR_INVALID, "pg_sample_writeback_guided_device: null argument");
  int rc = check_params(params, V);
  if (rc) return rc;
  if (n_rows < 0 || width < 1 || n_sel < 0 || P < 0 || V < 1) return fail(PG_ERR_INVALID, "bad shape");
  if (top_p == top_p && !(top_p > 0.f && top_p <= 1.0f))
    return fail(PG_ERR_INVALID, "pg_sample_writeback_guided_device: top_p must be in (0, 1] (NaN = off)");
  if (d_temperatures && iteration < 0) return fail(PG_ERR_INVALID, "pg_sample_writeback_guided_device: negative iteration with a temperature schedule");
  DrawGuideDev g;
  g.bias = d_bias;
  if (d_bias) { g.bias_rows = bias_rows; g.width = width; g.n_valid = params->n_valid; }
  g.temps = d_temperatures;
  g.n_temps = d_temperatures ? n_temperatures : 0;
  g.top_p = top_p;
  if ((rc = check_draw_guide(&g, "pg_sample_writeback_guided_device", width, params->n_valid, n_rows, (int64_t)iteration + 1))) return rc;
  return launch_sample_writeback((hipStream_t)stream, d_tokens, width, d_logits, V, 0, d_idx, d_row_map, n_sel, P, params, iteration,
                                 d_sampled_tokens, nullptr, nullptr, &g);
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
  const int cls = prof_class(kernel_class);
  const bool all_gemm = !strcmp(kernel_class, "gemm");       // the whole family: the four per-layer projections + the rest
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
  const int cls = prof_class(kernel_class);
  if (cls < 0) return fail(PG_ERR_INVALID, std::string("unknown kernel class ") + kernel_class);
  std::vector<std::string> seen;
  for (auto& r : h->e.prof.recs)
    if (r.cls == cls && !r.kernels.empty() && std::find(seen.begin(), seen.end(), r.kernels) == seen.end()) seen.push_back(r.kernels);
  std::string out;
  for (auto& k : seen) out += (out.empty() ? "" : " | ") + k;
  snprintf(buf, (size_t)buf_bytes, "%s", out.c_str());
  return PG_OK;
}

}  // extern "C"
