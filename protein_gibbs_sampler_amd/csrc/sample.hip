// The two integer/index ends of a Gibbs iteration, as data-parallel kernels:
//
//   mask_scatter_kernel      == mask_target_indexes           /root/reference/src/pgen/esm_sampler.py:259-262,
//                               (+ _single)                    esm_msa_sampler.py:255-264
//   sample_writeback_kernel  == generate_step + write-back    esm_sampler.py:8-45, 225-234;
//                                                              esm_msa_sampler.py:138-145, 238-248
//
// In the reference both are Python loops issuing B*P scalar tensor writes (6400 per iteration at
// config 2).  All P draws of an iteration read the same logits (no re-forward between positions), so
// they are independent: one thread per (row, slot).  A row of 33 logits is 132 B; the whole job is a
// few hundred KB -> latency-bound, one launch each.
//
// The draw is "pg_draw v1" (oracle/draw.py): every float op below is a separately rounded IEEE
// binary32 op -- this file is compiled with -ffp-contract=off -- so the kernel and the CPU oracle
// agree bit-for-bit given the same logits.
#include "../../include/pgibbs.h"
#include "kernels.h"

namespace pg {

#pragma clang fp contract(off)

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t& o0) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    const uint32_t n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  o0 = c0;
}

// exp(x), x <= 0, reproducible (oracle/draw.py::pg_exp)
__device__ __forceinline__ float pg_exp(float x) {
  const float z = x * 1.44269502162933349609375f;  // float32(log2 e)
  if (z < -126.0f) return 0.0f;
  const float n = floorf(z);
  const float f = z - n;
  float p = 0x1.b4d1dep-13f;
  p = p * f; p = p + 0x1.4ca4cep-10f;
  p = p * f; p = p + 0x1.3c4a8ap-7f;
  p = p * f; p = p + 0x1.c69f6ap-5f;
  p = p * f; p = p + 0x1.ebfc40p-3f;
  p = p * f; p = p + 0x1.62e430p-1f;
  p = p * f; p = p + 1.0f;
  const int bits = __float_as_int(p) + ((int)n << 23);
  return __int_as_float(bits);
}

constexpr int kGraphArgsOffset = 4;      // int32 words: d_iter[0] = iteration, SampleArgs from byte 16 on

struct SampleArgs {
  int32_t top_k;
  int32_t sample;       // 1: draw from all valid tokens regardless of top_k
  float temperature;
  int32_t use_temp;
  int32_t n_valid;
  int32_t valid_idx[32];
  uint32_t seed_lo, seed_hi, stream, row_id_base, iter;
  int32_t burnin;             // used with a device-side iteration counter: sample = (it < burnin)
};

// pg_draw v2: what a guided draw reads besides SampleArgs.  All device pointers; a null pointer / use_top_p 0
// switches that part off, and with all three off the guided kernel computes v1's bits.
struct GuideArgs {
  const float* bias;    // [bias_rows][width][n_valid] in valid-list order, -inf = forbidden; null: none
  const float* temps;   // [>= iterations of the call]: T = temps[it] and SampleArgs::temperature is not read; null: none
  int32_t bias_per_row; // 1: the table row is the draw's token row; 0: one shared row
  int32_t use_top_p;
  float top_p;
  int32_t it;           // call-local iteration (index into temps); a device-side counter is added to it
};
struct GuidedSampleArgs {
  SampleArgs s;         // first: the graph state block holds a GuidedSampleArgs, and the v1 kernel reads its SampleArgs prefix
  GuideArgs g;
};
template <bool Guided> struct DrawArgs { using type = SampleArgs; };
template <> struct DrawArgs<true> { using type = GuidedSampleArgs; };
__device__ __forceinline__ SampleArgs& sample_part(SampleArgs& a) { return a; }
__device__ __forceinline__ SampleArgs& sample_part(GuidedSampleArgs& a) { return a.s; }

// logits addressing: compact [n_sel*P][V] (engine path: LM head evaluated only at the sampled rows),
// or full [n_rows][width][V] (plug-in models).
// One WAVE per draw (round 4; it was one thread per draw -- a 32 x 32 rank loop and 32 exponentials in a single lane, 42 us
// however few draws there were, 3 % of a config-1 iteration): lane j holds valid entry j.  Every floating-point operation and its
// order is the one-thread form's (the cumulative sums are accumulated in rank order, one after the other, in a value all lanes
// hold), so the draws are the same bit for bit.
// Guided = false is pg_draw v1 and stays the code it was (the `if constexpr (Guided)` parts are not compiled into it); Guided = true
// is v2: bias and scheduled temperature before the rank, the forbidden entries cut from k, the nucleus cut after the sums.
template <bool Guided>
__global__ __launch_bounds__(256) void sample_writeback_kernel(int32_t* __restrict__ tokens, int width,
                                                              const float* __restrict__ logits, int V, int compact,
                                                              const int32_t* __restrict__ idx,
                                                              const int32_t* __restrict__ row_map, int64_t n_sel, int P,
                                                              typename DrawArgs<Guided>::type args, int32_t* __restrict__ sampled_tokens,
                                                              const int32_t* __restrict__ d_iter, unsigned* nonfinite) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (i >= n_sel * P) return;   // wave-uniform
  SampleArgs& a = sample_part(args);
  if (d_iter) {               // graph replay: the iteration number AND the sampling parameters live on the device, so one
    const int it = *d_iter;   // captured graph serves every iteration of every call with this shape (launch_graph_state)
    args = *(const typename DrawArgs<Guided>::type*)(d_iter + kGraphArgsOffset);
    idx += (size_t)it * n_sel * P;
    a.iter += (uint32_t)it;
    a.sample = it < a.burnin ? 1 : 0;
    if constexpr (Guided) args.g.it += it;
  }
  const int64_t s = i / P;
  const int slot = (int)(i - s * P);
  const int raw = idx[i];
  if (raw < 0) {
    if (sampled_tokens && lane == 0) sampled_tokens[i] = -1;
    return;
  }
  const int pos = raw & 0x3fffffff;
  if (pos >= width) {          // out-of-range position (the host entry points reject these; *_device callers are guarded here)
    if (sampled_tokens && lane == 0) sampled_tokens[i] = -1;
    return;
  }
  const int64_t trow = row_map ? (int64_t)row_map[s] : s;
  const float* row = compact ? logits + (size_t)i * V : logits + ((size_t)trow * width + pos) * V;

  const int nv = a.n_valid;
  int k = a.top_k;
  if (a.sample || k <= 0 || k > nv) k = nv;
  // this lane's entry of the valid list (static indices into the by-value struct: no private-memory copy)
  int my_valid = 0;
#pragma unroll
  for (int m = 0; m < 32; ++m)
    if (m == lane) my_valid = a.valid_idx[m];
  const bool mine = lane < nv;
  float v = 0.f;
  if (mine) {
    v = row[my_valid];
    // a non-finite logit (an overflowed fp16 operand upstream: inf -> NaN through the next LayerNorm) is reported, not sampled
    // from silently: the engine's entry points return PG_ERR_RANGE (Engine::range_check)
    if (nonfinite && !(fabsf(v) <= 3.0e38f)) *nonfinite = 1u;
    if constexpr (Guided) {
      if (args.g.bias) {
        const int64_t cell = (args.g.bias_per_row ? trow * width : (int64_t)0) + pos;
        v = v + args.g.bias[(size_t)cell * nv + lane];
      }
      if (args.g.temps) v = v / args.g.temps[args.g.it];
      else if (a.use_temp) v = v / a.temperature;
    } else {
      if (a.use_temp) v = v / a.temperature;
    }
  }
  if constexpr (Guided) {      // the forbidden entries (-inf) rank last: cutting k to the allowed count cuts exactly them
    const int n_allowed = __popcll(__ballot(mine && v > -INFINITY));
    if (k > n_allowed) k = n_allowed;
    if (k < 1) k = 1;          // a cell with nothing allowed (refused where the table is on the host): still a defined pick
  }
  // stable descending rank of every valid entry
  int rank = 0;
#pragma unroll
  for (int m = 0; m < 32; ++m) {
    if (m < nv) {                                      // wave-uniform
      const float vm = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), m));
      rank += (vm > v) || (vm == v && m < lane);
    }
  }
  // lane r receives the value and the valid-list position of the entry with rank r (rank is a permutation of 0..nv-1)
  const int dst = (mine ? rank : lane) * 4;            // idle lanes send to themselves
  const float ev = __builtin_bit_cast(float, __builtin_amdgcn_ds_permute(dst, __builtin_bit_cast(int, v)));
  const int ei = __builtin_amdgcn_ds_permute(dst, lane);
  const float top = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ev), 0));
  const float e = lane < k ? pg_exp(ev - top) : 0.f;
  float acc = 0.f, cum = 0.f;
#pragma unroll
  for (int r = 0; r < 32; ++r) {
    if (r < k) {                                       // wave-uniform
      const float er = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, e), r));
      acc = (r == 0) ? er : acc + er;
      if (lane == r) cum = acc;
    }
  }
  uint32_t w0;
  philox4x32_10(a.row_id_base + (uint32_t)s, a.iter, (uint32_t)slot, a.stream, a.seed_lo, a.seed_hi, w0);
  const float u = (float)(w0 >> 8) * 0x1.0p-24f;
  if constexpr (Guided) {      // nucleus: the shortest prefix whose sum reaches top_p of the whole; not in burn-in, as top_k
    if (args.g.use_top_p && !a.sample) {
      const float q = args.g.top_p * acc;
      const int kp = 1 + __popcll(__ballot(lane < k && cum < q));
      if (kp < k) {
        k = kp;
        acc = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, cum), k - 1));
      }
    }
  }
  const float t = u * acc;
  const unsigned long long hit = __ballot(lane < k && cum > t);
  const int jsel = hit ? (int)__builtin_ctzll(hit) : k - 1;
  const int pick = __builtin_amdgcn_readlane(ei, jsel);
  const int tok = __builtin_amdgcn_readlane(my_valid, pick);
  if (lane == 0) {
    if (sampled_tokens) sampled_tokens[i] = tok;
    if (!(raw & 0x40000000)) tokens[trow * width + pos] = tok;
  }
}

__global__ __launch_bounds__(256) void mask_scatter_kernel(int32_t* __restrict__ tokens, int width,
                                                          const int32_t* __restrict__ idx,
                                                          const int32_t* __restrict__ row_map, int64_t n_sel, int P,
                                                          int mask_idx, const int32_t* __restrict__ d_iter) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_sel * P) return;
  if (d_iter) idx += (size_t)(*d_iter) * n_sel * P;
  const int raw = idx[i];
  if (raw < 0 || (raw & 0x3fffffff) >= width) return;
  const int64_t s = i / P;
  const int64_t trow = row_map ? (int64_t)row_map[s] : s;
  tokens[trow * width + (raw & 0x3fffffff)] = mask_idx;
}

// The two numbers a log_softmax needs: mx = the maximum of at(0) ... at(n - 1), logsum = logf(sum of expf(at(v) - mx)).  The gather
// kernel and the table kernel both call this, so log p = x - mx - logsum carries the same bits in both (kernels that must agree
// bit for bit call the same function, in this translation unit and under its -ffp-contract=off).
template <typename At>
__device__ __forceinline__ void row_max_logsum(At at, int n, float& mx, float& logsum) {
  mx = at(0);
  for (int v = 1; v < n; ++v) mx = fmaxf(mx, at(v));
  float sum = 0.f;
  for (int v = 0; v < n; ++v) sum += expf(at(v) - mx);
  logsum = logf(sum);
}

// log p(target | context) at the selected rows: log_softmax over the FULL vocabulary then gather
// (== torch.log_softmax(logits, -1)[..., target], /root/reference/src/pgen/esm_sampler.py:340-345,
//  esm_msa_sampler.py:403-410).  One thread per selected entry; V <= 64 floats per row.
__global__ __launch_bounds__(256) void logprob_gather_kernel(const float* __restrict__ logits, int V, int compact, int width,
                                                            const int32_t* __restrict__ idx,
                                                            const int32_t* __restrict__ row_map,
                                                            const int32_t* __restrict__ targets, int64_t n_sel, int P,
                                                            float* __restrict__ out, unsigned* nonfinite) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_sel * P) return;
  const int pos = idx[i];
  if (pos < 0 || pos >= width) { out[i] = 0.f; return; }
  const int64_t s = i / P;
  const int64_t trow = row_map ? (int64_t)row_map[s] : s;
  const float* row = compact ? logits + (size_t)i * V : logits + ((size_t)trow * width + pos) * V;
  float mx, logsum;
  row_max_logsum([row](int v) { return row[v]; }, V, mx, logsum);
  const float lp = row[targets[i]] - mx - logsum;
  if (nonfinite && !(fabsf(mx) <= 3.0e38f)) *nonfinite = 1u;      // NaN or inf anywhere in the row ends up in mx or in lp
  if (nonfinite && lp != lp) *nonfinite = 1u;
  out[i] = lp;
}

int launch_logprob_gather(hipStream_t st, const float* logits, int V, int compact, int width, const int32_t* idx,
                          const int32_t* row_map, const int32_t* targets, int64_t n_sel, int P, float* out, unsigned* nonfinite) {
  const int64_t n = n_sel * P;
  if (n == 0) return 0;
  hipLaunchKernelGGL(logprob_gather_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, logits, V, compact, width, idx,
                     row_map, targets, n_sel, P, out, nonfinite);
  PG_HIP(hipGetLastError());
  return 0;
}

// The whole row instead of one entry of it: out[i][c] = log p(cols[c]) for c < n_cols, and optionally the entropy in nats,
// -sum p log p over the normalisation set (== pgen_msa_seq_probs.py:31-45 of the reference, whose probs_single no longer exists, and
// esm_sampler.py:340-345 before its gather).  norm PG_TABLE_NORM_VOCAB: log_softmax over all V logits, then the columns are picked --
// the value at a column is the gather kernel's for that target, bit for bit.  PG_TABLE_NORM_COLUMNS: log_softmax over the n_cols
// selected logits only (Categorical(logits = valid logits), what generate_step draws from without temperature or top-k).
// Addressing, skipped entries (zeros) and the nonfinite word are the gather kernel's.  One thread per scored entry: at most a few
// tens of thousands of entries of <= 64 floats.  A column outside 0 .. V-1 (the engine entries refuse it on the host) reads as NaN.
__global__ __launch_bounds__(256) void logprob_table_kernel(const float* __restrict__ logits, int V, int compact, int width,
                                                           const int32_t* __restrict__ idx,
                                                           const int32_t* __restrict__ row_map,
                                                           const int32_t* __restrict__ cols, int n_cols, int norm, int64_t n_sel,
                                                           int P, float* __restrict__ out, float* __restrict__ entropy,
                                                           unsigned* nonfinite) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_sel * P) return;
  float* o = out + (size_t)i * n_cols;
  const int pos = idx[i];
  if (pos < 0 || pos >= width) {
    for (int c = 0; c < n_cols; ++c) o[c] = 0.f;
    if (entropy) entropy[i] = 0.f;
    return;
  }
  const int64_t s = i / P;
  const int64_t trow = row_map ? (int64_t)row_map[s] : s;
  const float* row = compact ? logits + (size_t)i * V : logits + ((size_t)trow * width + pos) * V;
  auto at_col = [row, cols, V](int c) {
    const int v = cols[c];
    return (unsigned)v < (unsigned)V ? row[v] : __int_as_float(0x7fc00000);
  };
  auto at_row = [row](int v) { return row[v]; };
  const bool over_cols = norm == PG_TABLE_NORM_COLUMNS;
  float mx, logsum;
  if (over_cols) row_max_logsum(at_col, n_cols, mx, logsum);
  else row_max_logsum(at_row, V, mx, logsum);
  bool bad = !(fabsf(mx) <= 3.0e38f);                // as the gather kernel: NaN or inf in the row ends up in mx or in a log p
  if (over_cols)                                     // ... of which this form reads only the selected ones: look at the others too
    for (int v = 0; v < V; ++v) bad |= !(fabsf(row[v]) <= 3.0e38f);
  for (int c = 0; c < n_cols; ++c) {
    const float lp = at_col(c) - mx - logsum;
    bad |= lp != lp;
    o[c] = lp;
  }
  if (entropy) {
    float h = 0.f;
    const int n = over_cols ? n_cols : V;
    for (int v = 0; v < n; ++v) {
      const float lp = (over_cols ? at_col(v) : at_row(v)) - mx - logsum;
      const float pv = expf(lp);
      if (pv > 0.f) h -= pv * lp;                     // p log p -> 0 as p -> 0
    }
    bad |= h != h;
    entropy[i] = h;
  }
  if (nonfinite && bad) *nonfinite = 1u;
}

int check_logprob_table_args(int V, int n_cols, int norm, int64_t n_sel, int P) {
  if (V < 1 || V > 64) return fail(1, "logprob table: V must be in 1..64");
  if (n_cols < 1 || n_cols > V) return fail(1, "logprob table: n_cols must be in 1..V");
  if (norm != PG_TABLE_NORM_VOCAB && norm != PG_TABLE_NORM_COLUMNS)
    return fail(1, "logprob table: unknown norm (PG_TABLE_NORM_VOCAB or PG_TABLE_NORM_COLUMNS)");
  if (n_sel < 0 || P < 0) return fail(1, "logprob table: negative count");
  return 0;
}

int launch_logprob_table(hipStream_t st, const float* logits, int V, int compact, int width, const int32_t* idx,
                         const int32_t* row_map, const int32_t* cols, int n_cols, int norm, int64_t n_sel, int P, float* out,
                         float* entropy, unsigned* nonfinite) {
  if (int rc = check_logprob_table_args(V, n_cols, norm, n_sel, P)) return rc;
  const int64_t n = n_sel * P;
  if (n == 0) return 0;
  if (!logits || !idx || !cols || !out) return fail(1, "logprob table: null pointer");
  hipLaunchKernelGGL(logprob_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, logits, V, compact, width, idx,
                     row_map, cols, n_cols, norm, n_sel, P, out, entropy, nonfinite);
  PG_HIP(hipGetLastError());
  return 0;
}

__global__ void iter_counter_kernel(int32_t* d_iter, int set, int value) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *d_iter = set ? value : *d_iter + 1;
}
int launch_iter_counter(hipStream_t st, int32_t* d_iter, bool set, int value) {
  hipLaunchKernelGGL(iter_counter_kernel, dim3(1), dim3(64), 0, st, d_iter, set ? 1 : 0, value);
  PG_HIP(hipGetLastError());
  return 0;
}

bool DrawGuideDev::active() const { return bias || temps || (top_p == top_p && top_p < 1.0f); }

// what a guide's host tables hold, before anything is uploaded: the kernel assumes all of it
int check_draw_guide_tables(const pg_draw_guide* g, const char* who) {
  const std::string w(who);
  if (g->bias) {
    if (g->n_valid < 1 || g->n_valid > 32) return fail(1, w + ": the draw guide's n_valid must be in 1..32");
    if (g->width < 1 || g->bias_rows < 1) return fail(1, w + ": the draw guide's bias table needs width >= 1 and bias_rows >= 1");
    if ((double)g->bias_rows * g->width * g->n_valid > 2147483647.0) return fail(1, w + ": the draw guide's bias table has more than 2^31 - 1 entries");
    const int64_t cells = g->bias_rows * g->width;
    for (int64_t c = 0; c < cells; ++c) {
      const float* b = g->bias + c * g->n_valid;
      int allowed = 0;
      for (int j = 0; j < g->n_valid; ++j) {
        if (b[j] != b[j] || b[j] == INFINITY)
          return fail(1, w + ": the draw guide's bias holds " + (b[j] != b[j] ? "NaN" : "+inf") + " at row " + std::to_string(c / g->width) +
                             ", position " + std::to_string(c % g->width) + ", entry " + std::to_string(j) + " (entries are finite, or -inf = forbidden)");
        allowed += b[j] > -INFINITY;
      }
      if (!allowed)
        return fail(1, w + ": the draw guide's bias forbids every residue at row " + std::to_string(c / g->width) + ", position " +
                           std::to_string(c % g->width));
    }
  }
  if (g->temperatures) {
    if (g->n_temperatures < 1) return fail(1, w + ": the draw guide's temperature schedule is empty");
    for (int i = 0; i < g->n_temperatures; ++i)
      if (!(g->temperatures[i] > 0.f && g->temperatures[i] < INFINITY))
        return fail(1, w + ": the draw guide's temperature " + std::to_string(i) + " is not finite and > 0");
  }
  if (g->top_p == g->top_p && !(g->top_p > 0.f && g->top_p <= 1.0f)) return fail(1, w + ": the draw guide's top_p must be in (0, 1] (NaN = off)");
  return 0;
}

// the guide against the shape of the call that is about to draw with it: the kernel indexes the bias table by (token row, position,
// valid-list entry) and the schedule by the call-local iteration, so each of these is a bound on a device read
int check_draw_guide(const DrawGuideDev* g, const char* who, int width, int n_valid, int64_t token_rows, int64_t n_iters) {
  if (!g || !g->active()) return 0;
  const std::string w(who);
  if (g->bias) {
    if (g->width != width)
      return fail(1, w + ": the draw guide's bias table is " + std::to_string(g->width) + " positions wide, the token rows " + std::to_string(width));
    if (g->n_valid != n_valid)
      return fail(1, w + ": the draw guide's bias table has " + std::to_string(g->n_valid) + " entries per position, the valid list " + std::to_string(n_valid));
    if (g->bias_rows != 1 && g->bias_rows != token_rows)
      return fail(1, w + ": the draw guide's bias table has " + std::to_string(g->bias_rows) + " rows, which is neither 1 nor the call's " +
                         std::to_string(token_rows) + " token rows");
  }
  if (g->temps && g->n_temps < n_iters)
    return fail(1, w + ": the draw guide's temperature schedule has " + std::to_string(g->n_temps) + " entries, the call " + std::to_string(n_iters) +
                       " iterations");
  return 0;
}

static SampleArgs make_sample_args(const pg_sample_params* p, int iteration) {
  SampleArgs a;
  a.top_k = p->top_k;
  a.sample = iteration < p->burnin ? 1 : 0;   // sample=(ii < burnin), esm_sampler.py:231
  a.use_temp = (p->temperature == p->temperature) ? 1 : 0;  // NaN == None
  a.temperature = a.use_temp ? p->temperature : 1.0f;
  a.n_valid = p->n_valid;
  for (int j = 0; j < 32; ++j) a.valid_idx[j] = j < p->n_valid ? p->valid_idx[j] : 0;
  a.seed_lo = (uint32_t)(p->rng_seed & 0xffffffffu);
  a.seed_hi = (uint32_t)(p->rng_seed >> 32);
  a.stream = p->rng_stream;
  a.row_id_base = p->row_id_base;
  a.iter = (uint32_t)(p->iter_base + iteration);
  a.burnin = p->burnin;
  return a;
}

static GuidedSampleArgs make_guided_args(const pg_sample_params* p, int iteration, const DrawGuideDev* g) {
  GuidedSampleArgs a;
  a.s = make_sample_args(p, iteration);
  a.g.bias = g ? g->bias : nullptr;
  a.g.temps = g ? g->temps : nullptr;
  a.g.bias_per_row = g && g->bias_rows > 1 ? 1 : 0;
  a.g.use_top_p = g && g->top_p == g->top_p && g->top_p < 1.0f ? 1 : 0;
  a.g.top_p = a.g.use_top_p ? g->top_p : 1.0f;
  a.g.it = iteration;
  return a;
}

// graph state block: iteration counter + the call's sampling parameters and draw guide (passed by value: no host buffer has to
// outlive the call).  The block always holds a GuidedSampleArgs; the v1 kernel reads the SampleArgs it starts with.
__global__ void graph_state_kernel(int32_t* d_iter, int value, GuidedSampleArgs a) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    *d_iter = value;
    *(GuidedSampleArgs*)(d_iter + kGraphArgsOffset) = a;
  }
}
size_t graph_state_bytes() { return kGraphArgsOffset * 4 + sizeof(GuidedSampleArgs); }
int launch_graph_state(hipStream_t st, int32_t* d_iter, int iteration, const pg_sample_params* p, const DrawGuideDev* guide) {
  hipLaunchKernelGGL(graph_state_kernel, dim3(1), dim3(64), 0, st, d_iter, iteration, make_guided_args(p, 0, guide));
  PG_HIP(hipGetLastError());
  return 0;
}

int launch_mask_scatter(hipStream_t st, int32_t* tokens, int width, const int32_t* idx, const int32_t* row_map,
                        int64_t n_sel, int P, int mask_idx, const int32_t* d_iter) {
  const int64_t n = n_sel * P;
  if (n == 0) return 0;
  hipLaunchKernelGGL(mask_scatter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, tokens, width, idx, row_map,
                     n_sel, P, mask_idx, d_iter);
  PG_HIP(hipGetLastError());
  return 0;
}

int launch_sample_writeback(hipStream_t st, int32_t* tokens, int width, const float* logits, int V, int compact,
                            const int32_t* idx, const int32_t* row_map, int64_t n_sel, int P, const pg_sample_params* p,
                            int iteration, int32_t* sampled_tokens, const int32_t* d_iter, unsigned* nonfinite,
                            const DrawGuideDev* guide) {
  if (p->n_valid < 1 || p->n_valid > 32) return fail(1, "sample: n_valid must be in 1..32");
  for (int j = 0; j < p->n_valid; ++j)
    if (p->valid_idx[j] < 0 || p->valid_idx[j] >= V) return fail(1, "sample: valid_idx out of range");
  const int64_t n = n_sel * P;
  if (n == 0) return 0;
  if (guide && guide->active()) {      // pg_draw v2; the caller has checked the guide against this call's shape (check_draw_guide)
    const GuidedSampleArgs ga = make_guided_args(p, iteration, guide);
    hipLaunchKernelGGL(sample_writeback_kernel<true>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, tokens, width, logits, V,
                       compact, idx, row_map, n_sel, P, ga, sampled_tokens, d_iter, nonfinite);
    PG_HIP(hipGetLastError());
    return 0;
  }
  const SampleArgs a = make_sample_args(p, iteration);
  hipLaunchKernelGGL(sample_writeback_kernel<false>, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, tokens, width, logits, V,
                     compact, idx, row_map, n_sel, P, a, sampled_tokens, d_iter, nonfinite);      // one wave per draw
  PG_HIP(hipGetLastError());
  return 0;
}

}  // namespace pg
