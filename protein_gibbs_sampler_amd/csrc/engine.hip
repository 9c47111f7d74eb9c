// Engine implementation: weight upload (fp32 state dict -> device bf16/fp32), the ESM-1b forward as a
// chain of gfx950 kernels on one HIP stream, and the device-resident Gibbs loop
//   mask scatter -> forward -> LM head at the sampled rows -> draw + write-back
// which replaces the reference's per-iteration Python loop
// (/root/reference/src/pgen/esm_sampler.py:209-234) with zero host round trips per iteration.
#include <algorithm>

#include "engine.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "gemm_epilogue.h"
#include "ln_row.h"

namespace pg {

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
int fail(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
const char* last_error_cstr() { return g_last_error.c_str(); }

static thread_local std::string g_noted;
void note_kernel(const char* label, long tiles, int splits) {
  if (g_noted.size() > 512) return;
  if (!g_noted.empty()) g_noted += " + ";
  g_noted += label;
  if (tiles >= 0) g_noted += " " + std::to_string(tiles) + "t";
  if (splits > 1) g_noted += " x" + std::to_string(splits) + "k";
}
const std::string& noted_kernels() { return g_noted; }
void clear_noted_kernels() { g_noted.clear(); }

// ------------------------------------------------------------------------------------------------
// bumped whenever any workspace buffer is (re)allocated: a captured graph holds raw pointers and must be re-captured
static uint64_t g_alloc_epoch = 0;

int DevBuf::ensure(size_t need, hipStream_t s) {
  if (need <= bytes) return 0;
  ++g_alloc_epoch;
  size_t cap = need + need / 8 + 4096;
  void* np = nullptr;
  PG_HIP(hipMalloc(&np, cap));
  PG_HIP(hipMemsetAsync(np, 0, cap, s));
  if (p) {
    PG_HIP(hipStreamSynchronize(s));
    PG_HIP(hipFree(p));
  }
  p = np;
  bytes = cap;
  return 0;
}
void DevBuf::release() {
  if (p) (void)hipFree(p);
  p = nullptr;
  bytes = 0;
}

hipEvent_t Prof::get() {
  if (used == pool.size()) {
    hipEvent_t e;
    (void)hipEventCreate(&e);
    pool.push_back(e);
  }
  return pool[used++];
}
void Prof::reset() {
  recs.clear();
  used = 0;
}
void Prof::destroy() {
  for (auto e : pool) (void)hipEventDestroy(e);
  pool.clear();
  reset();
}

template <typename F> int Engine::timed(int cls, F&& f) {
  if (!prof.on || cls == PC_NONE) return f();
  hipEvent_t a = prof.get(), b = prof.get();
  clear_noted_kernels();
  PG_HIP(hipEventRecord(a, stream));
  int rc = f();
  PG_HIP(hipEventRecord(b, stream));
  prof.recs.push_back({cls, a, b, noted_kernels()});
  return rc;
}

const float* TensorMap::get(const std::string& name, int64_t numel, std::string& err) const {
  auto it = m.find(name);
  if (it == m.end()) {
    err = "missing tensor '" + name + "'";
    return nullptr;
  }
  if (it->second->numel != numel) {
    err = "tensor '" + name + "' has " + std::to_string(it->second->numel) + " elements, expected " + std::to_string(numel);
    return nullptr;
  }
  return it->second->data;
}

Engine::~Engine() {
  if (device >= 0) (void)hipSetDevice(device);
  for (void* p : owned) (void)hipFree(p);
  DevBuf* bufs[] = {&x, &h, &qkv, &ctx, &ffn, &sel_h, &sel_g, &logits, &d_tokens, &d_idx, &d_samp_tok, &d_samp_logits,
                    &d_rowmap, &scratch, &d_iter, &tmp_idx, &tmp_out, &x_sel, &ctx_sel, &h_sel, &ffn_sel, &ffn_f32, &scores, &splitk,
                    &chain_sync, &chain_part, &chain_snap, &repr_rows, &repr_pooled, &repr_ranges,
                    &contact_P, &contact_sums, &contact_logits, &contact_probs, &contact_attn, &contact_S};
  for (DevBuf* b : bufs) b->release();
  if (chain_err) (void)hipHostFree(chain_err);
  if (range_err) (void)hipHostFree(range_err);
  if (guide_bias_dev) (void)hipFree(guide_bias_dev);
  if (guide_temps_dev) (void)hipFree(guide_temps_dev);
  if (contact_w) (void)hipFree(contact_w);
  prof.destroy();
  if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
  if (own_stream) (void)hipStreamDestroy(own_stream);
}

// ------------------------------------------------------------------------------------------------
// weight upload
// ------------------------------------------------------------------------------------------------
namespace {
struct Uploader {
  Engine* e;
  const TensorMap* tm;
  const int precision;      // the engine's: OPS
  std::string err;

  // a device block the engine owns until it dies (keep), or one the caller frees; on failure null and err = "hipMalloc failed <what>"
  void* alloc(size_t bytes, const std::string& what, bool keep = true) {
    void* d = nullptr;
    if (hipMalloc(&d, bytes) != hipSuccess) { err = "hipMalloc failed " + what; return nullptr; }
    if (keep) e->owned.push_back(d);
    return d;
  }
  struct Staging {      // freed on every way out of its scope
    void* p;
    ~Staging() { if (p) (void)hipFree(p); }
  };
  float* f32(const std::string& name, int64_t numel) {
    const float* src = tm->get(name, numel, err);
    void* d = src ? alloc((size_t)numel * 4, "for " + name) : nullptr;
    if (!d) return nullptr;
    if (hipMemcpy(d, src, (size_t)numel * 4, hipMemcpyHostToDevice) != hipSuccess) { err = "H2D failed for " + name; return nullptr; }
    return (float*)d;
  }
  // concatenate several [n_i][K] fp32 matrices (each scaled) into one bf16 [sum n_i][K] device matrix + fp32 bias
  bool dense(DenseW& out, const std::vector<std::string>& prefixes, const std::vector<float>& scales, int n_each, int K) {
    const int parts = (int)prefixes.size();
    const int64_t N = (int64_t)n_each * parts;
    const int Kw = e->strict() ? 3 * K : K;      // strict: rows are [hi | lo | hi]
    const std::string what = "for " + prefixes[0];
    void* dw = alloc((size_t)N * Kw * 2, what);
    void* db = dw ? alloc((size_t)N * 4, what) : nullptr;
    Staging staging{db ? alloc((size_t)n_each * K * 4, what, false) : nullptr};
    void* tmp = staging.p;
    if (!tmp) return false;
    for (int p = 0; p < parts; ++p) {
      const float* w = tm->get(prefixes[p] + ".weight", (int64_t)n_each * K, err);
      const float* b = w ? tm->get(prefixes[p] + ".bias", n_each, err) : nullptr;
      if (!w || !b) return false;
      bool ok = hipMemcpy(tmp, w, (size_t)n_each * K * 4, hipMemcpyHostToDevice) == hipSuccess;
      if (e->strict())
        ok = ok && launch_split3_bf16(e->stream, (const float*)tmp, (bf16_t*)dw + (size_t)p * n_each * Kw, n_each, K, scales[p],
                                      false, true) == 0;
      else
        ok = ok && OPS(launch_f32_to_bf16, e->stream, (const float*)tmp, (bf16_t*)dw + (size_t)p * n_each * K, (int64_t)n_each * K, scales[p]) == 0;
      ok = ok && hipStreamSynchronize(e->stream) == hipSuccess;
      ok = ok && hipMemcpy((float*)db + (size_t)p * n_each, b, (size_t)n_each * 4, hipMemcpyHostToDevice) == hipSuccess;
      if (ok && scales[p] != 1.0f) ok = launch_scale_f32(e->stream, (float*)db + (size_t)p * n_each, n_each, scales[p]) == 0 &&
                                        hipStreamSynchronize(e->stream) == hipSuccess;
      if (!ok) { err = "upload failed for " + prefixes[p]; return false; }
    }
    out.w = (bf16_t*)dw;
    out.b = (float*)db;
    out.N = (int)N;
    out.K = K;
    return true;
  }
  // ESM-1's add_bias_kv: [bias_k | bias_v] as fp32 (strict mode) and as 16-bit operands of the engine's flavour
  bool bias_kv(EsmLayer& L, const std::string& kname, const std::string& vname, int d) {
    const float* bk = tm->get(kname, d, err);
    const float* bv = bk ? tm->get(vname, d, err) : nullptr;
    if (!bk || !bv) return false;
    void* d32 = alloc((size_t)2 * d * 4, "for " + kname);
    void* d16 = d32 ? alloc((size_t)2 * d * 2, "for " + kname) : nullptr;
    if (!d16) return false;
    bool ok = hipMemcpy(d32, bk, (size_t)d * 4, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy((float*)d32 + d, bv, (size_t)d * 4, hipMemcpyHostToDevice) == hipSuccess;
    ok = ok && OPS(launch_f32_to_bf16, e->stream, (const float*)d32, (bf16_t*)d16, 2 * d, 1.f) == 0;
    ok = ok && hipStreamSynchronize(e->stream) == hipSuccess;
    if (!ok) { err = "upload failed for " + kname; return false; }
    L.bias_kv32 = (float*)d32;
    L.bias_kv16 = (bf16_t*)d16;
    return true;
  }
  // a [q | k | v] projection with its rows regrouped per head (the fused column QKV + attention kernel's weight operand)
  bool headmajor(DenseW& out, const DenseW& in, int H) {
    void* dw = alloc((size_t)in.N * in.K * 2, "(head-major projection)");
    void* db = dw ? alloc((size_t)in.N * 4, "(head-major projection)") : nullptr;
    if (!db) return false;
    const bool ok = OPS(launch_headmajor_qkv, e->stream, in.w, in.b, (bf16_t*)dw, (float*)db, H, in.K) == 0 &&
                    hipStreamSynchronize(e->stream) == hipSuccess;
    if (!ok) { err = "head-major projection copy failed"; return false; }
    out.w = (bf16_t*)dw;
    out.b = (float*)db;
    out.N = in.N;
    out.K = in.K;
    return true;
  }
  bool ln(LnW& out, const std::string& prefix, int d) {
    out.g = f32(prefix + ".weight", d);
    out.b = out.g ? f32(prefix + ".bias", d) : nullptr;
    return out.g && out.b;
  }
};
}  // namespace

// ------------------------------------------------------------------------------------------------
// embedded models: the host side (what goes where; engine.h)
// ------------------------------------------------------------------------------------------------
namespace {
enum EmbedAxis { AX_SAME, AX_STREAM, AX_HEAD };
bool ends_with(const std::string& s, const char* t) {
  const size_t n = strlen(t);
  return s.size() >= n && !s.compare(s.size() - n, n, t);
}
}  // namespace

bool embedded_image(const std::string& name, const EmbedShape& es, const float* src, int64_t* rows, int64_t* cols, std::vector<float>* image) {
  const int64_t d = (int64_t)es.n_heads * es.width, D = (int64_t)es.n_heads * es.slot, f = es.d_ffn, V = es.vocab;
  EmbedAxis ra, ca = AX_SAME;
  int64_t R, C = 1;
  const bool w = ends_with(name, ".weight");
  const bool qkv = name.find("self_attn.q_proj.") != std::string::npos || name.find("self_attn.k_proj.") != std::string::npos ||
                   name.find("self_attn.v_proj.") != std::string::npos;
  if (name == "embed_tokens.weight") { ra = AX_SAME; R = V; ca = AX_STREAM; C = d; }
  else if (name == "lm_head.bias") { ra = AX_SAME; R = V; }
  else if (name.find("layer_norm") != std::string::npos) { ra = AX_STREAM; R = d; }
  else if (qkv) { ra = AX_HEAD; R = d; if (w) { ca = AX_STREAM; C = d; } }
  else if (name.find("self_attn.out_proj.") != std::string::npos) { ra = AX_STREAM; R = d; if (w) { ca = AX_HEAD; C = d; } }
  else if (name.find(".fc1.") != std::string::npos) { ra = AX_SAME; R = f; if (w) { ca = AX_STREAM; C = d; } }
  else if (name.find(".fc2.") != std::string::npos) { ra = AX_STREAM; R = d; if (w) { ca = AX_SAME; C = f; } }
  else if (name.rfind("lm_head.dense.", 0) == 0) { ra = AX_STREAM; R = d; if (w) { ca = AX_STREAM; C = d; } }
  else return false;
  if (!w && !ends_with(name, ".bias")) return false;
  *rows = R;
  *cols = C;
  if (!image) return true;
  const int half = es.width / 2, shift = (es.slot - es.width) / 2;
  auto to = [&](EmbedAxis a, int64_t i) { return a != AX_HEAD ? i : (i / es.width) * es.slot + (i % es.width) + ((i % es.width) < half ? 0 : shift); };
  const int64_t Rr = ra == AX_SAME ? R : D, Cr = ca == AX_SAME ? C : D;
  image->assign((size_t)(Rr * Cr), 0.0f);
  for (int64_t r = 0; r < R; ++r) {
    float* dst = image->data() + to(ra, r) * Cr;
    const float* s = src + r * C;
    if (ca != AX_HEAD) memcpy(dst, s, (size_t)C * 4);
    else for (int64_t c = 0; c < C; ++c) dst[to(ca, c)] = s[c];
  }
  return true;
}

int embedded_check(const pg_model_config* c, int head_slot) {
  if (c->arch != PG_ARCH_ESM2) return fail(PG_ERR_INVALID, "embedded head widths run for PG_ARCH_ESM2 only");
  const HeadWidth* hw = head_width(head_slot);
  if (!hw) return fail(PG_ERR_INVALID, "head slot " + std::to_string(head_slot) + ": a slot must be a built head width, " + head_widths_text(false));
  const int w = c->n_heads > 0 && c->d_model > 0 && c->d_model % c->n_heads == 0 ? c->d_model / c->n_heads : 0;
  if (w < 4 || w % 4 || w >= head_slot)
    return fail(PG_ERR_INVALID, "d_model " + std::to_string(c->d_model) + " with " + std::to_string(c->n_heads) + " heads in slots of " + std::to_string(head_slot) +
                                    ": an embedded head width must be a multiple of 4 and smaller than its slot");
  if (c->n_heads > hw->max_heads)
    return fail(PG_ERR_INVALID, "heads of " + std::to_string(w) + " in slots of " + std::to_string(head_slot) + ": the rotary and row kernels hold at most " +
                                    std::to_string(hw->max_heads) + " slots per row, not " + std::to_string(c->n_heads));
  return PG_OK;
}

int Engine::init_embedded(const pg_model_config* c, int head_slot, const pg_tensor* tensors, int n_tensors, int device_ordinal, int prec) {
  const int rc = embedded_check(c, head_slot);
  if (rc) return rc;
  pg_model_config run = *c;
  run.d_model = c->n_heads * head_slot;
  return init(&run, tensors, n_tensors, device_ordinal, prec, c->d_model / c->n_heads);
}

int Engine::init(const pg_model_config* c, const pg_tensor* tensors, int n_tensors, int device_ordinal, int prec, int live_head) {
  cfg = *c;
  d_live = live_head ? live_head * cfg.n_heads : cfg.d_model;
  precision = prec;
  device = -1;
  if (cfg.arch != PG_ARCH_ESM1B && cfg.arch != PG_ARCH_MSA1B && cfg.arch != PG_ARCH_ESM1 && cfg.arch != PG_ARCH_ESM2) return fail(PG_ERR_INVALID, "unknown arch");
  if (prec != PG_PREC_BF16 && prec != PG_PREC_FP32 && prec != PG_PREC_F16) return fail(PG_ERR_INVALID, "unknown precision mode");
  // d_model: a multiple of 64 for ESM-2 (esm2_t6_8M_UR50D: 320 = 5 x 64), of 128 for the other architectures.  The rule of 128 dates
  // from the first GEMM, whose tiles were 128 x 128 (N a multiple of 128).  Today every consumer of d_model on the ESM-2 path takes
  // multiples of 64: plan_gemm as N (64 x 64 tiles; 16 for the weight-streaming kernel) and as K (64; the strict mode's K' = 3K with
  // it), the split operand's 32-column groups, the row kernels (multiples of 4; the operand LayerNorm 32), the LM head and the
  // embedding (4); the forms that want more -- the LayerNorm-folding single-chain GEMM (K a multiple of 256), the fused row-LayerNorm
  // GEMM (N = 1280), the 128- and 256-wide tiles -- are admissions with a fallback, not requirements (DESIGN.md section 10 walks the
  // list).  The single-chain trunk (ESM-1b), the head-major column-attention weights and the tied-row kernels (MSA-1b) were not
  // walked, so those architectures keep the rule.  d_ffn stays at 128: the strict mode's fused GELU-and-split and the big tiles want
  // N = d_ffn in units of 256 / 128 and no released model needs less.
  if (cfg.d_model % (cfg.arch == PG_ARCH_ESM2 ? 64 : 128) || cfg.d_ffn % 128)
    return fail(PG_ERR_INVALID, cfg.arch == PG_ARCH_ESM2 ? "d_model must be a multiple of 64 (PG_ARCH_ESM2) and d_ffn of 128"
                                                         : "d_model and d_ffn must be multiples of 128");
  // head width (head_width.h): a width the attention and rotary kernels are built for, for this architecture; then no more heads than
  // the rotary and row kernels hold per row at that width; then a row width the row kernels take (ln_row.h: above 2560 features,
  // which only heads of 128 reach, whole 512-feature units)
  head_dim = cfg.n_heads > 0 && cfg.d_model % cfg.n_heads == 0 ? cfg.d_model / cfg.n_heads : 0;
  const HeadWidth* hw = head_width(head_dim);
  const std::string heads_of = "heads of " + std::to_string(head_dim);
  if (!hw)
    return fail(PG_ERR_INVALID, "d_model " + std::to_string(cfg.d_model) + " with " + std::to_string(cfg.n_heads) + " heads: head dim must be " +
                                    head_widths_text(true));
  if (hw->esm2_only && cfg.arch != PG_ARCH_ESM2)
    return fail(PG_ERR_INVALID, std::string(cfg.arch == PG_ARCH_ESM1B ? "ESM-1b" : cfg.arch == PG_ARCH_MSA1B ? "ESM-MSA-1b" : "ESM-1") + " with " + heads_of +
                                    ": head dim must be 64 for this architecture (" + heads_of + " run for PG_ARCH_ESM2 only)");
  if (cfg.n_heads > hw->max_heads)
    return fail(PG_ERR_INVALID, heads_of + ": the rotary and row kernels hold at most " + std::to_string(hw->max_heads) + " of them per row (d_model <= " +
                                    std::to_string(hw->max_heads * head_dim) + ": " + hw->model + "), not " + std::to_string(cfg.n_heads) + " (d_model " +
                                    std::to_string(cfg.d_model) + ")");
  if (!row_d_ok(cfg.d_model))
    return fail(PG_ERR_INVALID, "d_model " + std::to_string(cfg.d_model) + " with " + heads_of + ": the row kernels take up to 2560 features, and multiples of 512 up to 5120 above");
  if (cfg.vocab < 1 || cfg.vocab > 64) return fail(PG_ERR_INVALID, "vocab must be in 1..64");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(PG_ERR_NO_DEVICE, "no HIP device visible: this engine has no CPU fallback");
  if (device_ordinal < 0 || device_ordinal >= ndev) return fail(PG_ERR_INVALID, "Invalid cuda device number: cuda:" + std::to_string(device_ordinal));
  PG_HIP(hipSetDevice(device_ordinal));
  device = device_ordinal;
  PG_HIP(hipStreamCreateWithFlags(&own_stream, hipStreamNonBlocking));
  stream = own_stream;

  // an embedded model: the run-shape images of its natural tensors, alive until the upload below is done
  std::vector<std::vector<float>> images;
  std::vector<pg_tensor> run_tensors;
  if (live_head) {
    const EmbedShape es = {cfg.n_heads, live_head, head_dim, cfg.d_ffn, cfg.vocab};
    images.resize(n_tensors);
    for (int i = 0; i < n_tensors; ++i) {
      int64_t r = 0, cc = 0;
      if (!tensors[i].name || !embedded_image(tensors[i].name, es, nullptr, &r, &cc, nullptr)) continue;      // not a tensor the engine reads
      if (tensors[i].numel != r * cc)
        return fail(PG_ERR_WEIGHTS, std::string("tensor '") + tensors[i].name + "' has " + std::to_string(tensors[i].numel) + " elements, expected " + std::to_string(r * cc));
      embedded_image(tensors[i].name, es, tensors[i].data, &r, &cc, &images[i]);
      run_tensors.push_back({tensors[i].name, images[i].data(), (int64_t)images[i].size()});
    }
    tensors = run_tensors.data();
    n_tensors = (int)run_tensors.size();
  }
  TensorMap tm;
  for (int i = 0; i < n_tensors; ++i)
    if (tensors[i].name) tm.m[tensors[i].name] = &tensors[i];
  Uploader up{this, &tm, prec, ""};
  const int d = cfg.d_model, f = cfg.d_ffn, V = cfg.vocab;
  // head_dim^-0.5, folded into W_q and b_q.  A power of two at heads of 64 and 16 (exact in bf16).  32^-0.5 and 128^-0.5 are none:
  // still folded, as an fp32 factor applied to the fp32 checkpoint values BEFORE they are rounded to the 16-bit operand (or split into
  // the strict mode's bf16 pair) -- the kernels stay scale-free and the only new rounding is that fp32 product, 2^-24 relative, under
  // an operand rounding of 2^-9 / 2^-12 / 2^-17
  // An embedded model: its own width^-0.5, not the slot's -- the scores are those of the live head
  const float qs = live_head ? (float)pow((double)live_head, -0.5) : hw->q_scale;
  bool ok = true;
  ok = ok && (embed = up.f32("embed_tokens.weight", (int64_t)V * d));
  // ESM-2 has no position table (pos stays null: embed_ln_kernel adds nothing) -- positions enter through the rotation of q and k
  if (!esm2()) ok = ok && (pos = up.f32("embed_positions.weight", (int64_t)(cfg.max_positions + cfg.pad_idx + 1) * d));
  if (esm1()) {
    // untied output projection straight from the residual stream: logits = x embed_out^T + embed_out_bias
    ok = ok && (embed_out = up.f32("embed_out.weight", (int64_t)V * d));
    ok = ok && (head_bias = up.f32("embed_out.bias", V));
  } else {
    if (!esm2()) ok = ok && up.ln(ln_before, "emb_layer_norm_before", d);      // ESM-2: none (ln_before.g stays null)
    ok = ok && up.ln(ln_after, "emb_layer_norm_after", d);
    ok = ok && up.dense(head_dense, {"lm_head.dense"}, {1.0f}, d, d);
    ok = ok && up.ln(head_ln, "lm_head.layer_norm", d);
    ok = ok && (head_bias = up.f32("lm_head.bias", V));
  }
  if (ok && cfg.arch != PG_ARCH_MSA1B) {
    esm_layers.resize(cfg.n_layers);
    for (int i = 0; ok && i < cfg.n_layers; ++i) {
      const std::string p = "layers." + std::to_string(i) + ".";
      EsmLayer& L = esm_layers[i];
      ok = ok && up.ln(L.ln1, p + "self_attn_layer_norm", d);
      ok = ok && up.dense(L.qkv, {p + "self_attn.q_proj", p + "self_attn.k_proj", p + "self_attn.v_proj"}, {qs, 1.f, 1.f}, d, d);
      ok = ok && up.dense(L.out, {p + "self_attn.out_proj"}, {1.f}, d, d);
      ok = ok && up.ln(L.ffn.ln, p + "final_layer_norm", d);
      ok = ok && up.dense(L.ffn.fc1, {p + "fc1"}, {1.f}, f, d);
      ok = ok && up.dense(L.ffn.fc2, {p + "fc2"}, {1.f}, d, f);
      if (ok && esm1()) ok = up.bias_kv(L, p + "self_attn.bias_k", p + "self_attn.bias_v", d);
    }
  } else if (ok) {
    ok = ok && (msa_pos = up.f32("msa_position_embedding", (int64_t)cfg.max_msa_rows * d));
    msa_layers.resize(cfg.n_layers);
    for (int i = 0; ok && i < cfg.n_layers; ++i) {
      const std::string p = "layers." + std::to_string(i) + ".";
      MsaLayer& L = msa_layers[i];
      const std::string r = p + "row_self_attention.", cpre = p + "column_self_attention.", ff = p + "feed_forward_layer.";
      ok = ok && up.ln(L.ln_row, r + "layer_norm", d);
      ok = ok && up.dense(L.row_qkv, {r + "layer.q_proj", r + "layer.k_proj", r + "layer.v_proj"}, {1.f, 1.f, 1.f}, d, d);
      ok = ok && up.dense(L.row_out, {r + "layer.out_proj"}, {1.f}, d, d);
      ok = ok && up.ln(L.ln_col, cpre + "layer_norm", d);
      ok = ok && up.dense(L.col_qkv, {cpre + "layer.q_proj", cpre + "layer.k_proj", cpre + "layer.v_proj"}, {qs, 1.f, 1.f}, d, d);
      if (ok && !strict()) ok = up.headmajor(L.col_qkv_hm, L.col_qkv, cfg.n_heads);
      ok = ok && up.dense(L.col_out, {cpre + "layer.out_proj"}, {1.f}, d, d);
      ok = ok && up.ln(L.ffn.ln, ff + "layer_norm", d);
      ok = ok && up.dense(L.ffn.fc1, {ff + "layer.fc1"}, {1.f}, f, d);
      ok = ok && up.dense(L.ffn.fc2, {ff + "layer.fc2"}, {1.f}, d, f);
    }
  }
  if (!ok) return fail(PG_ERR_WEIGHTS, up.err.empty() ? std::string("weight upload failed") : up.err);
  if (esm2()) {
    if (cfg.max_positions < 1) return fail(PG_ERR_INVALID, "max_positions must be positive");
    rope_rows = cfg.max_positions + 2;              // like the learned tables
    const std::vector<float> tab = rope_table(rope_rows, head_dim, live_head);
    void* dt = nullptr;
    PG_HIP(hipMalloc(&dt, tab.size() * 4));
    owned.push_back(dt);
    PG_HIP(hipMemcpy(dt, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
    rope_tab = (float*)dt;
  }
  if (cfg.arch == PG_ARCH_ESM1B && !strict() && OPS(chain_trunk_ok, 32, d, f, cfg.n_heads)) {
    // the persistent single-chain trunk reads its weights through one device table
    std::vector<PgChainLayerW> tab(cfg.n_layers);
    for (int i = 0; i < cfg.n_layers; ++i) {
      const EsmLayer& L = esm_layers[i];
      tab[i] = {L.ln1.g, L.ln1.b, L.qkv.w, L.qkv.b, L.out.w, L.out.b, L.ffn.ln.g, L.ffn.ln.b, L.ffn.fc1.w, L.ffn.fc1.b, L.ffn.fc2.w, L.ffn.fc2.b};
    }
    void* dt = nullptr;
    PG_HIP(hipMalloc(&dt, tab.size() * sizeof(PgChainLayerW)));
    owned.push_back(dt);
    PG_HIP(hipMemcpy(dt, tab.data(), tab.size() * sizeof(PgChainLayerW), hipMemcpyHostToDevice));
    chain_layers = (PgChainLayerW*)dt;
    PG_HIP(hipHostMalloc((void**)&chain_err, sizeof(unsigned), hipHostMallocMapped));
    *chain_err = 0;
  }
  PG_HIP(hipHostMalloc((void**)&range_err, sizeof(unsigned), hipHostMallocMapped));
  *range_err = 0;
  PG_HIP(hipStreamSynchronize(stream));
  return PG_OK;
}

int Engine::range_check() {
  if (!range_err || !*range_err) return PG_OK;
  *range_err = 0;
  return fail(PG_ERR_RANGE, precision == PG_PREC_F16
                                ? "non-finite logits: a 16-bit tensor of the forward left the fp16 range (+-65504) -- run this model with "
                                  "precision bf16 (or fp32); the results of this call are invalid"
                                : "non-finite logits (NaN / inf in the weights or an overflow in the forward); the results of this call are invalid");
}

// esm_trunk's own predicate for the persistent launch (a call that would not take it is not worth a snapshot, a log entry and a
// forced synchronisation every kChainLogMax calls): no <pad> batch, the rows fit one or two 16-row MFMA tiles, and the
// LayerNorm-folding weight-streaming GEMMs accept the shape
bool Engine::chain_may_run(int B, int T) const {
  if (!(chain_layers && chain_err && !chain_disabled && !esm_pad_in_batch && T >= 1 && T <= 32 && (int64_t)B * T <= 32)) return false;
  const int64_t M = (int64_t)B * T;
  const int Mi = round_up((int)M, 16);
  const int d = cfg.d_model, f = cfg.d_ffn;
  if (batch_rows_for(B, T) > 2048 && Mi < 64) return false;                  // a tiny shard of a big job runs 64-row tiles (sel_gemm_rows)
  return gemm_ln_skinny_ok(Mi, 3 * d, d) && gemm_ln_skinny_ok(Mi, f, d) && OPS(chain_trunk_ok, Mi, d, f, cfg.n_heads);
}

int Engine::chain_log_call(int32_t* d_tok, int B, int T, const int32_t* d_idx_, int n_iters, int P, const pg_sample_params* sp,
                           float* lg, int32_t* st) {
  int rc;
  if (chain_log.size() >= kChainLogMax) {              // bound the log: check (and, if need be, recover) now
    PG_HIP(hipStreamSynchronize(stream));
    if ((rc = chain_check()) && !chain_replay_ok) return rc;
    chain_retry = false;
    if (chain_disabled) return PG_OK;
  }
  if ((rc = chain_snap.ensure(kChainSnapBytes * kChainLogMax, stream))) return rc;
  const size_t off = chain_log.size() * kChainSnapBytes;
  PG_HIP(hipMemcpyAsync((char*)chain_snap.p + off, d_tok, (size_t)B * T * 4, hipMemcpyDeviceToDevice, stream));
  chain_log.push_back({d_tok, B, T, d_idx_, n_iters, P, *sp, lg, st, off});
  return PG_OK;
}

// Call right after a synchronisation of `stream`.  PG_OK when no barrier of the persistent trunk timed out since the last check.
// Otherwise the kernel is switched off for this engine, the logged device-pointer calls are replayed on the per-layer launches
// (PG_OK if that was all there was to repair: pg_engine_synchronize), and a host-buffer entry point that is in flight is told to
// run again (chain_retry + PG_ERR_HIP: its inputs are intact in the caller's buffers).
int Engine::chain_check() {
  chain_replay_ok = false;
  if (!chain_err || !*chain_err) { chain_log.clear(); return PG_OK; }
  *chain_err = 0;
  // the timed-out launch may have left garbage activations behind, and the draw / log-probability kernels that ran on them may
  // have raised the non-finite flag: that verdict belongs to the abandoned launch, not to the replay (or the caller's retry) that
  // follows -- they raise it again if the logits really are non-finite
  if (range_err) *range_err = 0;
  if (chain_sync.p) (void)hipMemsetAsync(chain_sync.p, 0, chain_sync.bytes, stream);
  if (graph_exec) { (void)hipGraphExecDestroy(graph_exec); graph_exec = nullptr; graph_key.reset(); }   // it holds the persistent launch
  if (!chain_disabled)
    fprintf(stderr, "pgibbs: a device-wide barrier of the persistent single-chain trunk timed out (another persistent grid on this GPU?); "
                    "this engine uses the per-layer launches from now on\n");
  chain_disabled = true;
  chain_retry = true;
  if (!chain_log.empty()) {
    std::vector<ChainCall> log;
    log.swap(chain_log);
    std::vector<int32_t*> seen;
    for (const ChainCall& c : log) {
      if (std::find(seen.begin(), seen.end(), c.d_tok) == seen.end()) {
        seen.push_back(c.d_tok);
        PG_HIP(hipMemcpyAsync(c.d_tok, (char*)chain_snap.p + c.snap_off, (size_t)c.B * c.T * 4, hipMemcpyDeviceToDevice, stream));
      }
      int rc = esm_gibbs_device(c.d_tok, c.B, c.T, c.d_idx, c.n_iters, c.P, &c.sp, c.lg, c.st);
      if (rc) return rc;
    }
    PG_HIP(hipStreamSynchronize(stream));
    chain_replay_ok = true;
    return fail(PG_ERR_HIP, "single-chain trunk: a device-wide barrier timed out; the device-pointer calls since the last "
                            "synchronisation were run again on the per-layer launches (their results are valid)");
  }
  return fail(PG_ERR_HIP, "single-chain trunk: a device-wide barrier timed out (is another persistent kernel sharing this GPU? "
                          "PGIBBS_CHAIN_TRUNK=0 selects the per-layer launches); the results of this call are invalid");
}

// ------------------------------------------------------------------------------------------------
// forward ops: the launchers every 16-bit projection, every LayerNorm and the embedding go through (engine.h)
// ------------------------------------------------------------------------------------------------
int Engine::dense(int cls, const bf16_t* a, const DenseW& W, void* out, int rows, int epi, int m_live, bool use_splitk) {
  // the scratch first, its size after: splitk_ws may grow the buffer
  float* ws = use_splitk ? splitk_ws(rows, W.N, W.K, batch_rows) : nullptr;
  const size_t ws_bytes = use_splitk ? splitk.bytes : 0;
  return timed(cls, [&] { return OPS(launch_gemm_bf16, stream, a, W.w, W.b, out, rows, W.N, W.K, W.K, W.K, W.N, epi, ws, ws_bytes, m_live); });
}

int Engine::dense_ln(const float* x, const LnW& ln, const DenseW& W, bf16_t* out, int rows, int epi) {
  return timed(PC_GEMM, [&] { return OPS(launch_gemm_ln_skinny, stream, x, W.K, ln.g, ln.b, cfg.layer_norm_eps, W.w, W.b, out, rows, W.N, W.K, W.K, W.N, epi); });
}

int Engine::layer_norm(const float* x, const LnW& ln, bf16_t* h, int64_t M, bool dup, int colmajor_R, int colmajor_C) {
  return timed(PC_LN, [&] { return OPS(launch_layernorm_bf16, stream, x, ln.g, ln.b, h, M, cfg.d_model, cfg.layer_norm_eps, strict(), colmajor_R, colmajor_C, dup, d_live); });
}

// x = embedding (+ positions, emb_layer_norm_before) of M tokens, T per sequence; rows_per_msa > 0: an alignment batch (its row
// positions, no token dropout).  first_ln: in the same pass over the row also h = that LayerNorm of x, the first projection's operand
int Engine::embed_rows(const int32_t* d_tok, int64_t M, int T, int rows_per_msa, const LnW* first_ln) {
  return timed(PC_EMBED, [&] {
    return OPS(launch_embed_ln, stream, d_tok, embed, pos, msa_pos, ln_before.g, ln_before.b, x.as<float>(), M, T, cfg.d_model, cfg.pad_idx,
                           cfg.mask_idx, rows_per_msa ? 0 : cfg.token_dropout, rows_per_msa, cfg.layer_norm_eps, first_ln ? first_ln->g : nullptr,
                           first_ln ? first_ln->b : nullptr, first_ln ? h.as<bf16_t>() : nullptr, embed_scale(), d_live);
  });
}

// strict precision mode GEMM: one bf16 MFMA GEMM over the K-concatenated split operands (engine.h) reproduces an
// fp32 x fp32 product to ~2^-17 relative (the dropped lo.lo term); fp32 accumulation, small terms first.
int Engine::dense3(const bf16_t* x3, const DenseW& W, float* out, int Mp, bool accumulate) {
  return timed(PC_GEMM, [&] { return launch_gemm_split3(stream, x3, W.w, W.b, out, Mp, W.N, W.K, W.N, accumulate ? EPI_F32_RESID : EPI_F32); });
}

// GEMM height for the B*P selected rows (pruned last layer, LM head) and for a forward of few token rows.  Up to 48 rows would
// take the weight-streaming kernel, whose k order differs from the tile kernels': fine for a few chains (its regime), but in a
// big batch the height is raised to one 64-row tile so that a shard and the whole batch see the same arithmetic.
int Engine::sel_gemm_rows(int64_t n_sel, int64_t Np) const {
  if (n_sel > 256) return (int)Np;
  const int r = round_up((int)n_sel, 16);
  return (batch_rows > 2048 && r < 64) ? 64 : r;
}

// The split operand rows are [lo | hi | hi] per 32 columns; the fused three-product kernel reads [lo | hi] only (gemm_w16.hip), the
// plain kernels over K' = 3K all three blocks.  A producer (LayerNorm, fc1's epilogue) skips the duplicate block -- a fifth of a
// LayerNorm's traffic, a third of fc1's stores -- exactly when its consumer is the fused kernel.
bool Engine::dense3_wants_dup(const DenseW& W, int Mp, bool gelu) const {
  static const int nodup = env_int("PGIBBS_SPLIT3_NODUP", 1);
  if (!nodup) return true;
  if (gelu && W.N % 256 == 0 && Mp % 256 == 0) return false;          // dense3_gelu's fused form: always the 16-wave kernel
  return !gemm_split3_fused(Mp, W.N, W.K, EPI_F32);
}

// strict fc1: ffn = split3(gelu(x3 . W^T + b)).  Fused into the GEMM's epilogue when the 16-wave kernel can take the shape
// (d_ffn a multiple of 256), else an fp32 GEMM followed by the GELU-and-split pass.  The fused epilogue evaluates the GELU
// with the degree-5 fit of log2 Phi(-|x|) that the bf16 mode uses (abs error 3.2e-6, below the 2^-17 relative error of the
// split products at |x| ~ 1; 9 instead of 22 issue slots per element in an epilogue that nothing overlaps), the pass with erff.
// Full-size strict logits against the oracle with this: ESM-1b 5.8e-4, MSA-1b 4.6e-4 (5.7e-4 / 4.0e-4 with erff).
int Engine::dense3_gelu(const bf16_t* x3, const DenseW& W, int Mp, const DenseW* next) {
  if (W.N % 256 == 0 && Mp % 256 == 0) {
    // the rows leave without their duplicate hi block when the projection that reads them (fc2) never looks at it
    const int epi = next && !dense3_wants_dup(*next, Mp) ? EPI_SPLIT2_GELU : EPI_SPLIT3_GELU;
    return timed(PC_GEMM, [&] { return launch_gemm_split3(stream, x3, W.w, W.b, ffn.as<bf16_t>(), Mp, W.N, W.K, 3 * W.N, epi); });
  }
  int rc = ffn_f32.ensure((size_t)Mp * W.N * 4, stream);       // fp32 intermediate of the unfused form only
  if (rc || (rc = dense3(x3, W, ffn_f32.as<float>(), Mp, false))) return rc;
  return timed(PC_LN, [&] { return launch_split3_bf16(stream, ffn_f32.as<float>(), ffn.as<bf16_t>(), Mp, W.N, 1.f, true, false); });
}

// A K-split sums in a different order than the one-pass kernels, so the decision must not depend on how a batch is sharded:
// it is taken on the forward's token rows M (`batch_rows`), also for the pruned last layer whose GEMMs see only the B*P selected
// rows -- a 32-chain shard of config 3 (8256 token rows, 800 selected) must give the same logits bit for bit as the whole
// 256-chain batch (6400 selected), and did not while this looked at the selected rows.
// The scratch holds every K-split the launcher will run at this depth (gemm_splitk_ws_bytes: 4 at d_ffn 5120, 8 at 10240), so whether
// fc2 is split never depends on what this engine's grow-only buffer was sized for by an earlier call.
float* Engine::splitk_ws(int rows, int n, int K, int64_t batch_rows) {
  if (rows > 2048 || batch_rows > 2048) return nullptr;
  const size_t need = OPS(gemm_splitk_ws_bytes, rows, n, K);
  if (splitk.bytes < need && splitk.ensure(need, stream)) return nullptr;
  return splitk.as<float>();
}

// The rotary embedding's table [rows][hd], hd = the head dimension (64, or 32 / 128 / 16 with 16 / 64 / 8 in place of 32 below): [t][i] = cos,
// [t][32 + i] = sin of ang[t][i] = float(t) * inv_freq[i] (an fp32 product),
// inv_freq[i] = 1 / 10000^(2i / 64) in fp32 as fair-esm's RotaryEmbedding holds it (1.0 / (10000 ** (arange(0, 64, 2).float() / 64))).
// The power is taken in double and rounded to fp32 -- the values torch's fp32 pow and glibc's powf give; a vectorised fp32 pow (numpy's)
// is one ulp off at i = 5 and 27 --, the cosine and sine of the fp32 angle in double, rounded to fp32.
// An embedded head (live > 0: heads of `live` in slots of hd): column i < live / 2 of a half carries frequency i of a head of `live`,
// the other columns of the half cos = 1 and sin = 0 (they rotate structural zeros).
std::vector<float> rope_table(int rows, int hd, int live) {
  const int half = hd / 2, lhalf = live > 0 ? live / 2 : half;
  std::vector<float> tab((size_t)rows * hd);
  for (int i = 0; i < half; ++i) {
    if (i >= lhalf) {
      for (int t = 0; t < rows; ++t) tab[(size_t)t * hd + i] = 1.0f, tab[(size_t)t * hd + half + i] = 0.0f;
      continue;
    }
    // the exponent as torch forms it, a float32 quotient: exact for the built widths (powers of two), rounded for a head of 24
    const float inv_freq = 1.0f / (float)pow(10000.0, (double)((float)(2 * i) / (float)(2 * lhalf)));
    for (int t = 0; t < rows; ++t) {
      const float ang = (float)t * inv_freq;
      tab[(size_t)t * hd + i] = (float)cos((double)ang);
      tab[(size_t)t * hd + half + i] = (float)sin((double)ang);
    }
  }
  return tab;
}

int Engine::rope(void* qkv_rows, int64_t M, int T) {
  if (!esm2()) return PG_OK;
  return timed(PC_ROPE, [&] { return OPS(launch_rope, stream, qkv_rows, strict(), rope_tab, rope_rows, M, T, cfg.n_heads, 3 * cfg.d_model, head_dim); });
}

int Engine::size_activations(int64_t Mp) {
  if (Mp > 0x7fffffff / 4) return fail(PG_ERR_INVALID, "too many tokens in one call");
  const size_t d = cfg.d_model, f = cfg.d_ffn;
  const size_t w = strict() ? 3 : 1;                 // strict: h, ctx and ffn hold [lo | hi | hi] rows, qkv is fp32
  // Heads of 128 (ESM-2 15B) are the first models whose 16-bit activation buffers pass 2^31 bytes in one call (fc1's output at config
  // 2: 66048 x 20480 x 2 B = 2.7 GB; the strict mode's fp32 qkv 4.1 GB).  Every kernel that walks an [M][ld] buffer forms its row or
  // band base as a 64-bit product and keeps only per-band offsets in 32 bits (the list: DESIGN.md section 10, "Buffers of 2 GB and
  // more"), so no limit is set here beyond the row count above; tests/test_gpu_esm2_15b.py runs such a call against its shards.
  int rc;
  if ((rc = x.ensure((size_t)Mp * d * 4, stream))) return rc;
  if ((rc = h.ensure((size_t)Mp * w * d * 2, stream))) return rc;
  if ((rc = qkv.ensure((size_t)Mp * 3 * d * (strict() ? 4 : 2), stream))) return rc;
  if ((rc = ctx.ensure((size_t)Mp * w * d * 2, stream))) return rc;
  return ffn.ensure((size_t)Mp * w * f * 2, stream);
}

int Engine::ffn_strict(const FfnW& F, int Mi, int64_t M) {
  float* X = x.as<float>();
  bf16_t* H3 = h.as<bf16_t>();
  int rc;
  if ((rc = layer_norm(X, F.ln, H3, M, dense3_wants_dup(F.fc1, Mi, true)))) return rc;
  if ((rc = dense3_gelu(H3, F.fc1, Mi, &F.fc2))) return rc;
  return dense3(ffn.as<bf16_t>(), F.fc2, X, Mi, true);
}

template <typename Attn>
int Engine::strict_attention(const LnW& ln, const DenseW& qkv_w, const DenseW& out_w, int Mi, int64_t M, Attn&& attn) {
  float* X = x.as<float>();
  bf16_t* H3 = h.as<bf16_t>();
  int rc;
  if ((rc = layer_norm(X, ln, H3, M, dense3_wants_dup(qkv_w, Mi)))) return rc;
  if ((rc = dense3(H3, qkv_w, qkv.as<float>(), Mi, false))) return rc;
  if ((rc = attn(dense3_wants_dup(out_w, Mi) ? cfg.d_model : -cfg.d_model))) return rc;
  return dense3(ctx.as<bf16_t>(), out_w, X, Mi, true);
}

int Engine::ffn_block(const DenseW& out, const FfnW& F, const LnW* next_ln, int Mi, int64_t M, bool folded) {
  float* X = x.as<float>();
  bf16_t* Hh = h.as<bf16_t>();
  bf16_t* CTX = ctx.as<bf16_t>();
  bf16_t* FFN = ffn.as<bf16_t>();
  int rc;
  if (folded) {
    // the out-projection does not say its live rows and all three are "gemm_other": the launch-bound regime is not timed per projection
    if ((rc = dense(PC_GEMM, CTX, out, X, Mi, EPI_F32_RESID))) return rc;
    if ((rc = dense_ln(X, F.ln, F.fc1, FFN, Mi, EPI_BF16_GELU))) return rc;
    return dense(PC_GEMM, FFN, F.fc2, X, Mi, EPI_F32_RESID, (int)M, true);
  }
  if ((rc = resid_gemm_ln(PC_GEMM_OUT, CTX, out, X, Mi, M, F.ln, Hh))) return rc;
  if ((rc = dense(PC_GEMM_FC1, Hh, F.fc1, FFN, Mi, EPI_BF16_GELU, (int)M))) return rc;
  if (next_ln) return resid_gemm_ln(PC_GEMM_FC2, FFN, F.fc2, X, Mi, M, *next_ln, Hh, true);
  return dense(PC_GEMM_FC2, FFN, F.fc2, X, Mi, EPI_F32_RESID, (int)M, true);
}

bool Engine::prune_last(int64_t n_draws, int64_t token_rows) const {
  static const int prune = env_int("PGIBBS_PRUNE_LAST", 1);
  return prune && !strict() && n_draws > 0 && 2 * n_draws < token_rows;
}

int Engine::pruned_tail(const DenseW& out, const FfnW& F, const int32_t* sel_idx, const int32_t* sel_row_map, int P, int width,
                        int64_t n_sel, const int32_t* d_iter_, int Ni, bool ln_in_gemm) {
  const int d = cfg.d_model, f = cfg.d_ffn;
  const int64_t Np = round_up64(n_sel, kRowPad);
  int rc;
  if ((rc = x_sel.ensure((size_t)Np * d * 4, stream)) || (rc = ctx_sel.ensure((size_t)Np * d * 2, stream)) ||
      (rc = h_sel.ensure((size_t)Np * d * 2, stream)) || (rc = ffn_sel.ensure((size_t)Np * f * 2, stream))) return rc;
  float* XS = x_sel.as<float>();
  bf16_t* HS = h_sel.as<bf16_t>();
  bf16_t* FS = ffn_sel.as<bf16_t>();
  rc = timed(PC_HEAD, [&] {
    int r2 = launch_gather_rows(stream, x.as<float>(), XS, sel_idx, sel_row_map, P, width, n_sel, d * 4, d_iter_);
    if (r2) return r2;
    return launch_gather_rows(stream, ctx.as<bf16_t>(), ctx_sel.as<bf16_t>(), sel_idx, sel_row_map, P, width, n_sel, d * 2, d_iter_);
  });
  if (rc) return rc;
  // ffn_block's steps on the compact rows -- a body of its own: other buffers, Ni rows under one class, no projection says its live
  // rows (not the same request as saying Ni or n_sel), and the LayerNorm is folded by what Ni allows, not by the trunk's regime alone
  if ((rc = dense(PC_GEMM, ctx_sel.as<bf16_t>(), out, XS, Ni, EPI_F32_RESID))) return rc;
  if (ln_in_gemm && gemm_ln_skinny_ok(Ni, f, d)) {
    if ((rc = dense_ln(XS, F.ln, F.fc1, FS, Ni, EPI_BF16_GELU))) return rc;
  } else {
    if ((rc = layer_norm(XS, F.ln, HS, n_sel))) return rc;
    if ((rc = dense(PC_GEMM, HS, F.fc1, FS, Ni, EPI_BF16_GELU))) return rc;
  }
  return dense(PC_GEMM, FS, F.fc2, XS, Ni, EPI_F32_RESID, 0, true);
}

int Engine::trunk(const int32_t* d_tok, int B, int R, int C, const int32_t* sel_idx, const int32_t* sel_row_map, int P, int64_t n_sel,
                  const int32_t* d_iter_) {
  return cfg.arch == PG_ARCH_MSA1B ? msa_trunk(d_tok, B, R, C, sel_idx, sel_row_map, P, n_sel) : esm_trunk(d_tok, B, C, sel_idx, P, n_sel, d_iter_);
}

// The representations tap (engine.h): layer l of the numbering fair-esm's repr_layers uses is in x.  Layer n_layers goes through
// emb_layer_norm_after (ESM-1 has none: the raw stream), every other layer is copied; both forms write the live columns only and
// zeros at <pad> rows.  The means are taken over the staged rows of the same call.
int Engine::tap_layer(int l) {
  if (!tap || tap->next >= tap->layers.size() || tap->layers[tap->next] != l) return PG_OK;
  const size_t i = tap->next++;
  const int64_t M = (int64_t)tap->B * tap->T;
  const bool ln = l == cfg.n_layers && !esm1();
  float* rows = tap->rows + i * (size_t)M * d_live;
  int rc = timed(PC_REPR_ROWS, [&] {
    return launch_repr_rows(stream, x.as<float>(), ln ? ln_after.g : nullptr, ln ? ln_after.b : nullptr, tap->d_tok, cfg.pad_idx, rows, M,
                            cfg.d_model, d_live, cfg.layer_norm_eps);
  });
  if (rc || !tap->pooled) return rc;
  float* means = tap->pooled + i * (size_t)tap->n_pools * tap->B * d_live;
  return timed(PC_REPR_POOL, [&] { return launch_repr_pool(stream, rows, tap->d_pools, means, tap->n_pools, tap->B, tap->T, d_live); });
}

// The contacts tap (engine.h): block l's qkv is ready.  Its attention probabilities go to the one-layer staging buffer, or to the
// caller's slot when the map of this layer was asked for, and -- with a head to fold -- into the running contact logits.  Layers come
// in ascending order, so the channel order l * n_heads + h of the regression is fixed
int Engine::tap_attention(int l, const void* qkv_rows) {
  if (!ctap) return PG_OK;
  ContactTap& t = *ctap;
  const int d = cfg.d_model, H = cfg.n_heads;
  const size_t map = (size_t)t.B * H * t.T * t.T;
  float* Pl = contact_P.as<float>();
  if (t.next_attn < t.attn_layers.size() && t.attn_layers[t.next_attn] == l) Pl = t.attn_out + map * t.next_attn++;
  const SeqLayout chain = {1, t.T, 0, 1};
  const int32_t* key_tok = esm_pad_in_batch ? t.d_tok : nullptr;
  int rc = timed(PC_ATTN_PROBS, [&] {
    if (strict()) return launch_attn_probs_f32(stream, (const float*)qkv_rows, Pl, t.B, t.T, H, 3 * d, d, chain, key_tok, cfg.pad_idx, head_dim);
    return OPS(launch_attn_probs, stream, (const bf16_t*)qkv_rows, Pl, t.B, t.T, H, 3 * d, d, chain, key_tok, cfg.pad_idx, head_dim);
  });
  ++t.folded;
  if (rc || !t.fold) return rc;
  return timed(PC_CONTACT, [&] {
    return launch_contact_accumulate(stream, Pl, t.d_tok, cfg.eos_idx, cfg.pad_idx, contact_w + (size_t)l * H, contact_bias, l == 0,
                                     l == cfg.n_layers - 1, contact_sums.as<float>(), t.logits, t.contacts, t.B, t.T, H);
  });
}

// The MSA trunk's contacts tap (engine.h): block l's row qkv is ready.  The tap's own scores launch (the 16-bit MFMA kernel of
// msa_contact.hip, or the strict scores kernel) fills contact_S, the softmax writes the dense maps to the one-layer staging buffer or to
// the caller's slot, and the head folds them over the window 1 .. C - 1 of row 0 (no <eos> in the MSA alphabet: eos_idx -1, tail 0)
int Engine::tap_row_attention(int l, const void* qkv_rows) {
  if (!ctap) return PG_OK;
  ContactTap& t = *ctap;
  const int d = cfg.d_model, H = cfg.n_heads, C = t.T;
  const size_t map = (size_t)t.B * H * C * C;
  float* Pl = contact_P.as<float>();
  if (t.next_attn < t.attn_layers.size() && t.attn_layers[t.next_attn] == l) Pl = t.attn_out + map * t.next_attn++;
  float* S = contact_S.as<float>();
  const float row_scale = 0.125f / sqrtf((float)t.R);
  const int32_t* pad_tok = esm_pad_in_batch ? t.d_tok : nullptr;
  int rc = timed(PC_ATTN_PROBS, [&] {
    int r = strict() ? launch_msa_row_scores_f32(stream, (const float*)qkv_rows, S, t.B, t.R, C, H, 3 * d, d, row_scale, pad_tok, cfg.pad_idx)
                     : OPS(launch_msa_row_scores, stream, (const bf16_t*)qkv_rows, S, t.B, t.R, C, H, 3 * d, d, row_scale, pad_tok, cfg.pad_idx);
    return r ? r : launch_row_softmax_probs(stream, S, Pl, (int64_t)t.B * H * C, C, msa_row_scores_ld(C));
  });
  ++t.folded;
  if (rc || !t.fold) return rc;
  return timed(PC_CONTACT, [&] {
    return launch_contact_accumulate_window(stream, Pl, t.d_tok, -1, cfg.pad_idx, contact_w + (size_t)l * H, contact_bias, l == 0,
                                            l == cfg.n_layers - 1, contact_sums.as<float>(), t.logits, t.contacts, t.B, C, H, 0,
                                            (size_t)t.R * C);
  });
}

int Engine::set_contact_head(const float* weight, int n_weights, float bias) {
  if (contact_w) {
    PG_HIP(hipStreamSynchronize(stream));
    PG_HIP(hipFree(contact_w));
    contact_w = nullptr;
  }
  if (!weight) return PG_OK;
  PG_HIP(hipMalloc((void**)&contact_w, (size_t)n_weights * 4));
  PG_HIP(hipMemcpy(contact_w, weight, (size_t)n_weights * 4, hipMemcpyHostToDevice));
  contact_bias = bias;
  return PG_OK;
}

int Engine::esm_trunk(const int32_t* d_tok, int B, int T, const int32_t* sel_idx, int P, int64_t n_sel, const int32_t* d_iter_) {
  const int d = cfg.d_model, f = cfg.d_ffn;
  const int64_t M = (int64_t)B * T;
  const int64_t Mp = round_up64(M, kRowPad);
  int rc;
  if ((rc = size_activations(Mp))) return rc;
  batch_rows = batch_rows_for(B, T);
  float* X = x.as<float>();
  if (strict()) {
    float* QKVf = qkv.as<float>();
    const int Mi = (int)Mp;
    if ((rc = embed_rows(d_tok, M, T, 0, nullptr)) || (rc = tap_layer(0))) return rc;
    const SeqLayout chain = {1, T, 0, 1};
    for (int l = 0; l < cfg.n_layers; ++l) {
      const EsmLayer& L = esm_layers[l];
      rc = strict_attention(L.ln1, L.qkv, L.out, Mi, M, [&](int split_d) {
        int r = rope(QKVf, M, T);                                              // ESM-2 only
        if (r || (r = tap_attention(l, QKVf))) return r;
        return timed(PC_ATTN, [&] { return launch_attention_f32(stream, QKVf, ctx.as<bf16_t>(), split_d, B, T, cfg.n_heads, 3 * d, 3 * d, d, 2 * d, chain, esm_pad_in_batch ? d_tok : nullptr, cfg.pad_idx, L.bias_kv32, head_dim); });
      });
      if (rc || (rc = ffn_strict(L.ffn, Mi, M)) || (rc = tap_layer(l + 1))) return rc;
    }
    return PG_OK;
  }
  bf16_t* Hh = h.as<bf16_t>();
  bf16_t* QKV = qkv.as<bf16_t>();
  bf16_t* CTX = ctx.as<bf16_t>();
  // <= 256 rows: 64-row tiles, <= 48 rows the weight-streaming GEMM (buffers stay 256-padded) -- the latter not for a tiny shard
  // of a big job (sel_gemm_rows)
  const int Mi = sel_gemm_rows(M, Mp);
  // single chains (<= 32 token rows): LayerNorm is folded into the operand load of the weight-streaming QKV / fc1 GEMMs
  // (gemm_ln_skinny_kernel) -- two launches per layer less in the launch-bound regime
  const bool ln_in_gemm = !embedded() && gemm_ln_skinny_ok(Mi, 3 * d, d) && gemm_ln_skinny_ok(Mi, f, d);      // no live-width form

  // embedding + emb_layer_norm_before, and in the same pass over the row the first layer's LayerNorm (its bf16 operand rows)
  if ((rc = embed_rows(d_tok, M, T, 0, ln_in_gemm ? nullptr : &esm_layers[0].ln1)) || (rc = tap_layer(0))) return rc;
  // a single short chain: the persistent launch, when it may run.  With a selection it stops after the last layer's attention and
  // the pruned tail finishes on the selected rows.  A tap on a layer in between needs the per-layer launches of the same regime
  // (bit-identical with it) -- the persistent launch shows the stream only before its first and after its last layer; a contacts
  // tap needs every layer's qkv
  ChainRan ran = CHAIN_NOT_RUN;
  const bool tap_inside = tap && tap->wants_inner(cfg.n_layers);
  if (ln_in_gemm && !tap_inside && !ctap && (rc = chain_forward(B, T, Mi, sel_idx != nullptr, &ran))) return rc;
  if (ran == CHAIN_WHOLE_FORWARD) return tap_layer(cfg.n_layers);
  // last layer with a selection: only the selected rows are ever read again -> gather them and finish the layer on n_sel rows
  const EsmLayer& tail = esm_layers.back();
  auto finish_selected = [&] { return pruned_tail(tail.out, tail.ffn, sel_idx, nullptr, P, T, n_sel, d_iter_, sel_gemm_rows(n_sel, round_up64(n_sel, kRowPad)), ln_in_gemm); };
  if (ran == CHAIN_TO_LAST_ATTENTION) return finish_selected();
  for (int l = 0; l < cfg.n_layers; ++l) {
    const EsmLayer& L = esm_layers[l];
    // tile regime: Hh holds LN1(x), written by the previous layer's fc2 launch (or the LayerNorm kernel) -- see resid_gemm_ln
    if ((rc = ln_in_gemm ? dense_ln(X, L.ln1, L.qkv, QKV, Mi, EPI_BF16) : dense(PC_GEMM_QKV, Hh, L.qkv, QKV, Mi, EPI_BF16))) return rc;
    if ((rc = rope(QKV, M, T)) || (rc = tap_attention(l, QKV))) return rc;     // ESM-2 only: q and k rotated by their positions
    if ((rc = timed(PC_ATTN, [&] { return OPS(launch_attention_bf16, stream, QKV, CTX, B, T, cfg.n_heads, 3 * d, d, d, 2 * d, esm_pad_in_batch ? d_tok : nullptr, cfg.pad_idx, L.bias_kv16, head_dim); }))) return rc;
    const bool last = l == cfg.n_layers - 1;
    if (sel_idx && last) return finish_selected();
    if ((rc = ffn_block(L.out, L.ffn, last ? nullptr : &esm_layers[l + 1].ln1, Mi, M, ln_in_gemm)) || (rc = tap_layer(l + 1))) return rc;
  }
  return PG_OK;
}

// A single short chain (<= 32 token rows): every layer in ONE persistent launch (chain_trunk.hip; same bits as the per-layer
// launches of esm_trunk's folded regime, whose buffers it works on).  With stop_at_last_attention it ends after the last layer's
// attention.  *ran stays CHAIN_NOT_RUN when the shape, a <pad> batch or this engine's state (no table, switched off) rule it out
int Engine::chain_forward(int B, int T, int Mi, bool stop_at_last_attention, ChainRan* ran) {
  const int d = cfg.d_model, f = cfg.d_ffn;
  if (!(chain_layers && !chain_disabled && !esm_pad_in_batch && T <= 32 && (int64_t)B * T <= Mi && OPS(chain_trunk_ok, Mi, d, f, cfg.n_heads))) return PG_OK;
  int rc;
  if ((rc = chain_sync.ensure(OPS(chain_trunk_sync_bytes), stream)) || (rc = chain_part.ensure(OPS(chain_trunk_part_bytes, Mi, d), stream))) return rc;
  PgChainTrunkArgs ca;
  ca.layers = chain_layers; ca.n_layers = cfg.n_layers; ca.partial_last = stop_at_last_attention ? 1 : 0; ca.B = B; ca.T = T;
  ca.x = x.as<float>(); ca.qkv = qkv.as<bf16_t>(); ca.ctx = ctx.as<bf16_t>(); ca.ffn = ffn.as<bf16_t>();
  ca.part = chain_part.as<float>(); ca.sync = chain_sync.as<unsigned>();
  ca.err = chain_err; ca.eps = cfg.layer_norm_eps;
  rc = timed(PC_GEMM, [&] { return OPS(launch_chain_trunk, stream, ca, Mi, d); });
  if (rc == kChainTrunkUnfit) {              // the grid cannot be co-resident on this device: per-layer launches, for good
    chain_disabled = true;
    return PG_OK;
  }
  if (rc) return rc;
  // test hook: PGIBBS_CHAIN_TRUNK_FAULT=n makes the n-th persistent launch of the process report a barrier timeout
  static const int fault_at = env_int("PGIBBS_CHAIN_TRUNK_FAULT", 0);
  static int launches = 0;
  if (fault_at > 0 && ++launches == fault_at) *chain_err = 1;
  *ran = stop_at_last_attention ? CHAIN_TO_LAST_ATTENTION : CHAIN_WHOLE_FORWARD;
  return PG_OK;
}

// x[M_rows][d] += a[M_rows][K] W^T + b, then h = LayerNorm(x; ln) as the next GEMM's bf16 operand: the residual GEMM the dispatch
// picks, followed by the LayerNorm kernel at its HBM roofline.  (Normalising inside the GEMM was built in round 3, bit-identical
// and slower; it left the library in round 4: tools/probes/gemm_ln_fused.hip.  So was round 6's tile of whole 768-wide rows with the
// LayerNorm in its epilogue: 1.34-1.37 ms per launch against 1.26-1.28 ms for these two launches, EXPERIMENTS.md.)
int Engine::resid_gemm_ln(int cls, const bf16_t* a, const DenseW& W, float* x, int M_rows, int64_t M_real, const LnW& ln, bf16_t* h,
                          bool use_splitk, int colmajor_R, int colmajor_C) {
  const int rc = dense(cls, a, W, x, M_rows, EPI_F32_RESID, (int)M_real, use_splitk);
  return rc ? rc : layer_norm(x, ln, h, M_real, true, colmajor_R, colmajor_C);
}

// LM head evaluated ONLY at the selected rows: emb_layer_norm_after -> dense -> GELU ->
// LayerNorm -> tied decoder + bias.  d_idx == nullptr: every one of the n_sel rows of x in order.
int Engine::head(const int32_t* d_idx_, const int32_t* d_row_map, int P, int width, int64_t n_sel, float* d_logits,
                 const float* x_src) {
  if (!x_src) x_src = x.as<float>();
  const int d = cfg.d_model, V = cfg.vocab;
  const int64_t Np = round_up64(n_sel, kRowPad);
  int rc;
  if (esm1()) {
    // ESM-1: logits = x embed_out^T + embed_out_bias on the selected rows of the residual stream (no final LayerNorm, no dense);
    // the decoder kernel with its LayerNorm switched off (gamma == nullptr), fp32 throughout in every precision mode
    const float* rows = x_src;
    if (d_idx_) {
      if ((rc = sel_g.ensure((size_t)Np * d * 4, stream))) return rc;
      if ((rc = launch_gather_rows(stream, x_src, sel_g.as<float>(), d_idx_, d_row_map, P, width, n_sel, d * 4))) return rc;
      rows = sel_g.as<float>();
    }
    return timed(PC_HEAD, [&] { return launch_lm_tail(stream, rows, nullptr, nullptr, embed_out, head_bias, d_logits, n_sel, d, V, cfg.layer_norm_eps); });
  }
  if ((rc = sel_h.ensure((size_t)Np * d * 2, stream))) return rc;
  if ((rc = sel_g.ensure((size_t)Np * d * 4, stream))) return rc;
  const float eps = cfg.layer_norm_eps;
  if (strict()) {
    if ((rc = sel_h.ensure((size_t)Np * 3 * d * 2, stream))) return rc;
    if ((rc = OPS(launch_gather_ln_bf16, stream, x_src, d_idx_, d_row_map, P, width, ln_after.g, ln_after.b,
                                    sel_h.as<bf16_t>(), n_sel, d, eps, true, d_live))) return rc;
    if ((rc = dense3(sel_h.as<bf16_t>(), head_dense, sel_g.as<float>(), (int)Np, false))) return rc;
    if ((rc = launch_gelu_f32(stream, sel_g.as<float>(), Np * d))) return rc;
    return launch_lm_tail(stream, sel_g.as<float>(), head_ln.g, head_ln.b, embed, head_bias, d_logits, n_sel, d, V, eps, d_live);
  }
  return timed(PC_HEAD, [&] {
    int r = OPS(launch_gather_ln_bf16, stream, x_src, d_idx_, d_row_map, P, width, ln_after.g, ln_after.b,
                                  sel_h.as<bf16_t>(), n_sel, d, eps, false, d_live);
    if (r) return r;
    if ((r = dense(PC_NONE, sel_h.as<bf16_t>(), head_dense, sel_g.as<float>(), sel_gemm_rows(n_sel, Np), EPI_F32_GELU))) return r;
    return launch_lm_tail(stream, sel_g.as<float>(), head_ln.g, head_ln.b, embed, head_bias, d_logits, n_sel, d, V, eps, d_live);
  });
}

int Engine::masked_logits(int32_t* d_tok, int B, int R, int C, const int32_t* idx, const int32_t* mask_map, const int32_t* sel_map,
                          int64_t n_rows, int P, bool mask, int mask_idx, float* lg, const int32_t* dit) {
  const int64_t n_draws = n_rows * P;
  int rc;
  if (mask && P > 0)
    if ((rc = timed(PC_SAMPLE, [&] { return launch_mask_scatter(stream, d_tok, C, idx, mask_map, n_rows, P, mask_idx, dit); }))) return rc;
  const bool pruned = prune_last(n_draws, (int64_t)B * R * C);
  if ((rc = trunk(d_tok, B, R, C, pruned ? idx : nullptr, sel_map, P, n_draws, dit))) return rc;
  if (P == 0) return PG_OK;
  return pruned ? head(nullptr, nullptr, 1, 1, n_draws, lg, x_sel.as<float>()) : head(idx, sel_map, P, C, n_draws, lg);
}

int Engine::esm_gibbs_device(int32_t* d_tok, int B, int T, const int32_t* d_idx_, int n_iters, int P,
                             const pg_sample_params* sp, float* d_samp_logits_, int32_t* d_samp_tok_) {
  int rc = check_call(false, B, 1, T, n_iters, P);
  if (rc) return rc;
  if (B == 0 || n_iters == 0) return PG_OK;
  const int V = cfg.vocab;
  const int64_t n_sel_rows = B;              // one selected token row per chain
  const int64_t n_draws = (int64_t)B * P;
  if (!d_samp_logits_ && (rc = logits.ensure((size_t)(n_draws > 0 ? n_draws : 1) * V * 4, stream))) return rc;
  static const int use_graph = env_int("PGIBBS_GRAPH", 1);
  const bool pruned = prune_last(n_draws, (int64_t)B * T);

  // one Gibbs iteration; with dit != nullptr every iteration-dependent quantity is derived on the device from *dit
  auto iteration = [&](int it, const int32_t* dit) -> int {
    const int32_t* idx_it = dit ? d_idx_ : d_idx_ + (size_t)it * n_draws;
    float* lg = d_samp_logits_ ? d_samp_logits_ + (size_t)it * n_draws * V : logits.as<float>();
    int r = masked_logits(d_tok, B, 1, T, idx_it, nullptr, nullptr, n_sel_rows, P, sp->mask, sp->mask_idx, lg, dit);
    if (r || P == 0) return r;
    int32_t* st = d_samp_tok_ ? d_samp_tok_ + (size_t)it * n_draws : nullptr;
    return timed(PC_SAMPLE, [&] { return launch_sample_writeback(stream, d_tok, T, lg, V, 1, idx_it, nullptr, n_sel_rows, P, sp, dit ? 0 : it, st, dit, range_err, draw_guide()); });
  };

  // Launch-bound regime (few tokens: ~270 launches of a few microseconds each): capture ONE iteration as a hipGraph and
  // replay it.  Needs the pruned path (no per-iteration pointers besides the idx table), no per-iteration outputs, no
  // event profiling.  The iteration number and the sampling parameters (seed, burn-in, top-k ...) live in a device-side state
  // block, so the SAME graph is replayed by every later call of the same shape on the same buffers -- a generate() per
  // sequence (BASELINE config 1) captures once, not once per call.  Before a capture iteration 0 runs eagerly (it sizes every
  // workspace buffer: no allocation inside the capture).
  const bool graphable = use_graph && pruned && !prof.on && !d_samp_logits_ && !d_samp_tok_ && (int64_t)B * T <= 4096;
  auto epoch_pad = [&] { return g_alloc_epoch * 2 + (esm_pad_in_batch ? 1 : 0); };
  GraphKey key;
  if (graphable) key = {sp->mask, sp->mask_idx, d_tok, d_idx_, B, T, P, stream, epoch_pad(), job_items, draw_guide() != nullptr};
  const bool reuse = graphable && graph_exec && key == graph_key;
  if (!graphable || (!reuse && n_iters < 3)) {
    for (int it = 0; it < n_iters; ++it)
      if ((rc = iteration(it, nullptr))) return rc;
    return PG_OK;
  }
  int first = 0;
  if (!reuse) {
    if ((rc = d_iter.ensure(graph_state_bytes(), stream))) return rc;
    if ((rc = iteration(0, nullptr))) return rc;
    first = 1;
    key.epoch_pad = epoch_pad();      // a buffer grown by iteration 0 moved the epoch: the key must describe the state the graph is captured in
    if (graph_exec) { (void)hipGraphExecDestroy(graph_exec); graph_exec = nullptr; }
    hipGraph_t graph = nullptr;
    PG_HIP(hipStreamBeginCapture(stream, hipStreamCaptureModeThreadLocal));
    rc = iteration(0, d_iter.as<int32_t>());
    if (!rc) rc = launch_iter_counter(stream, d_iter.as<int32_t>(), false, 0);
    hipError_t ce = hipStreamEndCapture(stream, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    if (ce != hipSuccess) return fail(PG_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(ce));
    ce = hipGraphInstantiate(&graph_exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (ce != hipSuccess) { graph_exec = nullptr; return fail(PG_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(ce)); }
    graph_key = key;
    ++stat_graph_captures;
  }
  // replay: the counter selects the idx slice, the Philox iteration word and the burn-in flag; the parameters are this call's
  if ((rc = launch_graph_state(stream, d_iter.as<int32_t>(), first, sp, draw_guide()))) return rc;
  for (int it = first; it < n_iters; ++it) PG_HIP(hipGraphLaunch(graph_exec, stream));
  stat_graph_replays += n_iters - first;
  return PG_OK;
}

// ------------------------------------------------------------------------------------------------
// ESM-MSA-1b forward: tokens[B][R][C] -> x[B*R*C][d]
// ------------------------------------------------------------------------------------------------
int Engine::msa_trunk(const int32_t* d_tok, int B, int R, int C, const int32_t* sel_idx, const int32_t* sel_row_map, int P,
                      int64_t n_sel) {
  const int d = cfg.d_model, H = cfg.n_heads;
  const int64_t M = (int64_t)B * R * C;
  const int64_t Mp = round_up64(M, kRowPad);
  int rc;
  if ((rc = size_activations(Mp))) return rc;
  batch_rows = batch_rows_for(B, (int64_t)R * C);
  float* X = x.as<float>();
  bf16_t* Hh = h.as<bf16_t>();
  bf16_t* QKV = qkv.as<bf16_t>();
  bf16_t* CTX = ctx.as<bf16_t>();
  const int Mi = (int)Mp;
  const float row_scale = 0.125f / sqrtf((float)R);      // dh^-0.5 / sqrt(R): depends on R, applied to the scores
  // A batch that holds <pad> (a ragged list of MSAs padded to one tensor by the unmasked log_likelihood_batch, esm_msa_sampler.py:341,
  // 416-431; set by the host-token entry points): fair-esm's padding semantics -- tied row attention with q zeroed at <pad>
  // positions and row 0's <pad> columns filled with -10000 (the scores-through-scratch kernels), column attention with <pad> key
  // rows filled with -10000.  R, and with it the 1/sqrt(R) of the row attention, is the padded row count, as in the reference.
  const int32_t* pad_tok = esm_pad_in_batch ? d_tok : nullptr;
  if (pad_tok && precision == PG_PREC_F16)
    return fail(PG_ERR_UNSUPPORTED, "fp16 precision mode: batches with <pad> (ragged MSA lists) take the scores-through-scratch row "
                                    "attention, which exists for bf16 operands only -- use precision bf16 or fp32");
  if (strict()) {
    if ((rc = scores.ensure((size_t)B * H * C * msa_row_scores_ld(C) * 4, stream))) return rc;
    float* QKVf = qkv.as<float>();
    if ((rc = embed_rows(d_tok, M, C, R, nullptr))) return rc;
    const SeqLayout colS = {C, R * C, 1, C};
    for (int l = 0; l < cfg.n_layers; ++l) {
      const MsaLayer& L = msa_layers[l];
      rc = strict_attention(L.ln_row, L.row_qkv, L.row_out, Mi, M, [&](int split_d) {
        if (int r = tap_row_attention(l, QKVf)) return r;
        return timed(PC_ATTN, [&] { return launch_msa_row_attention_f32(stream, QKVf, scores.as<float>(), CTX, split_d, B, R, C, H, 3 * d, 3 * d, d, 2 * d, row_scale, pad_tok, cfg.pad_idx); });
      });
      if (rc) return rc;
      rc = strict_attention(L.ln_col, L.col_qkv, L.col_out, Mi, M, [&](int split_d) {
        return timed(PC_ATTN, [&] { return launch_attention_f32(stream, QKVf, CTX, split_d, (int64_t)B * C, R, H, 3 * d, 3 * d, d, 2 * d, colS, pad_tok, cfg.pad_idx); });
      });
      if (rc || (rc = ffn_strict(L.ffn, Mi, M))) return rc;
    }
    return PG_OK;
  }

  // embedding + emb_layer_norm_before, and in the same pass over the row the first layer's row-attention LayerNorm
  if ((rc = embed_rows(d_tok, M, C, R, &msa_layers[0].ln_row))) return rc;
  const SeqLayout col = {C, R * C, 1, C};                   // column c of msa b: rows (b*R + r)*C + c
  // Hh always holds the LayerNorm the next projection reads: written by the embedding pass / the LayerNorm after a residual GEMM
  for (int l = 0; l < cfg.n_layers; ++l) {
    const MsaLayer& L = msa_layers[l];
    // tied row attention
    if ((rc = dense(PC_GEMM_QKV, Hh, L.row_qkv, QKV, Mi, EPI_BF16))) return rc;
    if (C <= 576 && !pad_tok) {
      float* part = nullptr;
      // few workgroups: give the kernel scratch for its split-R mode (decided on the job's batch: the split changes the
      // order of the sum over alignment rows, and a shard must compute what the whole batch would)
      const size_t need = msa_row_split_scratch_bytes(B, R, C, H, (int)(job_batch(B) * H));
      if (need) {
        // the host entry points chunk a batch of templates so that this fits (api.hip); a device-pointer caller gets the reason
        if (need > ((size_t)1 << 31)) return fail(PG_ERR_INVALID, "too many MSAs in one call for the row-split attention scratch: use smaller batches");
        if ((rc = scores.ensure(need, stream))) return rc;           // the allocator's own error (out of memory)
        part = scores.as<float>();
      }
      if ((rc = tap_row_attention(l, QKV))) return rc;
      if ((rc = timed(PC_ATTN, [&] { return OPS(launch_msa_row_attention_bf16, stream, QKV, CTX, B, R, C, H, 3 * d, d, d, 2 * d, row_scale, part, part ? scores.bytes : 0, (int)(job_batch(B) * H)); }))) return rc;
    } else {
      // alignments wider than the MFMA row-attention kernel's register budget: fp32 scores through a scratch buffer
      if (precision == PG_PREC_F16)
        return fail(PG_ERR_UNSUPPORTED, "fp16 precision mode: alignments wider than 576 columns take the split-bf16 row attention, "
                                        "which exists for bf16 operands only -- use precision bf16 or fp32");
      if ((rc = scratch.ensure((size_t)Mp * 3 * d * 4, stream)) || (rc = scores.ensure((size_t)B * H * C * msa_row_scores_ld(C) * 4, stream))) return rc;
      if ((rc = tap_row_attention(l, QKV))) return rc;
      rc = timed(PC_ATTN, [&] {
        int r2 = launch_bf16_to_f32(stream, QKV, scratch.as<float>(), (int64_t)M * 3 * d);
        if (r2) return r2;
        return launch_msa_row_attention_f32(stream, scratch.as<float>(), scores.as<float>(), CTX, 0, B, R, C, H,
                                            3 * d, d, d, 2 * d, row_scale, pad_tok, cfg.pad_idx);
      });
      if (rc) return rc;
    }
    // column block: fused QKV projection + attention when the depth allows (gemm_colattn.hip: the LayerNorm writes its rows in
    // column-major token order, q / k / v never leave the CU; bit-identical context), else projection + attention kernel
    const bool col_fused = !pad_tok && colattn_ok(R, d, H) && L.col_qkv_hm.w;
    if ((rc = resid_gemm_ln(PC_GEMM_OUT, CTX, L.row_out, X, Mi, M, L.ln_col, Hh, false, col_fused ? R : 0, col_fused ? C : 0))) return rc;   // x += row_out(ctx); h = LN_col(x)
    if (col_fused) {
      if ((rc = timed(PC_GEMM_QKV, [&] { return OPS(launch_gemm_colattn, stream, Hh, L.col_qkv_hm.w, L.col_qkv_hm.b, CTX, B, R, C, H, d, d); }))) return rc;
    } else {
      // column attention (q pre-scaled by dh^-0.5 in the weights)
      if ((rc = dense(PC_GEMM_QKV, Hh, L.col_qkv, QKV, Mi, EPI_BF16))) return rc;
      if ((rc = timed(PC_ATTN, [&] { return OPS(launch_attention_seq_bf16, stream, QKV, CTX, (int64_t)B * C, R, H, 3 * d, d, d, 2 * d, col, pad_tok, cfg.pad_idx, nullptr); }))) return rc;
    }
    const bool last = l == cfg.n_layers - 1;
    // last layer: nothing but the selected rows is read again -> finish column out-projection and FFN on n_sel rows
    if (sel_idx && last) return pruned_tail(L.col_out, L.ffn, sel_idx, sel_row_map, P, C, n_sel, nullptr, (int)round_up64(n_sel, kRowPad), false);
    // x += col_out(ctx); h = LN_ffn(x); feed forward; h = LN_row of the next layer
    if ((rc = ffn_block(L.col_out, L.ffn, last ? nullptr : &msa_layers[l + 1].ln_row, Mi, M))) return rc;
  }
  return PG_OK;
}

// The tables of a draw guide, checked on the host and uploaded once; nullptr or a guide with nothing set clears it.  Work queued under
// the previous guide is waited for before its tables are freed.
int Engine::set_draw_guide(const pg_draw_guide* g) {
  int rc;
  if (g && (rc = check_draw_guide_tables(g, "pg_engine_set_draw_guide"))) return rc;      // before a device is touched
  DrawGuideDev next;
  if (g) {
    next.top_p = g->top_p;
    if (g->bias) { next.bias_rows = g->bias_rows; next.width = g->width; next.n_valid = g->n_valid; }
    if (g->temperatures) next.n_temps = g->n_temperatures;
  }
  const bool had = guide_bias_dev || guide_temps_dev;
  if (!had && !(g && (g->bias || g->temperatures))) {      // no table to free or to upload: no device call
    guide = next;
    return PG_OK;
  }
  PG_HIP(hipStreamSynchronize(stream));      // the caller (pg_engine_set_draw_guide) has made the engine's device current
  if (guide_bias_dev) (void)hipFree(guide_bias_dev);
  if (guide_temps_dev) (void)hipFree(guide_temps_dev);
  guide_bias_dev = guide_temps_dev = nullptr;
  guide = DrawGuideDev();
  if (g && g->bias) {
    const size_t bytes = (size_t)g->bias_rows * g->width * g->n_valid * 4;
    PG_HIP(hipMalloc((void**)&guide_bias_dev, bytes));
    PG_HIP(hipMemcpyAsync(guide_bias_dev, g->bias, bytes, hipMemcpyHostToDevice, stream));
    next.bias = guide_bias_dev;
  }
  if (g && g->temperatures) {
    PG_HIP(hipMalloc((void**)&guide_temps_dev, (size_t)g->n_temperatures * 4));
    PG_HIP(hipMemcpyAsync(guide_temps_dev, g->temperatures, (size_t)g->n_temperatures * 4, hipMemcpyHostToDevice, stream));
    next.temps = guide_temps_dev;
  }
  PG_HIP(hipStreamSynchronize(stream));      // the caller's host tables are free again
  guide = next;
  return PG_OK;
}

// embed_ln_kernel reads pos + p * d and msa_pos + (row % R) * d of tables of max_positions + pad_idx + 1 and max_msa_rows rows (init)
int Engine::check_call(bool msa, int B, int R, int C, int count0, int count1, int row0, int row1) const {
  if (msa && cfg.arch != PG_ARCH_MSA1B) return fail(PG_ERR_INVALID, "engine was not built for the MSA-1b architecture");
  if (!msa && !esm_family()) return fail(PG_ERR_INVALID, "engine was not built for an ESM-1b / ESM-1 / ESM-2 architecture");
  if (B < 0 || R < 1 || C < 1) return fail(PG_ERR_INVALID, "bad shape");
  if (msa && R > cfg.max_msa_rows) return fail(PG_ERR_INVALID, "MSA has more rows than msa_position_embedding");
  if (C > cfg.max_positions)
    return fail(PG_ERR_INVALID, msa ? "alignment longer than the learned position table" : "sequence longer than the learned position table");
  if (count0 < 0 || count1 < 0) return fail(PG_ERR_INVALID, "bad shape");
  if (row0 < 0 || row0 >= R || row1 < 0 || row1 >= R) return fail(PG_ERR_INVALID, "row index out of range");
  return PG_OK;
}

int Engine::msa_gibbs_device(int32_t* d_tok, int B, int R, int C, const int32_t* d_idx_, int n_iters, int P,
                             const pg_sample_params* sp, float* d_samp_logits_, int32_t* d_samp_tok_) {
  int rc = check_call(true, B, R, C, n_iters, P);
  if (rc) return rc;
  if (B == 0 || n_iters == 0) return PG_OK;
  const int V = cfg.vocab;
  const int64_t n_sel_rows = (int64_t)B * R;         // every row of every MSA draws its own P positions
  const int64_t n_draws = n_sel_rows * P;
  if (!d_samp_logits_ && (rc = logits.ensure((size_t)(n_draws > 0 ? n_draws : 1) * V * 4, stream))) return rc;
  for (int it = 0; it < n_iters; ++it) {
    const int32_t* idx_it = d_idx_ + (size_t)it * n_draws;
    float* lg = d_samp_logits_ ? d_samp_logits_ + (size_t)it * n_draws * V : logits.as<float>();
    if ((rc = masked_logits(d_tok, B, R, C, idx_it, nullptr, nullptr, n_sel_rows, P, sp->mask, sp->mask_idx, lg))) return rc;
    if (P == 0) continue;
    int32_t* st = d_samp_tok_ ? d_samp_tok_ + (size_t)it * n_draws : nullptr;
    if ((rc = timed(PC_SAMPLE, [&] { return launch_sample_writeback(stream, d_tok, C, lg, V, 1, idx_it, nullptr, n_sel_rows, P, sp, it, st, nullptr, range_err, draw_guide()); }))) return rc;
  }
  return PG_OK;
}

// generate_single for B templates of equal shape at once ("batch=32 templates").  Template b is token block
// b; step s masks row mask_row of every template and samples row target_row of template b at d_step_idx[s][b][0..P_max) with
// template b's own sampling parameters sp[b] (its own Philox key: the reference draws a fresh torch seed per call).  Every
// order-changing kernel choice is taken as if a template were alone (order_items = 1), so template b's logits and tokens are
// bit-identical with a B = 1 call on it -- and therefore independent of how templates are batched or sharded over GPUs.
int Engine::msa_single_device(int32_t* d_tok, int B, int R, int C, int mask_row, int target_row, const int32_t* d_step_idx,
                              const int32_t* step_sample_flag_host, int n_steps, int P_max, const pg_sample_params* sp,
                              float* d_samp_logits_, int32_t* d_samp_tok_) {
  int rc = check_call(true, B, R, C, n_steps, P_max, mask_row, target_row);
  if (rc) return rc;
  if (n_steps == 0 || B == 0) return PG_OK;
  const int V = cfg.vocab;
  if (B > 1 && (int64_t)R * C <= 2048) {
    // few-token regime: K-splits and the weight-streaming GEMM are picked by the local shape there, so a
    // batch would not reproduce the single calls -- run the templates one after the other (launch-bound either way)
    auto copy = [&](auto* dst, const auto* src, size_t n) -> int {
      PG_HIP(hipMemcpyAsync(dst, src, n * sizeof(*dst), hipMemcpyDeviceToDevice, stream));
      return PG_OK;
    };
    auto to_table = [&](auto* block, auto* table, size_t n) { return copy(table, block, n); };
    const size_t n1 = (size_t)n_steps * (P_max > 0 ? P_max : 1);
    for (int b = 0; b < B; ++b) {
      // template b's steps, contiguous [n_steps][P_max]
      if ((rc = tmp_idx.ensure((size_t)(n_steps * (size_t)P_max + 1) * 4, stream))) return rc;
      if ((rc = template_block_rows(tmp_idx.as<int32_t>(), d_step_idx, n_steps, B, b, 1, P_max, copy))) return rc;
      // per-template outputs land in scratch-free strided form: sample into temporaries, then scatter
      float* lg_b = nullptr;
      int32_t* st_b = nullptr;
      if (d_samp_logits_ || d_samp_tok_) {
        if ((rc = tmp_out.ensure(n1 * V * 4 + n1 * 4, stream))) return rc;
        lg_b = d_samp_logits_ ? tmp_out.as<float>() : nullptr;
        st_b = d_samp_tok_ ? (int32_t*)(tmp_out.as<float>() + n1 * V) : nullptr;
      }
      {
        GuideRowShift rows(*this, (int64_t)b * R, C);
        rc = msa_single_device(d_tok + (size_t)b * R * C, 1, R, C, mask_row, target_row, tmp_idx.as<int32_t>(), step_sample_flag_host,
                               n_steps, P_max, sp + b, lg_b, st_b);
      }
      if (rc) return rc;
      if (lg_b && (rc = template_block_rows(lg_b, d_samp_logits_, n_steps, B, b, 1, (size_t)P_max * V, to_table))) return rc;
      if (st_b && (rc = template_block_rows(st_b, d_samp_tok_, n_steps, B, b, 1, P_max, to_table))) return rc;
    }
    return PG_OK;
  }
  if ((rc = d_rowmap.ensure((size_t)2 * B * 4, stream))) return rc;
  std::vector<int32_t> maps((size_t)2 * B);
  for (int b = 0; b < B; ++b) {
    maps[b] = b * R + mask_row;
    maps[B + b] = b * R + target_row;
  }
  PG_HIP(hipMemcpyAsync(d_rowmap.p, maps.data(), maps.size() * 4, hipMemcpyHostToDevice, stream));
  PG_HIP(hipStreamSynchronize(stream));     // `maps` is a local buffer
  const int32_t* d_mask_map = d_rowmap.as<int32_t>();
  const int32_t* d_tgt_map = d_rowmap.as<int32_t>() + B;
  const int64_t n_draws = (int64_t)B * P_max;
  if (!d_samp_logits_ && (rc = logits.ensure((size_t)(n_draws > 0 ? n_draws : 1) * V * 4, stream))) return rc;
  struct OrderGuard { Engine& e; int64_t prev; ~OrderGuard() { e.order_items = prev; } } guard{*this, order_items};
  order_items = 1;
  for (int s = 0; s < n_steps; ++s) {
    const int32_t* idx_s = d_step_idx + (size_t)s * n_draws;
    float* lg = d_samp_logits_ ? d_samp_logits_ + (size_t)s * n_draws * V : logits.as<float>();
    // generate_single always masks (esm_msa_sampler.py:133), row -1 regardless of the target row
    if ((rc = masked_logits(d_tok, B, R, C, idx_s, d_mask_map, d_tgt_map, B, P_max, true, sp->mask_idx, lg))) return rc;
    if (P_max == 0) continue;
    int32_t* st = d_samp_tok_ ? d_samp_tok_ + (size_t)s * n_draws : nullptr;
    for (int b = 0; b < B; ++b) {           // one draw launch per template: its own Philox key, Philox row id = row_id_base
      pg_sample_params p = sp[b];
      p.burnin = step_sample_flag_host[s] ? 0x7fffffff : 0;   // sample=(pass_num < burn_in), esm_msa_sampler.py:143
      if ((rc = timed(PC_SAMPLE, [&] { return launch_sample_writeback(stream, d_tok, C, lg + (size_t)b * P_max * V, V, 1, idx_s + (size_t)b * P_max,
                                                                      d_tgt_map + b, 1, P_max, &p, s, st ? st + (size_t)b * P_max : nullptr, nullptr, range_err, draw_guide()); }))) return rc;
    }
  }
  return PG_OK;
}

}  // namespace pg
