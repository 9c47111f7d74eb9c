// The kernel-level test and measurement entries of include/pgibbs.h (pg_dbg_*; the two gather hooks live in comm.cpp).  No kernels here.
// Every entry has the same three steps: validate on the host (a wrong argument is PG_ERR_INVALID with a message, before a device is
// looked for); open a Dbg scope on the device; upload, check the scope once, launch, download.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "engine.h"
#include "gemm_epilogue.h"
#include "ln_row.h"

using namespace pg;

namespace {
// One entry's device, buffers and copies.  A failed allocation or copy is remembered and turns the calls after it into no-ops that
// return null: an entry asks check() once, after its uploads and before its first launch.  A null host pointer given to up() is an
// optional array the caller left out -- a null device pointer, not a failure.  Leaving the scope frees the buffers and restores
// the caller's device.
struct Dbg {
  int prev = -1;
  bool bad = false;
  std::vector<void*> bufs;
  Dbg() { (void)hipGetDevice(&prev); }
  ~Dbg() {
    for (void* p : bufs) (void)hipFree(p);
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  int open(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) return fail(PG_ERR_NO_DEVICE, "no HIP device visible");
    if (device < 0 || device >= n) return fail(PG_ERR_INVALID, "bad device ordinal");
    PG_HIP(hipSetDevice(device));
    return PG_OK;
  }
  template <typename T>
  T* alloc(size_t n) {      // zero-filled
    const size_t bytes = n ? n * sizeof(T) : 4;
    void* p = nullptr;
    if (bad || hipMalloc(&p, bytes) != hipSuccess) {
      bad = true;
      return nullptr;
    }
    bufs.push_back(p);
    (void)hipMemset(p, 0, bytes);
    return (T*)p;
  }
  template <typename T>
  void put(T* dev, const T* host, size_t n) {
    if (bad || !n) return;
    bad = hipMemcpy(dev, host, n * sizeof(T), hipMemcpyHostToDevice) != hipSuccess;
  }
  template <typename T>
  T* up(const T* host, size_t n) {
    T* p = host ? alloc<T>(n) : nullptr;
    put(p, host, p ? n : 0);
    return bad ? nullptr : p;
  }
  int check(const char* what = "hipMalloc failed") const { return bad ? fail(PG_ERR_HIP, what) : PG_OK; }
  template <typename T>
  int down(T* host, const T* dev, size_t n) const {
    PG_HIP(hipDeviceSynchronize());
    PG_HIP(hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost));
    return PG_OK;
  }
};

// fp32_ok: the entry also runs the strict mode's kernels; otherwise it takes the two 16-bit modes only
int dbg_precision(const char* who, int precision, bool fp32_ok) {
  if (precision == PG_PREC_BF16 || precision == PG_PREC_F16) return PG_OK;
  if (!fp32_ok) return fail(PG_ERR_INVALID, std::string(who) + ": precision must be PG_PREC_BF16 or PG_PREC_F16");
  return precision == PG_PREC_FP32 ? PG_OK : fail(PG_ERR_INVALID, "unknown precision mode");
}
// n device fp32 values -> the 16-bit operand type of `precision`
int to16(int precision, const float* src, bf16_t* dst, int64_t n, float scale = 1.f) {
  return OPS(launch_f32_to_bf16, nullptr, src, dst, n, scale);
}
// n device values of the 16-bit type of `precision` -> host fp32, widened through the device buffer `wide`
int down16(const Dbg& d, int precision, const bf16_t* rows, float* wide, float* host, int64_t n) {
  const int rc = OPS(launch_bf16_to_f32, nullptr, rows, wide, n);
  return rc ? rc : d.down(host, wide, (size_t)n);
}
// device rows in the strict mode's split operand layout (3 d bf16: split_operand.h, activation order) -> host fp32 rows hi + lo;
// also checks that the two hi copies agree
int split3_rows_to_host(const bf16_t* c3, float* dst, int64_t M, int d) {
  PG_HIP(hipDeviceSynchronize());
  std::vector<bf16_t> h((size_t)M * 3 * d);
  PG_HIP(hipMemcpy(h.data(), c3, h.size() * 2, hipMemcpyDeviceToHost));
  for (int64_t r = 0; r < M; ++r)
    for (int c = 0; c < d; ++c) {
      const size_t g = (size_t)r * 3 * d + split_lo_offset(c);
      const bf16_t lo = h[g], hi = h[g + kSplitHi], hi2 = h[g + kSplitDup];
      if (hi != hi2) return fail(PG_ERR_HIP, "split operand row: the two hi copies differ");
      dst[(size_t)r * d + c] = bf16_to_f32(hi) + bf16_to_f32(lo);
    }
  return PG_OK;
}
// the benches' operands: n values uniform in [-1, 1) from a 32-bit LCG
std::vector<float> lcg_uniform(size_t n, uint32_t seed) {
  std::vector<float> h(n);
  for (auto& v : h) {
    seed = seed * 1664525u + 1013904223u;
    v = (seed >> 8) * (1.0f / 8388608.0f) - 1.0f;
  }
  return h;
}
// 2 warm-up launches, then `iters` launches between two events on the null stream: *avg_ms = elapsed / iters
struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  ~EventPair() {
    if (a) (void)hipEventDestroy(a);
    if (b) (void)hipEventDestroy(b);
  }
};
template <typename Launch>
int time_launches(Launch&& launch, int iters, double* avg_ms) {
  EventPair ev;
  for (hipEvent_t* e : {&ev.a, &ev.b}) PG_HIP(hipEventCreate(e));
  int rc;
  for (int i = 0; i < 2; ++i)
    if ((rc = launch())) return rc;
  PG_HIP(hipEventRecord(ev.a, nullptr));
  for (int i = 0; i < iters; ++i)
    if ((rc = launch())) return rc;
  PG_HIP(hipEventRecord(ev.b, nullptr));
  PG_HIP(hipEventSynchronize(ev.b));
  float ms = 0;
  PG_HIP(hipEventElapsedTime(&ms, ev.a, ev.b));
  *avg_ms = ms / iters;
  return PG_OK;
}
// what a debug entry's launches recorded (note_kernel), into the caller's buffer
void dbg_noted_text(char* plan, int plan_bytes) {
  if (plan && plan_bytes > 0) snprintf(plan, (size_t)plan_bytes, "%s", noted_kernels().c_str());
}

// What pg_dbg_attention_kv and pg_dbg_msa_attention_tok do once their arguments are checked and their scope is open, around
// launch(dq, bq, out, dtok): qkv[M][3 d] and the optional tokens go up; strict: launch reads the fp32 dq (bq null) and writes split
// rows `out` [M][3 d], returned as hi + lo; otherwise it reads the 16-bit bq and writes 16-bit rows `out` [M][d], returned widened.
// Buffers of the entry's own are allocated in `s` before this is called, so that the one check covers them.
template <typename Launch>
int dbg_attention_run(Dbg& s, int precision, bool strict, const float* qkv, float* ctx, int64_t M, int d, const int32_t* tok, char* plan,
                      int plan_bytes, Launch&& launch) {
  const float* dq = s.up(qkv, (size_t)M * 3 * d);
  const int32_t* dtok = s.up(tok, (size_t)M);
  bf16_t* bq = strict ? nullptr : s.alloc<bf16_t>((size_t)M * 3 * d);
  bf16_t* out = s.alloc<bf16_t>((size_t)M * d * (strict ? 3 : 1));
  float* wide = strict ? nullptr : s.alloc<float>((size_t)M * d);
  int rc = s.check();
  if (rc) return rc;
  clear_noted_kernels();
  if (!strict && (rc = to16(precision, dq, bq, M * 3 * d))) return rc;
  if ((rc = launch(dq, bq, out, dtok))) return rc;
  dbg_noted_text(plan, plan_bytes);
  return strict ? split3_rows_to_host(out, ctx, M, d) : down16(s, precision, out, wide, ctx, M * d);
}
}  // namespace

extern "C" {

int pg_dbg_gemm(int device, int precision, const float* x, const float* w, const float* bias, float* out, int M, int N,
                int K, int epi) {
  return pg_dbg_gemm_v(device, precision, x, w, bias, out, M, N, K, epi, -1, -1, M, nullptr, 0);
}

/* pg_dbg_gemm with the kernel named: variant -1 = launch_gemm_bf16 (the process's PGIBBS_GEMM), else launch_gemm_bf16_variant with one
 * of the variants that compute a whole result; have_ws 0 / 1 = split-K scratch withheld / on offer whatever the epilogue, -1 = on offer
 * to the residual epilogue; plan (may be NULL): the text the GEMM launch alone recorded.  Everything is refused on the host before a
 * device is looked for; a shape plan_gemm refuses comes back as the launcher's error. */
int pg_dbg_gemm_v(int device, int precision, const float* x, const float* w, const float* bias, float* out, int M, int N, int K, int epi,
                  int variant, int have_ws, int m_live, char* plan, int plan_bytes) {
  if (plan && plan_bytes > 0) plan[0] = 0;
  int rc = dbg_precision("pg_dbg_gemm", precision, true);
  if (rc) return rc;
  if (!x || !w || !bias || !out || M < 1 || N % 64 || K % 64 || (plan && plan_bytes < 1)) return fail(PG_ERR_INVALID, "pg_dbg_gemm: bad argument");
  if (have_ws < -1 || have_ws > 1 || m_live < 0 || m_live > M) return fail(PG_ERR_INVALID, "pg_dbg_gemm_v: have_ws is -1, 0 or 1 and m_live 0 ... M");
  // the ablation instances (21 ..., 60 ..., 81 ..., 90) compute deliberately incomplete results: nothing to compare
  const bool whole = variant == 1 || variant == 2 || variant == 6 || variant == 7 || variant == 8 || variant == 20 || variant == 80;
  if (variant != -1 && !whole) return fail(PG_ERR_INVALID, "pg_dbg_gemm_v: variant must be -1, 1, 2, 6, 7, 8, 20 or 80");
  const bool strict = precision == PG_PREC_FP32;      // K-concatenated split-bf16 operands (engine.h dense3)
  if (strict && variant != -1) return fail(PG_ERR_UNSUPPORTED, "strict mode: launch_gemm_split3 has no variant (-1 only)");
  if (strict && epi == 5 && N % 256) return fail(PG_ERR_INVALID, "pg_dbg_gemm: the fused GELU-and-split epilogue needs N a multiple of 256");
  if (strict && epi != 0 && epi != 2 && epi != 5)
    return fail(PG_ERR_UNSUPPORTED, "strict mode: plain (0), residual (2) and fused GELU-split (5) epilogues only");
  Dbg d;
  if ((rc = d.open(device))) return rc;
  const int Mp = round_up(M, kRowPad), ks = strict ? 3 : 1;
  const int M16 = M <= 256 ? round_up(M, 16) : Mp;      // the rows the 16-bit kernels are given
  const bool out16 = !strict && (epi == 3 || epi == 4);      // bf16 outputs (the QKV / fc1 epilogues), widened to fp32 for the caller
  float* dx = d.alloc<float>((size_t)Mp * K);
  d.put(dx, x, (size_t)M * K);
  const float* dw = d.up(w, (size_t)N * K);
  const float* db = d.up(bias, (size_t)N);
  float* dout = d.alloc<float>((size_t)Mp * N);
  if (epi == 2) d.put(dout, out, (size_t)M * N);      // residual variant: out += x w^T + b
  bf16_t* bx = d.alloc<bf16_t>((size_t)Mp * K * ks);
  bf16_t* bw = d.alloc<bf16_t>((size_t)N * K * ks);
  // fc1's fused strict epilogue (5): operand rows [lo | hi | hi] of gelu(x w^T + b), returned as hi + lo
  bf16_t* o16 = strict && epi == 5 ? d.alloc<bf16_t>((size_t)Mp * 3 * N) : out16 ? d.alloc<bf16_t>((size_t)Mp * N) : nullptr;
  // the residual variant gets split-K scratch, as the engine gives its fc2 GEMMs (taken for deep K and few tiles); have_ws 1 offers
  // it to every epilogue (the plan takes it for the residual one only), 0 withholds it
  const bool offer = have_ws < 0 ? epi == 2 : have_ws == 1;
  const size_t ws_bytes = !strict && offer ? OPS(gemm_splitk_ws_bytes, Mp, N, K) : 0;
  float* ws = ws_bytes && ws_bytes <= ((size_t)1 << 30) ? (float*)d.alloc<char>(ws_bytes) : nullptr;
  if ((rc = d.check())) return rc;
  if (strict) {
    if ((rc = launch_split3_bf16(nullptr, dx, bx, Mp, K, 1.f, false, false))) return rc;
    if ((rc = launch_split3_bf16(nullptr, dw, bw, N, K, 1.f, false, true))) return rc;
    clear_noted_kernels();
    if (epi == 5) {
      if ((rc = launch_gemm_split3(nullptr, bx, bw, db, o16, Mp, N, K, 3 * N, EPI_SPLIT3_GELU))) return rc;
      dbg_noted_text(plan, plan_bytes);
      return split3_rows_to_host(o16, out, M, N);
    }
    if ((rc = launch_gemm_split3(nullptr, bx, bw, db, dout, Mp, N, K, N, epi == 2 ? EPI_F32_RESID : EPI_F32))) return rc;
    dbg_noted_text(plan, plan_bytes);
    return d.down(out, dout, (size_t)M * N);
  }
  if ((rc = to16(precision, dx, bx, (int64_t)Mp * K))) return rc;
  if ((rc = to16(precision, dw, bw, (int64_t)N * K))) return rc;
  clear_noted_kernels();
  void* o = out16 ? (void*)o16 : (void*)dout;
  const int e = out16 ? (epi == 4 ? EPI_BF16_GELU : EPI_BF16) : (epi == 2 ? EPI_F32_RESID : (epi ? EPI_F32_GELU : EPI_F32));
  rc = variant < 0 ? OPS(launch_gemm_bf16, nullptr, bx, bw, db, o, M16, N, K, K, K, N, e, ws, ws ? ws_bytes : 0, m_live)
                   : OPS(launch_gemm_bf16_variant, nullptr, bx, bw, db, o, M16, N, K, K, K, N, e, variant, ws, ws ? ws_bytes : 0, m_live);
  if (rc) return rc;
  dbg_noted_text(plan, plan_bytes);
  return out16 ? down16(d, precision, o16, dout, out, (int64_t)M * N) : d.down(out, dout, (size_t)M * N);
}

/* gemm_ln_skinny_kernel alone: out = LayerNorm(x; gamma, beta, eps) . w^T + bias (+ GELU) in the 16-bit type of `precision`.
 * x[M][K] holds the live rows, M = 1 .. 32; the kernel runs on Mi = 16 or 32 rows, and x_pad[Mi - M][K] (NULL: zeros) is what the rows
 * behind the live ones hold.  out[out_rows][N], out_rows >= Mi, is converted to 16 bits and uploaded first, the kernel writes its Mi
 * rows into it, and all out_rows rows come back widened: what the kernel does not write keeps the caller's pattern.  nb: 16-feature
 * blocks per workgroup, 0 = the launcher's choice.  plan (may be NULL): the text the launch recorded.  Everything is refused on the host
 * before a device is looked for. */
int pg_dbg_gemm_ln(int device, int precision, const float* x, const float* x_pad, const float* gamma, const float* beta, float eps,
                   const float* w, const float* bias, float* out, int out_rows, int M, int N, int K, int gelu, int nb, char* plan,
                   int plan_bytes) {
  if (plan && plan_bytes > 0) plan[0] = 0;
  int rc = dbg_precision("pg_dbg_gemm_ln", precision, false);
  if (rc) return rc;
  if (!x || !gamma || !beta || !w || !bias || !out || (plan && plan_bytes < 1)) return fail(PG_ERR_INVALID, "pg_dbg_gemm_ln: bad argument");
  if (M < 1 || M > 32) return fail(PG_ERR_INVALID, "pg_dbg_gemm_ln: M must be in 1 ... 32");
  if (N < 16 || N % 16 || N > 65536) return fail(PG_ERR_INVALID, "pg_dbg_gemm_ln: N must be a multiple of 16, at most 65536");
  if (K < 256 || K % 256) return fail(PG_ERR_INVALID, "pg_dbg_gemm_ln: K must be a multiple of 256");
  if (K / 256 > 5) return fail(PG_ERR_INVALID, "pg_dbg_gemm_ln: K / 256 must be in 1 ... 5");
  if (gelu < 0 || gelu > 1 || nb < 0 || nb > 2) return fail(PG_ERR_INVALID, "pg_dbg_gemm_ln: gelu is 0 or 1 and nb 0, 1 or 2");
  if (nb == 2 && N % 32) return fail(PG_ERR_INVALID, "pg_dbg_gemm_ln: two feature blocks per workgroup need N a multiple of 32");
  if (!(eps >= 0.f)) return fail(PG_ERR_INVALID, "pg_dbg_gemm_ln: eps must not be negative");
  const int Mi = round_up(M, 16);
  if (out_rows < Mi || out_rows > 4096) return fail(PG_ERR_INVALID, "pg_dbg_gemm_ln: out_rows must be in Mi ... 4096");
  if (!OPS(gemm_ln_skinny_ok, Mi, N, K)) return fail(PG_ERR_INVALID, "pg_dbg_gemm_ln: the kernel is switched off (PGIBBS_LN_SKINNY=0)");
  Dbg d;
  if ((rc = d.open(device))) return rc;
  float* dx = d.alloc<float>((size_t)Mi * K);
  d.put(dx, x, (size_t)M * K);
  if (x_pad) d.put(dx + (size_t)M * K, x_pad, (size_t)(Mi - M) * K);
  const float* dg = d.up(gamma, (size_t)K);
  const float* dbt = d.up(beta, (size_t)K);
  const float* dw = d.up(w, (size_t)N * K);
  const float* db = d.up(bias, (size_t)N);
  float* dout = d.up(out, (size_t)out_rows * N);      // the caller's pattern, fp32 on the way in and on the way out
  bf16_t* bw = d.alloc<bf16_t>((size_t)N * K);
  bf16_t* o16 = d.alloc<bf16_t>((size_t)out_rows * N);
  if ((rc = d.check())) return rc;
  if ((rc = to16(precision, dw, bw, (int64_t)N * K))) return rc;
  if ((rc = to16(precision, dout, o16, (int64_t)out_rows * N))) return rc;
  clear_noted_kernels();
  if ((rc = OPS(launch_gemm_ln_skinny, nullptr, dx, K, dg, dbt, eps, bw, db, o16, Mi, N, K, K, N, gelu ? EPI_BF16_GELU : EPI_BF16, nb))) return rc;
  dbg_noted_text(plan, plan_bytes);
  return down16(d, precision, o16, dout, out, (int64_t)out_rows * N);
}

int pg_dbg_gemm_bench(int device, int M, int N, int K, int epi, int variant, int iters, double* avg_ms) {
  if (!avg_ms || M % 16 || (M > 256 && M % 64) || N % 64 || K % 64 || iters < 1) return fail(PG_ERR_INVALID, "pg_dbg_gemm_bench: bad argument");
  if (variant == 90 && (K % 96 || (epi != EPI_F32 && epi != EPI_F32_RESID))) return fail(PG_ERR_INVALID, "variant 90: K = 3 x depth, fp32 epilogues");
  Dbg d;
  int rc = d.open(device);
  if (rc) return rc;
  const std::vector<float> h = lcg_uniform((size_t)(M > N ? M : N) * K, 12345u);
  const float* f = d.up(h.data(), h.size());
  bf16_t* bx = d.alloc<bf16_t>((size_t)round_up(M, kRowPad) * K);      // kernels may touch the padding rows of the last tile
  bf16_t* bw = d.alloc<bf16_t>((size_t)N * K);
  const float* db = d.alloc<float>((size_t)N);
  void* dout = d.alloc<float>((size_t)round_up(M, kRowPad) * N);
  const size_t ws_bytes = (epi == EPI_F32_RESID && M <= 8192) ? gemm_splitk_ws_bytes(M, N, K) : 0;
  float* ws = ws_bytes ? (float*)d.alloc<char>(ws_bytes) : nullptr;
  if ((rc = d.check())) return rc;
  if ((rc = to16(PG_PREC_BF16, f, bx, (int64_t)M * K))) return rc;
  if ((rc = to16(PG_PREC_BF16, f, bw, (int64_t)N * K, 0.05f))) return rc;
  // variant 90: the strict mode's fused three-product kernel on operands of logical depth K / 3 (K = 3 x depth, as the plain
  // kernels see them), so that "variant 2, K" and "variant 90, K" time the same arithmetic
  return time_launches([&] {
    if (variant == 90) return launch_gemm_split3_w16(nullptr, bx, bw, db, dout, M, N, K / 3, N, epi);
    return launch_gemm_bf16_variant(nullptr, bx, bw, db, dout, M, N, K, K, K, N, epi, variant, ws, ws ? ws_bytes : 0);
  }, iters, avg_ms);
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
  const int rc = dbg_precision("pg_dbg_attention_plan", precision, true);
  if (rc) return rc;
  if (!buf || buf_bytes < 2 || (kind != 0 && kind != 1) || n_seq_or_B < 1 || H < 1 || n_cu < 1 || (kind == 1 && (R < 1 || n_seq_or_B > 0x7fffffff)))
    return fail(PG_ERR_INVALID, "pg_dbg_attention_plan: bad argument");
  const bool strict = precision == PG_PREC_FP32;
  std::string text;
  if (kind == 0 && strict) attention_f32_plan_text(n_seq_or_B, T_or_C, H, head_dim, has_pad != 0, has_bias != 0, &text);
  else if (kind == 0) attention_plan_text(n_seq_or_B, T_or_C, H, head_dim, has_pad != 0, has_bias != 0, row_step, n_cu, &text);
  else if (strict) msa_row_f32_plan_text((int)n_seq_or_B, R, T_or_C, H, &text);
  else msa_row_plan_text((int)n_seq_or_B, R, T_or_C, H, order_bh, &text);
  snprintf(buf, (size_t)buf_bytes, "%s", text.c_str());
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
  Dbg s;
  int rc = s.open(device);
  if (rc) return rc;
  const int d = H * 64;
  const int64_t M = (int64_t)B * T, Mp = round_up64(M, kRowPad);
  const std::vector<float> h = lcg_uniform((size_t)std::max<int64_t>(Mp, 3 * d) * d, 777u);
  const float* fx = s.up(h.data(), (size_t)Mp * d);      // x, W and the bias all start at the sequence's first value
  const float* fw = s.up(h.data(), (size_t)3 * d * d);
  const float* db = s.up(h.data(), (size_t)3 * d);
  bf16_t* bx = s.alloc<bf16_t>((size_t)Mp * d);
  bf16_t* bw = s.alloc<bf16_t>((size_t)3 * d * d);
  bf16_t* bwh = s.alloc<bf16_t>((size_t)3 * d * d);
  float* dbh = s.alloc<float>((size_t)3 * d);
  bf16_t* qkv = s.alloc<bf16_t>((size_t)Mp * 3 * d);
  bf16_t* c1 = s.alloc<bf16_t>((size_t)Mp * d);
  bf16_t* c2 = s.alloc<bf16_t>((size_t)Mp * d);
  if ((rc = s.check())) return rc;
  if ((rc = to16(PG_PREC_BF16, fx, bx, Mp * d))) return rc;
  if ((rc = to16(PG_PREC_BF16, fw, bw, (int64_t)3 * d * d, 0.03f))) return rc;
  if ((rc = launch_headmajor_qkv(nullptr, bw, db, bwh, dbh, H, d))) return rc;
  auto fused = [&] { return launch_gemm_colattn(nullptr, bx, bwh, dbh, c1, B, T, 1, H, d, d); };
  auto proj = [&] { return launch_gemm_bf16(nullptr, bx, bw, db, qkv, (int)Mp, 3 * d, d, d, d, 3 * d, EPI_BF16); };
  auto attn = [&] { return launch_attention_bf16(nullptr, qkv, c2, B, T, H, 3 * d, d, d, 2 * d); };
  if ((rc = time_launches(fused, iters, ms + 0)) || (rc = time_launches(proj, iters, ms + 1)) || (rc = time_launches(attn, iters, ms + 2)))
    return rc;
  if (max_diff) {
    std::vector<bf16_t> a((size_t)M * d), b((size_t)M * d);
    if ((rc = s.down(a.data(), c1, a.size())) || (rc = s.down(b.data(), c2, b.size()))) return rc;
    double worst = 0;
    for (size_t i = 0; i < a.size(); ++i) worst = std::max(worst, (double)fabsf(bf16_to_f32(a[i]) - bf16_to_f32(b[i])));
    *max_diff = worst;
  }
  return PG_OK;
}

/* gemm_colattn_kernel alone (fused 1), or the two launches of the engine's unfused column block on the same 16-bit operands
 * (fused 0): x[B*R*C][d] in token order, w[3 d][d] (q rows first) and bias[3 d] -> context rows in token order.  The fused launch
 * gets what the engine gives it: the operand rows permuted on the host to column-major order (row (b*C + c)*R + r) in a buffer of
 * round_up(B*C*R, 256) rows whose rows behind the live ones hold pad_fill, and head-major weights from launch_headmajor_qkv.
 * ctx_inout[ctx_rows][d] goes up as the caller's pattern in the 16-bit type and comes back whole, widened.  Everything is refused on
 * the host before a device is looked for; the kernel switched off (PGIBBS_MSA_COLFUSE=0) is the launcher's own error. */
int pg_dbg_colattn(int device, int precision, const float* x, const float* w, const float* bias, float* ctx_inout, int64_t ctx_rows, int B,
                   int R, int C, int H, int fused, float pad_fill, char* plan, int plan_bytes) {
  if (plan && plan_bytes > 0) plan[0] = 0;
  int rc = dbg_precision("pg_dbg_colattn", precision, false);
  if (rc) return rc;
  if (!x || !w || !bias || !ctx_inout) return fail(PG_ERR_INVALID, "pg_dbg_colattn: null argument");
  if (B < 1 || C < 1 || H < 1) return fail(PG_ERR_INVALID, "pg_dbg_colattn: B, C and H must be at least 1");
  if (!(R == 32 || R == 64 || R == 128 || R == 256)) return fail(PG_ERR_INVALID, "pg_dbg_colattn: R must be 32, 64, 128 or 256");
  if (fused < 0 || fused > 1 || (plan && plan_bytes < 1)) return fail(PG_ERR_INVALID, "pg_dbg_colattn: fused is 0 or 1, and a plan buffer has room");
  if (!std::isfinite(pad_fill)) return fail(PG_ERR_INVALID, "pg_dbg_colattn: pad_fill must be finite");
  const double m_live = (double)B * R * C;
  if ((double)ctx_rows < m_live) return fail(PG_ERR_INVALID, "pg_dbg_colattn: ctx_rows must be at least B*R*C");
  if ((m_live + 255.0) * 3 * H * 64 > 2147483647.0 || (double)ctx_rows * H * 64 > 2147483647.0 || 3.0 * H * 64 * H * 64 > 2147483647.0)
    return fail(PG_ERR_INVALID, "pg_dbg_colattn: more than 2^31 - 1 values");
  Dbg s;
  if ((rc = s.open(device))) return rc;
  const int d = H * 64;
  const int64_t M = (int64_t)B * R * C, Mp = round_up64(M, kRowPad);
  // the operand rows as the launch reads them: column-major for the fused kernel, token order otherwise; pad_fill behind them
  std::vector<float> hx((size_t)Mp * d, pad_fill);
  for (int64_t t = 0; t < M; ++t) {
    const int64_t b = t / ((int64_t)R * C), r = t / C % R, c = t % C;
    const int64_t row = fused ? (b * C + c) * R + r : t;
    memcpy(&hx[(size_t)row * d], x + (size_t)t * d, (size_t)d * 4);
  }
  const float* dx = s.up(hx.data(), hx.size());
  const float* dw = s.up(w, (size_t)3 * d * d);
  const float* db = s.up(bias, (size_t)3 * d);
  float* dctx = s.up(ctx_inout, (size_t)ctx_rows * d);      // the caller's pattern, fp32 on the way in and on the way out
  bf16_t* bx = s.alloc<bf16_t>((size_t)Mp * d);
  bf16_t* bw = s.alloc<bf16_t>((size_t)3 * d * d);
  bf16_t* c16 = s.alloc<bf16_t>((size_t)ctx_rows * d);
  bf16_t* bwh = fused ? s.alloc<bf16_t>((size_t)3 * d * d) : nullptr;
  float* dbh = fused ? s.alloc<float>((size_t)3 * d) : nullptr;
  bf16_t* qkv = fused ? nullptr : s.alloc<bf16_t>((size_t)Mp * 3 * d);
  if ((rc = s.check("hipMalloc / copy failed"))) return rc;
  if ((rc = to16(precision, dx, bx, Mp * d))) return rc;
  if ((rc = to16(precision, dw, bw, (int64_t)3 * d * d))) return rc;
  if ((rc = to16(precision, dctx, c16, ctx_rows * d))) return rc;
  clear_noted_kernels();
  if (fused) {
    if ((rc = OPS(launch_headmajor_qkv, nullptr, bw, db, bwh, dbh, H, d))) return rc;
    if ((rc = OPS(launch_gemm_colattn, nullptr, bx, bwh, dbh, c16, B, R, C, H, d, d))) return rc;
  } else {
    const SeqLayout col = {C, R * C, 1, C};
    if ((rc = OPS(launch_gemm_bf16, nullptr, bx, bw, db, qkv, (int)Mp, 3 * d, d, d, d, 3 * d, EPI_BF16))) return rc;
    if ((rc = OPS(launch_attention_seq_bf16, nullptr, qkv, c16, (int64_t)B * C, R, H, 3 * d, d, d, 2 * d, col))) return rc;
  }
  dbg_noted_text(plan, plan_bytes);
  return down16(s, precision, c16, dctx, ctx_inout, ctx_rows * d);
}

int pg_dbg_layernorm(int device, const float* x, const float* gamma, const float* beta, float* y, int M, int d, float eps) {
  if (!x || !gamma || !beta || !y || M < 1 || d < 4) return fail(PG_ERR_INVALID, "pg_dbg_layernorm: bad argument");
  Dbg s;
  int rc = s.open(device);
  if (rc) return rc;
  const float* dx = s.up(x, (size_t)M * d);
  const float* dg = s.up(gamma, (size_t)d);
  const float* dbt = s.up(beta, (size_t)d);
  float* dy = s.alloc<float>((size_t)M * d);
  if ((rc = s.check())) return rc;
  if ((rc = launch_layernorm_f32(nullptr, dx, dg, dbt, dy, M, d, eps))) return rc;
  return s.down(y, dy, (size_t)M * d);
}

int pg_dbg_attention(int device, int precision, const float* qkv, float* ctx, int B, int T, int H) {
  return pg_dbg_attention_hd(device, precision, qkv, ctx, B, T, H, 64, nullptr, -1);
}

/* pg_dbg_attention with the head dimension (a width of head_width.h) and, optionally, the tokens of the keys: key_tok[B][T], keys whose token is
 * pad_idx are masked as in a ragged batch (NULL: none) */
int pg_dbg_attention_hd(int device, int precision, const float* qkv, float* ctx, int B, int T, int H, int head_dim,
                        const int32_t* key_tok, int pad_idx) {
  return pg_dbg_attention_kv(device, precision, qkv, ctx, B, T, H, head_dim, key_tok, pad_idx, nullptr, nullptr, nullptr, 0);
}

/* pg_dbg_attention_hd with ESM-1's bias key: bias_k / bias_v [H][head_dim] fp32 (both or neither), laid out as the engine lays them
 * out -- [bias_k | bias_v], k of head h at h*HD, v at (H + h)*HD -- in the operand type of `precision` (fp32 for the strict
 * kernels).  Everything is checked on the host before a device is looked for.  plan (may be NULL): the text the launch recorded */
int pg_dbg_attention_kv(int device, int precision, const float* qkv, float* ctx, int B, int T, int H, int head_dim,
                        const int32_t* key_tok, int pad_idx, const float* bias_k, const float* bias_v, char* plan, int plan_bytes) {
  if (plan && plan_bytes > 0) plan[0] = 0;
  int rc = dbg_precision("pg_dbg_attention_kv", precision, true);
  if (rc) return rc;
  if (!qkv || !ctx || B < 1 || T < 1 || H < 1 || (plan && plan_bytes < 1)) return fail(PG_ERR_INVALID, "pg_dbg_attention: bad argument");
  if (!head_width(head_dim)) return fail(PG_ERR_INVALID, "pg_dbg_attention_hd: head_dim must be " + head_widths_text(false));
  if (!bias_k != !bias_v) return fail(PG_ERR_INVALID, "pg_dbg_attention_kv: bias_k and bias_v come together or not at all");
  const std::string head_err = attention_head_error(head_dim, bias_k != nullptr);      // the plans' own refusal of a bias key at head 32
  if (!head_err.empty()) return fail(PG_ERR_INVALID, head_err);
  if ((double)B * T * 3 * H * head_dim > 2147483647.0) return fail(PG_ERR_INVALID, "pg_dbg_attention: more than 2^31 - 1 qkv values");
  Dbg s;
  if ((rc = s.open(device))) return rc;
  const int d = H * head_dim;
  const bool strict = precision == PG_PREC_FP32;
  float* bias32 = bias_k ? s.alloc<float>((size_t)2 * d) : nullptr;      // [bias_k | bias_v], d fp32 each
  if (bias_k) s.put(bias32, bias_k, (size_t)d), s.put(bias32 + d, bias_v, (size_t)d);
  bf16_t* bias16 = bias_k && !strict ? s.alloc<bf16_t>((size_t)2 * d) : nullptr;
  return dbg_attention_run(s, precision, strict, qkv, ctx, (int64_t)B * T, d, key_tok, plan, plan_bytes,
                           [&](const float* dq, const bf16_t* bq, bf16_t* out, const int32_t* dtok) {
    const SeqLayout chain = {1, T, 0, 1};
    if (strict) return launch_attention_f32(nullptr, dq, out, d, B, T, H, 3 * d, 3 * d, d, 2 * d, chain, dtok, pad_idx, bias32, head_dim);
    const int rc16 = bias_k ? to16(precision, bias32, bias16, 2 * d) : PG_OK;
    return rc16 ? rc16 : OPS(launch_attention_bf16, nullptr, bq, out, B, T, H, 3 * d, d, d, 2 * d, dtok, pad_idx, bias16, head_dim);
  });
}

/* LayerNorm as the engine's GEMMs read it: the operand rows launch_layernorm_bf16 writes in `precision`, widened to fp32 --
 * bf16 or fp16 rows, or (PG_PREC_FP32) the strict mode's split rows [lo | hi | hi] returned as hi + lo, the two hi copies checked */
int pg_dbg_layernorm_operand(int device, int precision, const float* x, const float* gamma, const float* beta, float* y, int M, int d,
                             float eps) {
  int rc = dbg_precision("pg_dbg_layernorm_operand", precision, true);
  if (rc) return rc;
  if (!x || !gamma || !beta || !y || M < 1 || d < 32 || d % 32) return fail(PG_ERR_INVALID, "pg_dbg_layernorm_operand: bad argument");
  Dbg s;
  if ((rc = s.open(device))) return rc;
  const bool split = precision == PG_PREC_FP32;
  const float* dx = s.up(x, (size_t)M * d);
  const float* dg = s.up(gamma, (size_t)d);
  const float* dbt = s.up(beta, (size_t)d);
  float* dy = s.alloc<float>((size_t)M * d);
  bf16_t* h = s.alloc<bf16_t>((size_t)M * d * (split ? 3 : 1));
  if ((rc = s.check())) return rc;
  if ((rc = OPS(launch_layernorm_bf16, nullptr, dx, dg, dbt, h, M, d, eps, split, 0, 0, true))) return rc;
  return split ? split3_rows_to_host(h, y, M, d) : down16(s, precision, h, dy, y, (int64_t)M * d);
}

/* ESM-2's rotary embedding on a host fp32 buffer qkv[B*T][3*H*64]: the q and k thirds rotated in place (row r at position r % T),
 * v left alone.  16-bit modes: through a device buffer of that type, the result widened back */
int pg_dbg_rope(int device, int precision, float* qkv, int B, int T, int H) {
  return pg_dbg_rope_hd(device, precision, qkv, B, T, H, 64);
}

/* pg_dbg_rope with the head dimension: a width of head_width.h, at most its max_heads heads */
int pg_dbg_rope_hd(int device, int precision, float* qkv, int B, int T, int H, int head_dim) {
  int rc = dbg_precision("pg_dbg_rope_hd", precision, true);
  if (rc) return rc;
  const HeadWidth* w = head_width(head_dim);
  if (!w) return fail(PG_ERR_INVALID, "pg_dbg_rope_hd: head_dim must be " + head_widths_text(false));
  if (!qkv || B < 1 || T < 1 || H < 1 || H > w->max_heads) return fail(PG_ERR_INVALID, "pg_dbg_rope: bad argument");
  Dbg s;
  if ((rc = s.open(device))) return rc;
  const int d = H * head_dim;
  const int64_t M = (int64_t)B * T, n = M * 3 * d;
  const std::vector<float> tab = rope_table(T, head_dim);
  float* dq = s.up(qkv, (size_t)n);
  const float* dtab = s.up(tab.data(), tab.size());
  bf16_t* bq = precision == PG_PREC_FP32 ? nullptr : s.alloc<bf16_t>((size_t)n);
  if ((rc = s.check())) return rc;
  if (precision == PG_PREC_FP32) {
    if ((rc = launch_rope(nullptr, dq, true, dtab, T, M, T, H, 3 * d, head_dim))) return rc;
    return s.down(qkv, dq, (size_t)n);
  }
  if ((rc = to16(precision, dq, bq, n))) return rc;
  if ((rc = OPS(launch_rope, nullptr, bq, false, dtab, T, M, T, H, 3 * d, head_dim))) return rc;
  return down16(s, precision, bq, dq, qkv, n);
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
  Dbg s;
  int rc = s.open(device);
  if (rc) return rc;
  const int d = H * 64;
  const int64_t M = (int64_t)B * R * C;
  const bool strict = which == 2 || which == 3;      // strict precision mode kernels: fp32 in, [lo | hi | hi] operand rows out
  const bool ragged = which == 0 && tok;
  // a ragged batch, as Engine::msa_trunk runs it: the 16-bit q, k, v widened to fp32, fp32 scores through a scratch buffer
  float* wide = ragged ? s.alloc<float>((size_t)M * 3 * d) : nullptr;
  float* sc = which == 2 || ragged ? s.alloc<float>((size_t)B * H * C * msa_row_scores_ld(C)) : nullptr;
  // scratch for the split-R mode (taken when B*H*ceil(C/64) < 384 and R >= 8), so the tests exercise both modes
  const size_t pbytes = (size_t)B * H * 16 * C * 576 * 4 + (size_t)B * H * (C / 16 + 9) * 18 * 1024;
  float* part = which == 0 && !tok && pbytes <= ((size_t)1 << 30) ? (float*)s.alloc<char>(pbytes) : nullptr;
  return dbg_attention_run(s, precision, strict, qkv, ctx, M, d, tok, plan, plan_bytes,
                           [&](const float* dq, const bf16_t* bq, bf16_t* out, const int32_t* dtok) {
    const SeqLayout col = {C, R * C, 1, C};
    if (which == 2) return launch_msa_row_attention_f32(nullptr, dq, sc, out, d, B, R, C, H, 3 * d, 3 * d, d, 2 * d, scale, dtok, pad_idx);
    if (which == 3) return launch_attention_f32(nullptr, dq, out, d, (int64_t)B * C, R, H, 3 * d, 3 * d, d, 2 * d, col, dtok, pad_idx);
    if (ragged) {
      const int rcw = launch_bf16_to_f32(nullptr, bq, wide, M * 3 * d);
      return rcw ? rcw : launch_msa_row_attention_f32(nullptr, wide, sc, out, 0, B, R, C, H, 3 * d, d, d, 2 * d, scale, dtok, pad_idx);
    }
    if (which == 0) return OPS(launch_msa_row_attention_bf16, nullptr, bq, out, B, R, C, H, 3 * d, d, d, 2 * d, scale, part, part ? pbytes : 0, 0);
    return OPS(launch_attention_seq_bf16, nullptr, bq, out, (int64_t)B * C, R, H, 3 * d, d, d, 2 * d, col, dtok, pad_idx);
  });
}

// ---- the row kernels of elementwise.hip ---------------------------------------------------------------------------------------------
// Every entry below checks its arguments on the host first -- shapes, then every token, position row, row_map entry and gathered
// row the kernel would read against the sizes the caller states -- and only then looks for a device: a wrong array is
// PG_ERR_INVALID with a message, never a GPU fault, and the refusals can be tested without a GPU.
extern "C++" {
namespace {
int dbg_row_width(const char* who, int d, int d_live) {
  if (!row_d_ok(d)) return
    fail(PG_ERR_INVALID, std::string(who) + ": d must be a multiple of 4 and <= 2560, or a multiple of 512 up to 5120");
  if (!row_live_ok(d, d_live)) return fail(PG_ERR_INVALID, std::string(who) + ": the live width must be a multiple of 4, at most d");
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
const char* const kCopyFailed = "hipMalloc / copy failed";
}  // namespace
}  // extern "C++"

/* The live-width forms (pgibbs.h; the pg_dbg_* entries are these at d_live = d): rows d wide in memory whose first d_live features are
 * the model's own.  Tables, rows and vectors are all d wide; h2 / h_inout come back with the caller's pattern wherever the kernel
 * wrote nothing */
static int dbg_embed_rows(const char* who, int device, int precision, const int32_t* tokens, int n_seq, int T, const float* embed, int V, int d,
                           const float* pos, int pos_rows, const float* msa_pos, int rows_per_msa, const float* gamma, const float* beta,
                           const float* gamma2, const float* beta2, int pad_idx, int mask_idx, int token_dropout, float eps, float embed_scale,
                           float* x, uint16_t* h2, int d_live) {
  int rc = dbg_precision(who, precision, false);
  if (rc) return rc;
  if (!tokens || !embed || !x || n_seq < 1 || T < 1 || V < 1 || (pos && pos_rows < 1) || rows_per_msa < 0 || (rows_per_msa > 0 && !msa_pos) ||
      !gamma != !beta || !gamma2 != !beta2 || !gamma2 != !h2)
    return fail(PG_ERR_INVALID, std::string(who) + ": bad argument");
  if ((rc = dbg_row_width(who, d, d_live))) return rc;
  if (d_live != d && gamma) return fail(PG_ERR_INVALID, std::string(who) + ": emb_layer_norm_before has no live-width form");
  const int64_t n_tok = (int64_t)n_seq * T;
  for (int64_t sq = 0; sq < n_seq; ++sq) {
    int n_before = 0;
    for (int t = 0; t < T; ++t) {
      const int32_t tok = tokens[sq * T + t];
      if (tok < 0 || tok >= V)
        return fail(PG_ERR_INVALID, std::string(who) + ": token " + std::to_string(tok) + " is outside the embedding table of " + std::to_string(V) + " rows");
      n_before += tok != pad_idx;
      const int p = tok == pad_idx ? pad_idx : n_before + pad_idx;      // embed_ln_kernel's position row
      if (pos && (p < 0 || p >= pos_rows))
        return fail(PG_ERR_INVALID, std::string(who) + ": position row " + std::to_string(p) + " is outside the position table of " + std::to_string(pos_rows) + " rows");
    }
  }
  Dbg s;
  if ((rc = s.open(device))) return rc;
  const int32_t* dtok = s.up(tokens, (size_t)n_tok);
  const float* de = s.up(embed, (size_t)V * d);
  const float* dp = s.up(pos, (size_t)pos_rows * d);
  const float* dm = rows_per_msa > 0 ? s.up(msa_pos, (size_t)rows_per_msa * d) : nullptr;
  const float* dg = s.up(gamma, (size_t)d);
  const float* db = s.up(beta, (size_t)d);
  const float* dg2 = s.up(gamma2, (size_t)d);
  const float* db2 = s.up(beta2, (size_t)d);
  float* dx = s.alloc<float>((size_t)n_tok * d);
  bf16_t* dh = h2 ? s.up((const bf16_t*)h2, (size_t)n_tok * d) : nullptr;      // the caller's pattern
  if ((rc = s.check(kCopyFailed))) return rc;
  if ((rc = OPS(launch_embed_ln, nullptr, dtok, de, dp, dm, dg, db, dx, n_tok, T, d, pad_idx, mask_idx, token_dropout, rows_per_msa, eps, dg2,
                db2, dh, embed_scale, d_live)))
    return rc;
  if ((rc = s.down(x, dx, (size_t)n_tok * d))) return rc;
  return h2 ? s.down(h2, dh, (size_t)n_tok * d) : PG_OK;
}

int pg_dbg_embed(int device, int precision, const int32_t* tokens, int n_seq, int T, const float* embed, int V, int d, const float* pos,
                 int pos_rows, const float* msa_pos, int rows_per_msa, const float* gamma, const float* beta, const float* gamma2,
                 const float* beta2, int pad_idx, int mask_idx, int token_dropout, float eps, float embed_scale, float* x, uint16_t* h2) {
  return dbg_embed_rows("pg_dbg_embed", device, precision, tokens, n_seq, T, embed, V, d, pos, pos_rows, msa_pos, rows_per_msa, gamma, beta, gamma2, beta2,
                                pad_idx, mask_idx, token_dropout, eps, embed_scale, x, h2, d);
}

int pg_embedded_embed_rows(int device, int precision, const int32_t* tokens, int n_seq, int T, const float* embed, int V, int d,
                           const float* pos, int pos_rows, const float* msa_pos, int rows_per_msa, const float* gamma, const float* beta,
                           const float* gamma2, const float* beta2, int pad_idx, int mask_idx, int token_dropout, float eps, float embed_scale,
                           float* x, uint16_t* h2, int d_live) {
  return dbg_embed_rows("pg_embedded_embed_rows", device, precision, tokens, n_seq, T, embed, V, d, pos, pos_rows, msa_pos, rows_per_msa, gamma, beta, gamma2, beta2, pad_idx, mask_idx, token_dropout, eps, embed_scale, x, h2, d_live);
}

static int dbg_layernorm_rows(const char* who, int device, int precision, const float* x, const float* gamma, const float* beta, uint16_t* h_inout,
                               int64_t h_rows, int M, int d, float eps, int form, int colmajor_R, int colmajor_C, int* kernel, int d_live) {
  int rc = dbg_precision(who, precision, false);
  if (rc) return rc;
  if (!x || !gamma || !beta || !h_inout || M < 1 || h_rows < M || form < 0 || form > 2 || colmajor_R < 0 || (colmajor_R > 0 && colmajor_C < 1))
    return fail(PG_ERR_INVALID, std::string(who) + ": bad argument");
  if (form && (precision != PG_PREC_BF16 || d % 32))
    return fail(PG_ERR_INVALID, std::string(who) + ": split rows are bf16 pairs in groups of 32 columns");
  if (row_d_ok(d) && !row_live_ok(d, d_live)) return fail(PG_ERR_INVALID, std::string(who) + ": the live width must be a multiple of 4, at most d");
  if ((rc = OPS(layernorm_bf16_check, M, d, form != 0, colmajor_R, colmajor_C, d_live))) return rc;
  Dbg s;
  if ((rc = s.open(device))) return rc;
  const size_t h_n = (size_t)h_rows * d * (form ? 3 : 1);
  const float* dx = s.up(x, (size_t)M * d);
  const float* dg = s.up(gamma, (size_t)d);
  const float* db = s.up(beta, (size_t)d);
  bf16_t* dh = s.up(h_inout, h_n);      // the caller's pattern: what the kernel leaves unwritten keeps it
  if ((rc = s.check(kCopyFailed))) return rc;
  unsigned stride_grid = 0;
  if (kernel) *kernel = OPS(layernorm_bf16_choice, M, d, colmajor_R, &stride_grid, d_live);
  if ((rc = OPS(launch_layernorm_bf16, nullptr, dx, dg, db, dh, M, d, eps, form != 0, colmajor_R, colmajor_C, form != 2, d_live))) return rc;
  return s.down(h_inout, dh, h_n);
}

int pg_dbg_layernorm_rows(int device, int precision, const float* x, const float* gamma, const float* beta, uint16_t* h_inout,
                          int64_t h_rows, int M, int d, float eps, int form, int colmajor_R, int colmajor_C, int* kernel) {
  return dbg_layernorm_rows("pg_dbg_layernorm_rows", device, precision, x, gamma, beta, h_inout, h_rows, M, d, eps, form, colmajor_R, colmajor_C, kernel, d);
}

int pg_embedded_layernorm_rows(int device, int precision, const float* x, const float* gamma, const float* beta, uint16_t* h_inout,
                               int64_t h_rows, int M, int d, float eps, int form, int colmajor_R, int colmajor_C, int* kernel, int d_live) {
  return dbg_layernorm_rows("pg_embedded_layernorm_rows", device, precision, x, gamma, beta, h_inout, h_rows, M, d, eps, form, colmajor_R, colmajor_C, kernel, d_live);
}

static int dbg_gather_ln_rows(const char* who, int device, int precision, const float* x, int64_t x_rows, const int32_t* idx, const int32_t* row_map, int64_t n_map,
                          int P, int width, const float* gamma, const float* beta, uint16_t* h_inout, int64_t h_rows, int64_t n_sel, int d,
                          float eps, int split, int d_live) {
  int rc = dbg_precision(who, precision, false);
  if (rc) return rc;
  if (!x || !gamma || !beta || !h_inout || x_rows < 1 || n_sel < 1 || h_rows < n_sel || P < 1 || width < 1 || (row_map && n_map < 1) ||
      split < 0 || split > 1)
    return fail(PG_ERR_INVALID, std::string(who) + ": bad argument");
  if ((rc = dbg_row_width(who, d, d_live))) return rc;
  if (split && (precision != PG_PREC_BF16 || d % 32))
    return fail(PG_ERR_INVALID, std::string(who) + ": split rows are bf16 pairs in groups of 32 columns");
  if (!idx) {      // identity: selected row r = token row r
    if (n_sel > x_rows) return fail(PG_ERR_INVALID, std::string(who) + ": more selected rows than source rows");
  } else {
    for (int64_t r = 0; r < n_sel; ++r)
      if (dbg_gather_src(who, r, idx[r], true, row_map, n_map, P, width, x_rows) == -2) return PG_ERR_INVALID;
  }
  Dbg s;
  if ((rc = s.open(device))) return rc;
  const size_t h_n = (size_t)h_rows * d * (split ? 3 : 1);
  const float* dx = s.up(x, (size_t)x_rows * d);
  const int32_t* di = s.up(idx, (size_t)n_sel);
  const int32_t* dm = s.up(row_map, (size_t)n_map);
  const float* dg = s.up(gamma, (size_t)d);
  const float* db = s.up(beta, (size_t)d);
  bf16_t* dh = s.up(h_inout, h_n);
  if ((rc = s.check(kCopyFailed))) return rc;
  if ((rc = OPS(launch_gather_ln_bf16, nullptr, dx, di, dm, P, width, dg, db, dh, n_sel, d, eps, split != 0, d_live))) return rc;
  return s.down(h_inout, dh, h_n);
}

int pg_dbg_gather_ln(int device, int precision, const float* x, int64_t x_rows, const int32_t* idx, const int32_t* row_map, int64_t n_map,
                     int P, int width, const float* gamma, const float* beta, uint16_t* h_inout, int64_t h_rows, int64_t n_sel, int d,
                     float eps, int split) {
  return dbg_gather_ln_rows("pg_dbg_gather_ln", device, precision, x, x_rows, idx, row_map, n_map, P, width, gamma, beta, h_inout, h_rows, n_sel, d, eps, split, d);
}

int pg_embedded_gather_ln(int device, int precision, const float* x, int64_t x_rows, const int32_t* idx, const int32_t* row_map, int64_t n_map,
                          int P, int width, const float* gamma, const float* beta, uint16_t* h_inout, int64_t h_rows, int64_t n_sel, int d,
                          float eps, int split, int d_live) {
  return dbg_gather_ln_rows("pg_embedded_gather_ln", device, precision, x, x_rows, idx, row_map, n_map, P, width, gamma, beta, h_inout, h_rows, n_sel, d, eps, split, d_live);
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
  Dbg s;
  int rc = s.open(device);
  if (rc) return rc;
  const char* ds = s.up((const char*)src, (size_t)src_rows * row_bytes);
  char* dd = s.up((const char*)dst_inout, (size_t)dst_rows * row_bytes);
  const int32_t* di = s.up(idx, (size_t)(n_iters > 0 ? n_iters : 1) * n_sel);
  const int32_t* dm = s.up(row_map, (size_t)n_map);
  const int32_t it32 = iter;
  const int32_t* dit = n_iters > 0 ? s.up(&it32, 1) : nullptr;
  if ((rc = s.check(kCopyFailed))) return rc;
  if ((rc = launch_gather_rows(nullptr, ds, dd, di, dm, P, width, n_sel, row_bytes, dit))) return rc;
  return s.down((char*)dst_inout, dd, (size_t)dst_rows * row_bytes);
}

int pg_dbg_split_rows(int device, const float* x, uint16_t* h_inout, int64_t h_rows, int rows, int K, float scale, int form, float* gelu_out) {
  if (!x || !h_inout || rows < 1 || h_rows < rows || K < 1) return fail(PG_ERR_INVALID, "pg_dbg_split_rows: bad argument");
  if (K % kSplitCols) return fail(PG_ERR_INVALID, "pg_dbg_split_rows: K must be a multiple of 32");
  if (form < 0 || form > 3) return fail(PG_ERR_INVALID, "pg_dbg_split_rows: form is weight (1) + through GELU (2)");
  if (form == 3) return fail(PG_ERR_INVALID, "pg_dbg_split_rows: GELU on a weight operand");
  if (form == 2 && scale != 1.0f) return fail(PG_ERR_INVALID, "pg_dbg_split_rows: the GELU form takes scale 1");
  if (form == 2 && !gelu_out) return fail(PG_ERR_INVALID, "pg_dbg_split_rows: the GELU form returns gelu_out");
  Dbg s;
  int rc = s.open(device);
  if (rc) return rc;
  const size_t h_n = (size_t)h_rows * 3 * K;
  float* dx = s.up(x, (size_t)rows * K);
  bf16_t* dh = s.up(h_inout, h_n);      // the caller's pattern
  if ((rc = s.check(kCopyFailed))) return rc;
  if ((rc = launch_split3_bf16(nullptr, dx, dh, rows, K, scale, form == 2, form == 1))) return rc;
  if ((rc = s.down(h_inout, dh, h_n))) return rc;
  if (form != 2) return PG_OK;
  if ((rc = launch_gelu_f32(nullptr, dx, (int64_t)rows * K))) return rc;
  return s.down(gelu_out, dx, (size_t)rows * K);
}

static int dbg_lm_tail_rows(const char* who, int device, const float* g, const float* gamma, const float* beta, const float* embed, const float* out_bias,
                        float* logits, int64_t n, int d, int V, float eps, int* small_kernel, int d_live) {
  if (!g || !embed || !out_bias || !logits || n < 1 || !gamma != !beta) return fail(PG_ERR_INVALID, std::string(who) + ": bad argument");
  if (V < 1 || V > 64) return fail(PG_ERR_INVALID, std::string(who) + ": vocab must be in 1..64");
  int rc = dbg_row_width(who, d, d_live);
  if (rc) return rc;
  Dbg s;
  if ((rc = s.open(device))) return rc;
  const float* dg = s.up(g, (size_t)n * d);
  const float* dga = s.up(gamma, (size_t)d);
  const float* dbe = s.up(beta, (size_t)d);
  const float* de = s.up(embed, (size_t)V * d);
  const float* dob = s.up(out_bias, (size_t)V);
  float* dl = s.up(logits, (size_t)n * V);      // the caller's pattern
  if ((rc = s.check(kCopyFailed))) return rc;
  if (small_kernel) *small_kernel = lm_tail_small(n, d) ? 1 : 0;
  if ((rc = launch_lm_tail(nullptr, dg, dga, dbe, de, dob, dl, n, d, V, eps, d_live))) return rc;
  return s.down(logits, dl, (size_t)n * V);
}

int pg_dbg_lm_tail(int device, const float* g, const float* gamma, const float* beta, const float* embed, const float* out_bias,
                   float* logits, int64_t n, int d, int V, float eps, int* small_kernel) {
  return dbg_lm_tail_rows("pg_dbg_lm_tail", device, g, gamma, beta, embed, out_bias, logits, n, d, V, eps, small_kernel, d);
}

int pg_embedded_lm_tail(int device, const float* g, const float* gamma, const float* beta, const float* embed, const float* out_bias,
                        float* logits, int64_t n, int d, int V, float eps, int* small_kernel, int d_live) {
  return dbg_lm_tail_rows("pg_embedded_lm_tail", device, g, gamma, beta, embed, out_bias, logits, n, d, V, eps, small_kernel, d_live);
}

/* ---- the two index ends of an iteration (csrc/sample.hip), in every form the engine launches ----
 * n_steps times: launch_mask_scatter (mask_idx >= 0), then launch_sample_writeback, on the null stream, downloading after each.
 * device_iter 0: the step's index table and iteration number are host arguments; 1: the launches Engine::gibbs captures, without the
 * graph -- launch_graph_state once, the table base, iteration 0 and the state block in every step, launch_iter_counter after it.
 * Everything is checked on the host before a device is looked for; with permit_out_of_range a position >= width goes through to the
 * kernels' own guards, which read and write nothing for it. */
int pg_dbg_sample(int device, int32_t* tokens_inout, int64_t n_rows, int width, const float* logits, int V, int compact, const int32_t* idx,
                  int n_tables, const int32_t* row_map, int64_t n_sel, int P, const pg_sample_params* params, int first_iter, int n_steps,
                  int device_iter, int mask_idx, int permit_out_of_range, int32_t* sampled_out, int32_t* masked_tokens_out,
                  unsigned* nonfinite_out) {
  return pg_guided_dbg_sample(device, tokens_inout, n_rows, width, logits, V, compact, idx, n_tables, row_map, n_sel, P, params, first_iter,
                              n_steps, device_iter, mask_idx, permit_out_of_range, sampled_out, masked_tokens_out, nonfinite_out, nullptr);
}

int pg_guided_sizeof_draw_guide(void) { return (int)sizeof(pg_draw_guide); }

/* pg_dbg_sample with a draw guide (pg_draw v2): the guide's tables are checked as pg_engine_set_draw_guide checks them and against this
 * call's shape as the Gibbs entries do, then uploaded; every draw launch is given them, and with device_iter 1 the state block holds them. */
int pg_guided_dbg_sample(int device, int32_t* tokens_inout, int64_t n_rows, int width, const float* logits, int V, int compact,
                         const int32_t* idx, int n_tables, const int32_t* row_map, int64_t n_sel, int P, const pg_sample_params* params,
                         int first_iter, int n_steps, int device_iter, int mask_idx, int permit_out_of_range, int32_t* sampled_out,
                         int32_t* masked_tokens_out, unsigned* nonfinite_out, const pg_draw_guide* guide) {
  if (!tokens_inout || !logits || !idx || !params || !sampled_out) return fail(PG_ERR_INVALID, "pg_dbg_sample: bad argument");
  if (n_rows < 1 || width < 1 || V < 1 || n_tables < 1 || n_sel < 1 || P < 1 || first_iter < 0 || n_steps < 1)
    return fail(PG_ERR_INVALID, "pg_dbg_sample: bad argument");
  if (compact < 0 || compact > 1 || device_iter < 0 || device_iter > 1 || permit_out_of_range < 0 || permit_out_of_range > 1)
    return fail(PG_ERR_INVALID, "pg_dbg_sample: compact, device_iter and permit_out_of_range are 0 or 1");
  if (masked_tokens_out && mask_idx < 0) return fail(PG_ERR_INVALID, "pg_dbg_sample: masked_tokens_out without a mask step (mask_idx < 0)");
  if ((int64_t)first_iter + n_steps > n_tables) return fail(PG_ERR_INVALID, "pg_dbg_sample: n_tables must be at least first_iter + n_steps");
  if (params->n_valid < 1 || params->n_valid > 32) return fail(PG_ERR_INVALID, "pg_dbg_sample: n_valid must be in 1..32");
  for (int j = 0; j < params->n_valid; ++j)
    if (params->valid_idx[j] < 0 || params->valid_idx[j] >= V) return fail(PG_ERR_INVALID, "pg_dbg_sample: valid_idx out of range");
  const double n_d = (double)n_sel * P;
  if (n_d * n_tables * (compact ? V : 1) > 2147483647.0 || (double)n_rows * width * (compact ? 1 : V) > 2147483647.0)
    return fail(PG_ERR_INVALID, "pg_dbg_sample: more than 2^31 - 1 values in one array");
  if (!row_map && n_sel > n_rows) return fail(PG_ERR_INVALID, "pg_dbg_sample: more selected rows than token rows");
  if (row_map)
    for (int64_t s = 0; s < n_sel; ++s)
      if (row_map[s] < 0 || row_map[s] >= n_rows)
        return fail(PG_ERR_INVALID, "pg_dbg_sample: row_map entry " + std::to_string(row_map[s]) + " is outside the " + std::to_string(n_rows) + " token rows");
  const size_t n = (size_t)n_sel * P, n_tok = (size_t)n_rows * width;
  if (!permit_out_of_range)
    for (size_t i = 0; i < n * n_tables; ++i)
      if (idx[i] >= 0 && (idx[i] & 0x3fffffff) >= width)
        return fail(PG_ERR_INVALID, "pg_dbg_sample: target position " + std::to_string(idx[i] & 0x3fffffff) + " is out of range for a token row of width " +
                                        std::to_string(width));
  int rc;
  DrawGuideDev g;
  if (guide) {
    if ((rc = check_draw_guide_tables(guide, "pg_guided_dbg_sample"))) return rc;
    g.top_p = guide->top_p;
    if (guide->bias) { g.bias = guide->bias; g.bias_rows = guide->bias_rows; g.width = guide->width; g.n_valid = guide->n_valid; }
    if (guide->temperatures) { g.temps = guide->temperatures; g.n_temps = guide->n_temperatures; }
    if ((rc = check_draw_guide(&g, "pg_guided_dbg_sample", width, params->n_valid, n_rows, (int64_t)first_iter + n_steps))) return rc;
  }
  Dbg d;
  if ((rc = d.open(device))) return rc;
  if (g.bias) g.bias = d.up(guide->bias, (size_t)g.bias_rows * g.width * g.n_valid);
  if (g.temps) g.temps = d.up(guide->temperatures, (size_t)g.n_temps);
  int32_t* dtok = d.up(tokens_inout, n_tok);
  const float* dlog = d.up(logits, compact ? n * n_tables * V : n_tok * V);
  const int32_t* didx = d.up(idx, n * n_tables);
  const int32_t* dmap = d.up(row_map, (size_t)n_sel);
  int32_t* dout = d.alloc<int32_t>(n);
  int32_t* dstate = device_iter ? (int32_t*)d.alloc<char>(graph_state_bytes()) : nullptr;
  unsigned* dnf = nonfinite_out ? d.alloc<unsigned>(1) : nullptr;
  if ((rc = d.check(kCopyFailed))) return rc;
  if (device_iter && (rc = launch_graph_state(nullptr, dstate, first_iter, params, &g))) return rc;
  for (int s = 0; s < n_steps; ++s) {
    const int it = first_iter + s;
    const int32_t* idx_s = device_iter ? didx : didx + (size_t)it * n;      // the kernels add *d_iter tables themselves
    if (mask_idx >= 0) {
      if ((rc = launch_mask_scatter(nullptr, dtok, width, idx_s, dmap, n_sel, P, mask_idx, dstate))) return rc;
      if (masked_tokens_out && (rc = d.down(masked_tokens_out + (size_t)s * n_tok, dtok, n_tok))) return rc;
    }
    d.put(dout, sampled_out + (size_t)s * n, n);      // the caller's pattern: an entry the kernel does not write keeps it
    if ((rc = d.check(kCopyFailed))) return rc;
    const float* lg = compact ? dlog + (size_t)it * n * V : dlog;
    if ((rc = launch_sample_writeback(nullptr, dtok, width, lg, V, compact, idx_s, dmap, n_sel, P, params, device_iter ? 0 : it, dout, dstate, dnf, &g)))
      return rc;
    if ((rc = d.down(sampled_out + (size_t)s * n, dout, n))) return rc;
    if (device_iter && (rc = launch_iter_counter(nullptr, dstate, false, 0))) return rc;
  }
  if ((rc = d.down(tokens_inout, dtok, n_tok))) return rc;
  return nonfinite_out ? d.down(nonfinite_out, dnf, 1) : PG_OK;
}

/* The two representation launchers (repr.hip) alone, on host fp32 buffers: rows_out[M][d_live] = launch_repr_rows of x[M][d] (gamma /
 * beta both given or both NULL; tokens[M] optional), then, with pools[n_pools][B][2] (M = B * T), pooled_out[n_pools][B][d_live] =
 * launch_repr_pool of those rows.  Everything is refused on the host before a device is looked for. */
int pg_repr_dbg_rows(int device, const float* x, int64_t M, int d, int d_live, const float* gamma, const float* beta, float eps,
                     const int32_t* tokens, int pad_idx, float* rows_out, int B, int T, const int32_t* pools, int n_pools, float* pooled_out) {
  if (!x || !rows_out || M < 1 || M > 0x7fffffff) return fail(PG_ERR_INVALID, "pg_repr_dbg_rows: bad argument");
  if (!row_d_ok(d) || !row_live_ok(d, d_live)) return fail(PG_ERR_INVALID, "pg_repr_dbg_rows: d or d_live is no width of the row kernels");
  if ((gamma == nullptr) != (beta == nullptr)) return fail(PG_ERR_INVALID, "pg_repr_dbg_rows: gamma and beta come together");
  if ((pools != nullptr) != (pooled_out != nullptr) || (pools && n_pools < 1)) return fail(PG_ERR_INVALID, "pg_repr_dbg_rows: pools and pooled_out come together");
  int rc;
  if (pools) {
    if (B < 1 || T < 1 || (int64_t)B * T != M) return fail(PG_ERR_INVALID, "pg_repr_dbg_rows: pooling needs M = B * T");
    if ((rc = repr_pools_check("pg_repr_dbg_rows", pools, n_pools, B, T))) return rc;
  }
  Dbg s;
  if ((rc = s.open(device))) return rc;
  const float* dx = s.up(x, (size_t)M * d);
  const float* dg = s.up(gamma, (size_t)d_live);
  const float* dbt = s.up(beta, (size_t)d_live);
  const int32_t* dtok = s.up(tokens, (size_t)M);
  const int32_t* dpools = s.up(pools, pools ? (size_t)n_pools * B * 2 : 0);
  float* drows = s.alloc<float>((size_t)M * d_live);
  float* dmeans = pools ? s.alloc<float>((size_t)n_pools * B * d_live) : nullptr;
  if ((rc = s.check())) return rc;
  if ((rc = launch_repr_rows(nullptr, dx, dg, dbt, dtok, pad_idx, drows, M, d, d_live, eps))) return rc;
  if (pools && (rc = launch_repr_pool(nullptr, drows, dpools, dmeans, n_pools, B, T, d_live))) return rc;
  if ((rc = s.down(rows_out, drows, (size_t)M * d_live))) return rc;
  return pools ? s.down(pooled_out, dmeans, (size_t)n_pools * B * d_live) : PG_OK;
}

/* The two contact launchers (contact.hip) alone, on host buffers.  pg_contact_dbg_probs: probs_out[n_seq][H][T][T] = launch_attn_probs
 * of qkv[n_seq * T][3 H head_dim] fp32 -- rounded to the 16-bit type of `precision` first, kept fp32 for PG_PREC_FP32 (the strict
 * launcher) -- read as the engine's ESM trunks hand it over (ld = 3 d, k at d, contiguous chains).  plan (may be NULL): the launcher's
 * plan text; with probs_out NULL the plan alone, without a device.  Everything is refused on the host before a device is looked for. */
int pg_contact_dbg_probs(int device, int precision, const float* qkv, int n_seq, int T, int H, int head_dim, const int32_t* key_tok, int pad_idx,
                         float* probs_out, char* plan, int plan_bytes) {
  if (plan && plan_bytes > 0) plan[0] = 0;
  int rc = dbg_precision("pg_contact_dbg_probs", precision, true);
  if (rc) return rc;
  if (n_seq < 1 || T < 1 || H < 1 || (plan && plan_bytes < 1) || (!probs_out && !plan) || (probs_out && !qkv))
    return fail(PG_ERR_INVALID, "pg_contact_dbg_probs: bad argument");
  if (!head_width(head_dim)) return fail(PG_ERR_INVALID, "pg_contact_dbg_probs: head_dim must be " + head_widths_text(false));
  const bool strict = precision == PG_PREC_FP32;
  if (!probs_out) {
    std::string text;
    if (strict) attn_probs_f32_plan_text(n_seq, T, H, head_dim, key_tok != nullptr, &text);
    else OPS(attn_probs_plan_text, n_seq, T, H, head_dim, key_tok != nullptr, &text);
    snprintf(plan, (size_t)plan_bytes, "%s", text.c_str());
    return PG_OK;
  }
  if ((double)n_seq * T * 3 * H * head_dim > 2147483647.0 || (double)n_seq * H * T * T > 2147483647.0)
    return fail(PG_ERR_INVALID, "pg_contact_dbg_probs: more than 2^31 - 1 values");
  Dbg s;
  if ((rc = s.open(device))) return rc;
  const int d = H * head_dim;
  const int64_t M = (int64_t)n_seq * T;
  const size_t n_map = (size_t)n_seq * H * T * T;
  const float* dq = s.up(qkv, (size_t)M * 3 * d);
  const int32_t* dtok = s.up(key_tok, (size_t)M);
  bf16_t* bq = strict ? nullptr : s.alloc<bf16_t>((size_t)M * 3 * d);
  float* dP = s.alloc<float>(n_map);
  if ((rc = s.check())) return rc;
  clear_noted_kernels();
  const SeqLayout chain = {1, T, 0, 1};
  if (strict) rc = launch_attn_probs_f32(nullptr, dq, dP, n_seq, T, H, 3 * d, d, chain, dtok, pad_idx, head_dim);
  else if (!(rc = to16(precision, dq, bq, M * 3 * d))) rc = OPS(launch_attn_probs, nullptr, bq, dP, n_seq, T, H, 3 * d, d, chain, dtok, pad_idx, head_dim);
  if (rc) return rc;
  dbg_noted_text(plan, plan_bytes);
  return s.down(probs_out, dP, n_map);
}

/* pg_contact_dbg_accumulate: launch_contact_accumulate of P[B][H][T][T] with the H weights w into logits_inout[B][T-2][T-2] (read
 * unless `first`), contacts_out (optional) written when `last`. */
int pg_contact_dbg_accumulate(int device, const float* P, const int32_t* tokens, int eos_idx, int pad_idx, const float* w, float bias, int first,
                              int last, float* logits_inout, float* contacts_out, int B, int T, int H) {
  if (!P || !tokens || !w || !logits_inout || B < 1 || H < 1) return fail(PG_ERR_INVALID, "pg_contact_dbg_accumulate: bad argument");
  if (T < 3) return fail(PG_ERR_INVALID, "pg_contact_dbg_accumulate: T must be at least 3");
  if ((double)B * H * T * T > 2147483647.0) return fail(PG_ERR_INVALID, "pg_contact_dbg_accumulate: more than 2^31 - 1 values");
  Dbg s;
  int rc;
  if ((rc = s.open(device))) return rc;
  const size_t n_win = (size_t)B * (T - 2) * (T - 2);
  const float* dP = s.up(P, (size_t)B * H * T * T);
  const int32_t* dtok = s.up(tokens, (size_t)B * T);
  const float* dw = s.up(w, (size_t)H);
  float* dlog = s.up(logits_inout, n_win);
  float* dcon = contacts_out ? s.alloc<float>(n_win) : nullptr;
  float* dsum = s.alloc<float>(contact_sums_floats(B, H, T));
  if ((rc = s.check())) return rc;
  if ((rc = launch_contact_accumulate(nullptr, dP, dtok, eos_idx, pad_idx, dw, bias, first != 0, last != 0, dsum, dlog, dcon, B, T, H))) return rc;
  if ((rc = s.down(logits_inout, dlog, n_win))) return rc;
  return contacts_out && last ? s.down(contacts_out, dcon, n_win) : PG_OK;
}

/* pg_contact_dbg_accumulate_window: the window form (launch_contact_accumulate_window).  The window is W = T - 1 - tail positions (tail 0 or
 * 1) and the tokens of item b are tokens[b * tok_stride .. + T - 1] of tokens[(B - 1) * tok_stride + T]; logits_inout / contacts_out
 * [B][W][W].  tail 1 with tok_stride T is pg_contact_dbg_accumulate. */
int pg_contact_dbg_accumulate_window(int device, const float* P, const int32_t* tokens, int eos_idx, int pad_idx, const float* w, float bias,
                                     int first, int last, float* logits_inout, float* contacts_out, int B, int T, int H, int tail,
                                     int64_t tok_stride) {
  const char* who = "pg_contact_dbg_accumulate_window";
  if (!P || !tokens || !w || !logits_inout || B < 1 || H < 1) return fail(PG_ERR_INVALID, std::string(who) + ": bad argument");
  if (tail != 0 && tail != 1) return fail(PG_ERR_INVALID, std::string(who) + ": tail must be 0 or 1");
  if (T < 2 + tail) return fail(PG_ERR_INVALID, std::string(who) + ": T must be at least " + std::to_string(2 + tail));
  if (tok_stride < T) return fail(PG_ERR_INVALID, std::string(who) + ": tok_stride must be at least T");
  if ((double)B * H * T * T > 2147483647.0 || (double)B * tok_stride > 2147483647.0)
    return fail(PG_ERR_INVALID, std::string(who) + ": more than 2^31 - 1 values");
  Dbg s;
  int rc;
  if ((rc = s.open(device))) return rc;
  const int W = T - 1 - tail;
  const size_t n_win = (size_t)B * W * W;
  const float* dP = s.up(P, (size_t)B * H * T * T);
  const int32_t* dtok = s.up(tokens, (size_t)(B - 1) * tok_stride + T);
  const float* dw = s.up(w, (size_t)H);
  float* dlog = s.up(logits_inout, n_win);
  float* dcon = contacts_out ? s.alloc<float>(n_win) : nullptr;
  float* dsum = s.alloc<float>(contact_window_sums_floats(B, H, T, tail));
  if ((rc = s.check())) return rc;
  if ((rc = launch_contact_accumulate_window(nullptr, dP, dtok, eos_idx, pad_idx, dw, bias, first != 0, last != 0, dsum, dlog, dcon, B, T, H, tail,
                                             (size_t)tok_stride))) return rc;
  if ((rc = s.down(logits_inout, dlog, n_win))) return rc;
  return contacts_out && last ? s.down(contacts_out, dcon, n_win) : PG_OK;
}

/* The two launchers of msa_contact.hip alone, on host buffers: probs_out[B][H][C][C] = launch_row_softmax_probs of launch_msa_row_scores
 * (precision bf16 / fp16: qkv rounded to that type first) or launch_msa_row_scores_f32 (PG_PREC_FP32: the fp32 values) of
 * qkv[B * R * C][3 H 64], read as Engine::msa_trunk hands a block's row qkv over (ld = 3 d, k at d), scores scaled by `scale`.  tok
 * (optional) [B][R][C] with pad_idx: the ragged semantics.  plan (may be NULL): the scores launcher's plan text; with probs_out NULL the
 * plan alone, without a device.  Everything is refused on the host before a device is looked for. */
int pg_msa_contact_dbg_probs(int device, int precision, const float* qkv, int B, int R, int C, int H, float scale, const int32_t* tok,
                             int pad_idx, float* probs_out, char* plan, int plan_bytes) {
  const char* who = "pg_msa_contact_dbg_probs";
  if (plan && plan_bytes > 0) plan[0] = 0;
  int rc = dbg_precision(who, precision, true);
  if (rc) return rc;
  if (B < 1 || R < 1 || C < 1 || H < 1 || (plan && plan_bytes < 1) || (!probs_out && !plan) || (probs_out && !qkv))
    return fail(PG_ERR_INVALID, std::string(who) + ": bad argument");
  const bool strict = precision == PG_PREC_FP32;
  if (!probs_out) {
    std::string text;
    if (strict) msa_row_scores_f32_plan_text(B, R, C, H, tok != nullptr, &text);
    else OPS(msa_row_scores_plan_text, B, R, C, H, tok != nullptr, &text);
    snprintf(plan, (size_t)plan_bytes, "%s", text.c_str());
    return PG_OK;
  }
  const int ldS = msa_row_scores_ld(C);
  if ((double)B * R * C * 3 * H * 64 > 2147483647.0 || (double)B * H * C * ldS > 2147483647.0)
    return fail(PG_ERR_INVALID, std::string(who) + ": more than 2^31 - 1 values");
  Dbg s;
  if ((rc = s.open(device))) return rc;
  const int d = H * 64;
  const int64_t M = (int64_t)B * R * C;
  const size_t n_map = (size_t)B * H * C * C;
  const float* dq = s.up(qkv, (size_t)M * 3 * d);
  const int32_t* dtok = s.up(tok, (size_t)M);
  bf16_t* bq = strict ? nullptr : s.alloc<bf16_t>((size_t)M * 3 * d);
  float* dS = s.alloc<float>((size_t)B * H * C * ldS);
  float* dP = s.alloc<float>(n_map);
  if ((rc = s.check())) return rc;
  clear_noted_kernels();
  if (strict) rc = launch_msa_row_scores_f32(nullptr, dq, dS, B, R, C, H, 3 * d, d, scale, dtok, pad_idx);
  else if (!(rc = to16(precision, dq, bq, M * 3 * d))) rc = OPS(launch_msa_row_scores, nullptr, bq, dS, B, R, C, H, 3 * d, d, scale, dtok, pad_idx);
  if (rc || (rc = launch_row_softmax_probs(nullptr, dS, dP, (int64_t)B * H * C, C, ldS))) return rc;
  dbg_noted_text(plan, plan_bytes);
  return s.down(probs_out, dP, n_map);
}

/* ---- embedded models: the host side of pg_engine_create_embedded, no device ---- */
int pg_embedded_image(const char* name, const float* src, int64_t numel, int n_heads, int head_width, int head_slot, int d_ffn, int vocab,
                      float* image, int64_t image_numel) {
  if (!name || !src || !image || n_heads < 1 || d_ffn < 1 || vocab < 1 || head_width < 2 || head_width % 2 || head_slot <= head_width || head_slot % 2)
    return fail(PG_ERR_INVALID, "pg_embedded_image: bad argument");
  const EmbedShape es = {n_heads, head_width, head_slot, d_ffn, vocab};
  int64_t r = 0, c = 0;
  if (!embedded_image(name, es, nullptr, &r, &c, nullptr)) return fail(PG_ERR_INVALID, std::string("pg_embedded_image: '") + name + "' is not a tensor of an ESM-2 model");
  if (numel != r * c) return fail(PG_ERR_INVALID, std::string("tensor '") + name + "' has " + std::to_string(numel) + " elements, expected " + std::to_string(r * c));
  std::vector<float> img;
  embedded_image(name, es, src, &r, &c, &img);
  if ((int64_t)img.size() != image_numel)
    return fail(PG_ERR_INVALID, std::string("pg_embedded_image: the image of '") + name + "' has " + std::to_string(img.size()) + " elements");
  memcpy(image, img.data(), img.size() * 4);
  return PG_OK;
}

int pg_embedded_rope_table(int rows, int head_width, int head_slot, float* table) {
  if (!table || rows < 1 || head_width < 2 || head_width % 2 || head_slot < head_width || head_slot % 2)
    return fail(PG_ERR_INVALID, "pg_embedded_rope_table: bad argument");
  const std::vector<float> tab = rope_table(rows, head_slot, head_width == head_slot ? 0 : head_width);
  memcpy(table, tab.data(), tab.size() * 4);
  return PG_OK;
}

}  // extern "C"
