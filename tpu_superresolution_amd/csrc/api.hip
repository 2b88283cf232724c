// extern "C" surface of libsrk.so (include/srk.h): argument validation + error reporting around the
// kernel launchers.  No torch types, no allocation, no synchronisation.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "adamw.h"
#include "kernels.h"
#include "tables.h"
#include "wgrad.h"

static thread_local char g_err[512] = "";

SrkOptTls& srk_opt_tls() {
  static thread_local SrkOptTls t = {};
  return t;
}

static SrkOpt** opt_table() {
  static SrkOpt* table[SRK_NUM_OPTS] = {};
  return table;
}

void srk_opt_register(SrkOpt* o) {
  if (o->id >= 0 && o->id < SRK_NUM_OPTS) opt_table()[o->id] = o;
}

void srk_opt_scope_begin(SrkOptTls* saved) {
  SrkOptTls& t = srk_opt_tls();
  *saved = t;
  for (int i = 0; i < SRK_NUM_OPTS; ++i)
    if (!((t.on >> i) & 1u) && opt_table()[i]) t.v[i] = opt_table()[i]->value;
  t.on = (1u << SRK_NUM_OPTS) - 1u;
}

void srk_opt_scope_end(const SrkOptTls& saved) { srk_opt_tls() = saved; }

int srk_current_device() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= SRK_MAX_DEVICES) return 0;
  return dev;
}

int srk_device_cus() {
  static SrkPerDevice<int> cus;
  int& c = cus.here();
  if (c == 0) {
    hipDeviceProp_t prop;
    int dev = 0;
    c = -1;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) c = prop.multiProcessorCount;
  }
  return c;
}

void srk_set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int srk_reserve_lds_fn(const void* fn, int bytes, SrkLdsState& st, bool refuse_spills, const char* err_fmt, ...) {
  signed char& s = st.here();
  if (s) return s > 0 ? SRK_OK : SRK_NOT_COVERED;
  hipFuncAttributes attr;
  const bool queried = !refuse_spills || hipFuncGetAttributes(&attr, fn) == hipSuccess;
  if (queried && refuse_spills && attr.localSizeBytes > 0) {
    s = -1;
    return SRK_NOT_COVERED;
  }
  if (queried && hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) == hipSuccess) {
    s = 1;
    return SRK_OK;
  }
  if (!err_fmt) {
    s = -1;
    return SRK_NOT_COVERED;
  }
  if (queried) {
    va_list ap;
    va_start(ap, err_fmt);
    vsnprintf(g_err, sizeof(g_err), err_fmt, ap);
    va_end(ap);
  } else {   // "<site>: cannot query the kernel", the site's name being what err_fmt has in front of its colon
    const char* colon = strchr(err_fmt, ':');
    srk_set_error("%.*s: cannot query the kernel", colon ? (int)(colon - err_fmt) : (int)strlen(err_fmt), err_fmt);
  }
  return SRK_E_LAUNCH;
}

int srk_check_launch(const char* what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    srk_set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return SRK_E_LAUNCH;
  }
  return SRK_OK;
}

// ---- timing probe ----------------------------------------------------------------------------------
#include <vector>
namespace {
struct Probe {
  int family = 0;
  bool active = false;
  size_t count = 0;
  size_t seen = 0;          // launches of the family since probe_begin
  int stride = 1;           // bracket every stride-th launch (option "probe_stride"): the two event records per launch
                            // cost ~2.5 us of stream time each, which matters at several hundred launches per step
  bool sampling = false;    // the launch between the current pre / post is a sampled one
  double flops = 0.0, bytes = 0.0;
  std::vector<hipEvent_t> ev0, ev1;
} g_probe;
}  // namespace

void srk_probe_pre(int family, hipStream_t stream, double flops, double bytes) {
  g_probe.sampling = false;
  if (!g_probe.active || family != g_probe.family || g_probe.count >= g_probe.ev0.size()) return;
  if ((g_probe.seen++ % (size_t)g_probe.stride) != 0) return;
  g_probe.sampling = true;
  hipEventRecord(g_probe.ev0[g_probe.count], stream);
  g_probe.flops += flops;
  g_probe.bytes += bytes;
}

void srk_probe_post(int family, hipStream_t stream) {
  if (!g_probe.sampling || !g_probe.active || family != g_probe.family) return;
  g_probe.sampling = false;
  hipEventRecord(g_probe.ev1[g_probe.count], stream);
  ++g_probe.count;
}

#define REQ_PTR(p) SRK_REQUIRE((p) != nullptr, SRK_E_NULL, "%s: null pointer '%s'", __func__, #p)
#define REQ_ALIGN(p) SRK_REQUIRE(srk_aligned(p, 16), SRK_E_ALIGN, "%s: '%s' is not 16-byte aligned", __func__, #p)

static int make_geom(const srk_win_geom* g, WinGeom* out, const char* fn) {
  SRK_REQUIRE(g->H > 0 && g->W > 0 && g->H % 8 == 0 && g->W % 8 == 0, SRK_E_SHAPE, "%s: H,W must be multiples of 8 (got %d,%d)",
              fn, g->H, g->W);
  SRK_REQUIRE(g->shift == 0 || g->shift == 4, SRK_E_SHAPE, "%s: shift must be 0 or 4 (got %d)", fn, g->shift);
  out->H = g->H;
  out->W = g->W;
  out->nWw = g->W / 8;
  out->nW = (g->H / 8) * (g->W / 8);
  out->shift = g->shift;
  return SRK_OK;
}

extern "C" {

const char* srk_version(void) { return "srk 0.1 (gfx950)"; }
const char* srk_last_error(void) { return g_err; }

int srk_window_partition(const void* x, void* out, int B, int H, int W, int C, int ws, int elem_bytes, srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(out);
  SRK_REQUIRE(B > 0 && C > 0 && ws > 0 && H > 0 && W > 0 && H % ws == 0 && W % ws == 0, SRK_E_SHAPE,
              "window_partition: H=%d,W=%d must be positive multiples of ws=%d", H, W, ws);
  return srk_launch_window_partition(x, out, B, H, W, C, ws, elem_bytes, 0, (hipStream_t)stream);
}

int srk_window_reverse(const void* windows, void* out, int B, int H, int W, int C, int ws, int elem_bytes, srk_stream_t stream) {
  REQ_PTR(windows); REQ_PTR(out);
  SRK_REQUIRE(B > 0 && C > 0 && ws > 0 && H > 0 && W > 0 && H % ws == 0 && W % ws == 0, SRK_E_SHAPE,
              "window_reverse: H=%d,W=%d must be positive multiples of ws=%d", H, W, ws);
  return srk_launch_window_partition(windows, out, B, H, W, C, ws, elem_bytes, 1, (hipStream_t)stream);
}

int srk_roll2d(const void* x, void* out, int B, int H, int W, int C, int sh, int sw, int elem_bytes, srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(out);
  SRK_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0, SRK_E_SHAPE, "roll2d: bad shape");
  return srk_launch_roll2d(x, out, B, H, W, C, sh, sw, elem_bytes, (hipStream_t)stream);
}

int srk_pixel_shuffle(const void* x, void* out, int B, int C, int H, int W, int r, int elem_bytes, srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(out);
  SRK_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && r > 0, SRK_E_SHAPE, "pixel_shuffle: bad shape");
  return srk_launch_pixel_shuffle(x, out, B, C, H, W, r, elem_bytes, (hipStream_t)stream);
}

int srk_shift_mask(float* mask, int H, int W, int ws, int shift, srk_stream_t stream) {
  REQ_PTR(mask);
  SRK_REQUIRE(ws > 0 && H % ws == 0 && W % ws == 0 && shift >= 0 && shift < ws, SRK_E_SHAPE,
              "shift_mask: shift_size must in 0-window_size (H=%d W=%d ws=%d shift=%d)", H, W, ws, shift);
  return srk_launch_shift_mask(mask, H, W, ws, shift, (hipStream_t)stream);
}

int srk_relative_position_index(int64_t* out, int ws, srk_stream_t stream) {
  REQ_PTR(out);
  SRK_REQUIRE(ws > 0 && ws <= 64, SRK_E_SHAPE, "relative_position_index: bad ws %d", ws);
  return srk_launch_rel_pos_index((long long*)out, ws, (hipStream_t)stream);
}

int srk_layernorm_fwd(const float* x, const float* gamma, const float* beta, uint16_t* y_bf16, float* y_f32, float* mean,
                      float* rstd, int rows, int C, int CP, const srk_win_geom* geom, srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(gamma); REQ_PTR(beta); REQ_ALIGN(x);
  SRK_REQUIRE(rows > 0, SRK_E_SHAPE, "layernorm: rows=%d", rows);
  SRK_REQUIRE((mean == nullptr) == (rstd == nullptr), SRK_E_NULL, "layernorm: mean/rstd must both be given or both null");
  WinGeom g;
  if (geom) {
    int rc = make_geom(geom, &g, "layernorm");
    if (rc) return rc;
    SRK_REQUIRE(rows % (g.H * g.W) == 0, SRK_E_SHAPE, "layernorm: rows %d not a multiple of H*W", rows);
  }
  return srk_launch_ln_fwd(x, gamma, beta, y_bf16, y_f32, mean, rstd, rows, C, CP, geom ? &g : nullptr, (hipStream_t)stream);
}

int srk_window_attention_fwd(const uint16_t* qkv, const float* bias_dense, uint16_t* out, int64_t B_, int nH,
                             const srk_win_geom* geom, srk_stream_t stream) {
  REQ_PTR(qkv); REQ_PTR(bias_dense); REQ_PTR(out); REQ_PTR(geom); REQ_ALIGN(qkv); REQ_ALIGN(out); REQ_ALIGN(bias_dense);
  WinGeom g;
  int rc = make_geom(geom, &g, "window_attention_fwd");
  if (rc) return rc;
  SRK_REQUIRE(B_ > 0 && B_ % g.nW == 0 && nH > 0 && nH <= 64, SRK_E_SHAPE, "window_attention_fwd: B_=%lld nW=%d nH=%d",
              (long long)B_, g.nW, nH);
  return srk_launch_attn_fwd(qkv, bias_dense, out, B_, nH, g, (hipStream_t)stream);
}

size_t srk_window_attention_bwd_scratch(int64_t B_, int nH) {
  return (size_t)srk_attn_bwd_slabs(B_, nH, nullptr) * nH * 4096 * sizeof(float);
}

int srk_window_attention_bwd(const uint16_t* qkv, const float* bias_dense, const uint16_t* d_out, uint16_t* d_qkv,
                             float* d_table, void* slab, int64_t B_, int nH, float scale, const srk_win_geom* geom,
                             srk_stream_t stream) {
  REQ_PTR(qkv); REQ_PTR(bias_dense); REQ_PTR(d_out); REQ_PTR(d_qkv); REQ_PTR(d_table); REQ_PTR(slab); REQ_PTR(geom);
  REQ_ALIGN(qkv); REQ_ALIGN(d_out); REQ_ALIGN(d_qkv); REQ_ALIGN(slab);
  WinGeom g;
  int rc = make_geom(geom, &g, "window_attention_bwd");
  if (rc) return rc;
  SRK_REQUIRE(B_ > 0 && B_ % g.nW == 0 && nH > 0 && nH <= 64, SRK_E_SHAPE, "window_attention_bwd: B_=%lld nW=%d nH=%d",
              (long long)B_, g.nW, nH);
  return srk_launch_attn_bwd(qkv, bias_dense, d_out, d_qkv, (float*)slab, d_table, B_, nH, g, scale, (hipStream_t)stream);
}

size_t srk_window_attention_bwd_fused_scratch(int64_t B_, int nH) {
  return (size_t)srk_qkv_attn_bwd_slabs(B_, nH, nH * 32, 192) * nH * 4096 * sizeof(float);
}

int srk_window_attention_bwd_fused(const uint16_t* xn, int lda, const uint16_t* w_qkv, const float* b_qkv, float scale,
                                   const uint16_t* d_x1, int ldg, const uint16_t* w_proj_t, const float* bias_dense, uint16_t* d_qkv,
                                   float* d_table, void* slab, int64_t B_, int nH, const srk_win_geom* geom, srk_stream_t stream) {
  REQ_PTR(xn); REQ_PTR(w_qkv); REQ_PTR(d_x1); REQ_PTR(w_proj_t); REQ_PTR(bias_dense); REQ_PTR(d_qkv); REQ_PTR(d_table); REQ_PTR(slab);
  REQ_PTR(geom); REQ_ALIGN(xn); REQ_ALIGN(w_qkv); REQ_ALIGN(d_x1); REQ_ALIGN(w_proj_t); REQ_ALIGN(d_qkv); REQ_ALIGN(slab);
  WinGeom g;
  int rc = make_geom(geom, &g, "window_attention_bwd_fused");
  if (rc) return rc;
  SRK_REQUIRE(B_ > 0 && B_ % g.nW == 0, SRK_E_SHAPE, "window_attention_bwd_fused: B_=%lld nW=%d", (long long)B_, g.nW);
  const int nslab = srk_qkv_attn_bwd_slabs(B_, nH, nH * 32, 192);
  SRK_REQUIRE(nslab > 0, SRK_E_UNSUPPORTED,
              "window_attention_bwd_fused: covers 6 heads x 32, K = 192 and at least one window per CU (got nH=%d B_=%lld)", nH,
              (long long)B_);
  rc = srk_launch_qkv_attn_bwd(xn, lda, w_qkv, b_qkv, scale, d_x1, ldg, w_proj_t, bias_dense, d_qkv, (float*)slab, B_, nH, nH * 32, 192, g,
                               (hipStream_t)stream);
  SRK_REQUIRE(rc != SRK_NOT_COVERED, SRK_E_UNSUPPORTED, "window_attention_bwd_fused: the kernel cannot run on this build / shape");
  if (rc) return rc;
  return srk_launch_rpb_reduce((const float*)slab, d_table, nslab, nH, (hipStream_t)stream);
}

int srk_rel_pos_bias_expand(const float* table, float* bias_dense, int nH, srk_stream_t stream) {
  REQ_PTR(table); REQ_PTR(bias_dense);
  return srk_launch_rpb_expand(table, bias_dense, nH, (hipStream_t)stream);
}

int srk_linear_bf16(const uint16_t* a, const uint16_t* w, const float* bias, uint16_t* y, int M, int N, int K, srk_stream_t stream) {
  REQ_PTR(a); REQ_PTR(w); REQ_PTR(y); REQ_ALIGN(a); REQ_ALIGN(w); REQ_ALIGN(y);
  GemmParams p = {};
  p.A = a; p.lda = K; p.Wt = w; p.M = M; p.N = N; p.K = K; p.bias = bias; p.outb = y; p.ldo = N;
  return srk_launch_gemm(LD_ROWS, EP_BF16, p, (hipStream_t)stream);
}

int srk_linear_wgrad_bf16(const uint16_t* y, const uint16_t* x, float* dw, float* db, int M, int N, int K, srk_stream_t stream) {
  REQ_PTR(y); REQ_PTR(x); REQ_PTR(dw); REQ_ALIGN(y); REQ_ALIGN(x);
  WgradParams p = {};
  p.Y = y; p.ldy = N; p.X = x; p.ldx = K; p.M = M; p.N = N; p.K = K; p.dW = dw; p.ldw = K; p.db = db;
  return srk_launch_wgrad(p, (hipStream_t)stream);
}

int srk_linear_wgrad_multi_bf16(const srk_wgrad_problem* problems, int count, int M, srk_stream_t stream) {
  REQ_PTR(problems);
  SRK_REQUIRE(count >= 1 && count <= 4 && M > 0, SRK_E_SHAPE, "linear_wgrad_multi: count=%d (1..4), M=%d", count, M);
  WgradParams ps[4] = {};
  for (int i = 0; i < count; ++i) {
    const srk_wgrad_problem& q = problems[i];
    REQ_PTR(q.y); REQ_PTR(q.x); REQ_PTR(q.dw); REQ_ALIGN(q.y); REQ_ALIGN(q.x);
    SRK_REQUIRE(q.N > 0 && q.K > 0 && q.N % 64 == 0 && q.K % 64 == 0, SRK_E_SHAPE, "linear_wgrad_multi: problem %d: N=%d K=%d (multiples of 64)", i,
                q.N, q.K);
    SRK_REQUIRE((q.ldy <= 0 || q.ldy >= q.N) && (q.ldx <= 0 || q.ldx >= q.K), SRK_E_SHAPE, "linear_wgrad_multi: problem %d: ldy=%d < N or ldx=%d < K",
                i, q.ldy, q.ldx);
    // the kernels read 16-byte pieces at y + m * ldy and x + m * ldx
    SRK_REQUIRE((q.ldy <= 0 || q.ldy % 8 == 0) && (q.ldx <= 0 || q.ldx % 8 == 0), SRK_E_ALIGN,
                "linear_wgrad_multi: problem %d: ldy=%d / ldx=%d must be multiples of 8 elements", i, q.ldy, q.ldx);
    ps[i].Y = static_cast<const bf16_t*>(q.y); ps[i].ldy = q.ldy > 0 ? q.ldy : q.N;
    ps[i].X = static_cast<const bf16_t*>(q.x); ps[i].ldx = q.ldx > 0 ? q.ldx : q.K;
    ps[i].M = M; ps[i].N = q.N; ps[i].K = q.K; ps[i].dW = q.dw; ps[i].ldw = q.K; ps[i].db = q.db;
  }
  return srk_launch_wgrad_multi(ps, count, (hipStream_t)stream);
}

int srk_conv3x3_bf16(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* y, int B, int H, int W, int CinP, int N,
                     srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(w); REQ_PTR(y); REQ_ALIGN(x); REQ_ALIGN(w); REQ_ALIGN(y);
  GemmParams p = {};
  p.A = x; p.Wt = w; p.M = B * H * W; p.N = N; p.K = 9 * CinP; p.B = B; p.H = H; p.W = W; p.CinP = CinP;
  p.bias = bias; p.outb = y; p.ldo = N;
  return srk_launch_gemm(LD_CONV3, EP_BF16, p, (hipStream_t)stream);
}

int srk_conv3x3_wgrad_bf16(const uint16_t* y, const uint16_t* x, float* dw, float* db, int B, int H, int W, int CinP, int N,
                           srk_stream_t stream) {
  REQ_PTR(y); REQ_PTR(x); REQ_PTR(dw); REQ_ALIGN(y); REQ_ALIGN(x);
  SRK_REQUIRE(B > 0 && H > 0 && W > 0 && (long long)B * H * W < (1ll << 31), SRK_E_SHAPE, "conv3x3_wgrad: B=%d H=%d W=%d", B, H, W);
  WgradParams p = {};
  p.Y = y; p.ldy = N; p.X = x; p.ldx = CinP; p.M = B * H * W; p.N = N; p.K = CinP; p.dW = dw; p.ldw = 9 * CinP; p.db = db;
  p.conv = 1; p.B = B; p.H = H; p.W = W; p.r = 1;
  return srk_launch_wgrad(p, (hipStream_t)stream);
}

int srk_cast_f32_bf16(const float* x, uint16_t* y, int64_t n, srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(y);
  SRK_REQUIRE(n > 0 && n % 4 == 0, SRK_E_SHAPE, "cast_f32_bf16: n=%lld must be a positive multiple of 4", (long long)n);
  REQ_ALIGN(x);
  SRK_REQUIRE(srk_aligned(y, 8), SRK_E_ALIGN, "cast_f32_bf16: 'y' is not 8-byte aligned");
  return srk_launch_cast_f32_bf16(x, y, n, (hipStream_t)stream);
}

int srk_probe_begin(int family, int capacity) {
  SRK_REQUIRE(!g_probe.active, SRK_E_STATE, "probe_begin: a probe is already active");
  SRK_REQUIRE(family >= 1 && family <= 7 && capacity > 0 && capacity <= (1 << 20), SRK_E_SHAPE, "probe_begin: bad arguments");
  while ((int)g_probe.ev0.size() < capacity) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
      srk_set_error("probe_begin: hipEventCreate failed");
      return SRK_E_LAUNCH;
    }
    g_probe.ev0.push_back(a);
    g_probe.ev1.push_back(b);
  }
  g_probe.family = family;
  g_probe.count = 0;
  g_probe.seen = 0;
  g_probe.flops = 0.0;
  g_probe.bytes = 0.0;
  g_probe.active = true;
  return SRK_OK;
}

int srk_probe_end(double* total_ms, double* flops, double* bytes, int* launches) {
  SRK_REQUIRE(g_probe.active, SRK_E_STATE, "probe_end: no active probe");
  g_probe.active = false;
  double ms = 0.0;
  for (size_t i = 0; i < g_probe.count; ++i) {
    float t = 0.f;
    if (hipEventSynchronize(g_probe.ev1[i]) != hipSuccess || hipEventElapsedTime(&t, g_probe.ev0[i], g_probe.ev1[i]) != hipSuccess) {
      srk_set_error("probe_end: event query failed");
      return SRK_E_LAUNCH;
    }
    ms += t;
  }
  if (total_ms) *total_ms = ms;
  if (flops) *flops = g_probe.flops;
  if (bytes) *bytes = g_probe.bytes;
  if (launches) *launches = (int)g_probe.count;
  return SRK_OK;
}

// ---- options ---------------------------------------------------------------------------------------------------------------------------
// Every option has ONE process-wide value (srk_set_option: seen by every thread, including the autograd engine's backward thread); a
// plan carries its own values (srk_swinir_plan_set_option), which live in a thread-private copy of the option set for the duration of
// each call on that plan (common.h: SrkOpt) -- two plans with different options can run in one process, also on two threads.
namespace {

int tune_get(int which) {
  int v[4];
  srk_gemm_stream_tune_get(&v[0], &v[1], &v[2], &v[3]);
  return v[which];
}
int tune_set(int which, int value) {
  int v[4];
  srk_gemm_stream_tune_get(&v[0], &v[1], &v[2], &v[3]);
  v[which] = value;
  srk_gemm_stream_tune(v[0], v[1], v[2], v[3]);
  return SRK_OK;
}
int wtune_get(int which) {
  int rows, nt;
  srk_wgrad_stream_tune_get(&rows, &nt);
  return which == 0 ? rows : nt;
}

struct OptEntry {
  const char* name;
  int (*get)();
  int (*set)(int);
};

const OptEntry kOptions[] = {
    {"gemm_stream", [] { return srk_gemm_stream_enabled(); }, [](int v) { srk_gemm_stream_enable(v); return (int)SRK_OK; }},
    {"attn_bwd_fused", [] { return srk_attn_bwd_fused_enabled(); }, [](int v) { srk_attn_bwd_fused_enable(v); return (int)SRK_OK; }},
    {"attn_fused", [] { return srk_attn_fused_mode(); }, [](int v) { srk_attn_fused_enable(v); return (int)SRK_OK; }},
    {"wgrad_stream_w8", [] { return srk_wgrad_w8_enabled(); }, [](int v) { srk_wgrad_w8_enable(v); return (int)SRK_OK; }},
    {"block_light", [] { return srk_block_light_enabled(); }, [](int v) { srk_block_light_enable(v); return (int)SRK_OK; }},
    {"mlp_bwd_fused", [] { return srk_mlp_bwd_fused_enabled(); }, [](int v) { srk_mlp_bwd_fused_enable(v); return (int)SRK_OK; }},
    {"mlp_dgelu_store", [] { return srk_mlp_dgelu_store_enabled(); }, [](int v) { srk_mlp_dgelu_store_enable(v); return (int)SRK_OK; }},
    {"mlp_fused", [] { return srk_mlp_fused_enabled(); }, [](int v) { srk_mlp_fused_enable(v); return (int)SRK_OK; }},
    {"wgrad_stream", [] { return srk_wgrad_stream_enabled(); }, [](int v) { srk_wgrad_stream_enable(v); return (int)SRK_OK; }},
    {"conv_wgrad_taps", [] { return srk_conv_wgrad_taps_mode(); }, [](int v) { srk_conv_wgrad_taps_enable(v); return (int)SRK_OK; }},
    {"conv_wgrad_roll", [] { return srk_conv_wgrad_roll_enabled(); }, [](int v) { srk_conv_wgrad_roll_enable(v); return (int)SRK_OK; }},
    {"wide_head_train", [] { return srk_wide_head_train_enabled(); }, [](int v) { srk_wide_head_train_enable(v); return (int)SRK_OK; }},
    {"wgrad_partials", [] { return srk_wgrad_partials_enabled(); }, [](int v) { srk_wgrad_partials_enable(v); return (int)SRK_OK; }},
    {"wgrad_stream_rows", [] { return wtune_get(0); },
     [](int v) {
       SRK_REQUIRE(v == 32 || v == 64, SRK_E_SHAPE, "wgrad_stream_rows: 32/64");
       srk_wgrad_stream_tune(v, -1);
       return (int)SRK_OK;
     }},
    {"wgrad_stream_nt", [] { return wtune_get(1); }, [](int v) { srk_wgrad_stream_tune(0, v != 0); return (int)SRK_OK; }},
    {"gemm_stream_bm", [] { return tune_get(0); },
     [](int v) {
       SRK_REQUIRE(v == 0 || v == 16 || v == 32 || v == 64, SRK_E_SHAPE, "gemm_stream_bm: 0/16/32/64");
       return tune_set(0, v);
     }},
    {"gemm_stream_ks2", [] { return tune_get(1); }, [](int v) { return tune_set(1, v < 0 ? -1 : (v != 0)); }},
    {"gemm_stream_split", [] { return tune_get(2); }, [](int v) { return tune_set(2, v < 0 ? -1 : (v != 0)); }},
    {"gemm_stream_nb", [] { return tune_get(3); },
     [](int v) {
       SRK_REQUIRE(v == 0 || v == 4 || v == 8, SRK_E_SHAPE, "gemm_stream_nb: 0/4/8");
       return tune_set(3, v);
     }},
    {"probe_stride", [] { return g_probe.stride; },       // the timing probe is one per process
     [](int v) {
       SRK_REQUIRE(v >= 1 && v <= 1024, SRK_E_SHAPE, "probe_stride: 1..1024");
       g_probe.stride = v;
       return (int)SRK_OK;
     }},
};

const OptEntry* find_option(const char* name) {
  for (const OptEntry& e : kOptions)
    if (strcmp(name, e.name) == 0) return &e;
  return nullptr;
}

}  // namespace

int srk_set_option(const char* name, int value) {
  REQ_PTR(name);
  const OptEntry* e = find_option(name);
  if (!e) {
    srk_set_error("srk_set_option: unknown option '%s'", name);
    return SRK_E_UNSUPPORTED;
  }
  return e->set(value);
}

int srk_get_option(const char* name, int* value) {
  REQ_PTR(name); REQ_PTR(value);
  const OptEntry* e = find_option(name);
  if (!e) {
    srk_set_error("srk_get_option: unknown option '%s'", name);
    return SRK_E_UNSUPPORTED;
  }
  *value = e->get();
  return SRK_OK;
}

int srk_probe_trread(const uint16_t* in, uint16_t* out, srk_stream_t stream) {
  REQ_PTR(in); REQ_PTR(out);
  return srk_launch_probe_trread(in, out, (hipStream_t)stream);
}

int srk_l1_loss_fwd_bwd(const float* pred, const float* target, float* d_pred, float* loss, uint32_t* nonfinite, int64_t n,
                        float grad_scale, srk_stream_t stream) {
  REQ_PTR(pred); REQ_PTR(target); REQ_PTR(loss); REQ_PTR(nonfinite);
  SRK_REQUIRE(n > 0, SRK_E_SHAPE, "l1_loss: n=%lld", (long long)n);
  return srk_launch_l1_loss(pred, target, d_pred, loss, nonfinite, n, grad_scale, (hipStream_t)stream);
}

int64_t srk_fft_loss_workspace(int B, int C, int H, int W) { return (int64_t)srk_fft_loss_workspace_bytes(B, C, H, W); }

int srk_fft_loss_fwd_bwd(const float* x, const float* y, void* workspace, int B, int C, int H, int W, int ortho, float alpha, float* d_x,
                         int accumulate, float* value, float* loss, srk_stream_t stream) {
  SRK_REQUIRE(x && y && workspace, SRK_E_NULL, "fft_loss: null pointer (x, y and workspace are required)");
  SRK_REQUIRE(B > 0 && C > 0 && H > 0 && W > 0 && (long long)B * C < 65536, SRK_E_SHAPE, "fft_loss: B=%d C=%d H=%d W=%d", B, C, H, W);
  SRK_REQUIRE(std::isfinite(alpha), SRK_E_SHAPE, "fft_loss: alpha=%g", (double)alpha);
  SRK_REQUIRE((ortho == 0 || ortho == 1) && (accumulate == 0 || accumulate == 1), SRK_E_SHAPE,
              "fft_loss: ortho and accumulate must be 0 or 1 (got %d, %d)", ortho, accumulate);
  SRK_REQUIRE(!accumulate || d_x, SRK_E_SHAPE, "fft_loss: accumulate needs the d_x to add to");
  SRK_REQUIRE(H <= 512 && W <= 512, SRK_E_UNSUPPORTED, "fft_loss: H, W <= 512 (got %dx%d)", H, W);
  const size_t n = sizeof(float) * (size_t)B * C * H * W;
  SRK_REQUIRE(!d_x || (!srk_ranges_overlap(d_x, n, x, n) && !srk_ranges_overlap(d_x, n, y, n)), SRK_E_SHAPE, "fft_loss: d_x overlaps x or y");
  return srk_launch_fft_loss(x, y, static_cast<float*>(workspace), B, C, H, W, ortho, alpha, d_x, accumulate, value, loss,
                             (hipStream_t)stream);
}

int64_t srk_wgrad_workspace_bytes(void) { return (int64_t)WS_WORKSPACE_BYTES; }

int srk_set_wgrad_workspace(void* workspace, int64_t bytes) {
  SRK_REQUIRE(bytes >= 0 && (workspace != nullptr || bytes == 0), SRK_E_SHAPE, "set_wgrad_workspace: null pointer with %lld bytes",
              (long long)bytes);
  srk_wgrad_bind_workspace(workspace, (size_t)bytes, nullptr, nullptr);
  return SRK_OK;
}

int srk_paired_crop_u8(const uint8_t* pool, const int64_t* lr_desc, const int64_t* hr_desc, float* lr_out, float* hr_out, int B,
                       int lr_patch, int scale, srk_stream_t stream) {
  REQ_PTR(pool); REQ_PTR(lr_desc); REQ_PTR(hr_desc); REQ_PTR(lr_out); REQ_PTR(hr_out);
  SRK_REQUIRE(B > 0 && B <= 65535 && lr_patch > 0 && scale > 0 && (long long)lr_patch * scale <= 8192, SRK_E_SHAPE,
              "paired_crop: B=%d patch=%d scale=%d", B, lr_patch, scale);
  int rc = srk_launch_crop_u8(pool, reinterpret_cast<const long long*>(lr_desc), lr_out, B, lr_patch, (hipStream_t)stream);
  if (rc) return rc;
  return srk_launch_crop_u8(pool, reinterpret_cast<const long long*>(hr_desc), hr_out, B, lr_patch * scale, (hipStream_t)stream);
}

int srk_crop_u8(const uint8_t* pool, const int64_t* desc, float* out, int B, int patch, srk_stream_t stream) {
  REQ_PTR(pool); REQ_PTR(desc); REQ_PTR(out);
  SRK_REQUIRE(B > 0 && B <= 65535 && patch > 0 && patch <= 8192, SRK_E_SHAPE, "crop_u8: B=%d (1..65535) patch=%d (1..8192)", B, patch);
  return srk_launch_crop_u8(pool, reinterpret_cast<const long long*>(desc), out, B, patch, (hipStream_t)stream);
}

int srk_dihedral_f32(const float* in, float* out, const int32_t* ops, int op_all, int B, int C, int H, int W, float alpha,
                     int accumulate, srk_stream_t stream) {
  REQ_PTR(in); REQ_PTR(out);
  SRK_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, SRK_E_SHAPE, "dihedral: B=%d C=%d H=%d W=%d must all be >= 1", B, C, H, W);
  SRK_REQUIRE(accumulate == 0 || accumulate == 1, SRK_E_SHAPE, "dihedral: accumulate must be 0 or 1 (got %d)", accumulate);
  if (ops) SRK_REQUIRE(H == W, SRK_E_SHAPE, "dihedral: per-sample op codes need square images (got %d x %d)", H, W);
  else SRK_REQUIRE(op_all >= 0 && op_all <= 7, SRK_E_SHAPE, "dihedral: op must be in 0..7 (got %d)", op_all);
  const double bytes = 4.0 * B * C * H * W;
  SRK_REQUIRE(bytes < 9.0e18, SRK_E_SHAPE, "dihedral: B=%d C=%d H=%d W=%d is too large", B, C, H, W);
  SRK_REQUIRE(!srk_ranges_overlap(in, (size_t)bytes, out, (size_t)bytes), SRK_E_SHAPE, "dihedral: in and out overlap (the transform is not done in place)");
  return srk_launch_dihedral_f32(in, out, reinterpret_cast<const int*>(ops), op_all, B, C, H, W, alpha, accumulate, (hipStream_t)stream);
}

int srk_resize_aa_f32(const float* x, float* out, int B, int C, int H, int W, int Ho, int Wo, int quant_bits, srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(out);
  SRK_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1 && Ho >= 1 && Wo >= 1, SRK_E_SHAPE, "resize_aa: B=%d C=%d H=%d W=%d Ho=%d Wo=%d must all be >= 1",
              B, C, H, W, Ho, Wo);
  SRK_REQUIRE(quant_bits == 0 || quant_bits == 8, SRK_E_SHAPE, "resize_aa: quant_bits must be 0 or 8 (got %d)", quant_bits);
  const double planes = (double)B * C, ib = 4.0 * planes * H * W, ob = 4.0 * planes * Ho * Wo;
  SRK_REQUIRE(planes <= 2147483647.0 && ib < 9.0e18 && ob < 9.0e18, SRK_E_SHAPE, "resize_aa: B=%d C=%d H=%d W=%d Ho=%d Wo=%d is too large", B, C, H,
              W, Ho, Wo);
  SRK_REQUIRE(!srk_ranges_overlap(x, (size_t)ib, out, (size_t)ob), SRK_E_SHAPE, "resize_aa: x and out overlap (the resize is not done in place)");
  SRK_REQUIRE((long long)H <= 8LL * Ho && (long long)W <= 8LL * Wo, SRK_E_UNSUPPORTED,
              "resize_aa: %d x %d -> %d x %d shrinks an axis by more than 8x (more than 33 taps)", H, W, Ho, Wo);
  return srk_launch_resize_aa_f32(x, out, B * C, H, W, Ho, Wo, quant_bits, (hipStream_t)stream);
}

int srk_crop_degrade_u8(const uint8_t* pool, const int64_t* hr_desc, float* lr_out, float* hr_out, int B, int lr_patch, int scale,
                        int quant_bits, srk_stream_t stream) {
  REQ_PTR(pool); REQ_PTR(hr_desc); REQ_PTR(lr_out); REQ_PTR(hr_out);
  SRK_REQUIRE(B > 0 && B <= 65535 && lr_patch > 0 && lr_patch <= 2048 && scale >= 2 && scale <= 4, SRK_E_SHAPE,
              "crop_degrade: B=%d (1..65535) patch=%d (1..2048) scale=%d (2..4)", B, lr_patch, scale);
  SRK_REQUIRE(quant_bits == 0 || quant_bits == 8, SRK_E_SHAPE, "crop_degrade: quant_bits must be 0 or 8 (got %d)", quant_bits);
  return srk_launch_crop_degrade_u8(pool, reinterpret_cast<const long long*>(hr_desc), lr_out, hr_out, B, lr_patch, scale, quant_bits,
                                    (hipStream_t)stream);
}

int srk_crop_degrade_blind_u8(const uint8_t* pool, const int64_t* desc10, float* lr_out, float* hr_out, int B, int lr_patch, int scale,
                              int quant_bits, srk_stream_t stream) {
  REQ_PTR(pool); REQ_PTR(desc10); REQ_PTR(lr_out); REQ_PTR(hr_out);
  SRK_REQUIRE(B > 0 && B <= 65535 && lr_patch > 0 && lr_patch <= 2048 && scale >= 2 && scale <= 4, SRK_E_SHAPE,
              "crop_degrade_blind: B=%d (1..65535) patch=%d (1..2048) scale=%d (2..4)", B, lr_patch, scale);
  SRK_REQUIRE(quant_bits == 0 || quant_bits == 8, SRK_E_SHAPE, "crop_degrade_blind: quant_bits must be 0 or 8 (got %d)", quant_bits);
  return srk_launch_crop_degrade_blind_u8(pool, reinterpret_cast<const long long*>(desc10), lr_out, hr_out, B, lr_patch, scale, quant_bits,
                                          (hipStream_t)stream);
}

int srk_degrade_blind_f32(const float* x, float* out, const int64_t* par4, int B, int C, int H, int W, int scale, int quant_bits,
                          srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(out); REQ_PTR(par4);
  SRK_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1, SRK_E_SHAPE, "degrade_blind: B=%d C=%d H=%d W=%d must all be >= 1", B, C, H, W);
  SRK_REQUIRE(scale >= 2 && scale <= 4 && H % scale == 0 && W % scale == 0, SRK_E_SHAPE,
              "degrade_blind: scale=%d must be in 2..4 and divide H=%d and W=%d", scale, H, W);
  SRK_REQUIRE(quant_bits == 0 || quant_bits == 8, SRK_E_SHAPE, "degrade_blind: quant_bits must be 0 or 8 (got %d)", quant_bits);
  const double planes = (double)B * C, ib = 4.0 * planes * H * W, ob = ib / ((double)scale * scale);
  SRK_REQUIRE(planes <= 2147483647.0 && ib < 9.0e18, SRK_E_SHAPE, "degrade_blind: B=%d C=%d H=%d W=%d is too large", B, C, H, W);
  SRK_REQUIRE(!srk_ranges_overlap(x, (size_t)ib, out, (size_t)ob), SRK_E_SHAPE, "degrade_blind: x and out overlap (the filter is not run in place)");
  return srk_launch_degrade_blind_f32(x, out, reinterpret_cast<const long long*>(par4), B, C, H, W, scale, quant_bits, (hipStream_t)stream);
}

int srk_blur2d_f32(const float* x, const float* psf, float* out, int B, int C, int H, int W, int ks, srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(psf); REQ_PTR(out);
  SRK_REQUIRE(srk_psf_ks_ok(ks), SRK_E_SHAPE, "blur2d: ks must be odd and in 1..21 (got %d)", ks);
  SRK_REQUIRE(srk_blur2d_shape_ok(B, C, H, W), SRK_E_SHAPE, "blur2d: B=%d C=%d H=%d W=%d must all be >= 1 and fit one launch", B, C, H, W);
  const size_t bytes = (size_t)(4.0 * B * C * H * W), kb = sizeof(float) * (size_t)B * ks * ks;
  SRK_REQUIRE(!srk_ranges_overlap(x, bytes, out, bytes) && !srk_ranges_overlap(psf, kb, out, bytes), SRK_E_SHAPE,
              "blur2d: out overlaps x or psf (the blur is not run in place)");
  return srk_launch_blur2d_f32(x, psf, out, B, C, H, W, ks, (hipStream_t)stream);
}

int srk_crop_degrade_psf_u8(const uint8_t* pool, const int64_t* desc10, const float* psf, int ks, float* lr_out, float* hr_out, int B,
                            int lr_patch, int scale, int quant_bits, srk_stream_t stream) {
  REQ_PTR(pool); REQ_PTR(desc10); REQ_PTR(psf); REQ_PTR(lr_out); REQ_PTR(hr_out);
  SRK_REQUIRE(srk_crop_degrade_shape_ok(B, lr_patch, scale), SRK_E_SHAPE, "crop_degrade_psf: B=%d (1..65535) patch=%d (1..2048) scale=%d (2..4)",
              B, lr_patch, scale);
  SRK_REQUIRE(quant_bits == 0 || quant_bits == 8, SRK_E_SHAPE, "crop_degrade_psf: quant_bits must be 0 or 8 (got %d)", quant_bits);
  SRK_REQUIRE(srk_psf_ks_ok(ks), SRK_E_SHAPE, "crop_degrade_psf: ks must be odd and in 1..21 (got %d)", ks);
  return srk_launch_crop_degrade_psf_u8(pool, reinterpret_cast<const long long*>(desc10), psf, ks, lr_out, hr_out, B, lr_patch, scale,
                                        quant_bits, (hipStream_t)stream);
}

int srk_jpeg_roundtrip_f32(const float* x, float* out, const int32_t* quality, int B, int C, int H, int W, int subsample, int16_t* coef_out,
                           srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(out); REQ_PTR(quality);
  SRK_REQUIRE(B >= 1 && H >= 1 && W >= 1, SRK_E_SHAPE, "jpeg_roundtrip: B=%d H=%d W=%d must all be >= 1", B, H, W);
  SRK_REQUIRE(C == 1 || C == 3, SRK_E_SHAPE, "jpeg_roundtrip: C must be 1 or 3 (got %d)", C);
  SRK_REQUIRE(subsample == 0 || subsample == 1, SRK_E_SHAPE, "jpeg_roundtrip: subsample must be 0 (4:4:4) or 1 (4:2:0) (got %d)", subsample);
  const double bytes = 4.0 * B * C * H * W;
  SRK_REQUIRE(bytes < 9.0e18, SRK_E_SHAPE, "jpeg_roundtrip: B=%d C=%d H=%d W=%d is too large", B, C, H, W);
  SRK_REQUIRE(!srk_ranges_overlap(x, (size_t)bytes, out, (size_t)bytes), SRK_E_SHAPE, "jpeg_roundtrip: x and out overlap (the blocks are not transformed in place)");
  return srk_launch_jpeg_roundtrip_f32(x, out, reinterpret_cast<const int*>(quality), B, C, H, W, subsample, reinterpret_cast<short*>(coef_out),
                                       (hipStream_t)stream);
}

int srk_noise_f32(const float* x, float* out, const int64_t* par4, int B, int C, int H, int W, int quant_bits, srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(out); REQ_PTR(par4);
  SRK_REQUIRE(srk_noise_shape_ok(B, C, H, W), SRK_E_SHAPE, "noise: B=%d H=%d W=%d must all be >= 1, C=%d must be 1 or 3, and the size must fit one launch",
              B, H, W, C);
  SRK_REQUIRE(srk_quant_bits_ok(quant_bits), SRK_E_SHAPE, "noise: quant_bits must be 0 or 8 (got %d)", quant_bits);
  const size_t bytes = (size_t)(4.0 * B * C * H * W);
  SRK_REQUIRE(!srk_ranges_overlap(x, bytes, out, bytes), SRK_E_SHAPE, "noise: x and out overlap (the stage is not run in place)");
  return srk_launch_noise_f32(x, out, reinterpret_cast<const long long*>(par4), B, C, H, W, quant_bits, (hipStream_t)stream);
}

int srk_filter2d_f32(const float* x, const float* tab, float* out, const int32_t* ext, int B, int C, int Hp, int Wp, int ks, int quant_bits,
                     srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(tab); REQ_PTR(out);
  SRK_REQUIRE(srk_psf_ks_ok(ks), SRK_E_SHAPE, "filter2d: ks must be odd and in 1..21 (got %d)", ks);
  SRK_REQUIRE(srk_filter2d_shape_ok(B, C, Hp, Wp, ks), SRK_E_SHAPE,
              "filter2d: B=%d C=%d must be >= 1, Hp=%d Wp=%d above R=%d (the reflection needs an extent > R), and the size must fit one launch", B, C,
              Hp, Wp, ks / 2);
  SRK_REQUIRE(srk_quant_bits_ok(quant_bits), SRK_E_SHAPE, "filter2d: quant_bits must be 0 or 8 (got %d)", quant_bits);
  const size_t bytes = (size_t)(4.0 * B * C * Hp * Wp), kb = sizeof(float) * (size_t)B * ks * ks, eb = ext ? sizeof(int32_t) * 2 * (size_t)B : 0;
  SRK_REQUIRE(!srk_ranges_overlap(x, bytes, out, bytes) && !srk_ranges_overlap(tab, kb, out, bytes) && !srk_ranges_overlap(ext, eb, out, bytes),
              SRK_E_SHAPE, "filter2d: out overlaps x, tab or ext (the filter is not run in place)");
  return srk_launch_filter2d_f32(x, tab, out, reinterpret_cast<const int*>(ext), B, C, Hp, Wp, ks, quant_bits, (hipStream_t)stream);
}

int srk_kernel_tables_f32(const double* desc, const float* bank, int n_bank, int kb, float* tab, int n, int ks, srk_stream_t stream) {
  REQ_PTR(desc); REQ_PTR(tab);
  SRK_REQUIRE(srk_psf_ks_ok(ks), SRK_E_SHAPE, "kernel_tables: ks must be odd and in 1..21 (got %d)", ks);
  SRK_REQUIRE(srk_tables_shape_ok(n, ks, bank != nullptr, n_bank, kb), SRK_E_SHAPE,
              "kernel_tables: n=%d must be >= 1, and the bank is absent (NULL, 0, 0) or has n_bank=%d >= 1 and kb=%d odd in 1..ks=%d", n, n_bank, kb, ks);
  const size_t tb = srk_tables_bytes(n, ks, sizeof(float)), db = sizeof(double) * 8 * (size_t)n, bb = bank ? srk_tables_bytes(n_bank, kb, sizeof(float)) : 0;
  SRK_REQUIRE(!srk_ranges_overlap(desc, db, tab, tb) && !srk_ranges_overlap(bank, bb, tab, tb), SRK_E_SHAPE,
              "kernel_tables: tab overlaps desc or bank");
  return srk_launch_kernel_tables_f32(desc, bank, n_bank, kb, tab, n, ks, (hipStream_t)stream);
}

int srk_resize_aa_ragged_f32(const float* x, const int32_t* ext_in, float* out, const int32_t* ext_out, int B, int C, int Hp, int Wp, int Hop,
                             int Wop, int quant_bits, srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(out);
  SRK_REQUIRE(srk_resize_ragged_shape_ok(B, C, Hp, Wp, Hop, Wop), SRK_E_SHAPE,
              "resize_aa_ragged: B=%d C=%d Hp=%d Wp=%d Hop=%d Wop=%d must all be >= 1 and fit one launch", B, C, Hp, Wp, Hop, Wop);
  SRK_REQUIRE(srk_quant_bits_ok(quant_bits), SRK_E_SHAPE, "resize_aa_ragged: quant_bits must be 0 or 8 (got %d)", quant_bits);
  const size_t ib = (size_t)(4.0 * B * C * Hp * Wp), ob = (size_t)(4.0 * B * C * Hop * Wop), eb = sizeof(int32_t) * 2 * (size_t)B;
  SRK_REQUIRE(!srk_ranges_overlap(x, ib, out, ob) && !srk_ranges_overlap(ext_in, ext_in ? eb : 0, out, ob) &&
                  !srk_ranges_overlap(ext_out, ext_out ? eb : 0, out, ob),
              SRK_E_SHAPE, "resize_aa_ragged: out overlaps x or an extent table (the resize is not done in place)");
  // the extents live in device memory: a dense batch is checked here, a ragged one by the caller that wrote the tables
  if (!ext_in && !ext_out)
    SRK_REQUIRE(srk_resize_factor_ok(Hp, Hop) && srk_resize_factor_ok(Wp, Wop), SRK_E_UNSUPPORTED,
                "resize_aa_ragged: %d x %d -> %d x %d shrinks an axis by more than 8x (more than 33 taps)", Hp, Wp, Hop, Wop);
  return srk_launch_resize_aa_ragged_f32(x, reinterpret_cast<const int*>(ext_in), out, reinterpret_cast<const int*>(ext_out), B, C, Hp, Wp, Hop,
                                         Wop, quant_bits, (hipStream_t)stream);
}

int srk_jpeg_roundtrip_ragged_f32(const float* x, float* out, const int32_t* quality, const int32_t* ext, int B, int C, int Hp, int Wp,
                                  int subsample, srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(out); REQ_PTR(quality);
  SRK_REQUIRE(srk_noise_shape_ok(B, C, Hp, Wp), SRK_E_SHAPE,
              "jpeg_roundtrip_ragged: B=%d Hp=%d Wp=%d must all be >= 1, C=%d must be 1 or 3, and the size must fit one launch", B, Hp, Wp, C);
  SRK_REQUIRE(srk_flag01_ok(subsample), SRK_E_SHAPE, "jpeg_roundtrip_ragged: subsample must be 0 (4:4:4) or 1 (4:2:0) (got %d)", subsample);
  const size_t bytes = (size_t)(4.0 * B * C * Hp * Wp);
  SRK_REQUIRE(!srk_ranges_overlap(x, bytes, out, bytes), SRK_E_SHAPE, "jpeg_roundtrip_ragged: x and out overlap (the blocks are not transformed in place)");
  return srk_launch_jpeg_roundtrip_ragged_f32(x, out, reinterpret_cast<const int*>(quality), reinterpret_cast<const int*>(ext), B, C, Hp, Wp,
                                              subsample, (hipStream_t)stream);
}

int srk_resize_ragged_mode_f32(const float* x, const int32_t* ext_in, float* out, const int32_t* ext_out, const int32_t* mode, int B, int C,
                               int Hp, int Wp, int Hop, int Wop, int quant_bits, srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(out);
  SRK_REQUIRE(srk_resize_ragged_shape_ok(B, C, Hp, Wp, Hop, Wop), SRK_E_SHAPE,
              "resize_ragged_mode: B=%d C=%d Hp=%d Wp=%d Hop=%d Wop=%d must all be >= 1 and fit one launch", B, C, Hp, Wp, Hop, Wop);
  SRK_REQUIRE(srk_quant_bits_ok(quant_bits), SRK_E_SHAPE, "resize_ragged_mode: quant_bits must be 0 or 8 (got %d)", quant_bits);
  const size_t ib = (size_t)(4.0 * B * C * Hp * Wp), ob = (size_t)(4.0 * B * C * Hop * Wop), eb = sizeof(int32_t) * 2 * (size_t)B;
  SRK_REQUIRE(!srk_ranges_overlap(x, ib, out, ob) && !srk_ranges_overlap(ext_in, ext_in ? eb : 0, out, ob) &&
                  !srk_ranges_overlap(ext_out, ext_out ? eb : 0, out, ob) && !srk_ranges_overlap(mode, mode ? eb / 2 : 0, out, ob),
              SRK_E_SHAPE, "resize_ragged_mode: out overlaps x, an extent table or mode (the resize is not done in place)");
  if (!ext_in && !ext_out)
    SRK_REQUIRE(srk_resize_factor_ok(Hp, Hop) && srk_resize_factor_ok(Wp, Wop), SRK_E_UNSUPPORTED,
                "resize_ragged_mode: %d x %d -> %d x %d shrinks an axis by more than 8x (the tile staging covers 8x)", Hp, Wp, Hop, Wop);
  return srk_launch_resize_ragged_mode_f32(x, reinterpret_cast<const int*>(ext_in), out, reinterpret_cast<const int*>(ext_out),
                                           reinterpret_cast<const int*>(mode), B, C, Hp, Wp, Hop, Wop, quant_bits, (hipStream_t)stream);
}

int srk_usm_sharpen_f32(const float* x, const float* taps, float* out, float* work, int B, int C, int H, int W, int ks, float weight,
                        float threshold, srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(taps); REQ_PTR(out); REQ_PTR(work);
  SRK_REQUIRE(srk_usm_shape_ok(B, C, H, W, ks), SRK_E_SHAPE,
              "usm_sharpen: B=%d H=%d W=%d must all be >= 1, C=%d must be 1 or 3, ks=%d odd and in 1..%d, and the size must fit one launch", B, H, W,
              C, ks, SRK_USM_MAX_KS);
  SRK_REQUIRE(srk_usm_extent_ok(H, W, ks), SRK_E_UNSUPPORTED, "usm_sharpen: a %d x %d image is not larger than R = %d (ks=%d)", H, W, ks / 2, ks);
  const size_t bytes = (size_t)(4.0 * B * C * H * W), kb = sizeof(float) * (size_t)ks;
  SRK_REQUIRE(!srk_ranges_overlap(x, bytes, out, bytes) && !srk_ranges_overlap(x, bytes, work, bytes) && !srk_ranges_overlap(out, bytes, work, bytes) &&
                  !srk_ranges_overlap(taps, kb, out, bytes) && !srk_ranges_overlap(taps, kb, work, bytes),
              SRK_E_SHAPE, "usm_sharpen: x, taps, out and work must not overlap");
  return srk_launch_usm_sharpen_f32(x, taps, out, work, B, C, H, W, ks, weight, threshold, (hipStream_t)stream);
}

int srk_crop_restore_u8(const uint8_t* pool, const int64_t* desc10, float* clean_out, float* degraded_out, int B, int patch, int out_chans,
                        int subsample, int quant_bits, srk_stream_t stream) {
  REQ_PTR(pool); REQ_PTR(desc10); REQ_PTR(clean_out); REQ_PTR(degraded_out);
  SRK_REQUIRE(srk_crop_restore_shape_ok(B, patch, out_chans), SRK_E_SHAPE, "crop_restore: B=%d (1..65535) patch=%d (1..2048) out_chans=%d (1 or 3)", B,
              patch, out_chans);
  SRK_REQUIRE(srk_flag01_ok(subsample), SRK_E_SHAPE, "crop_restore: subsample must be 0 (4:4:4) or 1 (4:2:0) (got %d)", subsample);
  SRK_REQUIRE(srk_quant_bits_ok(quant_bits), SRK_E_SHAPE, "crop_restore: quant_bits must be 0 or 8 (got %d)", quant_bits);
  const size_t bytes = sizeof(float) * (size_t)B * out_chans * patch * patch;          // <= 4 * 65535 * 3 * 2048^2 < 2^42
  SRK_REQUIRE(!srk_ranges_overlap(clean_out, bytes, degraded_out, bytes), SRK_E_SHAPE, "crop_restore: clean_out and degraded_out overlap");
  return srk_launch_crop_restore_u8(pool, reinterpret_cast<const long long*>(desc10), clean_out, degraded_out, B, patch, out_chans, subsample,
                                    quant_bits, (hipStream_t)stream);
}

// the checks srk_tile_gather_f32 and srk_tile_merge_f32 share; img is x or out, whichever the tiles must not overlap
static int tile_args(const char* fn, const float* tiles, const float* img, int t0, int n, int B, int C, int H, int W, int th, int tw,
                     int sy, int sx, TileAxis* ay, TileAxis* ax) {
  SRK_REQUIRE(B >= 1 && C >= 1 && H >= 1 && W >= 1 && th >= 1 && tw >= 1, SRK_E_SHAPE, "%s: B=%d C=%d H=%d W=%d th=%d tw=%d must all be >= 1",
              fn, B, C, H, W, th, tw);
  SRK_REQUIRE(th <= H && tw <= W, SRK_E_SHAPE, "%s: a %d x %d tile is larger than the %d x %d image", fn, th, tw, H, W);
  SRK_REQUIRE(sy >= 1 && sy <= th && sx >= 1 && sx <= tw, SRK_E_SHAPE, "%s: the stride must be in 1..tile (got %d for th=%d, %d for tw=%d)",
              fn, sy, th, sx, tw);
  *ay = srk_tile_axis(H, th, sy);
  *ax = srk_tile_axis(W, tw, sx);
  const long long grid = (long long)ay->k * ax->k;
  SRK_REQUIRE(t0 >= 0 && n >= 1 && (long long)t0 + n <= grid && grid <= 2147483647LL, SRK_E_SHAPE,
              "%s: the chunk [%d, %d + %d) is outside the grid of %d x %d tiles", fn, t0, t0, n, ay->k, ax->k);
  const double planes = (double)B * C, tb = 4.0 * n * planes * th * tw, ib = 4.0 * planes * H * W;
  SRK_REQUIRE(planes <= 2147483647.0 && tb < 9.0e18 && ib < 9.0e18, SRK_E_SHAPE, "%s: n=%d B=%d C=%d H=%d W=%d th=%d tw=%d is too large", fn, n,
              B, C, H, W, th, tw);
  SRK_REQUIRE(!srk_ranges_overlap(tiles, (size_t)tb, img, (size_t)ib), SRK_E_SHAPE, "%s: the tiles and the image overlap", fn);
  return SRK_OK;
}

int srk_tile_gather_f32(const float* x, float* tiles, int t0, int n, int B, int C, int H, int W, int th, int tw, int sy, int sx,
                        srk_stream_t stream) {
  REQ_PTR(x); REQ_PTR(tiles);
  TileAxis ay, ax;
  const int rc = tile_args("tile_gather", tiles, x, t0, n, B, C, H, W, th, tw, sy, sx, &ay, &ax);
  if (rc) return rc;
  return srk_launch_tile_gather_f32(x, tiles, t0, n, B * C, ay, ax, (hipStream_t)stream);
}

int srk_tile_merge_f32(const float* tiles, float* out, int t0, int n, int B, int C, int Ho, int Wo, int th, int tw, int sy, int sx,
                       int mode, srk_stream_t stream) {
  REQ_PTR(tiles); REQ_PTR(out);
  SRK_REQUIRE(mode == SRK_TILE_MEAN || mode == SRK_TILE_CENTER, SRK_E_SHAPE, "tile_merge: mode must be SRK_TILE_MEAN or SRK_TILE_CENTER (got %d)",
              mode);
  TileAxis ay, ax;
  const int rc = tile_args("tile_merge", tiles, out, t0, n, B, C, Ho, Wo, th, tw, sy, sx, &ay, &ax);
  if (rc) return rc;
  return srk_launch_tile_merge_f32(tiles, out, t0, n, B * C, ay, ax, mode, (hipStream_t)stream);
}

int srk_image_unpack(const void* src, float* dst, float* alpha, int B, int H, int W, int in_chans, int bits, int out_chans,
                     srk_stream_t stream) {
  SRK_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1, SRK_E_SHAPE, "image_unpack: B must be in 1..65535 and H, W >= 1 (got B=%d H=%d W=%d)",
              B, H, W);
  SRK_REQUIRE(in_chans >= 1 && in_chans <= 4 && (bits == 8 || bits == 16) && (out_chans == 1 || out_chans == 3), SRK_E_SHAPE,
              "image_unpack: in_chans must be in 1..4, bits 8 or 16, out_chans 1 or 3 (got %d, %d, %d)", in_chans, bits, out_chans);
  REQ_PTR(src); REQ_PTR(dst);
  SRK_REQUIRE(bits == 8 || srk_aligned(src, 2), SRK_E_ALIGN, "image_unpack: 16-bit samples at an odd address");
  SRK_REQUIRE(srk_aligned(dst, 4) && srk_aligned(alpha, 4), SRK_E_ALIGN, "image_unpack: 'dst' / 'alpha' is not 4-byte aligned");
  return srk_launch_image_unpack(src, dst, alpha, B, H, W, in_chans, bits, out_chans, (hipStream_t)stream);
}

int srk_image_pack(const float* y, const float* alpha, void* dst, uint32_t* counters, int B, int H, int W, int chans, int out_chans,
                   int bits, srk_stream_t stream) {
  SRK_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1, SRK_E_SHAPE, "image_pack: B must be in 1..65535 and H, W >= 1 (got B=%d H=%d W=%d)",
              B, H, W);
  SRK_REQUIRE((chans == 1 || chans == 3) && out_chans >= 1 && out_chans <= 4 && (bits == 8 || bits == 16), SRK_E_SHAPE,
              "image_pack: chans must be 1 or 3, out_chans in 1..4, bits 8 or 16 (got %d, %d, %d)", chans, out_chans, bits);
  REQ_PTR(y); REQ_PTR(dst);
  SRK_REQUIRE((out_chans & 1) || alpha != nullptr, SRK_E_NULL, "image_pack: out_chans %d needs 'alpha'", out_chans);
  SRK_REQUIRE(bits == 8 || srk_aligned(dst, 2), SRK_E_ALIGN, "image_pack: 16-bit samples at an odd address");
  SRK_REQUIRE(srk_aligned(y, 4) && srk_aligned(alpha, 4) && srk_aligned(counters, 4), SRK_E_ALIGN,
              "image_pack: 'y' / 'alpha' / 'counters' is not 4-byte aligned");
  return srk_launch_image_pack(y, alpha, dst, counters, B, H, W, chans, out_chans, bits, (hipStream_t)stream);
}

int64_t srk_batch_psnr_workspace(int64_t per_image, int B) {
  if (per_image <= 0 || B <= 0) return 0;
  return (int64_t)2 * sizeof(float) * B * srk_batch_psnr_chunks(per_image);
}

int srk_batch_psnr(const float* pred, const float* target, void* workspace, int B, int64_t per_image, float max_val, float* psnr,
                   float* psnr_sum, float* abs_sum, srk_stream_t stream) {
  REQ_PTR(pred); REQ_PTR(target); REQ_PTR(workspace);
  SRK_REQUIRE(B > 0 && B <= 1024 && per_image > 0, SRK_E_SHAPE, "batch_psnr: B=%d (1..1024) per_image=%lld", B, (long long)per_image);
  SRK_REQUIRE(max_val > 0.f, SRK_E_SHAPE, "batch_psnr: max_val=%g", (double)max_val);
  return srk_launch_batch_psnr(pred, target, static_cast<float*>(workspace), B, per_image, max_val, psnr, psnr_sum, abs_sum,
                               (hipStream_t)stream);
}

int srk_grad_sumsq(const float* grads, int64_t n, float* sumsq, srk_stream_t stream) {
  REQ_PTR(grads); REQ_PTR(sumsq);
  return srk_launch_sumsq(grads, n, sumsq, (hipStream_t)stream);
}

int srk_adamw_clip_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const float* sumsq,
                        float max_norm, float grad_div, float lr, float beta1, float beta2, float eps, float weight_decay,
                        int step, const int32_t* nonfinite, srk_stream_t stream) {
  REQ_PTR(params); REQ_PTR(grads); REQ_PTR(exp_avg); REQ_PTR(exp_avg_sq);
  SRK_REQUIRE(max_norm <= 0.f || sumsq != nullptr, SRK_E_NULL, "adamw: clipping needs sumsq");
  SRK_REQUIRE(step >= 1 && grad_div > 0.f, SRK_E_SHAPE, "adamw: step=%d grad_div=%f", step, grad_div);
  return srk_launch_adamw(params, grads, exp_avg, exp_avg_sq, n, sumsq, nonfinite, max_norm, grad_div, lr, beta1, beta2, eps,
                          weight_decay, step, (hipStream_t)stream);
}

int srk_adamw_clip_ema_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                            const float* sumsq, float max_norm, float grad_div, float lr, float beta1, float beta2, float eps,
                            float weight_decay, int step, float ema_decay, const int32_t* nonfinite, srk_stream_t stream) {
  REQ_PTR(params); REQ_PTR(grads); REQ_PTR(exp_avg); REQ_PTR(exp_avg_sq); REQ_PTR(ema);
  SRK_REQUIRE(max_norm <= 0.f || sumsq != nullptr, SRK_E_NULL, "adamw ema: clipping needs sumsq");
  SRK_REQUIRE(step >= 1 && grad_div > 0.f, SRK_E_SHAPE, "adamw ema: step=%d grad_div=%f", step, grad_div);
  SRK_REQUIRE(ema_decay >= 0.f && ema_decay < 1.f, SRK_E_SHAPE, "adamw ema: ema_decay=%g (0 <= decay < 1)", (double)ema_decay);
  return srk_launch_adamw_ema(params, grads, exp_avg, exp_avg_sq, ema, n, sumsq, nonfinite, max_norm, grad_div, lr, beta1, beta2, eps,
                              weight_decay, step, ema_decay, (hipStream_t)stream);
}

static int check_tensor_list(const char* fn, const void* const* const* lists, const char* const* names, int n_lists, const int64_t* numel,
                             int n_tensors) {
  SRK_REQUIRE(n_tensors > 0, SRK_E_SHAPE, "%s: n_tensors=%d", fn, n_tensors);
  SRK_REQUIRE(numel != nullptr, SRK_E_NULL, "%s: null pointer 'numel'", fn);
  for (int l = 0; l < n_lists; ++l) SRK_REQUIRE(lists[l] != nullptr, SRK_E_NULL, "%s: null pointer '%s'", fn, names[l]);
  for (int t = 0; t < n_tensors; ++t) {
    SRK_REQUIRE(numel[t] >= 0 && numel[t] <= ((int64_t)1 << 34), SRK_E_SHAPE, "%s: numel[%d]=%lld", fn, t, (long long)numel[t]);
    for (int l = 0; l < n_lists; ++l)
      SRK_REQUIRE(lists[l][t] != nullptr || numel[t] == 0, SRK_E_NULL, "%s: null pointer '%s[%d]'", fn, names[l], t);
  }
  return SRK_OK;
}

int srk_multi_grad_sumsq(const float* const* grads, const int64_t* numel, int n_tensors, float* sumsq, srk_stream_t stream) {
  const void* const* lists[1] = {(const void* const*)grads};
  const char* names[1] = {"grads"};
  const int rc = check_tensor_list(__func__, lists, names, 1, numel, n_tensors);
  if (rc != SRK_OK) return rc;
  REQ_PTR(sumsq);
  return srk_launch_multi_sumsq(grads, (const long long*)numel, n_tensors, sumsq, (hipStream_t)stream);
}

int srk_multi_adamw_clip_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                              const int64_t* numel, int n_tensors, const float* sumsq, float max_norm, float grad_div, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int step, const float* hyper,
                              const int32_t* nonfinite, srk_stream_t stream) {
  const void* const* lists[4] = {(const void* const*)params, (const void* const*)grads, (const void* const*)exp_avg,
                                 (const void* const*)exp_avg_sq};
  const char* names[4] = {"params", "grads", "exp_avg", "exp_avg_sq"};
  const int rc = check_tensor_list(__func__, lists, names, 4, numel, n_tensors);
  if (rc != SRK_OK) return rc;
  SRK_REQUIRE(max_norm <= 0.f || sumsq != nullptr, SRK_E_NULL, "multi adamw: clipping needs sumsq");
  SRK_REQUIRE(step >= 1 && grad_div > 0.f, SRK_E_SHAPE, "multi adamw: step=%d grad_div=%f", step, grad_div);
  return srk_launch_multi_adamw(params, grads, exp_avg, exp_avg_sq, (const long long*)numel, n_tensors, sumsq, nonfinite, hyper, max_norm,
                                grad_div, lr, beta1, beta2, eps, weight_decay, step, (hipStream_t)stream);
}

int srk_multi_adamw_clip_ema_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                  float* const* ema, const int64_t* numel, int n_tensors, const float* sumsq, float max_norm,
                                  float grad_div, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                  float ema_decay, const float* hyper, const int32_t* nonfinite, srk_stream_t stream) {
  const void* const* lists[5] = {(const void* const*)params, (const void* const*)grads, (const void* const*)exp_avg,
                                 (const void* const*)exp_avg_sq, (const void* const*)ema};
  const char* names[5] = {"params", "grads", "exp_avg", "exp_avg_sq", "ema"};
  const int rc = check_tensor_list(__func__, lists, names, 5, numel, n_tensors);
  if (rc != SRK_OK) return rc;
  SRK_REQUIRE(max_norm <= 0.f || sumsq != nullptr, SRK_E_NULL, "multi adamw ema: clipping needs sumsq");
  SRK_REQUIRE(step >= 1 && grad_div > 0.f, SRK_E_SHAPE, "multi adamw ema: step=%d grad_div=%f", step, grad_div);
  SRK_REQUIRE(ema_decay >= 0.f && ema_decay < 1.f, SRK_E_SHAPE, "multi adamw ema: ema_decay=%g (0 <= decay < 1)", (double)ema_decay);
  return srk_launch_multi_adamw_ema(params, grads, exp_avg, exp_avg_sq, ema, (const long long*)numel, n_tensors, sumsq, nonfinite, hyper,
                                    max_norm, grad_div, lr, beta1, beta2, eps, weight_decay, step, ema_decay, (hipStream_t)stream);
}

int srk_adamw_hyper(float lr, float beta1, float beta2, int step, float* out3) {
  REQ_PTR(out3);
  SRK_REQUIRE(step >= 1, SRK_E_SHAPE, "adamw_hyper: step=%d", step);
  out3[0] = lr;
  adamw_bias_corrections(beta1, beta2, step, &out3[1], &out3[2]);
  return SRK_OK;
}

}  // extern "C"
