// Backward of the small-window attention of attn_small.hip: ws x ws windows with ws = 2 .. 7 (N = ws * ws <= 49 tokens), for gfx950
// (v_mfma_f32_16x16x32_bf16, fp32 softmax and reductions).  Reference: WindowAttention.forward network_swinir.py:114-145 and the
// roll / window_partition / window_reverse of SwinTransformerBlock.forward :240-279, backwards.
//
//   S = scale q k^T + table[rpi] (+ mask),  P = softmax(S),  O = P v
//   dV = P^T dO,  dP = dO v^T,  dS = P (dP - rowsum(P dP)),  dq = scale dS k,  dk = scale dS^T q,  d table[rpi] += dS
//
// The forward's conventions hold throughout: q, k, v and dO are read in raster token order (roll + partition in the row addresses),
// head h at columns which * CA + 32 h, head_dim zero-padded to 32, q NOT pre-scaled; the bias is the table column indexed in closed
// form; the shift mask is arithmetic and applies to the last window row / column only; a window is padded to NK = 32 / 64 keys that
// are EXCLUDED from the softmax.  S and P are recomputed from the same bf16 operands with the forward's scale / bias / mask / exp2
// path.
//
// One 64-thread workgroup (one wave) per (window, head) -- the LDS tiles are private to the wave.  K, Q and dO of the window
// (NK rows, zero rows beyond N) are staged in LDS, the V and K row fragments stay in registers.  Two passes, as attn256_bwd.hip:
//   pass 1 (16 queries at a time; lane = query, registers = keys -- the forward's layout): S^T and dP^T, softmax, the row
//          statistics (max * log2e, 1 / sum, rowsum(P dP)) to LDS, dS; dq^T = K^T dS^T with dS^T from the accumulators as the B operand.
//          PADDED QUERIES (computed from clamped indices in the forward, never stored) get dS = 0 exactly, so that they add nothing
//          to dk, dv and d table.  d table: the dS tile goes to LDS as fp32 [16][NK] and every lane GATHERS the pairs of its own
//          table entries (lane, lane + 64, lane + 128) into registers -- no LDS float atomics;
//   pass 2 (16 keys at a time; lane = key, registers = queries): S and dP recomputed per pair of query tiles, P and dS rebuilt from
//          the saved row statistics, dV^T += dO^T P, dK^T += Q^T dS; padded keys have P = 0 and no row to store.
// Windows partition the tokens and the (window, head) workgroups partition the columns, so every element of d_qkv[0..T)[0..3 CA)
// is written exactly once (column blocks beyond num_heads * 32, if CA has any, by zero-writing workgroups).  The table gradient
// leaves as one dense partial column per workgroup (fully written: the scratch needs no zeroing), summed by
// win_small_table_reduce_kernel with one float atomic per element and 32-window slice.
#include <hip/hip_runtime.h>

#include "attn_common.h"
#include "kernels.h"

namespace {

constexpr int KP = 40;          // LDS row pitch (elements) of the bf16 tiles: 80-byte rows, 16-byte aligned (as attn_small.hip)

struct SmallBwdParams {
  const bf16_t* qkv;    // [T][ldq]
  const bf16_t* dout;   // [T][ldo] gradient of the attention output
  const float* table;   // [(2 ws - 1)^2][nH]
  bf16_t* dqkv;         // [T][ldq]
  float* tpart;         // [window][nH][(2 ws - 1)^2] partial table gradient
  int ldq, ldo, CA;
  int B, H, W, shift, nH, nHc, nWh, nWw;      // nHc = CA / 32 column blocks (>= nH)
  float scale;
};

// transposed fragment in accumulator k order: slots (g, i) = rows k0 + 4 g + i (i < 4) and k0 + 16 + 4 g + i - 4, columns c0 .. c0 + 15
__device__ __forceinline__ bf16x8_t tr_acc(const bf16_t* tile, int k0, int c0, int lane) {
  const int g = lane >> 4;
  return cat4(lds_tr_read(tr_addr(tile, KP, k0 + 4 * g, c0, lane)), lds_tr_read(tr_addr(tile, KP, k0 + 16 + 4 * g, c0, lane)));
}

template <int WS>
__global__ __launch_bounds__(64) void win_small_attn_bwd_kernel(const SmallBwdParams p) {
  constexpr int N = WS * WS;
  constexpr int NT = N > 32 ? 4 : 2;                   // key tiles of 16
  constexpr int NK = 16 * NT;                          // padded keys; the queries are padded to the same count in pass 2
  constexpr int QT = (N + 15) / 16;                    // query tiles of 16 that hold a real query
  constexpr int QP = NT / 2;                           // pairs of query tiles in pass 2
  constexpr int TW = 2 * WS - 1;
  constexpr int TR = TW * TW;                          // bias table rows
  constexpr int TRP = (TR + 3) & ~3;
  constexpr int NU = (TR + 63) / 64;                   // table entries per lane
  constexpr int DP = NK + 4;                           // pitch of the fp32 dS tile
  __shared__ __attribute__((aligned(16))) bf16_t Ks[NK * KP];
  __shared__ __attribute__((aligned(16))) bf16_t Qs[NK * KP];
  __shared__ __attribute__((aligned(16))) bf16_t Os[NK * KP];
  __shared__ __attribute__((aligned(16))) float stats[NK * 4];      // max * log2e, 1 / sum, rowsum(P dP)
  __shared__ __attribute__((aligned(16))) float dsl[16 * DP];       // dS of one query tile
  __shared__ float tab[TRP];
  const int lane = threadIdx.x;
  const int r16 = lane & 15, g = lane >> 4;

  const int h = blockIdx.x % p.nHc;
  const int wflat = blockIdx.x / p.nHc;
  const int nW = p.nWh * p.nWw;
  const int b = wflat / nW, w = wflat - b * nW;
  const int wy = w / p.nWw, wx = w - wy * p.nWw;
  const long long tok0 = (long long)b * p.H * p.W;
  const int sh = p.shift;
  const bool need_mask = sh > 0 && (wy == p.nWh - 1 || wx == p.nWw - 1);

  // window-local token l (< N) -> raster token: roll(-shift) + window_partition
  auto token = [&](int l) -> long long {
    const int ly = l / WS, lx = l - ly * WS;
    int y = wy * WS + ly + sh, x = wx * WS + lx + sh;
    if (y >= p.H) y -= p.H;
    if (x >= p.W) x -= p.W;
    return tok0 + (long long)y * p.W + x;
  };
  auto label = [&](int l) {
    const int ly = l / WS, lx = l - ly * WS;
    return region3(wy * WS + ly, p.H, WS, sh) * 3 + region3(wx * WS + lx, p.W, WS, sh);
  };

  if (h >= p.nH) {        // a column block of CA that holds no head: its gradient is zero (uniform over the workgroup)
    for (int idx = lane; idx < N * 12; idx += 64) {
      const int row = idx / 12, c = idx - row * 12;
      *reinterpret_cast<uint4*>(p.dqkv + token(row) * p.ldq + (c >> 2) * p.CA + h * 32 + 8 * (c & 3)) = make_uint4(0, 0, 0, 0);
    }
    return;
  }

  // ---- stage K, Q, dO (zero rows beyond N) and the head's table column ---------------------------------------------------------
  for (int idx = lane; idx < NK * 4; idx += 64) {
    const int row = idx >> 2, ch = idx & 3;
    uint4 kv = make_uint4(0, 0, 0, 0), qv = kv, ov = kv;
    if (row < N) {
      const long long t = token(row);
      const bf16_t* src = p.qkv + t * p.ldq + h * 32 + 8 * ch;
      qv = *reinterpret_cast<const uint4*>(src);
      kv = *reinterpret_cast<const uint4*>(src + p.CA);
      ov = *reinterpret_cast<const uint4*>(p.dout + t * p.ldo + h * 32 + 8 * ch);
    }
    *reinterpret_cast<uint4*>(Ks + row * KP + 8 * ch) = kv;
    *reinterpret_cast<uint4*>(Qs + row * KP + 8 * ch) = qv;
    *reinterpret_cast<uint4*>(Os + row * KP + 8 * ch) = ov;
  }
  for (int i = lane; i < TR; i += 64) tab[i] = p.table[(long long)i * p.nH + h];

  // row fragments of K and V: lane (r16, g) = row 16 j + r16, columns 8 g .. 8 g + 7 (A operand of pass 1, B operand of pass 2)
  const bf16x8_t zero8 = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};
  bf16x8_t kf[NT], vf[NT];
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int kl = 16 * j + r16;
    kf[j] = vf[j] = zero8;
    if (kl < N) {
      const bf16_t* src = p.qkv + token(kl) * p.ldq + p.CA + h * 32 + 8 * g;
      kf[j] = *reinterpret_cast<const bf16x8_t*>(src);
      vf[j] = *reinterpret_cast<const bf16x8_t*>(src + p.CA);
    }
  }
  __syncthreads();

  // =========================== pass 1: lane = query r16 of the tile, registers = keys 16 j + 4 g + e ===========================
  float tacc[NU];
#pragma unroll
  for (int u = 0; u < NU; ++u) tacc[u] = 0.f;
#pragma unroll 1
  for (int qt = 0; qt < QT; ++qt) {
    const int ql = 16 * qt + r16;
    const bool qreal = ql < N;
    const int qc = qreal ? ql : N - 1;                 // padded query rows: clamped indices, as the forward
    const int qy = qc / WS, qx = qc - qy * WS;
    const int qlab = need_mask ? label(qc) : 0;
    const bf16x8_t qf = *reinterpret_cast<const bf16x8_t*>(Qs + ql * KP + 8 * g);      // zero for a padded query
    const bf16x8_t of = *reinterpret_cast<const bf16x8_t*>(Os + ql * KP + 8 * g);

    f32x4_t s[NT], dp[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[j], qf, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      dp[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[j], of, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
    }
    // s[j][e] = S[query ql][key 16 j + 4 g + e], dp likewise
    float mx = -3.0e38f;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int kl = 16 * j + 4 * g + e;
        const bool kreal = kl < N;
        const int kc = kreal ? kl : N - 1;
        const int ky = kc / WS, kx = kc - ky * WS;
        float v = s[j][e] * p.scale + tab[(qy - ky + WS - 1) * TW + (qx - kx + WS - 1)];
        if (need_mask && label(kc) != qlab) v += -100.0f;      // network_swinir.py:235 (-100, not -inf)
        s[j][e] = v;
        if (kreal) mx = fmaxf(mx, v);
      }
    mx = xrow_max4(mx);
    const float mxl = mx * SRK_L2E;
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool kreal = 16 * j + 4 * g + e < N;
        const float pv = kreal ? __builtin_amdgcn_exp2f(s[j][e] * SRK_L2E - mxl) : 0.f;   // padded keys: probability exactly 0
        s[j][e] = pv;
        sum += pv;
      }
    const float inv = __builtin_amdgcn_rcpf(xrow_sum4(sum));
    float dl = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s[j][e] *= inv;
        dl += s[j][e] * dp[j][e];
      }
    dl = xrow_sum4(dl);
    if (g == 0) *reinterpret_cast<float4*>(stats + ql * 4) = make_float4(mxl, inv, dl, 0.f);
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
      for (int e = 0; e < 4; ++e) s[j][e] = qreal ? s[j][e] * (dp[j][e] - dl) : 0.f;      // dS; exactly 0 for a padded query
      *reinterpret_cast<float4*>(dsl + r16 * DP + 16 * j + 4 * g) = make_float4(s[j][0], s[j][1], s[j][2], s[j][3]);
    }
    f32x4_t aq[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int jj = 0; jj < NT / 2; ++jj) {
      const uint2 lo = pack_bf4(s[2 * jj][0], s[2 * jj][1], s[2 * jj][2], s[2 * jj][3]);
      const uint2 hi = pack_bf4(s[2 * jj + 1][0], s[2 * jj + 1][1], s[2 * jj + 1][2], s[2 * jj + 1][3]);
      const bf16x8_t dsf = __builtin_bit_cast(bf16x8_t, make_uint4(lo.x, lo.y, hi.x, hi.y));
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) aq[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_acc(Ks, 32 * jj, 16 * dt, lane), dsf, aq[dt], 0, 0, 0);
    }
    // aq[dt][e] = dq[query ql][d = 16 dt + 4 g + e]
    if (qreal) {
      bf16_t* qdst = p.dqkv + token(ql) * p.ldq + h * 32;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
        *reinterpret_cast<uint2*>(qdst + 16 * dt + 4 * g) =
            pack_bf4(aq[dt][0] * p.scale, aq[dt][1] * p.scale, aq[dt][2] * p.scale, aq[dt][3] * p.scale);
    }
    __syncthreads();      // the dS tile is in LDS
    // d table: entry i = (dy + ws - 1)(2 ws - 1) + (dx + ws - 1) collects dS[(qy, qx)][(qy - dy, qx - dx)] of the tile's real queries
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      const int i = lane + 64 * u;
      if (i < TR) {
        const int dy = i / TW - (WS - 1), dx = i - (i / TW) * TW - (WS - 1);
        float a = 0.f;
        for (int qq = 0; qq < 16; ++qq) {
          const int q = 16 * qt + qq;
          if (q >= N) break;
          const int y = q / WS, x = q - y * WS;
          const int ky = y - dy, kx = x - dx;
          if ((unsigned)ky < (unsigned)WS && (unsigned)kx < (unsigned)WS) a += dsl[qq * DP + ky * WS + kx];
        }
        tacc[u] += a;
      }
    }
    __syncthreads();      // before the next tile overwrites it
  }
  {
    float* tp = p.tpart + ((long long)wflat * p.nH + h) * TR;
#pragma unroll
    for (int u = 0; u < NU; ++u)
      if (lane + 64 * u < TR) tp[lane + 64 * u] = tacc[u];
  }

  // =========================== pass 2: lane = key r16 of tile j, registers = queries 16 qt + 4 g + e ===========================
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int kl = 16 * j + r16;
    const bool kreal = kl < N;
    const int kc = kreal ? kl : N - 1;
    const int ky = kc / WS, kx = kc - ky * WS;
    const int klab = need_mask ? label(kc) : 0;
    f32x4_t av[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
    f32x4_t ak[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int qp = 0; qp < QP; ++qp) {
      uint2 pl[2], dl2[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int qt = 2 * qp + u;
        const bf16x8_t qa = *reinterpret_cast<const bf16x8_t*>(Qs + (16 * qt + r16) * KP + 8 * g);
        const bf16x8_t oa = *reinterpret_cast<const bf16x8_t*>(Os + (16 * qt + r16) * KP + 8 * g);
        // sa[e] = q . k of (query 16 qt + 4 g + e, key kl);  da[e] = dO . v of the same pair
        const f32x4_t sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa, kf[j], f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        const f32x4_t da = __builtin_amdgcn_mfma_f32_16x16x32_bf16(oa, vf[j], f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
        float pv[4], dv[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int ql = 16 * qt + 4 * g + e;
          const bool real = kreal && ql < N;           // a padded query or key: P = dS = 0 (its statistics may not exist)
          const int qc = ql < N ? ql : N - 1;
          const int qy = qc / WS, qx = qc - qy * WS;
          const float4 st = *reinterpret_cast<const float4*>(stats + ql * 4);
          float v = sa[e] * p.scale + tab[(qy - ky + WS - 1) * TW + (qx - kx + WS - 1)];
          if (need_mask && label(qc) != klab) v += -100.0f;
          const float pe = __builtin_amdgcn_exp2f(v * SRK_L2E - st.x) * st.y;
          pv[e] = real ? pe : 0.f;                                             // P
          dv[e] = real ? pe * (da[e] - st.z) : 0.f;                            // dS
        }
        pl[u] = pack_bf4(pv[0], pv[1], pv[2], pv[3]);
        dl2[u] = pack_bf4(dv[0], dv[1], dv[2], dv[3]);
      }
      // B operands over the 32 queries of the pair in accumulator k order; A = dO^T / Q^T by transposing reads in that order
      const bf16x8_t pfb = __builtin_bit_cast(bf16x8_t, make_uint4(pl[0].x, pl[0].y, pl[1].x, pl[1].y));
      const bf16x8_t dfb = __builtin_bit_cast(bf16x8_t, make_uint4(dl2[0].x, dl2[0].y, dl2[1].x, dl2[1].y));
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        av[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_acc(Os, 32 * qp, 16 * dt, lane), pfb, av[dt], 0, 0, 0);
        ak[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(tr_acc(Qs, 32 * qp, 16 * dt, lane), dfb, ak[dt], 0, 0, 0);
      }
    }
    // av[dt][e] = dv[key kl][d = 16 dt + 4 g + e], ak likewise (dk = scale dS^T q)
    if (kreal) {
      bf16_t* dst = p.dqkv + token(kl) * p.ldq + h * 32;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        *reinterpret_cast<uint2*>(dst + p.CA + 16 * dt + 4 * g) =
            pack_bf4(ak[dt][0] * p.scale, ak[dt][1] * p.scale, ak[dt][2] * p.scale, ak[dt][3] * p.scale);
        *reinterpret_cast<uint2*>(dst + 2 * p.CA + 16 * dt + 4 * g) = pack_bf4(av[dt][0], av[dt][1], av[dt][2], av[dt][3]);
      }
    }
  }
}

// d table[i][h] += sum over the windows of the partial columns of head h: blockIdx.z takes a 32-window slice and adds its sum with one
// float atomic per element (the pattern of win256_table_reduce_kernel)
__global__ __launch_bounds__(256) void win_small_table_reduce_kernel(const float* __restrict__ tpart, float* __restrict__ dtable, long long nwin,
                                                                      int nH, int rows) {
  const int i = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y;
  if (i >= rows) return;
  const long long w0 = (long long)blockIdx.z * 32, w1 = min(nwin, w0 + 32);
  const float* src = tpart + (long long)h * rows + i;
  const long long stride = (long long)nH * rows;
  float a = 0.f;
  long long wdx = w0;
  for (; wdx + 8 <= w1; wdx += 8) {
    float v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = src[(wdx + u) * stride];
#pragma unroll
    for (int u = 0; u < 8; ++u) a += v[u];
  }
  for (; wdx < w1; ++wdx) a += src[wdx * stride];
  atomicAdd(dtable + (long long)i * nH + h, a);
}

template <int WS>
int launch_bwd(const SmallBwdParams& p, hipStream_t stream) {
  const long long grid = (long long)p.B * p.nWh * p.nWw * p.nHc;
  SRK_REQUIRE(grid > 0 && grid < (1LL << 31), SRK_E_SHAPE, "win_small attention backward: bad grid %lld", grid);
  hipLaunchKernelGGL(win_small_attn_bwd_kernel<WS>, dim3((unsigned)grid), dim3(64), 0, stream, p);
  return srk_check_launch("win_small_attn_bwd");
}

}  // namespace

size_t srk_win_small_attention_bwd_scratch(int B, int H, int W, int ws, int num_heads) {
  if (B <= 0 || H <= 0 || W <= 0 || num_heads <= 0 || ws < 2 || ws > 7) return 0;
  const size_t nwin = (size_t)B * (H / ws) * (W / ws);
  const size_t bytes = nwin * (size_t)num_heads * (size_t)((2 * ws - 1) * (2 * ws - 1)) * sizeof(float);
  return (bytes + 255) / 256 * 256;
}

int srk_win_small_attention_bwd(const uint16_t* qkv, int ldq, int CA, const float* table, const uint16_t* d_out, int ldo, uint16_t* d_qkv,
                                float* d_table, void* scratch, int B, int H, int W, int ws, int shift, int num_heads, float scale,
                                srk_stream_t stream) {
  SRK_REQUIRE(qkv && table && d_out && d_qkv && d_table, SRK_E_NULL, "win_small attention backward: null pointer");
  SRK_REQUIRE(ws >= 2 && ws <= 7, SRK_E_UNSUPPORTED, "win_small attention backward: window_size %d is outside 2..7", ws);
  SRK_REQUIRE(B > 0 && H > 0 && W > 0 && H % ws == 0 && W % ws == 0, SRK_E_SHAPE,
              "win_small attention backward: the %dx%d map must be a multiple of the window %d", H, W, ws);
  SRK_REQUIRE(shift >= 0 && shift < ws, SRK_E_SHAPE, "shift_size must in 0-window_size");
  SRK_REQUIRE(srk_qkv_layout_ok(num_heads, CA, ldq, ldo, 8), SRK_E_SHAPE, "win_small attention backward: bad layout nH=%d CA=%d ldq=%d ldo=%d", num_heads, CA, ldq, ldo);
  SRK_REQUIRE(scratch || srk_win_small_attention_bwd_scratch(B, H, W, ws, num_heads) == 0, SRK_E_NULL,
              "win_small attention backward: null scratch (srk_win_small_attention_bwd_scratch bytes)");
  SRK_REQUIRE(srk_aligned(qkv, 16) && srk_aligned(d_out, 16) && srk_aligned(d_qkv, 16) && srk_aligned(scratch, 16) && srk_aligned(table, 4) &&
                  srk_aligned(d_table, 4),
              SRK_E_ALIGN, "win_small attention backward: qkv, d_out, d_qkv and scratch must be 16-byte, table and d_table 4-byte aligned");
  SmallBwdParams p;
  p.qkv = reinterpret_cast<const bf16_t*>(qkv); p.dout = reinterpret_cast<const bf16_t*>(d_out); p.table = table;
  p.dqkv = reinterpret_cast<bf16_t*>(d_qkv); p.tpart = static_cast<float*>(scratch);
  p.ldq = ldq; p.ldo = ldo; p.CA = CA; p.B = B; p.H = H; p.W = W; p.shift = shift; p.nH = num_heads; p.nHc = CA / 32;
  p.nWh = H / ws; p.nWw = W / ws; p.scale = scale;
  const hipStream_t st = (hipStream_t)stream;
  const long long nwin = (long long)B * p.nWh * p.nWw;
  const int rows = (2 * ws - 1) * (2 * ws - 1);
  const long long nz = (nwin + 31) / 32;
  SRK_REQUIRE(nz <= 65535, SRK_E_SHAPE, "win_small attention backward: %lld windows are more than the table reduction takes", nwin);
  int rc;
  switch (ws) {
    case 2: rc = launch_bwd<2>(p, st); break;
    case 3: rc = launch_bwd<3>(p, st); break;
    case 4: rc = launch_bwd<4>(p, st); break;
    case 5: rc = launch_bwd<5>(p, st); break;
    case 6: rc = launch_bwd<6>(p, st); break;
    default: rc = launch_bwd<7>(p, st); break;
  }
  if (rc) return rc;
  hipLaunchKernelGGL(win_small_table_reduce_kernel, dim3((rows + 255) / 256, num_heads, (unsigned)nz), dim3(256), 0, st, p.tpart,
                     d_table, nwin, num_heads, rows);
  return srk_check_launch("win_small_table_reduce");
}
