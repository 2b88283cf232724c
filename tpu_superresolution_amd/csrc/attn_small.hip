// (Shifted-)window attention, forward, for SMALL windows: ws x ws with ws = 2 .. 7 (N = ws * ws <= 49 tokens), for gfx950
// (v_mfma_f32_16x16x32_bf16, fp32 softmax).  Reference: WindowAttention.forward network_swinir.py:114-145 plus the roll /
// window_partition / window_reverse of SwinTransformerBlock.forward :240-279; the shift mask is calculate_mask :216-237 with
// shift = ws // 2, evaluated arithmetically from region labels (region3 of attn_common.h).
//
// q, k, v are read straight from the qkv projection's output in raster token order ([T][ldq] bf16, head h at columns
// which * CA + 32 h .. +31, head_dim zero-padded to 32, q NOT pre-scaled): roll + partition are folded into the row addresses of
// the loads, reverse + the inverse roll into the rows of the store.  The bias comes from the relative_position_bias_table parameter
// itself ([(2 ws - 1)^2][nH] fp32): the head's column is staged in LDS and indexed in closed form,
// (yq - yk + ws - 1)(2 ws - 1) + (xq - xk + ws - 1)  (network_swinir.py:89-103).
//
// A window is padded to 16 NT keys (NT = 2 for N <= 32, else 4) and to 16-query tiles.  Unlike the DAT / OCA zero-vector
// convention of attn256.hip, padded KEYS ARE EXCLUDED: they take no part in the row max and their probability is exactly 0 (their
// V rows in LDS are zero, so 0 * V adds nothing).  Padded query rows are computed from clamped indices and never stored; every real
// query sees at least its own key (same region), so row maxima stay finite.
//
// One workgroup per window, one wave per head (heads beyond the wave count are walked in rounds).  Per (window, head) the wave
//   holds the K fragments in registers (A operand of S^T = K Q^T: lane (r16, g) = K[key 16 j + r16][8 g .. 8 g + 7], one 16-byte
//     load of a 64-byte head row per lane),
//   stages V (zero rows for padded keys) and the head's bias column in a wave-private LDS region,
//   then per 16-query tile: S^T (NT MFMAs; a lane holds, for its query r16, keys 16 j + 4 g + 0..3), scale + bias + mask, softmax
//   with the row max / sum over the four 16-lane rows (permlane swaps), O^T = V^T P^T with P straight from the accumulators as the B
//   operand and V^T from LDS through the transposing read (ds_read_b64_tr_b16) -- the same operand maps as attn256.hip.
#include <hip/hip_runtime.h>

#include "attn_common.h"
#include "kernels.h"

namespace {

constexpr int KP = 40;          // LDS row pitch (elements) of the V tile: 80-byte rows, 16-byte aligned
constexpr int MAX_WAVES = 8;    // waves (= heads in flight) per workgroup

struct SmallParams {
  const bf16_t* qkv;   // [T][ldq]
  bf16_t* out;         // [T][ldo]
  const float* table;  // [(2 ws - 1)^2][nH]
  int ldq, ldo, CA;
  int B, H, W, shift, nH, nWh, nWw;
  float scale;
};

template <int WS>
__global__ __launch_bounds__(64 * MAX_WAVES) void win_small_attn_fwd_kernel(const SmallParams p) {
  constexpr int N = WS * WS;
  constexpr int NT = N > 32 ? 4 : 2;                   // key tiles of 16 (even: the P.V product takes two per K step)
  constexpr int NK = 16 * NT;
  constexpr int QT = (N + 15) / 16;                    // query tiles of 16
  constexpr int TW = 2 * WS - 1;
  constexpr int TR = TW * TW;                          // bias table rows
  constexpr int TRP = (TR + 3) & ~3;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int nwave = blockDim.x >> 6;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r16 = lane & 15, g = lane >> 4;
  bf16_t* Vs = reinterpret_cast<bf16_t*>(smem) + wave * NK * KP;                                // [NK][KP]
  float* tab = reinterpret_cast<float*>(reinterpret_cast<bf16_t*>(smem) + nwave * NK * KP) + wave * TRP;

  const int nW = p.nWh * p.nWw;
  const int b = blockIdx.x / nW, w = blockIdx.x - b * nW;
  const int wy = w / p.nWw, wx = w - wy * p.nWw;
  const long long tok0 = (long long)b * p.H * p.W;
  const int sh = p.shift;
  // interior windows of a shifted map have one region label throughout: only the last window row / column is masked
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
  const bf16x8_t zero8 = bf16x8_t{0, 0, 0, 0, 0, 0, 0, 0};

  for (int h0 = 0; h0 < p.nH; h0 += nwave) {          // trip count uniform over the workgroup
    const int h = h0 + wave;
    const bool act = h < p.nH;                         // uniform over the wave
    if (h0 > 0) __syncthreads();                       // the previous round's LDS reads are done
    if (act) {
      for (int idx = lane; idx < NK * 4; idx += 64) {  // V rows (zero for padded keys): 4 lanes x 16 B per 64-byte head row
        const int row = idx >> 2, ch = idx & 3;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (row < N) v = *reinterpret_cast<const uint4*>(p.qkv + token(row) * p.ldq + 2 * p.CA + h * 32 + 8 * ch);
        *reinterpret_cast<uint4*>(Vs + row * KP + 8 * ch) = v;
      }
      for (int i = lane; i < TR; i += 64) tab[i] = p.table[(long long)i * p.nH + h];
    }
    __syncthreads();
    if (!act) continue;

    bf16x8_t kf[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const int kl = 16 * j + r16;
      kf[j] = kl < N ? *reinterpret_cast<const bf16x8_t*>(p.qkv + token(kl) * p.ldq + p.CA + h * 32 + 8 * g) : zero8;
    }

#pragma unroll 1
    for (int qt = 0; qt < QT; ++qt) {
      const int ql = 16 * qt + r16;
      const bool qreal = ql < N;
      const int qc = qreal ? ql : N - 1;               // padded query rows: clamped indices (computed, never stored)
      const int qy = qc / WS, qx = qc - qy * WS;
      const long long qtok = token(qc);
      const int qlab = need_mask ? label(qc) : 0;
      const bf16x8_t qf = qreal ? *reinterpret_cast<const bf16x8_t*>(p.qkv + qtok * p.ldq + h * 32 + 8 * g) : zero8;

      f32x4_t s[NT];
#pragma unroll
      for (int j = 0; j < NT; ++j) s[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[j], qf, f32x4_t{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);

      // s[j][e] = S[query ql][key 16 j + 4 g + e]
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

      // O^T = V^T P^T: B operand K slots (g, 0..7) = keys 32 jj + 4 g + 0..3 and 32 jj + 16 + 4 g + 0..3 of this lane's query
      f32x4_t o[2] = {f32x4_t{0.f, 0.f, 0.f, 0.f}, f32x4_t{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
      for (int jj = 0; jj < NT / 2; ++jj) {
        const uint2 lo = pack_bf4(s[2 * jj][0], s[2 * jj][1], s[2 * jj][2], s[2 * jj][3]);
        const uint2 hi = pack_bf4(s[2 * jj + 1][0], s[2 * jj + 1][1], s[2 * jj + 1][2], s[2 * jj + 1][3]);
        typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
        const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, u32x4{lo.x, lo.y, hi.x, hi.y});
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const bf16x4_t a0 = lds_tr_read(tr_addr(Vs, KP, 32 * jj + 4 * g, 16 * dt, lane));
          const bf16x4_t a1 = lds_tr_read(tr_addr(Vs, KP, 32 * jj + 16 + 4 * g, 16 * dt, lane));
          const bf16x8_t vf = bf16x8_t{a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf, o[dt], 0, 0, 0);
        }
      }
      // lane holds O[query ql][d = 16 dt + 4 g + 0..3]
      if (qreal) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
          *reinterpret_cast<uint2*>(p.out + qtok * p.ldo + h * 32 + 16 * dt + 4 * g) =
              pack_bf4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
      }
    }
  }
}

template <int WS>
int launch(const SmallParams& p, hipStream_t stream) {
  constexpr int N = WS * WS;
  constexpr int NK = 16 * (N > 32 ? 4 : 2);
  constexpr int TRP = ((2 * WS - 1) * (2 * WS - 1) + 3) & ~3;
  const int nwave = p.nH < MAX_WAVES ? p.nH : MAX_WAVES;
  const size_t lds = (size_t)nwave * (NK * KP * sizeof(bf16_t) + TRP * sizeof(float));    // <= 8 x 5.8 KB
  const long long grid = (long long)p.B * p.nWh * p.nWw;
  SRK_REQUIRE(grid > 0 && grid < (1LL << 31), SRK_E_SHAPE, "win_small attention: bad grid %lld", grid);
  hipLaunchKernelGGL(win_small_attn_fwd_kernel<WS>, dim3((unsigned)grid), dim3(64 * nwave), lds, stream, p);
  return srk_check_launch("win_small_attn_fwd");
}

}  // namespace

int srk_win_small_attention_fwd(const uint16_t* qkv, int ldq, int CA, const float* table, uint16_t* out, int ldo, int B, int H, int W,
                                int ws, int shift, int num_heads, float scale, srk_stream_t stream) {
  SRK_REQUIRE(qkv && table && out, SRK_E_NULL, "win_small attention: null pointer");
  SRK_REQUIRE(ws >= 2 && ws <= 7, SRK_E_UNSUPPORTED, "win_small attention: window_size %d is outside 2..7", ws);
  SRK_REQUIRE(B > 0 && H > 0 && W > 0 && H % ws == 0 && W % ws == 0, SRK_E_SHAPE,
              "win_small attention: the %dx%d map must be a multiple of the window %d", H, W, ws);
  SRK_REQUIRE(shift >= 0 && shift < ws, SRK_E_SHAPE, "shift_size must in 0-window_size");
  SRK_REQUIRE(srk_qkv_layout_ok(num_heads, CA, ldq, ldo, 4), SRK_E_SHAPE, "win_small attention: bad layout nH=%d CA=%d ldq=%d ldo=%d", num_heads, CA, ldq, ldo);
  SRK_REQUIRE(srk_aligned(qkv, 16) && srk_aligned(out, 8), SRK_E_ALIGN,
              "win_small attention: qkv must be 16-byte and out 8-byte aligned");
  SmallParams p;
  p.qkv = reinterpret_cast<const bf16_t*>(qkv); p.out = reinterpret_cast<bf16_t*>(out); p.table = table;
  p.ldq = ldq; p.ldo = ldo; p.CA = CA; p.B = B; p.H = H; p.W = W; p.shift = shift; p.nH = num_heads;
  p.nWh = H / ws; p.nWw = W / ws; p.scale = scale;
  const hipStream_t st = (hipStream_t)stream;
  switch (ws) {
    case 2: return launch<2>(p, st);
    case 3: return launch<3>(p, st);
    case 4: return launch<4>(p, st);
    case 5: return launch<5>(p, st);
    case 6: return launch<6>(p, st);
    default: return launch<7>(p, st);
  }
}
