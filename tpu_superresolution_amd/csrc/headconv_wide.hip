// Backward of a wide one-step image head: the 3x3 conv, pad 1, of UpsampleOneStep ('pixelshuffledirect') with 17 .. 64 output channels
// (SwinIR-light x3: 27, x4: 48; x8 gray: 64), padded to CoP = 32, 48 or 64.  The narrow family (misc.hip / convwgrad.hip, CoP 4 or 16)
// stays as it is; this file is what srk_widehead_grad_prep / _wgrad / _dgrad (include/srk.h) run.
//
// Data contracts (those of the narrow family): x bf16 NHWC [B*H*W][CinP], gy fp32 [B*H*W][CoP], parameters fp32 [Co][Cin][3][3],
// Cin <= CinP, CinP % 64 == 0, CinP <= 256.  Pixels are walked by their FLAT index p = (b*H + y)*W + x: the tap (ky, kx) of pixel p is
// the flat pixel p + (ky-1)*W + (kx-1) whenever (y + ky-1, x + kx-1) lies inside the image, and a per-pixel 9-bit mask says when it
// does.  So no kernel here depends on W being a multiple of anything, and an odd pixel count only leaves part of the last tile unused.
//
// Arithmetic: the fp32-INPUT matrix instruction (v_mfma_f32_32x32x2_f32 in the dgrad, v_mfma_f32_16x16x4_f32 in the wgrad).  It is
// bit for bit a k-ordered fmaf chain in fp32, so gy and the weights are used as the fp32 values they are: there is NO hi + lo split
// and the number of split products is 0 (the bf16 x of the wgrad converts to fp32 exactly).  It runs at 1/16 of the bf16 rate, which
// at B = 32, 64 x 64, 60 -> 48 channels is a floor of about 46 us per launch -- the price of an exact fp32 gradient.
//
//   widehead_dgrad_kernel<COP>   dx[p][ci] = sum_tap sum_co gy[p - off(tap)][co] W[co][ci][tap]      GEMM M = pixels, N = CinP, K = 9 COP
//     one workgroup = 128 pixels x one 64-channel slice of ci (grid.y = CinP / 64); wave w owns pixels 32w .. 32w+31 and two 32x32
//     accumulators.  Per source row dy the 130-pixel segment of gy that the three taps of that row read is staged once
//     ([130][COP + 1] fp32, 33.8 KB at COP 64); the weights are staged per tap ([COP][64] fp32, 16 KB at COP 64), never whole.
//     LDS: 50.2 KB (COP 64), 37.8 KB (48), 25.4 KB (32), static.
//   widehead_wgrad_kernel<COP, ROLL>   dW[co][ci][tap] += sum_p x[p + off(tap)][ci] gy[p][co],  db[co] += sum_p gy[p][co]
//     one workgroup = one 64-channel slice of ci (grid.y) x a run of 64-pixel chunks (grid.x splits); wave w owns input channels
//     16w .. 16w+15 and 9 x COP/16 accumulators of 16x16 (144 registers at COP 64), summed over the whole run, then added to dW with
//     fp32 atomics: the accumulators go through LDS in the layout of dW so that every atomic instruction covers 256 contiguous bytes.
//     x lives in LDS as bf16 in a ring of 256 flat pixels (32 KB): ROLL (W <= 95) loads the window [p0 - W - 1, p0 + 64 + W] once and
//     then only the 64 new pixels per chunk -- x and gy are read once per run; wider images (ROLL = false, the fallback) reload the
//     three 66-pixel row segments of every chunk (x three times, gy once).  gy: one chunk [64][COP] fp32 (16 KB at COP 64).
//     LDS: 49.3 KB (COP 64), 45.2 KB (48), 41.1 KB (32): no ring of gy and a 16-channel epilogue overlay instead of the 64 KB ring that
//     COP = 64 would cost the narrow kernel's layout; two workgroups per CU (__launch_bounds__(256, 2): 256 registers).
#include <hip/hip_runtime.h>

#include "common.h"
#include "kernels.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

constexpr int DG_PIX = 128;            // pixels per dgrad workgroup
constexpr int DG_SEG = DG_PIX + 2;     // one row segment of gy with its one-pixel halo
constexpr int WG_CHUNK = 64;           // pixels per wgrad chunk
constexpr int WG_RING = 256;           // flat pixels the x ring holds
constexpr int WG_WMAX = (WG_RING - WG_CHUNK - 2) / 2;   // 95: widest image whose window 2 W + 66 fits the ring
constexpr int WG_MIN_CHUNKS = 4;       // a workgroup walks at least this many chunks when there are that many (fewer atomics)

// bit ky*3 + kx: pixel (y + sign*(ky-1), x + sign*(kx-1)) of the image that holds flat pixel p is inside it
__device__ __forceinline__ unsigned tap_mask(long long p, int H, int W, int sign) {
  const int x = (int)(p % W), y = (int)((p / W) % H);
  unsigned m = 0;
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int yy = y + sign * (t / 3 - 1), xx = x + sign * (t % 3 - 1);
    if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) m |= 1u << t;
  }
  return m;
}

template <int COP>
__global__ __launch_bounds__(256) void widehead_dgrad_kernel(const float* __restrict__ gy, const float* __restrict__ wgt,
                                                             bf16_t* __restrict__ dx, int H, int W, int Cin, int CinP, int Co,
                                                             long long npix) {
  constexpr int GS = COP + 1;                    // odd row stride: the 32 pixel lanes of an A read fall into 32 banks
  __shared__ float gl[DG_SEG * GS];
  __shared__ __attribute__((aligned(16))) float wl[COP * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long p0 = (long long)blockIdx.x * DG_PIX;
  const int ci0 = blockIdx.y * 64;
  const int j = wave * 32 + (lane & 31), kh = lane >> 5;
  const long long pm = p0 + j;
  const unsigned mask = pm < npix ? tap_mask(pm, H, W, -1) : 0u;      // the source of tap (ky, kx) is (y - (ky-1), x - (kx-1))
  f32x16_t acc0 = {}, acc1 = {};
  for (int tap = 0; tap < 9; ++tap) {
    const int ky = tap / 3, kx = tap % 3;
    __syncthreads();                             // the previous tap's reads of wl (and of gl, when the row changes) are done
    if (kx == 0) {                               // source row y - (ky-1): flat pixels p0 - (ky-1) W - 1 .. + 129
      const long long base = p0 - (long long)(ky - 1) * W - 1;
      for (int idx = tid; idx < DG_SEG * (COP / 4); idx += 256) {
        const int i = idx / (COP / 4), c4 = (idx % (COP / 4)) * 4;
        const long long q = base + i;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q >= 0 && q < npix) v = *reinterpret_cast<const float4*>(gy + q * COP + c4);
        float* d = gl + i * GS + c4;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
      }
    }
    for (int idx = tid; idx < COP * 64; idx += 256) {
      const int co = idx >> 6, ci = ci0 + (idx & 63);
      wl[idx] = (co < Co && ci < Cin) ? wgt[((long long)co * Cin + ci) * 9 + tap] : 0.f;
    }
    __syncthreads();
    const bool ok = (mask >> tap) & 1u;
    const float* arow = gl + (j + 2 - kx) * GS;  // q - base = j - (kx-1) + 1
    const float* bcol = wl + (lane & 31);
#pragma unroll 8
    for (int k2 = 0; k2 < COP / 2; ++k2) {
      const int k = 2 * k2 + kh;
      const float av = arow[k];
      const float a = ok ? av : 0.f;             // a select, not a product: what lies outside the image may be anything
      acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bcol[k * 64], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bcol[k * 64 + 32], acc1, 0, 0, 0);
    }
  }
  // C/D map of the 32x32 forms: column = lane & 31 (ci), row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5) (pixel)
  const int ci = ci0 + (lane & 31);
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const long long p = p0 + wave * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * kh;
    if (p >= npix) continue;
    dx[p * CinP + ci] = f2bf(ci < Cin ? acc0[reg] : 0.f);                  // pad channels: +0
    dx[p * CinP + ci + 32] = f2bf(ci + 32 < Cin ? acc1[reg] : 0.f);
  }
}

template <int COP, bool ROLL>
__global__ __launch_bounds__(256, 2) void widehead_wgrad_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gy,
                                                                float* __restrict__ dW, float* __restrict__ db, int H, int W, int Cin,
                                                                int CinP, int Co, long long npix, int chunks_per_wg) {
  constexpr int NT = COP / 16;
  constexpr int XR_FLOATS = WG_RING * 64 / 2;                              // the bf16 ring, counted in floats
  __shared__ __attribute__((aligned(16))) float sm[XR_FLOATS + WG_CHUNK * COP];
  __shared__ unsigned short msk[WG_CHUNK];
  static_assert(16 * 64 * 9 <= XR_FLOATS + WG_CHUNK * COP, "the epilogue overlay [16 co][64 ci][9] must fit the ring + gy");
  bf16_t* xr = reinterpret_cast<bf16_t*>(sm);                              // [WG_RING][64]
  float* gl = sm + XR_FLOATS;                                              // [WG_CHUNK][COP]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ci0 = blockIdx.y * 64;
  const long long nchunks = (npix + WG_CHUNK - 1) / WG_CHUNK;
  const long long c_begin = (long long)blockIdx.x * chunks_per_wg;
  const long long c_end = c_begin + chunks_per_wg < nchunks ? c_begin + chunks_per_wg : nchunks;
  if (c_begin >= c_end || ci0 >= Cin) return;                              // uniform over the workgroup
  const long long p_end = c_end * WG_CHUNK < npix ? c_end * WG_CHUNK : npix;
  f32x4_t acc[9][NT];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[t][n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.f;
  const int m_ci = wave * 16 + (lane & 15), kp = lane >> 4;
  for (long long ch = c_begin; ch < c_end; ++ch) {
    const long long p0 = ch * WG_CHUNK;
    __syncthreads();                                                       // the previous chunk's reads are done
    if constexpr (ROLL) {
      // window of this chunk: flat pixels p0 - W - 1 .. p0 + 64 + W; all but the last 64 are there already after the first chunk
      const long long lo = ch == c_begin ? p0 - W - 1 : p0 + W + 1;
      const int count = (int)(p0 + WG_CHUNK + W + 1 - lo);                 // 2 W + 66 <= WG_RING, then 64
      for (int idx = tid; idx < count * 8; idx += 256) {
        const long long q = lo + (idx >> 3);
        const int v8 = (idx & 7) * 8;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (q >= 0 && q < npix) v = *reinterpret_cast<const uint4*>(x + q * CinP + ci0 + v8);
        *reinterpret_cast<uint4*>(xr + (int)(q & (WG_RING - 1)) * 64 + v8) = v;
      }
    } else {
      for (int idx = tid; idx < 3 * (WG_CHUNK + 2) * 8; idx += 256) {      // slot = ky * 66 + i  <->  flat p0 + (ky-1) W - 1 + i
        const int slot = idx >> 3, v8 = (idx & 7) * 8;
        const long long q = p0 + (long long)(slot / (WG_CHUNK + 2) - 1) * W - 1 + slot % (WG_CHUNK + 2);
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (q >= 0 && q < npix) v = *reinterpret_cast<const uint4*>(x + q * CinP + ci0 + v8);
        *reinterpret_cast<uint4*>(xr + slot * 64 + v8) = v;
      }
    }
    for (int idx = tid; idx < WG_CHUNK * (COP / 4); idx += 256) {
      const int i = idx / (COP / 4), c4 = (idx % (COP / 4)) * 4;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (p0 + i < p_end) v = *reinterpret_cast<const float4*>(gy + (p0 + i) * COP + c4);
      *reinterpret_cast<float4*>(gl + i * COP + c4) = v;
    }
    if (tid < WG_CHUNK) msk[tid] = p0 + tid < p_end ? (unsigned short)tap_mask(p0 + tid, H, W, +1) : (unsigned short)0;
    __syncthreads();
    if (blockIdx.y == 0 && lane < COP) {                                   // db: wave w sums pixels 16w .. 16w+15 of the chunk
#pragma unroll 4
      for (int i = 0; i < 16; ++i) dbacc += gl[(wave * 16 + i) * COP + lane];
    }
    for (int ks = 0; ks < WG_CHUNK / 4; ++ks) {
      const int i = ks * 4 + kp;                                           // this lane's pixel of the k-step
      const unsigned m = msk[i];
      float b[NT];
#pragma unroll
      for (int n = 0; n < NT; ++n) b[n] = gl[i * COP + n * 16 + (lane & 15)];
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        int slot;
        if constexpr (ROLL) slot = (int)((p0 + i + (long long)(t / 3 - 1) * W + (t % 3 - 1)) & (WG_RING - 1));
        else slot = (t / 3) * (WG_CHUNK + 2) + i + t % 3;
        const float xv = bf2f(xr[slot * 64 + m_ci]);
        const float a = ((m >> t) & 1u) ? xv : 0.f;
#pragma unroll
        for (int n = 0; n < NT; ++n) acc[t][n] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[n], acc[t][n], 0, 0, 0);
      }
    }
  }
  if (blockIdx.y == 0 && lane < Co) atomicAdd(db + lane, dbacc);
  // C/D map of the 16x16 forms: column = lane & 15 (co), row = 4 (lane >> 4) + reg (ci).  Sixteen output channels at a time go through
  // LDS as [co][ci][tap], the layout of dW, whose rows [co][ci0 .. ci0+63][0 .. 8] are contiguous in memory.
  float* ep = sm;
  const int ncont = (Cin - ci0 < 64 ? Cin - ci0 : 64) * 9;
#pragma unroll
  for (int n = 0; n < NT; ++n) {
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) ep[((lane & 15) * 64 + wave * 16 + 4 * kp + reg) * 9 + t] = acc[t][n][reg];
    __syncthreads();
    for (int col = 0; col < 16; ++col) {
      const int co = n * 16 + col;
      if (co >= Co) break;
      float* dst = dW + ((long long)co * Cin + ci0) * 9;
      for (int idx = tid; idx < ncont; idx += 256) atomicAdd(dst + idx, ep[col * 576 + idx]);
    }
  }
}

template <int COP>
int launch_dgrad(const float* gy, const float* wgt, bf16_t* dx, int H, int W, int Cin, int CinP, int Co, long long npix,
                 hipStream_t stream) {
  const dim3 grid((unsigned)((npix + DG_PIX - 1) / DG_PIX), (unsigned)(CinP / 64));
  hipLaunchKernelGGL(widehead_dgrad_kernel<COP>, grid, dim3(256), 0, stream, gy, wgt, dx, H, W, Cin, CinP, Co, npix);
  return srk_check_launch("widehead_dgrad");
}

template <int COP>
int launch_wgrad(const bf16_t* x, const float* gy, float* dW, float* db, int H, int W, int Cin, int CinP, int Co, long long npix,
                 hipStream_t stream) {
  const int slices = CinP / 64;
  const long long nchunks = (npix + WG_CHUNK - 1) / WG_CHUNK;
  const long long target = 512 / slices;                                   // two workgroups per CU over the whole launch
  long long cpw = (nchunks + target - 1) / target;
  if (cpw < WG_MIN_CHUNKS) cpw = WG_MIN_CHUNKS;
  const dim3 grid((unsigned)((nchunks + cpw - 1) / cpw), (unsigned)slices);
  if (W <= WG_WMAX)
    hipLaunchKernelGGL((widehead_wgrad_kernel<COP, true>), grid, dim3(256), 0, stream, x, gy, dW, db, H, W, Cin, CinP, Co, npix, (int)cpw);
  else
    hipLaunchKernelGGL((widehead_wgrad_kernel<COP, false>), grid, dim3(256), 0, stream, x, gy, dW, db, H, W, Cin, CinP, Co, npix, (int)cpw);
  return srk_check_launch("widehead_wgrad");
}

SrkOpt g_wide_head_train{OPT_WIDE_HEAD_TRAIN, 0};

}  // namespace

void srk_wide_head_train_enable(int on) { g_wide_head_train = on ? 1 : 0; }
int srk_wide_head_train_enabled() { return g_wide_head_train; }

int srk_launch_widehead_dgrad(const float* gy, const float* wgt, bf16_t* dx, int B, int H, int W, int Cin, int CinP, int Co, int CoP,
                              hipStream_t stream) {
  SRK_REQUIRE(srk_widehead_conv_shape_ok(B, H, W, Cin, CinP, Co, CoP), SRK_E_SHAPE, "widehead dgrad: B=%d H=%d W=%d Cin=%d CinP=%d Co=%d CoP=%d",
              B, H, W, Cin, CinP, Co, CoP);
  const long long npix = (long long)B * H * W;
  if (CoP == 32) return launch_dgrad<32>(gy, wgt, dx, H, W, Cin, CinP, Co, npix, stream);
  if (CoP == 48) return launch_dgrad<48>(gy, wgt, dx, H, W, Cin, CinP, Co, npix, stream);
  return launch_dgrad<64>(gy, wgt, dx, H, W, Cin, CinP, Co, npix, stream);
}

int srk_launch_widehead_wgrad(const bf16_t* x, const float* gy, float* dW, float* db, int B, int H, int W, int Cin, int CinP, int Co,
                              int CoP, hipStream_t stream) {
  SRK_REQUIRE(srk_widehead_conv_shape_ok(B, H, W, Cin, CinP, Co, CoP), SRK_E_SHAPE, "widehead wgrad: B=%d H=%d W=%d Cin=%d CinP=%d Co=%d CoP=%d",
              B, H, W, Cin, CinP, Co, CoP);
  const long long npix = (long long)B * H * W;
  if (CoP == 32) return launch_wgrad<32>(x, gy, dW, db, H, W, Cin, CinP, Co, npix, stream);
  if (CoP == 48) return launch_wgrad<48>(x, gy, dW, db, H, W, Cin, CinP, Co, npix, stream);
  return launch_wgrad<64>(x, gy, dW, db, H, W, Cin, CinP, Co, npix, stream);
}

extern "C" {

int srk_widehead_grad_prep(const float* d_pred, float* gy, int B, int Cimg, int Hc, int Wc, int H, int W, int r, int CoP, float inv_range,
                           srk_stream_t stream) {
  SRK_REQUIRE(d_pred && gy, SRK_E_NULL, "widehead_grad_prep: null pointer");
  SRK_REQUIRE(srk_widehead_prep_shape_ok(B, Cimg, Hc, Wc, H, W, r, CoP), SRK_E_SHAPE,
              "widehead_grad_prep: B=%d Cimg=%d crop %dx%d H=%d W=%d r=%d CoP=%d (CoP 32, 48 or 64, Cimg*r*r <= CoP, crop inside %dx%d)", B, Cimg,
              Hc, Wc, H, W, r, CoP, H * r, W * r);
  SRK_REQUIRE(srk_aligned(gy, 16), SRK_E_ALIGN, "widehead_grad_prep: gy must be 16-byte aligned");
  return srk_launch_img_grad_prep(d_pred, gy, B, Cimg, Hc, Wc, H, W, r, CoP, inv_range, (hipStream_t)stream);
}

int srk_widehead_wgrad(const uint16_t* x, const float* gy, float* dw, float* db, int B, int H, int W, int Cin, int CinP, int Co, int CoP,
                       srk_stream_t stream) {
  SRK_REQUIRE(x && gy && dw && db, SRK_E_NULL, "widehead_wgrad: null pointer");
  SRK_REQUIRE(srk_widehead_conv_shape_ok(B, H, W, Cin, CinP, Co, CoP), SRK_E_SHAPE,
              "widehead_wgrad: B=%d H=%d W=%d Cin=%d CinP=%d Co=%d CoP=%d (CoP 32, 48 or 64, Co <= CoP, Cin <= CinP, CinP a multiple of 64, <= 256)",
              B, H, W, Cin, CinP, Co, CoP);
  SRK_REQUIRE(srk_aligned(x, 16) && srk_aligned(gy, 16), SRK_E_ALIGN, "widehead_wgrad: x and gy must be 16-byte aligned");
  return srk_launch_widehead_wgrad(x, gy, dw, db, B, H, W, Cin, CinP, Co, CoP, (hipStream_t)stream);
}

int srk_widehead_dgrad(const float* gy, const float* weight, uint16_t* dx, int B, int H, int W, int Cin, int CinP, int Co, int CoP,
                       srk_stream_t stream) {
  SRK_REQUIRE(gy && weight && dx, SRK_E_NULL, "widehead_dgrad: null pointer");
  SRK_REQUIRE(srk_widehead_conv_shape_ok(B, H, W, Cin, CinP, Co, CoP), SRK_E_SHAPE,
              "widehead_dgrad: B=%d H=%d W=%d Cin=%d CinP=%d Co=%d CoP=%d (CoP 32, 48 or 64, Co <= CoP, Cin <= CinP, CinP a multiple of 64, <= 256)",
              B, H, W, Cin, CinP, Co, CoP);
  SRK_REQUIRE(srk_aligned(gy, 16) && srk_aligned(dx, 16), SRK_E_ALIGN, "widehead_dgrad: gy and dx must be 16-byte aligned");
  return srk_launch_widehead_dgrad(gy, weight, dx, B, H, W, Cin, CinP, Co, CoP, (hipStream_t)stream);
}

}  // extern "C"
