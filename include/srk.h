/* srk -- super-resolution kernels for AMD MI355X (gfx950): the C ABI of libsrk.so.
 *
 * This is the drop-in boundary of the MI355X-native SwinIR path.  The reference
 * (ViacheslavTimofeev/tpu_superresolution) has no FFI: its boundary is the Python module
 * modules/network_swinir.py (constructor + forward + state_dict) and the training step in
 * modules/finetune_swinir.py.  Each entry point below names the reference code it replaces.
 * The Python side (tpu_superresolution_amd/) binds these with ctypes; see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a raw DEVICE address (tensor.data_ptr()); the caller owns all memory,
 *     kernels never allocate; `stream` is a hipStream_t (0 = default stream);
 *   - all work is enqueued asynchronously on `stream`; no entry point synchronises;
 *   - return value 0 (SRK_OK) or a negative SRK_E_* code; the message of the last error of the
 *     calling thread is returned by srk_last_error();
 *   - "bf16" is raw bfloat16 bits (uint16_t); token tensors use channels padded to a multiple of
 *     64 ("CP"); pad columns are zero.
 */
#ifndef SRK_H_
#define SRK_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SRK_OK 0
#define SRK_E_SHAPE (-1)
#define SRK_E_NULL (-2)
#define SRK_E_UNSUPPORTED (-3)
#define SRK_E_LAUNCH (-4)
#define SRK_E_ALIGN (-5)
#define SRK_E_STATE (-6)

typedef void* srk_stream_t;

const char* srk_version(void);
const char* srk_last_error(void);

/* ---- bit-exact index operations (stand-alone; elem_bytes in {2,4,8}) ------------------------- */
/* window_partition  network_swinir.py:33-45   x [B,H,W,C] -> out [B*nW, ws, ws, C] */
int srk_window_partition(const void* x, void* out, int B, int H, int W, int C, int ws, int elem_bytes, srk_stream_t stream);
/* window_reverse    network_swinir.py:48-62   windows [B*nW, ws, ws, C] -> out [B,H,W,C] */
int srk_window_reverse(const void* windows, void* out, int B, int H, int W, int C, int ws, int elem_bytes, srk_stream_t stream);
/* torch.roll(x, shifts=(sh,sw), dims=(1,2))  network_swinir.py:249-252, :269-272 */
int srk_roll2d(const void* x, void* out, int B, int H, int W, int C, int sh, int sw, int elem_bytes, srk_stream_t stream);
/* nn.PixelShuffle(r) on NCHW   network_swinir.py:585,588,609   x [B,C*r*r,H,W] -> out [B,C,H*r,W*r] */
int srk_pixel_shuffle(const void* x, void* out, int B, int C, int H, int W, int r, int elem_bytes, srk_stream_t stream);
/* SwinTransformerBlock.calculate_mask  network_swinir.py:216-237   mask fp32 [nW, ws*ws, ws*ws] in {0,-100} */
int srk_shift_mask(float* mask, int H, int W, int ws, int shift, srk_stream_t stream);
/* relative_position_index  network_swinir.py:92-103   out int64 [ws*ws, ws*ws] */
int srk_relative_position_index(int64_t* out, int ws, srk_stream_t stream);

/* ---- building-block kernels (internal layouts; used by the executor and by the parity tests) -- */
typedef struct {
  int H, W;     /* token grid (multiples of 8) */
  int shift;    /* 0 or 4 (window 8) */
} srk_win_geom;

/* nn.LayerNorm over C (eps 1e-5)  network_swinir.py:199,205,519-528,725.  x fp32 [rows][CP]; outputs
 * y_bf16 / y_f32 [rows][CP] (either may be null), mean/rstd fp32 [rows] (may be null).  If geom is
 * non-null the output is in WINDOW order: row m reads token roll+partition(m) (:249-256). */
int srk_layernorm_fwd(const float* x, const float* gamma, const float* beta, uint16_t* y_bf16, float* y_f32,
                      float* mean, float* rstd, int rows, int C, int CP, const srk_win_geom* geom, srk_stream_t stream);
/* softmax(q k^T + rel-pos-bias + shift-mask) v   network_swinir.py:124-142.
 * qkv bf16 [3][B_][nH][64][32] (q pre-scaled), bias_dense fp32 [nH][64][64], out bf16 [B_*64][nH*32]. */
int srk_window_attention_fwd(const uint16_t* qkv, const float* bias_dense, uint16_t* out, int64_t B_, int nH,
                             const srk_win_geom* geom, srk_stream_t stream);
/* gradient of the above.  d_out bf16 [B_*64][nH*32]; d_qkv bf16 [B_*64][3*nH*32] (columns which,h,d);
 * d_table fp32 [225][nH] is ACCUMULATED; slab = scratch of srk_window_attention_bwd_scratch() bytes, fully written before it is
 * read (needs no zeroing).  Every element of d_qkv is written (columns head_dim .. 31 of a head come out 0 when they are 0 in qkv
 * and d_out). */
int srk_window_attention_bwd(const uint16_t* qkv, const float* bias_dense, const uint16_t* d_out, uint16_t* d_qkv,
                             float* d_table, void* slab, int64_t B_, int nH, float scale, const srk_win_geom* geom,
                             srk_stream_t stream);
size_t srk_window_attention_bwd_scratch(int64_t B_, int nH);
/* The same gradient with q/k/v RE-PROJECTED from the saved LayerNorm output and the gradient of the output projection folded in
 * (csrc/attn_bwd_fused.hip; classical width only: nH = 6, head_dim padded to 32, C padded to 192, B_ >= number of CUs; anything
 * else returns SRK_E_UNSUPPORTED).  network_swinir.py:121-143 backwards: xn bf16 [B_*64][lda] = norm1 output in window order,
 * w_qkv bf16 [576][192] / b_qkv fp32 [576] (packed, q rows first, heads padded 30 -> 32), d_x1 bf16 [B_*64][ldg] = gradient of
 * the attention branch output in window order, w_proj_t bf16 [192 attention channel][192 channel] (d attn_out = d_x1 . w_proj_t^T),
 * d_qkv bf16 [B_*64][576]; d_table fp32 [225][6] is ACCUMULATED; slab = scratch of ..._bwd_fused_scratch() bytes. */
int srk_window_attention_bwd_fused(const uint16_t* xn, int lda, const uint16_t* w_qkv, const float* b_qkv, float scale,
                                   const uint16_t* d_x1, int ldg, const uint16_t* w_proj_t, const float* bias_dense, uint16_t* d_qkv,
                                   float* d_table, void* slab, int64_t B_, int nH, const srk_win_geom* geom, srk_stream_t stream);
size_t srk_window_attention_bwd_fused_scratch(int64_t B_, int nH);
/* dense bias [nH][64][64] from table [225][nH]   network_swinir.py:127-129 */
int srk_rel_pos_bias_expand(const float* table, float* bias_dense, int nH, srk_stream_t stream);
/* y[M][N] = a[M][K] . w[N][K]^T + bias  (bf16 in, fp32 accumulate, bf16 out); K % 64 == 0, N % 64 == 0 */
int srk_linear_bf16(const uint16_t* a, const uint16_t* w, const float* bias, uint16_t* y, int M, int N, int K, srk_stream_t stream);
/* dw[N][K] += y[M][N]^T . x[M][K] ; db[N] += colsum(y)   (bf16 in, fp32 out, accumulating; db may be null).  Any M > 0 (rows beyond M are
 * never read); N % 64 == 0, K % 64 == 0 (else SRK_E_SHAPE); y and x 16-byte aligned (else SRK_E_ALIGN). */
int srk_linear_wgrad_bf16(const uint16_t* y, const uint16_t* x, float* dw, float* db, int M, int N, int K, srk_stream_t stream);
/* Up to four of these with the same M as ONE launch (the four linear layers of a transformer block: the launch then fills the chip with
 * few row splits per tile).  Problems of one TILE CLASS go out together -- the class of a problem is (c(N), c(K)) with c(v) = 3 if v % 192 == 0,
 * else 2 if v % 128 == 0, else 1 (the tile is 64 c(N) x 64 c(K)); a list that mixes classes is launched one problem after the other.
 * ldy / ldx: row strides in elements (0: N / K).  dw [N][K] and db [N] (or null) are ACCUMULATED, as srk_linear_wgrad_bf16.
 * Checked on the host before any launch: SRK_E_SHAPE for count outside 1..4, M <= 0, N or K not a positive multiple of 64, ldy < N, ldx < K;
 * SRK_E_NULL for a null problems / y / x / dw; SRK_E_ALIGN for y or x not 16-byte aligned and for ldy % 8 != 0 or ldx % 8 != 0 (the kernels
 * read 16-byte pieces at y + m * ldy and x + m * ldx). */
typedef struct {
  const void* y; int ldy;      /* bf16 [M][ldy]: gradient of the layer output */
  const void* x; int ldx;      /* bf16 [M][ldx]: layer input */
  float* dw; float* db;
  int N, K;
} srk_wgrad_problem;
int srk_linear_wgrad_multi_bf16(const srk_wgrad_problem* problems, int count, int M, srk_stream_t stream);
/* 3x3/s1/p1 conv on NHWC bf16 [B][H][W][CinP] with packed weights [N][9*CinP] (tap-major), + bias -> bf16 NHWC [..][N] */
int srk_conv3x3_bf16(const uint16_t* x, const uint16_t* w, const float* bias, uint16_t* y, int B, int H, int W, int CinP, int N,
                     srk_stream_t stream);
/* dw[N][9*CinP] += conv weight gradient (y = d output NHWC bf16 [..][N], x = input NHWC bf16 [..][CinP]); db += sum y (db may be null).
 * dw is tap-major: column ((dy + 1) * 3 + (dx + 1)) * CinP + ci.  B, H, W > 0, N % 64 == 0, CinP % 64 == 0 (else SRK_E_SHAPE); y and x
 * 16-byte aligned (else SRK_E_ALIGN). */
int srk_conv3x3_wgrad_bf16(const uint16_t* y, const uint16_t* x, float* dw, float* db, int B, int H, int W, int CinP, int N,
                           srk_stream_t stream);
/* y[i] = bf16(x[i]), round to nearest even, NaN stays NaN (one packed conversion per pair; fp32 subnormals are converted like every other
 * value, not flushed).  SRK_E_NULL: null x / y; SRK_E_SHAPE: n <= 0 or n % 4 != 0; SRK_E_ALIGN: x not 16-byte or y not 8-byte aligned. */
int srk_cast_f32_bf16(const float* x, uint16_t* y, int64_t n, srk_stream_t stream);
/* on-device check of the ds_read_b64_tr_b16 contract the kernels rely on: in u16 [64][16], out u16 [64][8] */
int srk_probe_trread(const uint16_t* in, uint16_t* out, srk_stream_t stream);

/* Timing probe for the roofline leg of bench.py: while a probe is active every launch of the chosen kernel
 * family (1 linear GEMM, 2 conv GEMM, 3 linear wgrad, 4 conv wgrad, 5 attention fwd, 6 attention bwd) is bracketed
 * by HIP events on its own stream.  srk_probe_end synchronises those events and returns the summed kernel time,
 * the summed ALGORITHMIC (un-padded) FLOPs and HBM bytes (each operand read / result written once) and the
 * launch count.  Not thread-safe; one probe at a time.  srk_set_option("probe_stride", s) brackets only every s-th
 * launch of the family (a uniform sample when s is coprime with the per-block launch pattern): the two event records
 * per launch otherwise cost a few percent of a step. */
int srk_probe_begin(int family, int capacity);
int srk_probe_end(double* total_ms, double* flops, double* bytes, int* launches);

/* Kernel-selection switches (A/B testing; results are equivalent up to fp32 summation order).
 *   "gemm_stream" 1 (default) / 0: use the persistent LDS-DMA GEMM (csrc/gemm_stream.hip) for the block GEMMs it
 *   covers, or always the tile-per-workgroup GEMM (csrc/gemm.hip).  Env SRK_GEMM_STREAM=0 sets the initial value.
 *   "gemm_stream_bm" 0/16/32/64, "gemm_stream_ks2" -1/0/1, "gemm_stream_split" -1/0/1, "gemm_stream_nb" 0/4/8:
 *   tile-shape overrides of that kernel (0 / -1 = the measured per-epilogue defaults); used by tools/stream_sweep.py.
 *   "probe_stride" 1..1024: see srk_probe_begin.
 *   "wgrad_stream_w8" 1 (default) / 0: the streaming weight-gradient kernel runs eight waves per workgroup (4 x 2 blocks of
 *   48 x 96 of the 192 x 192 tile, two waves per SIMD) or four (2 x 2 blocks of 96 x 96); same sums in the same order.
 *   "block_light" 1 (default) / 0: SwinIR-light width (C <= 64, 6 heads x d <= 16, hidden <= 128), inference: each Swin block is
 *   ONE kernel (csrc/block_light.hip: LayerNorms, qkv, window attention, proj, MLP and both residuals of a window in LDS and
 *   registers) or the layer-per-launch path.
 *   "mlp_bwd_fused" 1 (default) / 0: the MLP half of a Swin block's backward as one kernel (csrc/gemm_stream.hip: fc2 dgrad, GELU',
 *   fc1 dgrad and the norm2 backward; d u stays on the CU between the two GEMMs) or the two streaming GEMMs.
 *   "mlp_dgelu_store" 1 (default) / 0: between the fused MLP forward and the fused MLP backward of a training plan the u buffer
 *   carries bf16(gelu'(u)) instead of bf16(u) (the backward's only use of u; its front waves then multiply instead of evaluating
 *   erf + exp per element).  Read by the training forward; changing "mlp_bwd_fused" / "gemm_stream" between that forward and its
 *   backward is then an error (SRK_E_UNSUPPORTED).  The forward's outputs do not depend on it.
 *   "attn_bwd_fused" 1 (default) / 0: attention backward with q/k/v re-projected from the saved norm1 output and the output-
 *   projection dgrad folded in (csrc/attn_bwd_fused.hip; classical width; the training forward then stores no q/k/v), or the
 *   dgrad GEMM + csrc/attn.hip on q/k/v saved by the forward.  Read when a training forward lays out its workspace.
 *   "attn_fused" 2 (default) / 1 / 0: qkv projection + window attention forward in one kernel per window
 *   (csrc/attn_fused.hip; classical width: 6 heads x 32, C padded to 192) as three 4-wave workgroups per CU (2) or one 8-wave
 *   workgroup per CU (1), or the projection GEMM + attention kernel (0).
 *   "wgrad_stream" 1 (default) / 0: LDS-DMA ring variant of the 192x192 linear weight-gradient tile or the
 *   register-staged one (both in csrc/wgrad.hip).
 *   "conv_wgrad_taps" 2 (default) / 1 / 0: all-taps conv weight gradient with the LDS-DMA ring / register-staged
 *   (csrc/convwgrad.hip, incl. the MFMA image-head kernels), or the per-tap tiles of wgrad.hip + the VALU image head.
 *   "conv_wgrad_roll" 1 (default) / 0: with conv_wgrad_taps = 2, the LDS-DMA kernel keeps a rolling window of X image rows in
 *   LDS (one new row per 64-pixel run; W = 64 and W = 128, other widths run the per-run staging) or stages a fresh
 *   3 x 66-pixel halo for every run.  At W = 64 both give the same dW bits.  The MFMA image-head kernel (srk_smallconv_wgrad)
 *   follows the same option: X rows and the fp32 dY by LDS-DMA into rings, or both staged through registers.
 *   "wgrad_stream_rows" 32 (default) / 64: rows per ring stage of the linear kernel (6 or 3 stages in the 144 KB ring);
 *   "wgrad_stream_nt" 1 (default) / 0: streaming cache policy on its operand DMAs.
 *   "wgrad_partials" 1 (default) / 0: the streaming weight-gradient kernels write their per-split partial tiles to the
 *   caller's workspace (srk_set_wgrad_workspace; the model executor uses a region of its own workspace) and a reduce
 *   kernel adds their sum to dW in a fixed order, or every split adds into dW with fp32 atomics (order-dependent
 *   rounding, ~20 us slower per launch; also what happens when no workspace is registered).
 *   "wide_head_train" 0 (default) / 1: a SwinIR plan whose 'pixelshuffledirect' head has 17 .. 64 output channels (light x3: 27,
 *   x4: 48) trains: srk_swinir_forward(training = 1) keeps what the backward reads and srk_swinir_backward runs the head through
 *   srk_widehead_grad_prep / _wgrad / _dgrad (csrc/headconv_wide.hip); with 0 both calls return SRK_E_UNSUPPORTED for such a head.
 *   The gradient of the head's output is then [T][round_up(Cout, 16)] fp32 in the workspace: the option changes the workspace
 *   layout, so set it before the first srk_swinir_workspace_bytes query.  Heads of at most 16 channels are not affected.
 * Unknown names return SRK_E_UNSUPPORTED.
 * Scope: srk_set_option / srk_get_option act on ONE process-wide value per option (every thread reads it, including the autograd
 * engine's backward thread).  A plan carries its own values -- srk_swinir_plan_set_option -- which hold, in a thread-private copy of
 * the option set, for the duration of each call on that plan: two plans with different options can live in one process and run on
 * two threads.  "probe_stride" belongs to the one-per-process timing probe.  The cached device properties and the "LDS limit raised"
 * flags of the kernels are keyed by device id. */
int srk_set_option(const char* name, int value);
int srk_get_option(const char* name, int* value);

/* ---- training-step pieces  (finetune_swinir.py:148-179) ------------------------------------------ */
/* F.l1_loss(pred, target) (:66-67, :163) forward + backward in one pass; also counts non-finite pred
 * values (assert_finite :133-143, :164).  loss (fp32 scalar) and nonfinite (uint32) are ACCUMULATED
 * (zero them first); d_pred may be null; grad_scale multiplies d_pred (1.0 for a plain backward). */
int srk_l1_loss_fwd_bwd(const float* pred, const float* target, float* d_pred, float* loss, uint32_t* nonfinite,
                        int64_t n, float grad_scale, srk_stream_t stream);
/* The pixel objectives of SR fine-tuning with the semantics of the L1 entry above (csrc/loss.hip): kind SRK_LOSS_L1 = mean |d|,
 * SRK_LOSS_MSE = mean d^2, SRK_LOSS_CHARBONNIER = mean sqrt(d^2 + eps^2) (eps > 0; other kinds do not read eps), d = pred - target
 * over n fp32 elements.  loss[0] += the mean (weight 1: srk_ssim_loss_fwd_bwd can add its term to the same scalar); nonfinite
 * (uint32, may be null) += the number of non-finite pred values; d_pred (may be null) = grad_scale * d loss / d pred, stored when
 * accumulate == 0 and added to what d_pred holds when accumulate == 1.  Unlike the L1 entry the loss sum is formed in a FIXED order
 * (per-workgroup partials in `workspace`, srk_pixel_loss_workspace(n) bytes owned by the caller, plus one finishing workgroup): two
 * calls give the same bits.  SRK_E_NULL: null pred / target / loss / workspace; SRK_E_SHAPE: n <= 0, unknown kind, Charbonnier with
 * eps <= 0, accumulate not 0 / 1. */
#define SRK_LOSS_L1 0
#define SRK_LOSS_MSE 1
#define SRK_LOSS_CHARBONNIER 2
int64_t srk_pixel_loss_workspace(int64_t n);
int srk_pixel_loss_fwd_bwd(const float* pred, const float* target, float* d_pred, float* loss, uint32_t* nonfinite, int64_t n, int kind,
                           float eps, float grad_scale, int accumulate, void* workspace, srk_stream_t stream);
/* SSIM as a training term: S = srk_ssim's batch mean of x against y (fp32 [B][C][H][W]; the same 11-tap Gaussian, K constants and
 * VALID filter; the taps are normalised in fp64 here, which moves S by up to ~3e-6 against srk_ssim's fp32-normalised taps).
 * ssim_mean[0] = S (may be null); loss[0] += alpha * (1 - S) (may be null); d_x (fp32 [B][C][H][W], may be null) receives
 * -alpha * dS/dx, stored when accumulate == 0 and added when accumulate == 1; there is no gradient for y.  One fused kernel per
 * 32 x 32 tile of input pixels (no per-pixel intermediates in HBM), fixed-order sums, no float atomics: reproducible.  Nothing
 * outside d_x[0 .. B*C*H*W) and the two scalars is written.  workspace: srk_ssim_loss_workspace(B, C, H, W) bytes.
 * SRK_E_UNSUPPORTED: H or W < 11; SRK_E_SHAPE: B, C outside srk_ssim's limits (B <= 1024, B*C < 65536), data_range <= 0, d_x
 * overlapping x or y; SRK_E_NULL: null x / y / workspace. */
int64_t srk_ssim_loss_workspace(int B, int C, int H, int W);
int srk_ssim_loss_fwd_bwd(const float* x, const float* y, void* workspace, int B, int C, int H, int W, float data_range, float alpha,
                          float* d_x, int accumulate, float* ssim_mean, float* loss, srk_stream_t stream);
/* Frequency loss as a training term (csrc/fft_loss.hip): the L1 distance between the 2-D real FFTs of x and y (fp32
 * [B][C][H][W]), the basicsr-style FFTLoss.  With d = x - y, D = rfft2(d) unnormalised, Wh = W / 2 + 1, s = 1 (ortho == 0) or
 * 1 / sqrt(H W) (ortho == 1) and N = 2 B C H Wh:  L = (s / N) sum_{u < H, v < Wh} |Re D| + |Im D|, which equals
 * F.l1_loss(stack([rfft2(x).real, rfft2(x).imag], -1), the same of y).  value[0] = L (may be null); loss[0] += alpha * L (may be
 * null); d_x (fp32 [B][C][H][W], may be null for a value-only call) receives alpha * dL/dx, stored when accumulate == 0 and added
 * when accumulate == 1; there is no gradient for y.  The gradient is the true adjoint over the half spectrum,
 * (s / N) Re sum_{u, v < Wh} G[u][v] exp(+2 pi i (u y / H + v x / W)) with G = sign(Re D) + i sign(Im D), sign(0) = 0: no Hermitian
 * doubling of the interior columns.  At the self-conjugate bins (u in {0, H/2}, v in {0, W/2}; halves of even extents only) the
 * imaginary part is structurally zero and contributes neither to L nor to the gradient.  One transform of d, as fp32 matrix
 * products on the fp32-input MFMA with twiddle tables built on the device by the same call (fp64 sincospi, rounded once); D itself
 * never goes to memory.  Fixed-order sums, no float atomics, no host read: reproducible and capturable.  Nothing outside
 * d_x[0 .. B*C*H*W), the two scalars and the workspace is written.  workspace: srk_fft_loss_workspace(B, C, H, W) bytes (0 for a
 * shape the entry refuses).  Any 1 <= H, W <= 512, odd sizes included.
 * SRK_E_NULL: null x / y / workspace; SRK_E_SHAPE: B, C, H or W <= 0, B*C >= 65536, a non-finite alpha, ortho or accumulate not
 * 0 / 1, accumulate with a null d_x, d_x overlapping x or y; SRK_E_UNSUPPORTED: H or W > 512. */
int64_t srk_fft_loss_workspace(int B, int C, int H, int W);
int srk_fft_loss_fwd_bwd(const float* x, const float* y, void* workspace, int B, int C, int H, int W, int ortho, float alpha,
                         float* d_x, int accumulate, float* value, float* loss, srk_stream_t stream);
/* Optional workspace of the stand-alone weight-gradient entry points (srk_linear_wgrad_bf16, srk_conv3x3_wgrad_bf16):
 * srk_wgrad_workspace_bytes() bytes of device memory owned by the caller, registered for the CALLING THREAD until replaced
 * (null / 0 unregisters).  With it the row-splits of a weight-gradient tile are summed in a fixed order (reproducible dW);
 * without it they are added with fp32 atomics.  The library never allocates device memory itself.  srk_swinir_backward
 * does not need this: it carves the region out of its own workspace. */
int64_t srk_wgrad_workspace_bytes(void);
int srk_set_wgrad_workspace(void* workspace, int64_t bytes);

/* Data path on the device (first slice): the paired transform of the training set -- ToImage +
 * ToDtype(scale=True), _ensure_3ch and paired_random_crop (finetune_swinir.py:80-110) -- from a pool of pre-decoded 8-bit
 * images in device memory.  pool: the images back to back, each [H][W][C] uint8 with C = 1 or 3.  lr_desc / hr_desc: B
 * descriptors of six int64 {byte offset in pool, H, W, C | (wide << 8), top, left} in DEVICE memory (wide = 1: little-endian
 * uint16 samples at an even byte offset, value = u16 / 65535); the caller draws (top, left) for the LR
 * side (the reference's random.randint pair, :101-102), the HR descriptor carries (top * scale, left * scale) and must lie
 * inside its image (the caller checks; the kernel does not).  lr_out: fp32 [B][3][P][P], hr_out: fp32 [B][3][P*scale][P*scale];
 * value = u8 / 255 in IEEE fp32, a gray image is repeated into three channels: bit-identical to the host transform. */
int srk_paired_crop_u8(const uint8_t* pool, const int64_t* lr_desc, const int64_t* hr_desc, float* lr_out, float* hr_out, int B,
                       int lr_patch, int scale, srk_stream_t stream);
/* One side of srk_paired_crop_u8 (the same kernel): B windows of patch x patch, descriptors and conversion as there, into
 * out fp32 [B][3][patch][patch].  What cuts the extended window of the second-order degradation, whose side is no multiple of the
 * HR patch's.  SRK_E_NULL: a null pointer; SRK_E_SHAPE: B outside 1..65535, patch outside 1..8192. */
int srk_crop_u8(const uint8_t* pool, const int64_t* desc, float* out, int B, int patch, srk_stream_t stream);
/* D4 transform of a batch of fp32 NCHW images (flip / rot90 augmentation of a training batch, the forward and inverse transforms of
 * the x8 self-ensemble).  op in 0..7: bit 0 = horizontal flip (x -> W-1-x), bit 1 = vertical flip (y -> H-1-y), bit 2 = transpose,
 * applied in that order: T_op = Tr^b2 . V^b1 . H^b0.
 * in [B][C][H][W]; out [B][C][Ho][Wo], (Ho, Wo) = (W, H) when bit 2 is set, else (H, W).
 * ops: DEVICE int32 [B] (one code per sample; only the low three bits are read) or null = op_all for every sample.
 * With ops != null the geometry must not depend on the codes: H == W is required (SRK_E_SHAPE otherwise).
 * accumulate == 0: out = alpha * T(in); accumulate == 1: out += alpha * T(in).  in and out must not overlap (SRK_E_SHAPE).
 * op_all outside 0..7, B / C / H / W < 1: SRK_E_SHAPE.  Nothing outside out[0 .. B*C*H*W) is written.  With alpha == 1 and
 * accumulate == 0 the values are moved, not multiplied: every bit pattern (NaN payloads included) arrives unchanged. */
int srk_dihedral_f32(const float* in, float* out, const int32_t* ops, int op_all, int B, int C, int H, int W, float alpha,
                     int accumulate, srk_stream_t stream);
/* Antialiased bicubic resampling (csrc/resize.hip): the Keys cubic with a = -0.5 in the convention of PIL's Image.BICUBIC and of
 * F.interpolate(mode='bicubic', antialias=True, align_corners=False).  Per axis n_in -> n_out with scale = n_in / n_out (fp64):
 * support = 2 max(scale, 1); output i has centre c = scale (i + 0.5) and taps [lo, hi) = [max(int(c - support + 0.5), 0),
 * min(int(c + support + 0.5), n_in)) with w_j = k((j + lo - c + 0.5) / max(scale, 1)) divided by their sum: taps outside the image are
 * dropped and the rest renormalised, nothing is clamped or mirrored.  The weights are evaluated in fp64 and rounded once to fp32; the
 * horizontal pass runs first, then the vertical pass, each an ascending-tap chain of fp32 fused multiply-adds starting from 0.
 * x fp32 [B][C][H][W] -> out fp32 [B][C][Ho][Wo], up or down.  quant_bits == 0: the filtered value; quant_bits == 8:
 * (float)rint(clamp(v, 0, 1) * 255) / 255.0f, what an 8-bit image file of the result decodes to.  An output is NaN exactly when a tap of
 * its footprint (zero weights included) is.  One launch, no device allocation, the horizontal-pass result stays in LDS; nothing
 * outside out[0 .. B*C*Ho*Wo) is written.  SRK_E_NULL: null x / out; SRK_E_SHAPE: a non-positive extent, quant_bits other than 0 / 8,
 * x and out overlapping, a size that does not fit one launch; SRK_E_UNSUPPORTED: an axis shrinking by more than 8x (more than 33 taps). */
int srk_resize_aa_f32(const float* x, float* out, int B, int C, int H, int W, int Ho, int Wo, int quant_bits, srk_stream_t stream);
/* Training pairs from HR images only: the HR patch of srk_paired_crop_u8 and its antialiased bicubic degradation in ONE launch.
 * pool / hr_desc: as srk_paired_crop_u8 -- B descriptors {byte offset, H, W, C | (wide << 8), top, left} in DEVICE memory; top and left
 * are in HR pixels, multiples of scale (2..4), and top / scale + P <= H / scale, left / scale + P <= W / scale (the caller checks; the
 * kernel does not, it only keeps its loads inside the image).  hr_out: fp32 [B][3][P*scale][P*scale], bit-identical to what
 * srk_paired_crop_u8 writes for the descriptor.  lr_out: fp32 [B][3][P][P] = rows top / scale .. and columns left / scale .. of the
 * (H / scale, W / scale) downscale of the image's top-left (H - H % scale, W - W % scale) region: taps are bounded by that region, not
 * by the patch, so the patch is BIT-IDENTICAL to the same window of srk_resize_aa_f32 on the whole converted region (the two entries
 * share their device routines).  A gray source is filtered once and written to three channels.  quant_bits as above (LR only).
 * SRK_E_NULL: a null pointer; SRK_E_SHAPE: B outside 1..65535, lr_patch outside 1..2048, scale outside 2..4, quant_bits other than 0 / 8. */
int srk_crop_degrade_u8(const uint8_t* pool, const int64_t* hr_desc, float* lr_out, float* hr_out, int B, int lr_patch, int scale,
                        int quant_bits, srk_stream_t stream);
/* Blind degradation (csrc/degrade.hip): the antialiased bicubic downscale above behind a per-sample Gaussian blur, plus per-sample noise.
 * Parameters, four int64 slots per sample (slots 6..9 of a ten-slot descriptor, or one row of par4):
 *   [6] fp32 bits of sigma_y (low word) and sigma_x (high word), HR pixels, each in [0, 2.5]
 *   [7] fp32 bits of sigma_n (low word) and gain (high word), image units, each in [0, 1]
 *   [8] noise_id, 64 bits        [9] flags: bit 0 = gray noise (one draw for all channels)
 * Blur: an axis-aligned anisotropic Gaussian.  Per axis R = ceil(3 sigma) (<= 8), g[d] = exp(-d^2 / (2 sigma^2)), d = -R..R, normalised
 * in fp64, composed with the cubic taps (lo_c, w_c[j]) of the resize -- the fp64 values before their rounding -- into one table per
 * output i: W[m] = sum_j w_c[j] g[m - lo_c - j] for m in [max(lo_c - R, 0), min(hi_c + R, n_in)), divided by its sum (mass outside the
 * image is dropped and the rest renormalised, the border rule of the resize); fp64 with contraction off, rounded once to fp32.  At
 * factors 2 / 3 / 4 that is at most 8 + 16, 12 + 16 and 16 + 16 taps; the two passes of the resize run unchanged on the composed
 * tables (horizontal first, ascending-tap fmaf chains from 0).  An axis with sigma == 0 takes the cubic table itself.
 * Noise, on the filtered fp32 value v and before the 8-bit rounding: v + sqrtf(sigma_n^2 + gain * fmaxf(v, 0)) * z, in fp32 without
 * contraction.  z = sqrtf(-2 logf(u1)) * cospif(2 u2), u1 = ((r0 >> 8) + 1) * 2^-24, u2 = (r1 >> 8) * 2^-24, (r0, r1) the first two
 * words of Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85) on the counter (x, y, ch, 0) under
 * the key (low word, high word of noise_id): x, y are the output's coordinates in the WHOLE downscaled image, ch its channel, or 0
 * with gray noise -- which a one-channel image always gets.  sigma_n == 0 && gain == 0: nothing is added, the bits of v pass through.
 * With both sigmas 0 and no noise the outputs are BIT-IDENTICAL to srk_resize_aa_f32 / srk_crop_degrade_u8.
 * The host checks the ranges; for ANY bit pattern the kernels clamp R to 0..8 (sigma <= 0 or NaN: no blur) and sigma_n, gain to
 * [0, 16] (NaN: 0), and stay inside their tables and their output.  One launch, no device allocation.
 *
 * srk_degrade_blind_f32: x fp32 [B][C][H][W] -> out fp32 [B][C][H/scale][W/scale]; par4 DEVICE int64 [B][4] = slots 6..9.
 * SRK_E_NULL: a null pointer; SRK_E_SHAPE: a non-positive extent, scale outside 2..4 or not dividing H and W, quant_bits other than
 * 0 / 8, x and out overlapping, a size that does not fit one launch. */
int srk_degrade_blind_f32(const float* x, float* out, const int64_t* par4, int B, int C, int H, int W, int scale, int quant_bits,
                          srk_stream_t stream);
/* srk_crop_degrade_u8 with the blind degradation: desc10 = B descriptors of TEN int64 in DEVICE memory, [0..5] the six of
 * srk_crop_degrade_u8, [6..9] as above.  hr_out is never blurred or noised: bit-identical to srk_crop_degrade_u8's.  lr_out is
 * BIT-IDENTICAL to the window of srk_degrade_blind_f32 on the whole converted region with the same four slots (the counter takes image
 * coordinates; the two entries share their device routines).  A gray source is filtered once, gets one draw and is written to three
 * channels.  Errors as srk_crop_degrade_u8. */
int srk_crop_degrade_blind_u8(const uint8_t* pool, const int64_t* desc10, float* lr_out, float* hr_out, int B, int lr_patch, int scale,
                              int quant_bits, srk_stream_t stream);
/* General 2-D blur (csrc/blur2d.hip): a rotated, generalized or plateau Gaussian, or a measured point-spread function, as a table.
 * A PSF table is ks x ks fp32, ks odd in 1..21, R = (ks - 1) / 2; one table per sample, psf = DEVICE fp32 [B][ks][ks].
 * The blur is a CORRELATION (cv2.filter2D's convention: no flip of the table) with the border rule of the resize applied per blurred
 * pixel -- mass outside the image is dropped and the rest renormalised:
 *   num(p, q)  = sum over a, b ascending (a outer, b inner) of K[a][b] * x(p + a - R, q + b - R)      -- only taps inside the image
 *   mass(p, q) = the same chain with x == 1
 *   blurred    = num / mass
 * Each chain is acc = fmaf(K[a][b], x, acc) from 0 in fp32, no other contraction; the division is IEEE and is performed at every pixel,
 * in the interior too: one code path, one set of bits.  (An interior pixel may take a mass computed once by the same chain.)
 * fmaf(0, x, acc) == acc for finite x, so a table zero-padded, centred, to a larger ks gives IDENTICAL bits on finite images: one ks
 * per launch is enough for a batch of mixed sizes.  A pixel is NaN exactly when an in-image tap of its ks x ks window is.
 * The host (ops) checks a table: taps finite and >= 0, K[R][R] > 0 (so mass > 0 everywhere), fp64 sum within 1e-3 of 1.  The kernels
 * check nothing of it: for ANY table bits they stay inside their buffers, and the values are then unspecified.
 *
 * srk_blur2d_f32: x fp32 [B][C][H][W] -> out of the same shape, sample b blurred with table b.  out must overlap neither x nor psf.
 * One launch, no device allocation; nothing outside out[0 .. B*C*H*W) is written and nothing outside x and psf is read.
 * SRK_E_NULL: a null pointer; SRK_E_SHAPE: a non-positive extent, ks even or outside 1..21, an overlap, a size that does not fit one launch. */
int srk_blur2d_f32(const float* x, const float* psf, float* out, int B, int C, int H, int W, int ks, srk_stream_t stream);
/* srk_crop_degrade_blind_u8 with the 2-D blur in place of the composed Gaussian: LR = noise(resize_aa(blur2d(HR))).  desc10 as there;
 * slot 6 (the sigma pair) is reserved and ignored.  The blur and the resize are both bounded by the image's top-left
 * (H - H % scale, W - W % scale) region; the resize runs the plain cubic tables of srk_resize_aa_f32 on the blurred values; noise and the
 * 8-bit rounding are those of srk_degrade_blind_f32, counter on whole-image LR coordinates.  hr_out is never blurred: bit-identical to
 * srk_crop_degrade_u8's.  lr_out is BIT-IDENTICAL to the window of srk_blur2d_f32 on the whole converted region followed by
 * srk_degrade_blind_f32 with sigma (0, 0) and the same slots 7..9 (the entries share their device routines).  Within R + 2 scale HR
 * pixels of the region's border this differs from srk_crop_degrade_blind_u8 at the same Gaussian: that entry renormalises once per LR
 * output (one composed table), this one per blurred pixel and then per cubic table; in the interior the two agree to rounding.
 * A gray source is blurred and filtered once, gets one draw and is written to three channels.  One launch for the batch.
 * Errors as srk_crop_degrade_blind_u8, plus SRK_E_SHAPE for ks even or outside 1..21. */
int srk_crop_degrade_psf_u8(const uint8_t* pool, const int64_t* desc10, const float* psf, int ks, float* lr_out, float* hr_out, int B,
                            int lr_patch, int scale, int quant_bits, srk_stream_t stream);
/* JPEG round trip (csrc/jpeg.hip): what a baseline JPEG file of an 8-bit image at quality q decodes to, as a closed-form fp32 pipeline.
 * No entropy coding is done: it is lossless and changes nothing.  x, out fp32 [B][C][H][W], C = 1 or 3, H, W >= 1 (no multiple of 8
 * needed); subsample 0 = 4:4:4, 1 = 4:2:0 (has effect only with C == 3); quality DEVICE int32 [B], each in 1..100, or 0 = sample b is
 * passed through bit for bit, NaNs included.  The host checks the range; the kernel clamps any other bit pattern into 0..100.
 * Per sample, every operation in fp32 without contraction:
 *  1. Level.  p = rintf(fminf(fmaxf(v, 0), 1) * 255); NaN gives 0, k / 255.0f gives k: the stage composes with the 8-bit forms of
 *     srk_crop_degrade_u8 and srk_crop_degrade_blind_u8.
 *  2. Colour (C == 3), JFIF full range, each result rintf-ed and clamped to 0..255 as an encoder's 8-bit component planes are:
 *       Y  = fmaf(0.114f, B, fmaf(0.587f, G, 0.299f * R))
 *       Cb = fmaf(0.5f, B, fmaf(-0.331264108f, G, fmaf(-0.168735892f, R, 128)))
 *       Cr = fmaf(-0.081312411f, B, fmaf(-0.418687589f, G, fmaf(0.5f, R, 128)))
 *     With C == 1 the plane is Y.
 *  3. Grid.  8 x 8 blocks anchored at (0, 0); the MCU is 8 x 8, or 16 x 16 with subsample.  The plane is extended to a whole number
 *     of MCUs by replicating its last row and column (libjpeg's edge rule); results outside H x W are dropped.  With subsample a
 *     chroma sample is the unrounded mean (a + b + c + d) * 0.25f of its 2 x 2 cell (exact in fp32).
 *  4. Forward DCT.  Subtract 128.  D[u][k] = 1/2 c_u cos((2k + 1) u pi / 16), c_0 = 1/sqrt(2), evaluated in fp64 and rounded once to
 *     fp32.  Horizontal pass, then vertical pass, each an ascending-k chain acc = fmaf(D[u][k], x[k], acc) from 0.
 *  5. Quantisation.  ITU-T T.81 Annex K table K.1 for Y, K.2 for Cb and Cr, natural order, scaled the libjpeg way:
 *     s = q < 50 ? 5000 / q : 200 - 2 q, Q = clamp((base * s + 50) / 100, 1, 255) in integers; k = rintf(c / Q) with IEEE division;
 *     c' = k * Q (exact).
 *  6. Inverse.  Vertical pass, then horizontal pass, acc = fmaf(D[k][y], c'[k], acc) from 0; add 128; each component is
 *     fminf(fmaxf(rintf(.), 0), 255).  Chroma is upsampled by replication (not libjpeg's "fancy" triangle filter).
 *  7. Back to RGB with cb = Cb - 128, cr = Cr - 128, each rintf-ed and clamped to 0..255, out = level / 255.0f:
 *       R = fmaf(1.402f, cr, Y)    G = fmaf(-0.714136286f, cr, fmaf(-0.344136286f, cb, Y))    B = fmaf(1.772f, cb, Y)
 *     With C == 1, out = Y / 255.0f.
 * coef_out (a test port; production callers pass NULL): the quantised coefficients k as int16 [B][C][Hm][Wm], Hm, Wm = H, W rounded
 * up to the MCU, natural order in place: coefficient (u, v) of block (by, bx) at row 8 by + u, column 8 bx + v.  With subsample a
 * chroma plane fills only its top-left [Hm / 2][Wm / 2]; the rest is not written, and neither is anything of a sample with quality 0.
 * One launch, no device allocation; nothing outside out[0 .. B C H W) and the stated part of coef_out is written.
 * SRK_E_NULL: null x, out or quality; SRK_E_SHAPE: a non-positive extent, C not 1 or 3, subsample not 0 or 1, x and out overlapping, a
 * size that does not fit one launch. */
int srk_jpeg_roundtrip_f32(const float* x, float* out, const int32_t* quality, int B, int C, int H, int W, int subsample, int16_t* coef_out,
                           srk_stream_t stream);
/* Scale-1 restoration (csrc/restore.hip): denoising and JPEG-artifact pairs.  "clean" is the target, "degraded" the network input;
 * both have the same size.  degraded = jpeg_roundtrip(noise(convert(image))): the noise stage of the blind degradation and the JPEG
 * round trip above, with no resize in between.  Parameters are slots 6..9 as above, except that slot 6 carries no blur.
 *
 * srk_noise_f32: x fp32 [B][C][H][W] -> out of the same shape, C = 1 or 3; par4 DEVICE int64 [B][4] = slots 6..9, slot 6 ignored.
 * out = the noise formula of srk_degrade_blind_f32 per element (the same device routine), counter (x, y, ch, 0) on IMAGE coordinates,
 * ch = 0 with gray noise, which a one-channel image always gets; key = noise_id.  sigma_n == 0 && gain == 0: the bits of x pass
 * through.  quant_bits 0 | 8 as srk_resize_aa_f32.  out must not overlap x.  One launch, no device allocation; nothing outside
 * out[0 .. B*C*H*W) is written.  SRK_E_NULL: a null pointer; SRK_E_SHAPE: a non-positive extent, C not 1 or 3, quant_bits other than
 * 0 / 8, x and out overlapping, a size that does not fit one launch. */
int srk_noise_f32(const float* x, float* out, const int64_t* par4, int B, int C, int H, int W, int quant_bits, srk_stream_t stream);
/* Training pairs at scale 1, ONE launch for the batch.  pool and slots 0..5 of desc10 as srk_crop_degrade_u8: {byte offset, H, W,
 * C | (wide << 8), top, left}; top and left are ANY image pixels with top + patch <= H and left + patch <= W (the caller checks; the
 * kernel does not, it only keeps its loads inside the image).  Slot 6: low word = JPEG quality as int32, 0 = no JPEG stage, any other
 * bit pattern is clamped into 0..100 as srk_jpeg_roundtrip_f32 does; slots 7..9 = sigma_n / gain, noise_id, flags as above.
 * clean_out, degraded_out: fp32 [B][out_chans][patch][patch], out_chans = 1 or 3.
 * Conversion: stored sample / 255 (/ 65535 when wide) in IEEE fp32, as srk_paired_crop_u8.  out_chans 3: a gray source is repeated -- it
 * gets one noise draw and is coded as a gray JPEG written three times.  out_chans 1: a gray source as is; an RGB source becomes the
 * integer luma (4899 R + 9617 G + 1868 B + 8192) >> 14 of the stored samples, u8 or u16 alike (the coefficients sum to 16384, the sum
 * fits 32 bits), which is then divided as above.  clean_out is the converted window and nothing else.
 * degraded_out is the window at (top, left) of the WHOLE-IMAGE chain: noise keyed on image coordinates; 8 x 8 blocks (16 x 16 MCUs
 * with subsample) anchored at the IMAGE's (0, 0), the image extended by replicating its last row and column, and the noise of a
 * replicated pixel is that of the pixel it replicates.  It is BIT-IDENTICAL to the same window of srk_noise_f32 followed, where the
 * quality is > 0, by srk_jpeg_roundtrip_f32 on the whole converted image (the entries share their device routines).  Quality 0
 * stores the noised (with quant_bits 8: rounded) values; with a quality > 0 the level step of the round trip does the rounding and
 * quant_bits has no further effect.  subsample has effect only when three distinct planes are coded (out_chans 3, RGB source).
 * No device allocation, no intermediate image; nothing outside the two outputs is written.
 * SRK_E_NULL: a null pointer; SRK_E_SHAPE: B outside 1..65535, patch outside 1..2048, out_chans not 1 or 3, subsample not 0 or 1,
 * quant_bits other than 0 / 8, the two outputs overlapping. */
int srk_crop_restore_u8(const uint8_t* pool, const int64_t* desc10, float* clean_out, float* degraded_out, int B, int patch, int out_chans,
                        int subsample, int quant_bits, srk_stream_t stream);
/* Ragged batches (csrc/ragged.h, ragged.hip, filter2d.hip): the stages of the second-order degradation -- blur, resize, noise, JPEG,
 * twice, then a sinc filter -- give every sample its own intermediate size.  The contract of the three entries below, stated once:
 *   - the buffer is fp32 [B][C][Hp][Wp]; ext is DEVICE int32 [B][2] = (h_b, w_b) with 1 <= h_b <= Hp and 1 <= w_b <= Wp;
 *   - sample b occupies the top-left h_b x w_b of each of its planes, at row pitch Wp; the rest of the buffer is padding;
 *   - a ragged kernel never reads an input element outside a sample's extents and never writes an output element outside them
 *     (padding may hold anything, NaNs included, and output padding keeps its bits);
 *   - the grid covers the padded extents times B; a workgroup whose tile misses its sample's extents leaves before any barrier;
 *   - ext == NULL means dense: every sample is Hp x Wp;
 *   - the host that wrote ext checks it (the entries cannot: it is device memory and no entry synchronises); for ANY bit pattern in
 *     ext the kernels clamp into 1..Hp / 1..Wp and stay inside their buffers.
 * One launch each, no device allocation.
 *
 * srk_filter2d_f32: a SIGNED table -- a sinc (ringing) filter, or any table of srk_blur2d_f32 -- as a CORRELATION with a reflect-101
 * border (cv2.filter2D's default; Real-ESRGAN's filter2D).  tab = DEVICE fp32 [B][ks][ks], ks odd in 1..21, R = (ks - 1) / 2:
 *   out(p, q) = sum over a, b ascending (a outer, b inner) of K[a][b] * x(rho(p + a - R, h), rho(q + b - R, w))
 *   rho(i, n) = i < 0 ? -i : (i >= n ? 2 (n - 1) - i : i), then clamped into 0..n-1
 * as the chain acc = fmaf(K[a][b], x, acc) from 0 in fp32, no other contraction.  No mass and no division (srk_blur2d_f32's rule needs
 * a mass that a signed table does not have).  The reflection is exact for h, w > R, which the host requires of every sample at the R
 * of its own table; the clamp keeps any other extent in bounds.  fmaf(0, x, acc) == acc for finite x: a table zero-padded, centred,
 * to a larger ks gives IDENTICAL bits on finite images -- also on a sample that is smaller than the padded R, where the clamped
 * positions are read and multiplied by 0 -- so one ks per launch is enough for a batch of mixed table and image sizes.  quant_bits 0 | 8 as srk_resize_aa_f32.  A delta table (centre tap 1, every other tap +-0) is a
 * pass-through: with quant_bits 0 the words of x are copied, NaN payloads and -0 included.  The host (ops) checks a table: taps
 * finite, fp64 sum within 1e-3 of 1, no sign rule.  out must overlap none of x, tab, ext.
 * SRK_E_NULL: null x / tab / out; SRK_E_SHAPE: B or C < 1, ks even or outside 1..21, Hp or Wp <= R, quant_bits other than 0 / 8, an
 * overlap, a size that does not fit one launch. */
int srk_filter2d_f32(const float* x, const float* tab, float* out, const int32_t* ext, int B, int C, int Hp, int Wp, int ks, int quant_bits,
                     srk_stream_t stream);
/* srk_resize_aa_f32 per sample: x [B][C][Hp][Wp] with ext_in -> out [B][C][Hop][Wop] with ext_out, sample b resized from
 * (h_b, w_b) to (ho_b, wo_b) by the tables of those two extents on the tile grid from (0, 0) of srk_resize_aa_f32 (the entries share
 * their device routines): sample b is BIT-IDENTICAL to srk_resize_aa_f32 on that sample alone.  Either table may be NULL (dense).
 * An axis of a sample shrinking by more than 8x is not supported.  With both tables NULL the entry checks that itself; otherwise the
 * CALLER checks it from its host copy of the tables (ops.resize_aa_ragged does) -- the kernel then still stays in bounds, it drops the
 * taps past the 33rd.  SRK_E_NULL: null x / out; SRK_E_SHAPE: a non-positive extent, quant_bits other than 0 / 8, out overlapping x
 * or a table, a size that does not fit one launch; SRK_E_UNSUPPORTED: a dense call shrinking an axis by more than 8x. */
int srk_resize_aa_ragged_f32(const float* x, const int32_t* ext_in, float* out, const int32_t* ext_out, int B, int C, int Hp, int Wp, int Hop,
                             int Wop, int quant_bits, srk_stream_t stream);
/* srk_jpeg_roundtrip_f32 per sample: the 8 x 8 grid is anchored at (0, 0) of each sample and its last row and column at (h_b, w_b)
 * are replicated into the last MCU (the entries share their device routines): sample b is BIT-IDENTICAL to srk_jpeg_roundtrip_f32 on
 * that sample alone.  Quality 0 copies the in-extent words of the sample.  No coefficient port.
 * SRK_E_NULL: null x / out / quality; SRK_E_SHAPE: a non-positive extent, C not 1 or 3, subsample not 0 or 1, x and out overlapping, a
 * size that does not fit one launch. */
int srk_jpeg_roundtrip_ragged_f32(const float* x, float* out, const int32_t* quality, const int32_t* ext, int B, int C, int Hp, int Wp,
                                  int subsample, srk_stream_t stream);
/* The noise stage of a ragged chain is srk_noise_f32 on the padded buffer: its counter is (x, y, ch) only, so inside the extents its
 * bits are those of the dense call on the sample alone; what it writes into the padding is never read. */
/* srk_resize_aa_ragged_f32 with a resize rule per sample (csrc/resize_modes.hip): the ragged contract, the arguments, the tile grid and
 * the filter (resize.h: rs_filter, horizontal pass first, ascending-tap fmaf chains from 0) are those of srk_resize_aa_ragged_f32; only
 * the per-output tap list differs.  mode = DEVICE int32 [B], NULL = every sample mode 0; any other bit pattern is clamped into 0..2.
 * Per axis n_in -> n_out, the table arithmetic in fp64 (contraction off), the weights rounded once to fp32:
 *   0 cubic, antialiased     the taps of srk_resize_aa_f32: the sample is BIT-IDENTICAL to srk_resize_aa_ragged_f32
 *   1 bilinear, not antialiased   scale = n_in / n_out, src = max(scale (i + 0.5) - 0.5, 0), i0 = min(floor(src), n_in - 1),
 *                            l = src - i0; taps i0 and min(i0 + 1, n_in - 1) with weights 1 - l and l; where both are one pixel, one
 *                            tap of weight 1 (F.interpolate(mode='bilinear', align_corners=False) on an explicit size)
 *   2 area                   lo = (i n_in) / n_out, hi = ((i + 1) n_in + n_out - 1) / n_out in 64-bit integers; hi - lo taps of
 *                            weight 1 / (hi - lo) (adaptive average pooling)
 * An axis shrinking by more than 8x is not supported in ANY mode (the tile staging needs it, not the tap count): checked as
 * srk_resize_aa_ragged_f32 checks it -- by the entry for a dense call, by the caller for ragged tables.
 * SRK_E_NULL: null x / out; SRK_E_SHAPE: a non-positive extent, quant_bits other than 0 / 8, out overlapping x, a table or mode, a
 * size that does not fit one launch; SRK_E_UNSUPPORTED: a dense call shrinking an axis by more than 8x. */
int srk_resize_ragged_mode_f32(const float* x, const int32_t* ext_in, float* out, const int32_t* ext_out, const int32_t* mode, int B, int C,
                               int Hp, int Wp, int Hop, int Wop, int quant_bits, srk_stream_t stream);
/* Unsharp mask of a dense batch (csrc/usm.hip), Real-ESRGAN's USMSharp with its table k k^T evaluated separably.  x, out: fp32
 * [B][C][H][W], C 1 or 3; taps = DEVICE fp32 [ks], ks odd in 1..51, R = (ks - 1) / 2, H, W > R; work = DEVICE fp32 [B][C][H][W]
 * (SRK_USM_WORK_FLOATS(B, C, H, W) floats), provided by the caller: the library allocates nothing.  The contract -- contraction off,
 * every sum an ascending-tap chain acc = fmaf(taps[j], v, acc) from 0, rho the reflect-101 index of srk_filter2d_f32, clamped:
 *   G(v)(p, q) = the horizontal pass h(p, q) = sum_j taps[j] v(p, rho(q + j - R, W)), then sum_i taps[i] h(rho(p + i - R, H), q)
 *   blur = G(x);  res = x - blur;  mask = (fabsf(res) * 255.0f > threshold) ? 1.f : 0.f;  soft = G(mask)
 *   sharp = fminf(fmaxf(x + weight * res, 0.f), 1.f);  out = soft * sharp + (1.0f - soft) * x
 * Two launches of one kernel: the first leaves res in out and mask in work, the second reads both and writes out.  Nothing outside
 * out and work is written; x, taps, out and work are pairwise distinct.
 * SRK_E_NULL: null x / taps / out / work; SRK_E_SHAPE: B, H or W < 1, C not 1 or 3, ks even or outside 1..51, an overlap, a size that
 * does not fit one launch; SRK_E_UNSUPPORTED: H or W <= R. */
#define SRK_USM_MAX_KS 51
#define SRK_USM_WORK_FLOATS(B, C, H, W) ((size_t)(B) * (size_t)(C) * (size_t)(H) * (size_t)(W))
int srk_usm_sharpen_f32(const float* x, const float* taps, float* out, float* work, int B, int C, int H, int W, int ks, float weight,
                        float threshold, srk_stream_t stream);
/* Blur and sinc tables built on the device (csrc/tables.hip): n tables of srk_blur2d_f32 / srk_crop_degrade_psf_u8 / srk_filter2d_f32
 * from a few numbers each, so that the host draws variates and uploads no table.  tab = DEVICE fp32 [n][ks][ks], ks odd in 1..21;
 * desc = DEVICE fp64 [n][8] = (kind, ks_own, A, B2, C, beta, cutoff, bank_index), the integers carried exactly as doubles; bank =
 * DEVICE fp32 [n_bank][kb][kb] (measured PSFs the host has checked) or NULL with n_bank = kb = 0.
 * Table i has side ks_own <= ks (kind 5: kb), centred in its ks x ks slot and surrounded by +0 words.  With R = (ks_own - 1) / 2,
 * row a <-> y = a - R, column b <-> x = b - R, the unnormalised tap e(x, y) in fp64 is
 *   kind 0 delta        the centre tap 1, every other tap +0; written as such
 *   kind 1 gaussian     exp(-0.5 q)
 *   kind 2 generalized  exp(-0.5 pow(q, beta))
 *   kind 3 plateau      1 / (pow(q, beta) + 1)
 *   kind 4 sinc         cutoff J1(cutoff r) / (2 pi r), r = sqrt(x^2 + y^2); the centre tap cutoff^2 / (4 pi)
 *   kind 5 bank         the words of bank[bank_index], copied: no arithmetic, -0 / denormals / NaN payloads kept
 * q = (A x^2 + B2 x y) + C y^2 with the integer products exact and no contraction: A, B2, C are the coefficients of the inverse
 * covariance, which the host forms (blur_kernels._quad_coef), so q has the host's bits.  J1(z) is the trapezoid rule on Bessel's
 * integral, (sum over j = 1..511 ascending of f_j, + 0.5 (f_0 + f_512)) / 512 with f_j = cos(t_j - z sin t_j), t_j = j (pi / 512),
 * t_512 = pi; it is evaluated ONCE per distinct x^2 + y^2 of the grid and looked up by that integer, so a sinc table is exactly 8-fold
 * symmetric.  Kinds 1..4: S = the fp64 sum of e over the own ks_own^2 taps, sequential, row-major ascending from 0; the tap is
 * (float)(e / S), one IEEE division and one rounding; fp32 denormal results are kept.  This order is the contract: it does not depend
 * on the launch shape, and equal descriptors give equal words wherever they stand in the batch.
 * The host that wrote desc checks it (ops.kernel_tables does); for ANY bit pattern in desc the kernel stays inside its buffers:
 * kind outside [0, 6) or NaN counts as 0, kind 5 with a NULL bank as 0, ks_own is clamped into 1..ks (NaN: 1) and an even value lowered
 * by one, bank_index is clamped into 0..n_bank-1 (NaN: 0); a NaN parameter gives a NaN table.  One launch, one workgroup per table, no
 * device allocation; nothing outside tab[0 .. n*ks*ks) is written.  tab must overlap neither desc nor bank.
 * SRK_E_NULL: null desc / tab; SRK_E_SHAPE: n < 1, ks even or outside 1..21, a bank triple that is neither (NULL, 0, 0) nor
 * (pointer, n_bank >= 1, kb odd in 1..ks), an overlap. */
int srk_kernel_tables_f32(const double* desc, const float* bank, int n_bank, int kb, float* tab, int n, int ks, srk_stream_t stream);
/* Tiled inference (csrc/tile.hip): crop a chunk of overlapping tiles out of an fp32 NCHW batch, run a model on them as a batch of
 * n * B, and merge the chunk's outputs into the output image.
 * Tile grid, per axis with extent N, tile t (1 <= t <= N) and stride s (1 <= s <= t; overlap = t - s): k = ceil((N - t) / s) + 1
 * tiles, origin o_i = min(i * s, N - t) -- range(0, N - t, s) + [N - t], the last tile pulled back to the border.  The 2-D grid is
 * row-major, tile index iy * kx + ix; a chunk is the tiles t0 .. t0 + n - 1.
 * srk_tile_gather_f32: tiles [n][B][C][th][tw] <- the crops of x [B][C][H][W].
 * srk_tile_merge_f32: tiles [n][B][C][th][tw] -> out [B][C][Ho][Wo], every extent in OUTPUT pixels.  Chunks must be merged in
 * ascending order and together cover the grid once.
 *   SRK_TILE_MEAN: out[p] = (((0 + y_a[p]) + y_b[p]) + ...) / count over the tiles covering p in ascending tile index, sequential
 *     fp32 adds and one correctly rounded fp32 division by the integer count.  A launch starts a pixel from 0 when its first covering
 *     tile is in the chunk and from out[p] otherwise, adds the chunk's covering tiles, and divides iff the last covering tile is in
 *     the chunk: out may start uninitialised, and the bits do not depend on how the grid is cut into chunks.
 *   SRK_TILE_CENTER: out[p] is copied (bit pattern kept) from one tile: per axis the covering tile that maximises
 *     min(p - o, o + t - 1 - p), ties to the lower index; written in the chunk that holds that tile.
 * A launch writes no pixel that no tile of its chunk covers and nothing outside out[0 .. B*C*Ho*Wo) / tiles[0 .. n*B*C*th*tw).
 * SRK_E_SHAPE, before any launch: a non-positive extent or n, t0 < 0, th > H, tw > W, a stride outside 1..t, t0 + n > ky * kx, an
 * unknown mode, a grid that does not fit one launch, tiles overlapping x / out. */
#define SRK_TILE_MEAN 0
#define SRK_TILE_CENTER 1
int srk_tile_gather_f32(const float* x, float* tiles, int t0, int n, int B, int C, int H, int W, int th, int tw, int sy, int sx,
                        srk_stream_t stream);
int srk_tile_merge_f32(const float* tiles, float* out, int t0, int n, int B, int C, int Ho, int Wo, int th, int tw, int sy, int sx,
                       int mode, srk_stream_t stream);
/* Image files to and from the device (csrc/image_io.hip): B images of one size, interleaved 8- or 16-bit samples as a decoder
 * delivers them <-> planar fp32 in [0, 1] as the models take it.  One launch each, no host read, no upload: capturable.
 * srk_image_unpack: src [B][H][W][in_chans] of uint8 (bits 8) or uint16 in host byte order (bits 16) -> dst fp32 [B][out_chans][H][W],
 *   out_chans 1 or 3; value = (float)s / 255.0f or / 65535.0f as an IEEE division (the convention of srk_paired_crop_u8).
 *   in_chans 1 | 2 (gray, gray + alpha): the gray sample, once or three times; in_chans 3 | 4 (RGB, RGB + alpha): R, G, B at out_chans 3,
 *   the integer luma (4899 R + 9617 G + 1868 B + 8192) >> 14 of the stored samples at out_chans 1.  The last sample of in_chans 2 | 4 is
 *   alpha: it goes to alpha fp32 [B][1][H][W] when that pointer is non-null and is dropped otherwise (alpha is ignored at in_chans 1 | 3).
 *   src needs no alignment beyond that of a sample.
 * srk_image_pack: y fp32 [B][chans][H][W], chans 1 or 3 (+ alpha fp32 [B][1][H][W]) -> dst [B][H][W][out_chans] samples.
 *   q(v), max = 255 or 65535: NaN -> 0, v <= 0 -> 0 (-0.0 and -Inf too), v >= 1 -> max, else rintf(v * max): one fp32 product, rounded
 *   half-to-even -- the (x * 255).round() of the public test scripts, not a truncation.
 *   out_chans 1: gray -- with chans 3 the integer luma above of the QUANTISED R, G, B (at either depth); 2: gray + q(alpha);
 *   3: RGB -- with chans 1 the sample three times; 4: RGB + q(alpha).  alpha is read at out_chans 2 | 4 only.
 *   counters: null, or DEVICE uint32[2] that the launch ADDS to -- [0] the non-finite input values, [1] the finite ones outside
 *   [0, 1], over y and (at out_chans 2 | 4) alpha.  Integer sums: exact, whatever the order.
 * Nothing outside dst[0 .. B*H*W*out_chans) samples (and alpha[0 .. B*H*W)) is written.  Checked on the host before any launch, in
 * this order: SRK_E_SHAPE -- B, H or W < 1, B > 65535, in_chans outside 1..4, chans not 1 or 3, bits not 8 or 16, out_chans not
 * 1 or 3 (unpack) / outside 1..4 (pack); SRK_E_NULL -- null src / dst / y, null alpha at out_chans 2 | 4 of pack; SRK_E_ALIGN -- an odd
 * src (unpack) or dst (pack) at 16 bits, an fp32 array or counters not 4-byte aligned. */
int srk_image_unpack(const void* src, float* dst, float* alpha, int B, int H, int W, int in_chans, int bits, int out_chans,
                     srk_stream_t stream);
int srk_image_pack(const float* y, const float* alpha, void* dst, uint32_t* counters, int B, int H, int W, int chans, int out_chans,
                   int bits, srk_stream_t stream);
/* Validation metrics of one batch in one pass (first slice): per-image PSNR of the images clamped to [0, 1]
 * (batch_psnr, finetune_swinir.py:69-74: 20 log10(max_val / sqrt(mse + 1e-8)), mse over the per_image = C*H*W elements of an
 * image) and the sum of |pred - target| over the batch for the validation L1 (F.l1_loss, :66-67, used by validate :181-207).
 * pred / target: fp32 [B][per_image].  psnr: fp32 [B] or null.  psnr_sum / abs_sum: fp32 scalars or null, ACCUMULATED (zero
 * them before the first batch; one host read at the end of the validation loop replaces the reference's per-batch .item()).
 * workspace: srk_batch_psnr_workspace(per_image, B) bytes of device memory owned by the caller.  Sums are formed in a fixed
 * order (no atomics): results are reproducible.  B <= 1024. */
int64_t srk_batch_psnr_workspace(int64_t per_image, int B);
int srk_batch_psnr(const float* pred, const float* target, void* workspace, int B, int64_t per_image, float max_val, float* psnr,
                   float* psnr_sum, float* abs_sum, srk_stream_t stream);
/* evaluate.py:24-29 on the device: psnr[b] = 20 log10(max_val / sqrt(max(mse_b, 1e-10))) of fp32 [B][per_image] images, NO
 * clamp; mean = their batch mean (what the reference's psnr() returns).  psnr / mean may be null.  workspace:
 * srk_eval_psnr_workspace bytes.  Fixed-order sums. */
int64_t srk_eval_psnr_workspace(int64_t per_image, int B);
int srk_eval_psnr(const float* x, const float* y, void* workspace, int B, int64_t per_image, float max_val, float* psnr, float* mean,
                  srk_stream_t stream);
/* pytorch_msssim.ssim(X, Y, data_range, size_average) as called at train.py:169 / evaluate.py:127,195: fp32 NCHW images, 11-tap
 * Gaussian (sigma 1.5) VALID separable filter, K = (0.01, 0.03); per_image[b] = mean over channels of the per-channel map mean
 * (size_average=False), mean = batch mean (size_average=True); either may be null.  H, W >= 11.  PARITY UNPINNED: the package
 * is a third-party dependency absent from the reference tree (sr_environment.yml:165); restated from its published algorithm. */
int64_t srk_ssim_workspace(int B, int C, int H, int W);
int srk_ssim(const float* x, const float* y, void* workspace, int B, int C, int H, int W, float data_range, float* per_image, float* mean,
             srk_stream_t stream);
/* Benchmark-protocol PSNR / SSIM: the scores the SwinIR / HAT / DAT papers report -- 8-bit, border-cropped, on the
 * BT.601 luma or on the colour planes, on a 0..255 scale, per image.  One definition, all in fp32:
 *   quantise  q(x) = rintf(c(x) * 255.0f); c clamps to [0, 1] by comparisons (x < 0 -> 0, x > 1 -> 1, else x), so a NaN stays a
 *             NaN and reaches the result; one multiply, then round-half-to-even (numpy's .round() in the published test
 *             scripts; NOT the truncation of a PNG dump)
 *   crop      rows [border, H - border), columns [border, W - border): Hc x Wc = (H - 2 border) x (W - 2 border)
 *   mode Y    C == 3: one plane, t = 65.481f * qR; t = fmaf(128.553f, qG, t); t = fmaf(24.966f, qB, t); Y = 16.0f + t / 255.0f
 *             (one IEEE division, one add); C == 1: the plane is q itself (a single-channel image is its own luma)
 *   mode RGB  the C planes of q, any C >= 1
 *   PSNR      10 log10(255^2 / mse), mse = sqsum / (Cm Hc Wc) over the cropped planes of ONE image; mse == 0 gives +inf; sums in
 *             fp32 in a fixed order, no atomics
 *   SSIM      srk_ssim on the planes with data_range 255 (needs Hc, Wc >= 11).  Restated from the published algorithm: PARITY
 *             with the third-party test scripts (BasicSR, OpenCV) is UNPINNED, neither is available to compare with.
 * srk_bench_planes_f32: pred / target fp32 [B][C][H][W] -> planes_pred / planes_target fp32 [B][Cm][Hc][Wc] (Cm = 1 in mode Y,
 * C in mode RGB; either may be null: nothing is written for it) and, in the same pass, the per-workgroup sums of the squared
 * plane differences into workspace (srk_bench_workspace(B, Cm, Hc, Wc) bytes, caller-owned).  Every input element inside the crop
 * is read once, none outside it; nothing outside the planes and the workspace is written.
 * srk_bench_psnr: finishes that workspace: sqsum[b], psnr[b] (fp32 [B], either may be null) and psnr_sum[0] += sum_b psnr[b]
 * (may be null; zero it before the first batch, read it once after the last, like srk_batch_psnr's).
 * SRK_E_NULL: null pred / target / workspace; all three outputs of srk_bench_psnr null.  SRK_E_SHAPE: B outside 1..1024, a
 * non-positive extent, border < 0, 2 border >= H or W, an unknown mode, mode Y with C other than 1 or 3, C * H beyond 2^31 - 1,
 * planes overlapping an input.  srk_bench_workspace returns 0 for such arguments. */
#define SRK_BENCH_Y 0
#define SRK_BENCH_RGB 1
int64_t srk_bench_workspace(int B, int Cm, int Hc, int Wc);
int srk_bench_planes_f32(const float* pred, const float* target, float* planes_pred, float* planes_target, void* workspace, int B, int C,
                         int H, int W, int border, int mode, srk_stream_t stream);
int srk_bench_psnr(const void* workspace, int B, int Cm, int Hc, int Wc, float* sqsum, float* psnr, float* psnr_sum,
                   srk_stream_t stream);
/* No-reference quality (NIQE): Mittal et al., "Making a completely blind image quality analyzer", in the form of BasicSR's
 * calculate_niqe, the score the Real-ESRGAN / BSRGAN / SwinIR real-SR papers print for files without ground truth.  Restated from the
 * published algorithm: PARITY UNPINNED (neither BasicSR, pyiqa, OpenCV nor the MATLAB code is available to compare with); tests hold it
 * against an independent fp64 restatement (tests/niqe_ref.py).  The device computes the four stages below; the AGGD fit, the
 * 36-dimensional Gaussian and the distance are host fp64 (niqe.py).  One definition:
 *   plane     x fp32 [B][C][H][W] in [0, 1], C 1 or 3.  q = rintf(c(x) * 255.0f), c the comparison clamp of srk_bench_planes_f32 (a NaN
 *             stays).  C == 3: Y = rintf(16.0f + t / 255.0f), t the fma chain of srk_bench_planes_f32 (BasicSR rounds the luma); C == 1:
 *             the plane is q.  `border` pixels are cropped on every side, then the top-left Hk x Wk is kept, Hk = floor((H - 2 border) /
 *             bs) * bs, Wk likewise; bs is the block side (published: 96; any even bs >= 8).  The plane is integer-valued, 0..255.
 *   half      scale 2 is the half-size antialiased cubic (a = -0.5) of the plane in the MATLAB imresize(., 0.5) convention: per axis
 *             out[i] = sum_k T[k] in[2 i - 3 + k] / 256, T = [-3, -9, 29, 111, 111, 29, -9, -3], symmetric border (index -1-k -> k,
 *             n+k -> n-1-k).  Both passes are formed in int32 (the plane holds integers: |S| <= 304^2 * 255, exact, so the order of the
 *             passes does not show); out = (float)S * 2^-16, one rounding.  A plane that does not hold integers 0..255 gives no defined
 *             value (and no fault: the samples are converted to int).
 *   MSCN      under a 7 x 7 window w (49 fp32 taps in row-major order, device memory, not assumed separable; replicate border), in the
 *             centred form: d = v - v_centre (exact); a = sum w d and b = sum w d^2 by fmaf over the taps in row-major order;
 *             sigma = sqrtf(fabsf(b - a a)); m = -a / (sigma + 1.0f).  For sum w = 1 this is BasicSR's (v - mu) / (sqrt|E[v^2] - mu^2| + 1);
 *             the naive form cancels at 255^2 in fp32 (max |dm| 7e-3 on smooth images against 2e-7 for the centred form).  One
 *             divergence: on an exactly flat 7 x 7 neighbourhood m is exactly 0 (such a pixel counts on neither side below), where fp64
 *             BasicSR yields +-1e-14 noise of either sign.
 *   moments   blocks of bs x bs pixels (bs at scale 1, bs / 2 at scale 2: the same grid of nbh x nbw blocks).  Five maps per block: m, and
 *             m * roll(m, s) for s = (0,1), (1,0), (1,1), (1,-1), the roll circular inside the block (np.roll of the block), each product
 *             one fp32 multiply.  Per map five numbers: count of p < 0, sum of p^2 over p < 0, count of p > 0, sum of p^2 over p > 0,
 *             sum of |p| -> mom fp32 [B][nbh nbw][5][5].  Sums are fp32 in a fixed order, no atomics: two runs give equal bits.  sharp
 *             fp32 [B][nbh nbw]: the block mean of sigma (what the pristine fit selects blocks by).
 * srk_niqe_plane_f32: x -> plane fp32 [B][Hk][Wk].  srk_niqe_half_f32: plane fp32 [B][H][W], H and W even and >= 4 -> half fp32
 * [B][H/2][W/2].  srk_niqe_mscn_f32: plane [B][H][W], any H, W >= 1 -> mscn and (nullable) sigma, fp32 [B][H][W].
 * srk_niqe_moments_f32: mscn (and sigma, nullable together with sharp) [B][H][W], H and W multiples of bs; bs in 4..4096 here, any parity
 * (the scale-2 call passes half of an even block side >= 8; counts stay exact in fp32).  No workspace; nothing outside the stated outputs
 * is written; the library allocates nothing.
 * SRK_E_NULL: a null pointer (sigma without sharp or sharp without sigma included).  SRK_E_SHAPE: B outside 1..65535, an extent outside
 * 1..2^20, C not 1 or 3, border < 0, bs odd or < 8 (plane; outside 4..4096 for moments), H or W odd or < 4 (half), H or W not a multiple
 * of bs (moments), a grid that does not fit, an output overlapping another buffer.  SRK_E_UNSUPPORTED: fewer than one block (plane:
 * after the border crop; moments: H or W < bs). */
int srk_niqe_plane_f32(const float* x, float* plane, int B, int C, int H, int W, int border, int bs, srk_stream_t stream);
int srk_niqe_half_f32(const float* plane, float* half, int B, int H, int W, srk_stream_t stream);
int srk_niqe_mscn_f32(const float* plane, const float* win49, float* mscn, float* sigma, int B, int H, int W, srk_stream_t stream);
int srk_niqe_moments_f32(const float* mscn, const float* sigma, float* mom, float* sharp, int B, int H, int W, int bs,
                         srk_stream_t stream);
/* Full-reference scores: PSNR-B, MS-SSIM: two scores of image files against ground truth that the papers this library follows
 * print -- PSNR-B (Yim & Bovik, "Quality assessment of deblocked images") in the form of SwinIR's calculate_psnrb, beside PSNR and SSIM in
 * every JPEG-artifact table, and MS-SSIM (Wang, Simoncelli & Bovik 2003) in the form of pytorch_msssim.ms_ssim, the package srk_ssim
 * restates.  Neither the SwinIR / BasicSR test scripts nor pytorch_msssim is available to compare with: both are restated from the
 * published algorithms, PARITY UNPINNED; tests hold them against an independent fp64 restatement (tests/fullref_ref.py).  Both work on
 * the planes of srk_bench_planes_f32: 8-bit quantised, border-cropped, BT.601 luma or colour planes, scale 0..255, fp32 [B][Cm][Hc][Wc].
 * PSNR-B, per image and plane c, p the RESTORED plane and t the target:
 *   mse_c     mean of (p - t)^2
 *   D sums    the boundary columns are x = 7, 15, 23, ... with x < Wc - 1, the boundary rows likewise with Hc.  Dh_b = sum over all rows
 *             and boundary columns of (p[y][x] - p[y][x+1])^2, Dh_n the same sum over the other columns 0 <= x <= Wc - 2; Dv_b, Dv_n the
 *             same two sums along the rows.  fp32, each term one fmaf, a fixed order, no atomics: two runs give equal bits
 *   counts    AS PUBLISHED: n_bh = Hc (Wc / 8 - 1), n_bv = Wc (Hc / 8 - 1) (integer divisions), n_nh = Hc (Wc - 1) - n_bh,
 *             n_nv = Wc (Hc - 1) - n_bv.  For an extent that is 1 (mod 8) the sums hold one more boundary line than n_b* counts
 *             (Wc = 17: columns 7 and 15, n_bh = Hc); the published counts are kept
 *   bef_c     D_b = (Dh_b + Dv_b) / (n_bh + n_bv), D_n = (Dh_n + Dv_n) / (n_nh + n_nv);
 *             bef_c = (3 / log2(min(Hc, Wc))) (D_b - D_n) if D_b > D_n, else 0
 *   psnrb     mean over c of 10 log10(255^2 / (mse_c + bef_c)); a zero denominator gives +inf; a NaN in a plane reaches the result
 * srk_psnrb: one streaming pass (a workgroup takes a run of rows of one plane and reads the one row below it: every plane element is read
 * by at most two workgroups) into workspace (srk_psnrb_workspace(B, Cm, Hc, Wc) bytes, caller-owned), then one finishing workgroup.
 * sums fp32 [B][Cm][5] = (sum of (p - t)^2, Dh_b, Dh_n, Dv_b, Dv_n), psnrb fp32 [B]; either may be null.  Nothing outside the outputs and
 * the workspace is written.  SRK_E_NULL: null planes / workspace, both outputs null.  SRK_E_SHAPE: B outside 1..1024, B Cm >= 65536, a
 * non-positive extent, Cm * Hc beyond 2^31 - 1, an output or the workspace overlapping an input.  SRK_E_UNSUPPORTED: Hc < 16 or Wc < 16
 * (no block boundary: the published code divides 0 by 0).  srk_psnrb_workspace returns 0 for all of these.
 * MS-SSIM, `levels` levels (published: 5, weights 0.0448, 0.2856, 0.3001, 0.2363, 0.1333):
 *   level s   srk_ssim's map quantities on the current planes: the same 11-tap Gaussian, VALID filter and K, C1 = (0.01 data_range)^2,
 *             C2 = (0.03 data_range)^2.  Two per-channel means: S = mean of the SSIM map, CS = mean of (2 s12 + C2) / (s11 + s22 + C2)
 *   between   both images pass through avg_pool2d(kernel 2, stride 2, padding = extent % 2, count_include_pad=True): an odd extent gains
 *             one line of zeros in front, that cell is still divided by 4, the output extent is (n + n % 2) / 2; a pooled value is
 *             ((a + b) + (c + d)) * 0.25f, row-major.  Integer planes 0..255 stay exactly representable through four poolings
 *   score     per channel ms_c = prod_{s < levels - 1} max(CS_s,c, 0)^w_s * max(S_{levels-1},c, 0)^w_{levels-1}; per image the mean over the
 *             channels.  The product is the caller's (metrics.ms_ssim forms it in host fp64)
 * srk_msssim: x, y fp32 [B][C][H][W] -> means fp32 [levels][B][C][2] = (S, CS).  One launch per level -- it also writes the pooled planes of
 * both images for the next level from the tile it holds, each pooled cell by exactly one workgroup -- and one finishing launch.  workspace:
 * srk_msssim_workspace(B, C, H, W, levels) bytes, caller-owned; in floats, level s = 1 .. levels - 1 in order: the pooled x planes
 * [B][C][H_s][W_s], then the pooled y planes; behind them the per-tile sums.  Fixed-order sums: two runs give equal bits.
 * SRK_E_NULL: a null pointer.  SRK_E_SHAPE: B, C outside srk_ssim's limits (B <= 1024, B C < 65536), levels outside 1..5, H or W outside
 * 1..2^20, data_range <= 0, means or the workspace overlapping an input or each other.  SRK_E_UNSUPPORTED: the smaller side not above
 * 10 * 2^(levels - 1) (160 for five levels: the coarsest planes must hold the window).  srk_msssim_workspace returns 0 for all of these. */
int64_t srk_psnrb_workspace(int B, int Cm, int Hc, int Wc);
int srk_psnrb(const float* planes_pred, const float* planes_target, void* workspace, int B, int Cm, int Hc, int Wc, float* sums, float* psnrb,
              srk_stream_t stream);
int64_t srk_msssim_workspace(int B, int C, int H, int W, int levels);
int srk_msssim(const float* x, const float* y, void* workspace, int B, int C, int H, int W, int levels, float data_range, float* means,
               srk_stream_t stream);
/* sum of squares of a flat fp32 gradient, ACCUMULATED into sumsq[0] (for clip_grad_norm_ :170) */
int srk_grad_sumsq(const float* grads, int64_t n, float* sumsq, srk_stream_t stream);
/* clip_grad_norm_(max_norm) + AdamW step (:168-171, :303) on flat fp32 buffers.  The clip coefficient is
 * computed on the device from sumsq[0] (no host sync); grads are first divided by grad_div (world size).
 * max_norm <= 0 disables clipping.  step is the 1-based step count.  nonfinite: optional DEVICE counter (the one
 * srk_l1_loss_fwd_bwd fills, :133-143); when it is non-zero, or when the gradient norm itself is NaN/Inf, the call leaves
 * params and both moments untouched -- the reference raises before backward/step (:159-165), so the weights survive the raise.
 * beta1 / beta2 are read as the decimals they were written as (the shortest decimal that rounds to the fp32): 1 - beta and the bias
 * corrections are formed from it in fp64 and rounded once, as torch does. */
int srk_adamw_clip_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                        const float* sumsq, float max_norm, float grad_div, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int step, const int32_t* nonfinite, srk_stream_t stream);
/* srk_adamw_clip_step that also keeps an exponential moving average of the weights: after the update of element i,
 * ema[i] = ema_decay * ema[i] + (1 - ema_decay) * params[i] with the NEW params[i] (still in a register: one more read and one more
 * write of an fp32 array).  params / exp_avg / exp_avg_sq come out bit for bit as from srk_adamw_clip_step.  A gated call (nonfinite,
 * NaN / Inf norm) leaves ema untouched together with the weights and moments.  ema_decay in [0, 1) (else SRK_E_SHAPE; NaN too); it is
 * read as the decimal it was written as, like the betas.  ema_decay = 0 copies the weights.  Null ema: SRK_E_NULL. */
int srk_adamw_clip_ema_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                            const float* sumsq, float max_norm, float grad_div, float lr, float beta1, float beta2, float eps,
                            float weight_decay, int step, float ema_decay, const int32_t* nonfinite, srk_stream_t stream);
/* The same two over a LIST of separate fp32 tensors (the parameters of a host-orchestrated model: HAT, DAT), in the multi-tensor-apply
 * form: grads / params / exp_avg / exp_avg_sq are HOST arrays of n_tensors DEVICE pointers, numel the element counts (>= 0; a tensor
 * of 0 elements is skipped).  The table of a chunk of tensors travels by value in the kernel arguments: no upload, no allocation, no
 * host wait, so both calls can be captured into a hipGraph; launches per call = ceil(n_tensors / chunk), chunk = 160 (sumsq) / 80
 * (step).  Tensors need 4-byte alignment only (16-byte access where every pointer of a tensor allows it).
 * srk_multi_grad_sumsq ACCUMULATES the total sum of squares into sumsq[0].
 * srk_multi_adamw_clip_step: the arithmetic, the gate (nonfinite, NaN / Inf norm) and the arguments of srk_adamw_clip_step, element for
 * element the same function.  hyper: optional DEVICE {lr, 1 - beta1^step, sqrt(1 - beta2^step)} (what srk_adamw_hyper computes on the
 * host); when given it replaces lr and step, so a captured launch follows the learning rate and the step count that the host writes
 * there before every replay.  SRK_E_SHAPE: n_tensors <= 0, a negative count, step < 1, grad_div <= 0; SRK_E_NULL: a null list, or a null entry
 * with a non-zero count. */
int srk_multi_grad_sumsq(const float* const* grads, const int64_t* numel, int n_tensors, float* sumsq, srk_stream_t stream);
int srk_multi_adamw_clip_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                              const int64_t* numel, int n_tensors, const float* sumsq, float max_norm, float grad_div, float lr,
                              float beta1, float beta2, float eps, float weight_decay, int step, const float* hyper,
                              const int32_t* nonfinite, srk_stream_t stream);
/* srk_multi_adamw_clip_step with the EMA of srk_adamw_clip_ema_step: ema is a fifth HOST array of n_tensors DEVICE pointers.  The
 * chunk is 72 tensors (a fifth pointer per tensor in the by-value table), so launches per call = ceil(n_tensors / 72); the call
 * without EMA keeps its 80.  ema_decay is a launch-time constant (frozen into a captured launch); hyper as above.  Checks of
 * srk_multi_adamw_clip_step, plus SRK_E_NULL for a null ema list or a null ema[i] with a non-zero count and SRK_E_SHAPE for an
 * ema_decay outside [0, 1) or NaN. */
int srk_multi_adamw_clip_ema_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                                  float* const* ema, const int64_t* numel, int n_tensors, const float* sumsq, float max_norm,
                                  float grad_div, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                                  float ema_decay, const float* hyper, const int32_t* nonfinite, srk_stream_t stream);
/* HOST: out3 = {lr, 1 - beta1^step, sqrt(1 - beta2^step)} exactly as the step kernels' launchers compute them. */
int srk_adamw_hyper(float lr, float beta1, float beta2, int step, float* out3);

/* ---- generic GEMM / 3x3 conv with the fused epilogues, for host-orchestrated models (HAT: tpu_superresolution_amd/hat_arch.py)
 * D[m][n] = sum_k A[m][k] W[n][k] (+ epilogue).  A bf16: SRK_LD_ROWS [M][lda]; SRK_LD_CONV3 NHWC [B][H][Wd][CinP] (3x3, pad 1,
 * K = 9 * CinP tap-major).  W bf16 [N][K].  N % 64 == 0 (N == 16 for the image head), K % 64 == 0. */
enum { SRK_LD_ROWS = 0, SRK_LD_CONV3 = 1,
       SRK_LD_CONV3_PS = 2 /* 3x3 conv whose NHWC source is stored pixel-shuffled by r (Cs stored channels): dgrad of conv + PixelShuffle */ };
enum { SRK_EP_BF16 = 0,       /* outb = bf16(v + bias) */
       SRK_EP_GELU = 3,       /* outb2 = bf16(gelu(u)), u = v + bias; outb = bf16(u) if not null (kept for a backward pass) */
       SRK_EP_RES = 4,        /* outf = res + v + bias (fp32) [+ outb bf16 copy] [+ LayerNorm of the new row -> xn_out, N == 64/128/192] */
       SRK_EP_LRELU = 6,      /* outb = bf16(leaky_relu(v + bias, scale)) */
       SRK_EP_PS = 7,         /* conv + PixelShuffle(r): W rows permuted to (i*r + j)*Cs + c; store is the shuffled NHWC tensor */
       SRK_EP_IMG = 8,        /* N == 16: outf NCHW image [B][Cimg][Hc][Wc] = v * inv_range + mean[c] (crop) */
       SRK_EP_PS_IMG = 9,     /* N == 16: conv + PixelShuffle(r) straight into the NCHW image (UpsampleOneStep), n = c*r*r + i*r + j */
       SRK_EP_RES_BF16 = 10,  /* outb = bf16(res + v + bias) */
       SRK_EP_DGELU = 5,      /* outb = bf16(v * gelu'(aux))            (backward through an exact-erf GELU; aux = pre-activation) */
       SRK_EP_DLRELU = 11,    /* outb = bf16(v * (aux > 0 ? 1 : scale)) (backward through LeakyReLU; aux = its output) */
       SRK_EP_F32_BF16 = 12,  /* outf = v (fp32) [+ outb = bf16(v)] */
       SRK_EP_LNBWD = 13,     /* v = gradient of a LayerNorm OUTPUT row (N = the padded width, <= 192): LayerNorm backward through (ln_x, ln_mean,
                                 ln_rstd, ln_gamma) fused in: outf += d x in place (fp32 gradient stream), outb = bf16(outf * rowscale) or null,
                                 ln_dgamma / ln_dbeta ACCUMULATED.  A dgrad GEMM whose consumer is a LayerNorm backward (no bias) */
       SRK_EP_MLP_FUSED = 100 /* (reserved; see srk_mlp_fused_fwd) */ };
typedef struct {
  int loader, epilogue;
  const void* A; int lda;
  const void* W;
  int M, N, K;
  int B, H, Wd, CinP;          /* conv geometry (M == B*H*Wd) */
  int r, Cs;                   /* SRK_EP_PS */
  const float* bias;
  float* outf; void* outb; void* outb2;
  const float* res; const void* aux;
  int ldo;                     /* row stride (elements) of outf / outb / res */
  float scale;                 /* SRK_EP_LRELU slope */
  float inv_range; float mean[4]; int Cimg, Hc, Wc;     /* SRK_EP_IMG */
  void* xn_out; float* xn_mean; float* xn_rstd; const float* xn_gamma; const float* xn_beta; int xn_C;   /* SRK_EP_RES fused LayerNorm */
  const float* rowscale; int rows_per_sample;   /* SRK_EP_RES: outf = res + rowscale[m / rows_per_sample] * (v + bias)  (DropPath factor per sample) or null */
  const float* ln_x; const float* ln_mean; const float* ln_rstd; const float* ln_gamma; float* ln_dgamma; float* ln_dbeta; int ln_C;   /* SRK_EP_LNBWD */
} srk_gemm_args;
/* Checked on the host before any launch: SRK_E_NULL when an output / operand the epilogue needs is null (outb: BF16 / LRELU / RES_BF16 /
 * PS / DGELU / DLRELU; outb2: GELU; outf: RES / IMG / PS_IMG / F32_BF16 / LNBWD; res: RES / RES_BF16; aux: DGELU / DLRELU); SRK_E_SHAPE
 * for an image head without N == 16, 1 <= Cimg <= 4, Cimg * r * r <= 16 (PS_IMG, r >= 1), 0 < Hc <= H * r, 0 < Wc <= Wd * r (r = 1
 * for IMG); for PS without r >= 1, Cs % 64 == 0, N == r * r * Cs; for a fused LayerNorm without 0 < xn_C <= N and ldo == N;
 * SRK_E_UNSUPPORTED for a (loader, epilogue) pair that is not built (LD_ROWS: BF16 GELU RES RES_BF16 LRELU DGELU DLRELU LNBWD;
 * LD_CONV3: all but LNBWD; LD_CONV3_PS: BF16 DLRELU). */
int srk_gemm_ex(const srk_gemm_args* args, srk_stream_t stream);
/* Mlp.forward + residual (+ next LayerNorm) in one kernel (csrc/gemm_stream.hip): out = res + gelu(xn W1^T + b1) W2^T + b2.
 * xn bf16 [M][192], W1 bf16 [384][192], W2 bf16 [192][384], res / out fp32 [M][192]; C 180 / hidden 360 zero-padded. */
int srk_mlp_fused_fwd(const uint16_t* xn, const uint16_t* w1, const float* b1, const uint16_t* w2, const float* b2, const float* res,
                      float* out, uint16_t* out_bf16, uint16_t* xn_next, float* xn_mean, float* xn_rstd, const float* xn_gamma,
                      const float* xn_beta, int xn_C, int M, srk_stream_t stream);
/* SwinTransformerBlock.forward (network_swinir.py:239-279: LN1, roll + window partition, WindowAttention :114-145, reverse, residual,
 * LN2, Mlp :25-28, residual) as ONE kernel at the SwinIR-light width (csrc/block_light.hip; inference, no DropPath).
 * x, y: fp32 [B*H*W][64] token-major, channels >= C zero (y may alias x); y_bf16: optional bf16 copy of y.  Packed bf16 weights:
 * wqkv [3*192][64] (row = which*192 + head*32 + d), wproj [64][192] (column = head*32 + d), w1 [128][64], w2 [64][128]; fp32
 * biases in the same padded order; bias_dense [6][64][64] = table[rpi]; C <= 64, num_heads == 6, head_dim <= 16, hidden <= 128,
 * H and W multiples of 8, shift 0 or 4.  Checked on the host before any launch: SRK_E_NULL for a null operand (y_bf16 and the four
 * biases may be null: no copy, a zero bias); SRK_E_SHAPE unless B, H, W > 0, H and W multiples of 8, shift 0 or 4, 0 < C <= 64,
 * 0 < hidden <= 128, num_heads * head_dim == C; SRK_E_ALIGN unless x, y, the four weights, the biases that are given and bias_dense
 * are 16-byte aligned (float4 / eight-bf16 accesses) and y_bf16 is 8-byte aligned; SRK_E_UNSUPPORTED for any other width (heads
 * other than 6, head_dim > 16) and when the option "block_light" is 0 (the message names the option). */
int srk_swin_block_fwd(const float* x, float* y, uint16_t* y_bf16, const float* norm1_w, const float* norm1_b, const float* norm2_w,
                       const float* norm2_b, const uint16_t* wqkv, const float* bqkv, const uint16_t* wproj, const float* bproj,
                       const uint16_t* w1, const float* b1, const uint16_t* w2, const float* b2, const float* bias_dense, float scale,
                       int C, int num_heads, int head_dim, int hidden, int B, int H, int W, int shift, srk_stream_t stream);
/* image -> padded, normalised NHWC4 (check_image_size + (x - mean) * range, hat_arch.py:963-975) and conv_first (fp32 VALU).
 * srk_img_prep: x fp32 NCHW [B][Cimg][H0][W0] -> out fp32 [B][H][W][4], 'reflect' padding at the bottom / right, one IEEE subtract and one
 * IEEE multiply per value, channels >= Cimg are +0.  SRK_E_NULL: null x / out / mean3; SRK_E_SHAPE unless B > 0, 1 <= Cimg <= 3,
 * H0 <= H < 2 H0, W0 <= W < 2 W0 (reflection needs pad <= extent - 1); SRK_E_ALIGN unless out is 16-byte aligned.
 * srk_stem_conv: img4 fp32 [B][H][W][4], weight fp32 [C][Cin][3][3], bias fp32 [C] -> out fp32 [B*H*W][CP], columns C..CP-1 are +0.
 * SRK_E_NULL for any null pointer; SRK_E_SHAPE unless B, H, W > 0, 1 <= Cin <= 4, 1 <= C <= CP, CP % 4 == 0, CP <= 256 (the kernel stages
 * (36 CP + 576) floats in LDS); SRK_E_ALIGN unless img4 and out are 16-byte aligned.  All checked on the host before any launch. */
int srk_img_prep(const float* x, float* out, int B, int Cimg, int H0, int W0, int H, int W, float range, const float* mean3, srk_stream_t stream);
int srk_stem_conv(const float* img4, const float* weight, const float* bias, float* out, int B, int H, int W, int Cin, int C, int CP,
                  srk_stream_t stream);

/* ---- HAT (reference hat_arch.py) ------------------------------------------------------------------------------------------------
 * Window attention with 256 queries per window, forward.  qkv bf16 [T][ldq] in RASTER token order straight from the qkv linear
 * (q | k | v at columns 0 / CA / 2 CA, head h at +32 h, head_dim zero-padded to 32, q NOT pre-scaled); out bf16 [T][ldo] raster.
 * bias: table_rows == 0: dense fp32 [num_heads][256][NK]; table_rows > 0 (16 x 16 windows): the relative_position_bias_table
 * parameter itself, fp32 [table_rows][num_heads] (961 rows, 1521 for the overlapping form) -- the kernel stages the head's
 * column in LDS and evaluates relative_position_index_SA / _OCA (:881-918) in closed form, negative OCA indices wrapped.  overlap == 0: (shifted) window self-attention, wh x ww windows with
 * wh * ww == 256 (WindowAttention.forward :163-197 + the roll / partition / reverse of HAB.forward :298-319; the shift mask of
 * calculate_mask :921-941 is evaluated arithmetically).  overlap == 8: overlapping cross-attention of OCAB.forward :403-432
 * (16 x 16 queries, 24 x 24 zero-padded keys, NK = 576). */
int srk_win256_attention_fwd(const uint16_t* qkv, int ldq, int CA, const float* bias, int table_rows, uint16_t* out, int ldo, int B, int H,
                             int W, int wh, int ww, int shift_y, int shift_x, int num_heads, float scale, int overlap, srk_stream_t stream);
/* The same with the H x W map zero-padded at the bottom / right to an Hp x Wp window frame (DAT: Adaptive_Spatial_Attention.forward
 * dat_arch.py:376-384 pads q, k, v to a multiple of the larger split; windows, cyclic shift and shift mask live on the frame, a padded
 * token is a zero vector that takes part in its window's softmax with score = bias, padded output rows are dropped) and with
 * windows of 256 OR 128 tokens (wh * ww; 128: split_size [8, 16], dense bias [num_heads][128][128]).  Hp, Wp multiples of wh, ww. */
int srk_win_attention_fwd_padded(const uint16_t* qkv, int ldq, int CA, const float* bias, int table_rows, uint16_t* out, int ldo, int B, int H,
                                 int W, int Hp, int Wp, int wh, int ww, int shift_y, int shift_x, int num_heads, float scale, int overlap,
                                 srk_stream_t stream);
/* ---- SwinIR with small windows (csrc/attn_small.hip) -------------------------------------------------------------------------------
 * (Shifted-)window attention forward for ws x ws windows, 2 <= ws <= 7 (N = ws^2 <= 49 tokens; WindowAttention.forward
 * network_swinir.py:114-145 + the roll / partition / reverse of SwinTransformerBlock.forward :240-279).  qkv bf16 [T][ldq] in RASTER
 * token order (q | k | v at columns 0 / CA / 2 CA, head h at +32 h, head_dim zero-padded to 32, q NOT pre-scaled); out bf16 [T][ldo]
 * raster.  table: the relative_position_bias_table parameter fp32 [(2 ws - 1)^2][num_heads], indexed in closed form; shift > 0 applies
 * the mask of calculate_mask :216-237 for the H x W map.  Windows are padded to 32 / 64 keys that are EXCLUDED from the softmax.
 * SRK_E_UNSUPPORTED outside 2 <= ws <= 7, SRK_E_SHAPE when H or W is not a multiple of ws. */
int srk_win_small_attention_fwd(const uint16_t* qkv, int ldq, int CA, const float* table, uint16_t* out, int ldo, int B, int H, int W,
                                int ws, int shift, int num_heads, float scale, srk_stream_t stream);
/* Gradient of srk_win_small_attention_fwd (csrc/attn_small_bwd.hip; WindowAttention.forward network_swinir.py:114-145 and the roll /
 * partition / reverse of SwinTransformerBlock.forward :240-279 backwards), same conventions: qkv as the forward read it; d_out bf16
 * [T][ldo] raster = gradient of the attention output (head h at columns 32 h, ldo % 8 == 0); d_qkv bf16 [T][ldq] in the layout of
 * qkv (q gradient w.r.t. the UNSCALED q, as qkv holds it) is WRITTEN: every element of rows 0 .. T - 1, columns 0 .. 3 CA - 1, nothing
 * else (no pre-zeroing; columns head_dim .. 31 of a head come out 0 when they are 0 in qkv and d_out); d_table fp32
 * [(2 ws - 1)^2][num_heads] is ACCUMULATED.  Padded queries and padded keys contribute exactly nothing.  scratch:
 * srk_win_small_attention_bwd_scratch bytes, 16-byte aligned, fully written before it is read (needs no zeroing).
 * SRK_E_UNSUPPORTED outside 2 <= ws <= 7, SRK_E_SHAPE when H or W is not a multiple of ws or shift is outside [0, ws). */
size_t srk_win_small_attention_bwd_scratch(int B, int H, int W, int ws, int num_heads);
int srk_win_small_attention_bwd(const uint16_t* qkv, int ldq, int CA, const float* table, const uint16_t* d_out, int ldo,
                                uint16_t* d_qkv, float* d_table, void* scratch, int B, int H, int W, int ws, int shift,
                                int num_heads, float scale, srk_stream_t stream);
/* ChannelAttention gate of CAB (:41-57): gate[b][c] = out_scale * sigmoid(W2 relu(W1 mean_b + b1) + b2), mean over the HW tokens
 * of x bf16 [B*HW][CP]; w1 [S][C], w2 [C][S] fp32 (the 1x1 convs).  workspace: srk_channel_gate_workspace bytes, fully written before
 * it is read (needs no zeroing).  The pad columns C..CP-1 of x are read (their sums land in the workspace) but their means are never
 * used: they may hold anything, NaN included.  Every element of gate fp32 [B][CP] is written: columns C..CP-1 receive +0.  The sums
 * run in a fixed order without atomics: two calls give the same bits.  SRK_E_NULL: a null pointer; SRK_E_SHAPE unless 1 <= B < 65536,
 * HW > 0, 1 <= C <= CP, CP % 64 == 0, CP <= 256, 1 <= S <= 64; SRK_E_ALIGN unless x is 16-byte aligned (eight bf16 per load).  All
 * checked on the host before any launch. */
size_t srk_channel_gate_workspace(int B, int HW, int CP);
int srk_channel_gate(const uint16_t* x, void* workspace, const float* w1, const float* b1, const float* w2, const float* b2, float out_scale,
                     float* gate, int B, int HW, int C, int CP, int S, srk_stream_t stream);
/* same with the hidden activation selectable: act 0 ReLU (HAT), 1 GELU (DAT's channel_interaction, dat_arch.py:315-321, BatchNorm folded) */
int srk_channel_gate_act(const uint16_t* x, void* workspace, const float* w1, const float* b1, const float* w2, const float* b2, float out_scale,
                         float* gate, int B, int HW, int C, int CP, int S, int act, srk_stream_t stream);
/* HAB.forward :322-323: x += conv * gate[sample] in place (fp32 [rows][CP]) and, if xn != null, xn = bf16(LayerNorm(x)) over the C real
 * columns (eps 1e-5, gamma / beta fp32 [C]); sample = row / rows_per_sample, gate fp32 [rows / rows_per_sample][CP] as srk_channel_gate
 * wrote it (pad columns 0).  All CP columns of x and conv are read and all CP columns of x written: a pad column of x receives
 * x + conv * 0, so the pad columns of conv must be finite.  The LayerNorm mean is taken from the sum over ALL CP columns: the pad columns
 * of x must be zero on entry (they stay zero); the variance runs over the C real columns only.  xn bf16 [rows][CP]: pad columns +0.
 * With xn == null gamma and beta may be null and only x is written.  SRK_E_NULL: null x / conv / gate, or xn without gamma / beta;
 * SRK_E_SHAPE unless rows > 0, rows_per_sample > 0 dividing rows, 1 <= C <= CP; SRK_E_ALIGN unless x and gate are 16-byte and conv and
 * xn 8-byte aligned; SRK_E_UNSUPPORTED for a CP other than 64 / 128 / 192 / 256.  All checked on the host before any launch. */
int srk_cab_add_ln(float* x, const uint16_t* conv, const float* gate, const float* gamma, const float* beta, uint16_t* xn, int64_t rows,
                   int rows_per_sample, int C, int CP, srk_stream_t stream);

/* ---- training pieces for the host-orchestrated models (csrc/hat_train.hip, csrc/attn256_bwd.hip) ----------------------------------
 * Gradient of srk_win256_attention_fwd (table-indexed bias, 16 x 16 windows; WindowAttention.forward hat_arch.py:163-197 and
 * OCAB.forward :403-439 backwards).  d_out bf16 [T][ldo] raster = gradient of the attention output; d_qkv bf16 [T][ldq] in the
 * layout of qkv (q gradient w.r.t. the UNSCALED q, as qkv holds it); d_table fp32 [table_rows][num_heads] is ACCUMULATED (the
 * negative relative_position_index_OCA entries wrap, :911-918); scratch: srk_win256_attention_bwd_scratch bytes.  In the
 * overlapping form the key / value gradients of a token are summed over the (up to four) key windows that hold it.  shift_y and
 * shift_x are independent, any 0 <= shift < 16 (the mask comes from the region labels of the slices (0, -16), (-16, -shift),
 * (-shift, end) per axis; the overlapping form takes no shift).  Every element of rows 0 .. T - 1, columns 0 .. 3 CA - 1 of d_qkv is
 * written; the scratch is fully written before it is read (needs no zeroing). */
size_t srk_win256_attention_bwd_scratch(int B, int H, int W, int num_heads, int CA, int table_rows, int overlap);
int srk_win256_attention_bwd(const uint16_t* qkv, int ldq, int CA, const float* table, int table_rows, const uint16_t* d_out, int ldo,
                             uint16_t* d_qkv, float* d_table, void* scratch, int B, int H, int W, int shift_y, int shift_x, int num_heads,
                             float scale, int overlap, srk_stream_t stream);
/* Gradient of `x += conv * gate[sample]`, gate = srk_channel_gate(conv) (HAB.forward :322 with CAB :41-75): g fp32 [B*HW][CP] is the
 * gradient of the sum, conv bf16 the second CAB conv's output, gate fp32 [B][CP] as the forward produced it.  d_conv bf16 [B*HW][CP] =
 * g * gate + (gradient through the average pool); dw1 [S][C], db1 [S], dw2 [C][S], db2 [C] are ACCUMULATED (float atomics, one addend per
 * sample); dmean fp32 [B][CP] scratch, fully written (the pool gradient per token; pad columns +0).  The hidden activation is ReLU.
 * workspace: srk_cab_bwd_workspace bytes, fully written before it is read.  The pad columns C..CP-1 of conv are read but never used
 * (anything, NaN included); those of g must be finite and those of gate zero: every column of d_conv is written and a pad column
 * receives bf16(g * gate + 0).  SRK_E_NULL: a null pointer; SRK_E_SHAPE unless 1 <= B < 65536, HW > 0, 1 <= C <= CP, CP % 64 == 0,
 * CP <= 256, 1 <= S <= 64; SRK_E_ALIGN unless conv, g, gate and dmean are 16-byte and d_conv 8-byte aligned.  All checked on the host
 * before any launch. */
size_t srk_cab_bwd_workspace(int B, int HW, int CP);
int srk_cab_bwd(const uint16_t* conv, const float* g, const float* gate, void* workspace, const float* w1, const float* b1, const float* w2,
                const float* b2, float out_scale, float* dw1, float* db1, float* dw2, float* db2, float* dmean, uint16_t* d_conv, int B, int HW,
                int C, int CP, int S, srk_stream_t stream);
/* LayerNorm backward over C of CP columns: dy bf16 [rows][CP]; x, mean, rstd as srk_layernorm_fwd saw / produced them;
 * gx fp32 [rows][CP] = (accumulate ? gx : 0) + dx; gx_bf16 (optional) = bf16(gx); dgamma / dbeta fp32 [C] ACCUMULATED (elements >= C are
 * not touched).  Pad columns C..CP-1: dx is 0 there, so with accumulate == 0 gx and gx_bf16 receive +0, and with accumulate == 1 gx keeps
 * the value it held (0 + old; a -0 becomes +0) and gx_bf16 receives bf16 of it -- a caller that wants zero pads under accumulate == 1 must
 * hand in a gx whose pads are zero.  SRK_E_NULL: a null pointer other than gx_bf16; SRK_E_SHAPE unless rows > 0, 1 <= C <= CP,
 * CP % 64 == 0, CP <= 256; SRK_E_ALIGN unless x and gx are 16-byte and dy and gx_bf16 8-byte aligned. */
int srk_layernorm_bwd(const uint16_t* dy, const float* x, const float* mean, const float* rstd, const float* gamma, float* gx,
                      uint16_t* gx_bf16, float* dgamma, float* dbeta, int rows, int C, int CP, int accumulate, srk_stream_t stream);
/* element-wise helpers of a backward pass: a += b and ab_bf16 = bf16(a); a += float(b); out = a + b.  Each is a fixed sequence of IEEE
 * fp32 operations (one add; one round-to-nearest-even conversion where bf16 is stored, NaN stays NaN; fp32 subnormals are neither
 * flushed on input nor on output).  SRK_E_NULL: a null pointer; SRK_E_SHAPE: n not a positive multiple of 4; SRK_E_ALIGN: an fp32 array
 * not 16-byte or a bf16 array not 8-byte aligned (float4 / four-bf16 accesses). */
int srk_add_f32_bf16(float* a, const float* b, uint16_t* ab_bf16, int64_t n, srk_stream_t stream);
int srk_add_bf16_into_f32(float* a, const uint16_t* b, int64_t n, srk_stream_t stream);
int srk_add_f32(float* out, const float* a, const float* b, int64_t n, srk_stream_t stream);
/* image head backwards: d_pred fp32 NCHW [B][Cimg][Hc][Wc] -> gy fp32 [B*H*W][CoP] (times inv_range; r > 1: un-pixel-shuffled, column
 * c*r*r + i*r + j of pixel (y, x) = d_pred[c][y*r + i][x*r + j]); columns >= Cimg*r*r and everything outside the Hc x Wc crop are zero.
 * SRK_E_SHAPE unless B, H, W > 0, r >= 1, CoP is 4 or 16, 1 <= Cimg, Cimg*r*r <= CoP, 0 < Hc <= H*r, 0 < Wc <= W*r.
 * srk_smallconv_wgrad / _dgrad: weight / input gradients of a 3x3 conv with few output channels (conv_last, UpsampleOneStep), fp32
 * parameters [Co][Cin][3][3]: dw and db [Co] are ACCUMULATED from x bf16 NHWC [..][CinP] and gy; dx bf16 NHWC [..][CinP] is WRITTEN (pad
 * channels >= Cin zero).  SRK_E_SHAPE unless B, H, W > 0, CoP is 4 or 16, 1 <= Co <= CoP, 1 <= Cin <= CinP, CinP % 64 == 0, CinP <= 256;
 * SRK_E_ALIGN unless x, gy and dx are 16-byte aligned; SRK_E_NULL for any null pointer (db included). */
int srk_img_grad_prep(const float* d_pred, float* gy, int B, int Cimg, int Hc, int Wc, int H, int W, int r, int CoP, float inv_range,
                      srk_stream_t stream);
int srk_smallconv_wgrad(const uint16_t* x, const float* gy, float* dw, float* db, int B, int H, int W, int Cin, int CinP, int Co, int CoP,
                        srk_stream_t stream);
int srk_smallconv_dgrad(const float* gy, const float* weight, uint16_t* dx, int B, int H, int W, int Cin, int CinP, int Co, int CoP,
                        srk_stream_t stream);
/* The same three launches for a WIDE one-step head, 17 .. 64 output channels padded to CoP = 32, 48 or 64 (csrc/headconv_wide.hip);
 * data contracts as above: d_pred fp32 NCHW, gy fp32 [B*H*W][CoP], x / dx bf16 NHWC [..][CinP], parameters fp32 [Co][Cin][3][3].
 * srk_widehead_grad_prep: the function of srk_img_grad_prep (one fp32 multiply per element: bit-exact; columns >= Cimg*r*r and
 * everything outside the Hc x Wc crop are zero).  srk_widehead_wgrad: dw and db [Co] are ACCUMULATED; every workgroup sums its run
 * of pixels in registers and adds it with fp32 atomics, so the rounding of the last bits depends on the order the workgroups finish
 * in (as the narrow kernel).  srk_widehead_dgrad: dx is WRITTEN, all CinP columns, the pad channels >= Cin as +0.  gy and the
 * weights enter the matrix cores as the fp32 values they are (v_mfma_f32_*_f32: an fp32 fmaf chain; no hi + lo bf16 split, no split
 * products); x converts exactly.  Any B, H, W > 0 gives the right answer, odd pixel counts included: the kernels walk flat pixel
 * indices and mask the taps that leave the image.  srk_widehead_wgrad keeps the x window of a run in LDS and reads x once when
 * W <= 95 (the light family's 64 x 64 training patches); wider images take the same kernel with the three 66-pixel row segments of
 * every 64-pixel chunk staged afresh (x read three times; same sums per workgroup).  srk_widehead_dgrad has one path.
 * SRK_E_NULL for any null pointer (db included); SRK_E_SHAPE unless B, H, W > 0, B*H*W < 2^31, CoP is 32, 48 or 64, and for the prep
 * 1 <= r <= 8, 1 <= Cimg, Cimg*r*r <= CoP, 0 < Hc <= H*r, 0 < Wc <= W*r (H*r, W*r < 2^31), for the conv gradients 1 <= Co <= CoP,
 * 1 <= Cin <= CinP, CinP % 64 == 0, CinP <= 256; SRK_E_ALIGN unless x, gy and dx are 16-byte aligned.  All checked on the host before
 * any HIP call.  srk_img_grad_prep / srk_smallconv_* keep their contract (CoP 4 or 16). */
int srk_widehead_grad_prep(const float* d_pred, float* gy, int B, int Cimg, int Hc, int Wc, int H, int W, int r, int CoP, float inv_range,
                           srk_stream_t stream);
int srk_widehead_wgrad(const uint16_t* x, const float* gy, float* dw, float* db, int B, int H, int W, int Cin, int CinP, int Co, int CoP,
                       srk_stream_t stream);
int srk_widehead_dgrad(const float* gy, const float* weight, uint16_t* dx, int B, int H, int W, int Cin, int CinP, int Co, int CoP,
                       srk_stream_t stream);
/* conv_first backwards: dw [C][Cin][3][3], db [C] ACCUMULATED from the padded NHWC4 image and gy fp32 [B*H*W][CP].  SRK_E_SHAPE unless
 * B, H, W > 0, 1 <= Cin <= 4, 1 <= C <= CP, C <= 256, CP % 4 == 0; SRK_E_ALIGN unless img4 and gy are 16-byte aligned.  With CP == 192, at
 * least 16384 pixels (a multiple of 32) and a registered workspace (srk_set_wgrad_workspace) the sums are formed in a fixed order. */
int srk_stem_wgrad(const float* img4, const float* gy, float* dw, float* db, int B, int H, int W, int Cin, int C, int CP, srk_stream_t stream);
/* srk_conv3x3_wgrad_bf16 with y stored pixel-shuffled by r (the gradient of a conv + PixelShuffle(r) output, Cs stored channels):
 * y bf16 [B][H*r][W*r][Cs], row n = (i*r + j)*Cs + c of dw takes y[b][h*r + i][w*r + j][c].  SRK_E_SHAPE unless B, H, W > 0, r >= 1,
 * Cs % 8 == 0 and N == r*r*Cs (and N % 64 == 0, CinP % 64 == 0); SRK_E_ALIGN unless y and x are 16-byte aligned. */
int srk_conv3x3_wgrad_ps_bf16(const uint16_t* y, const uint16_t* x, float* dw, float* db, int B, int H, int W, int CinP, int N, int r, int Cs,
                              srk_stream_t stream);
/* srk_mlp_fused_fwd that also stores u = xn W1^T + b1 and h = gelu(u) (bf16 [M][384]) for a backward pass */
int srk_mlp_fused_fwd_train(const uint16_t* xn, const uint16_t* w1, const float* b1, const uint16_t* w2, const float* b2, const float* res,
                            float* out, uint16_t* out_bf16, uint16_t* u_out, uint16_t* h_out, uint16_t* xn_next, float* xn_mean,
                            float* xn_rstd, const float* xn_gamma, const float* xn_beta, int xn_C, const float* rowscale, int rows_per_sample,
                            int M, srk_stream_t stream);
/* dst[m][c] = bf16(float(src[m][c]) * f[m / rows_per_sample])  (a DropPath factor on a bf16 gradient copy; dst may alias src; rows need
 * not be a multiple of rows_per_sample; one IEEE multiply, one round-to-nearest-even conversion).  SRK_E_NULL: a null pointer;
 * SRK_E_SHAPE unless rows > 0, rows_per_sample > 0 and CP is a positive multiple of 4; SRK_E_ALIGN unless src and dst are 8-byte aligned. */
int srk_rowscale_bf16(const uint16_t* src, uint16_t* dst, const float* f, int64_t rows, int rows_per_sample, int CP, srk_stream_t stream);

/* ---- DAT (reference dat_arch.py), inference pieces; token-major bf16 [T][ld], channels padded per head to 32 -------------------------
 * Depth-wise 3x3 conv, pad 1, over C8*8 channels of x (column 0 of the slice given): out = act((conv(x)) * scale + shift) * mul.
 * w fp32 [C8*8][9]; scale / shift fp32 [C8*8] carry the conv bias and an inference BatchNorm folded by the caller
 * (dat_arch.py:310-314, :463-467); act 0 none / 1 GELU; mul (optional) is SGFN's x1 in x1 * DWconv(LN(x2)) (:48-54). */
int srk_dwconv3x3(const uint16_t* x, int ldx, const float* w, const float* scale, const float* shift, const uint16_t* mul, int ldm, uint16_t* out,
                  int ldo, int B, int H, int W, int C8, int act, srk_stream_t stream);
/* The DW-conv branch of a DAT block with its BatchNorm FROZEN (eval mode inside a training step), ONE token pass with two outputs:
 * pre = bf16(conv(x) + bias)  (what the backward and the weight gradient read; bit-equal to srk_dwconv3x3 with scale = 1, shift = bias,
 * act 0) and out = bf16(gelu(pre * bn_scale + bn_shift)) evaluated on the rounded pre (bn_scale / bn_shift fp32 [C8*8]: rows 0 / 1 of
 * srk_bn_frozen_coeffs).  Replaces srk_dwconv3x3 + srk_chan_stats + srk_affine_act_bf16 of the batch-statistics path.
 * srk_dwconv3x3_bn_act_launches: launches of it in this process so far (tests assert that the path was taken). */
int srk_dwconv3x3_bn_act(const uint16_t* x, int ldx, const float* w, const float* bias, const float* bn_scale, const float* bn_shift, uint16_t* pre,
                         int ldpre, uint16_t* out, int ldo, int B, int H, int W, int C8, srk_stream_t stream);
long long srk_dwconv3x3_bn_act_launches(void);
/* LayerNorm (eps 1e-5) over C channels of a bf16 row slice -> bf16 [rows][ldo], columns C..CP_out-1 written as +0 (SpatialGate.norm :46).
 * Two-pass statistics (the variance from x - mean).  Columns C..CP_out-1 of x are never used (they may hold anything, NaN included);
 * columns >= CP_out of out are not written.  ldx >= the 8-column pieces that cover C and ldo >= CP_out are the caller's to keep: the
 * launcher checks only that both are multiples of 8. */
int srk_rowln_bf16(const uint16_t* x, int ldx, const float* gamma, const float* beta, uint16_t* out, int ldo, int64_t rows, int C, int CP_out,
                   srk_stream_t stream);
/* spatial_interaction (:322-327, :475-480): gate[t] = sigmoid(b3 + w3 . gelu(W0 x_t + b0)); W0 fp32 [S][CP] (BatchNorm folded, zero at pads) */
int srk_spatial_gate(const uint16_t* x, int ldx, const float* W0, const float* b0, const float* w3, float b3, int S, float* gate, int64_t rows,
                     int CP, srk_stream_t stream);
/* the same with b3 read from device memory (a parameter that changes every training step: no host round trip) */
int srk_spatial_gate_dev(const uint16_t* x, int ldx, const float* W0, const float* b0, const float* w3, const float* b3, int S, float* gate,
                         int64_t rows, int CP, srk_stream_t stream);
/* out = a * ga + b * gb with one gate per token (tgate [rows]) and one per (sample, channel) (cgate [B][CP]); tok_gate_on_a selects
 * which operand takes the token gate (:430-436 spatial block: 0; :518-524 channel block: 1).  Gates are post-sigmoid.
 * a, b and out are contiguous [rows][CP]: the entry point takes no row stride. */
int srk_dual_gate_combine(const uint16_t* a, const uint16_t* b, const float* cgate, const float* tgate, uint16_t* out, int64_t rows,
                          int rows_per_sample, int CP, int tok_gate_on_a, srk_stream_t stream);
/* Adaptive_Channel_Attention core (:481-505): per sample and head, q / k columns L2-normalised over the N tokens, logits
 * (d x d) * temperature[h], softmax, applied to v.  qkv bf16 [B*N][ldq] (q | k | v at 0 / CA / 2 CA, head h at +32 h); out bf16
 * [B*N][ldo] (head-padded channels).  Fixed-order reductions. */
size_t srk_channel_attention_workspace(int B, int N, int num_heads);
int srk_channel_attention_fwd(const uint16_t* qkv, int ldq, int CA, const float* temperature, void* workspace, uint16_t* out, int ldo, int B,
                              int N, int num_heads, int head_dim, srk_stream_t stream);

/* Backward of Mlp + residual + the LayerNorm in front of it as ONE kernel (autograd of hat_arch.py:86-92 + :324 / network_swinir.py:25-28
 * + :277): d u = (g W2) * gelu'(u) -> du_out, d xn = d u W1, LayerNorm backward through (ln_x, mean, rstd, gamma): gx += d x in place
 * (fp32), gxb = bf16(gx * rowscale[row / rows_per_sample]) (or null), d_gamma / d_beta ACCUMULATED.  Layouts as srk_mlp_fused_fwd with
 * the weights transposed: w2t [384][192], w1t [192][384]; C = 180, M % 64 == 0, M >= 64 * #CUs, else SRK_E_UNSUPPORTED. */
int srk_mlp_fused_bwd(const uint16_t* g, const uint16_t* w2t, const uint16_t* u, uint16_t* du_out, const uint16_t* w1t, const float* ln_x,
                      const float* ln_mean, const float* ln_rstd, const float* ln_gamma, float* gx, uint16_t* gxb, const float* rowscale,
                      int rows_per_sample, float* d_gamma, float* d_beta, int C, int M, srk_stream_t stream);

/* ---- the fused per-block Swin kernels in the form the SwinIR executor launches them (csrc/hat_train.hip; for parity tests and
 * host-orchestrated models).  Every buffer 16-byte aligned (else SRK_E_ALIGN); a srk_win_geom needs H, W multiples of 8, shift 0 or 4
 * and a row count that is a multiple of H*W (else SRK_E_SHAPE); "not covered" is SRK_E_UNSUPPORTED with a message, nothing written. */
/* srk_mlp_fused_fwd_train plus: u_out / h_out may BOTH be null (inference); u_dgelu != 0: u_out receives bf16(gelu'(u)) of the unrounded
 * u instead of bf16(u) (needs u_out; what srk_mlp_fused_bwd_ex reads with u_is_dgelu); xn_geom non-null: xn_next / xn_mean / xn_rstd rows
 * are in WINDOW order of that geometry (the next block's norm1 with its roll + window partition), null: token order. */
int srk_mlp_fused_fwd_ex(const uint16_t* xn, const uint16_t* w1, const float* b1, const uint16_t* w2, const float* b2, const float* res,
                         float* out, uint16_t* out_bf16, uint16_t* u_out, uint16_t* h_out, int u_dgelu, uint16_t* xn_next, float* xn_mean,
                         float* xn_rstd, const float* xn_gamma, const float* xn_beta, int xn_C, const srk_win_geom* xn_geom,
                         const float* rowscale, int rows_per_sample, int M, srk_stream_t stream);
/* srk_mlp_fused_bwd plus: u_is_dgelu != 0: u holds gelu'(u) (d u = bf16((g W2) * u)); out_geom non-null: row t of the bf16 copy gxb is
 * stored at its WINDOW-order row of that geometry (gx, ln_x, the statistics and rowscale stay in token order). */
int srk_mlp_fused_bwd_ex(const uint16_t* g, const uint16_t* w2t, const uint16_t* u, int u_is_dgelu, uint16_t* du_out, const uint16_t* w1t,
                         const float* ln_x, const float* ln_mean, const float* ln_rstd, const float* ln_gamma, float* gx, uint16_t* gxb,
                         const srk_win_geom* out_geom, const float* rowscale, int rows_per_sample, float* d_gamma, float* d_beta, int C, int M,
                         srk_stream_t stream);
/* launches of the fused MLP kernels in this process so far, per (backward, u holds gelu'(u)) variant */
long long srk_mlp_fused_launches(int backward, int u_dgelu);
/* qkv projection + window attention forward as one kernel per window (csrc/attn_fused.hip; network_swinir.py:121-142), whichever kernel
 * option "attn_fused" selects (2: three 4-wave workgroups per CU, falling back to 1: one 8-wave workgroup per CU, when its configuration
 * fails; 0 and every shape the kernels do not cover -- nH != 6, B_ < #CUs -- is SRK_E_UNSUPPORTED).  xn bf16 [B_*64][lda] norm1 output in
 * window order, w_qkv bf16 [576][192] / b_qkv fp32 [576] or null (q rows first, heads padded 30 -> 32), qkv_out bf16 [3][B_][6][64][32]
 * or null, out bf16 [B_*64][192].  bias_dense fp32 [6][64][64]: the kernels rebuild the 225-entry relative-position table from it (offset
 * (dy, dx) is read at query (max(dy,0), max(dx,0)), key (max(-dy,0), max(-dx,0))), so it must be table[relative_position_index] as
 * srk_rel_pos_bias_expand writes it -- an arbitrary dense bias is NOT supported.  srk_qkv_attn_fwd3_launches / ..._fwd8_launches:
 * launches of the 4-wave / 8-wave kernel in this process so far (tests assert which one ran). */
int srk_qkv_window_attention_fwd(const uint16_t* xn, int lda, const uint16_t* w_qkv, const float* b_qkv, float scale, uint16_t* qkv_out,
                                 const float* bias_dense, uint16_t* out, int64_t B_, int nH, const srk_win_geom* geom, srk_stream_t stream);
long long srk_qkv_attn_fwd3_launches(void);
long long srk_qkv_attn_fwd8_launches(void);
/* attention output projection + window reverse + un-roll + residual (+ DropPath factor, + norm2 of the new row) (network_swinir.py:143,
 * :265-277): with t = token(geom, m), out[t] = res[t] + rowscale[t / rows_per_sample] * (ao[m] . w_proj^T + b_proj); xn_out non-null:
 * xn_out[t] = bf16(LayerNorm(out[t]) over xn_C), xn_mean[t], xn_rstd[t].  ao bf16 [B_*64][192] window order, w_proj bf16 [192][192],
 * res / out fp32 [T][192] token order (not aliased), rowscale fp32 [T / rows_per_sample] or null.  Streaming or tile kernel as srk_gemm_ex
 * picks them; with a rowscale the streaming kernel serves rows_per_sample == H*W only (a sample is an image, as in the model: it takes a
 * window-ordered tile's sample from its image), any other rows_per_sample dividing T runs on the tile kernel.
 * srk_gemm_stream_launches: launches of the streaming GEMM kernels in this process so far (tests assert which path ran). */
int srk_proj_residual_fwd(const uint16_t* ao, const uint16_t* w_proj, const float* b_proj, const float* res, float* out, const float* rowscale,
                          int rows_per_sample, uint16_t* xn_out, float* xn_mean, float* xn_rstd, const float* xn_gamma, const float* xn_beta,
                          int xn_C, int64_t B_, const srk_win_geom* geom, srk_stream_t stream);
long long srk_gemm_stream_launches(void);
/* d xn1 = d_qkv . w_qkv_t^T with norm1's backward, the window reverse and the un-roll in its epilogue: row m (window order; ln_mean /
 * ln_rstd indexed by m) belongs to token t = token(geom, m); gx[t] += d x (fp32, in place), gxb[t] = bf16(gx[t] * rowscale[t /
 * rows_per_sample]) or null, d_gamma / d_beta ACCUMULATED.  ln_skip non-null (the RSTB skip fold): the row result is gx[t] + d x +
 * ln_skip[t], stored to ln_skip[t] (gx untouched), gxb its scaled bf16 copy.  d_qkv bf16 [B_*64][576], w_qkv_t bf16 [192][576],
 * ln_x / gx / ln_skip fp32 [T][192] token order; rowscale and kernel choice as above. */
int srk_qkv_dgrad_lnbwd(const uint16_t* d_qkv, const uint16_t* w_qkv_t, const float* ln_x, const float* ln_mean, const float* ln_rstd,
                        const float* ln_gamma, float* gx, uint16_t* gxb, const float* rowscale, int rows_per_sample, float* ln_skip,
                        float* d_gamma, float* d_beta, int C, int64_t B_, const srk_win_geom* geom, srk_stream_t stream);

/* ---- DAT training pieces (csrc/dat_train.hip, csrc/attn_rect_bwd.hip) -----------------------------------------------------------
 * Token-sized work and token reductions only: the per-channel / per-sample functions in between (train-mode BatchNorm coefficients
 * dat_arch.py:301-313 / :464-476, channel_interaction on the pooled [B][C] vector, the d x d channel-attention matrices :497-503,
 * the DynamicPosBias MLP :93-130) are evaluated by the caller on the reductions these return (tpu_superresolution_amd/dat_train.py).
 * All bf16 operands are row-major [rows][ld] with 8-element (16-byte) aligned rows; C8 = channels / 8. */
/* backward of srk_win_attention_fwd_padded with a dense bias: d_qkv (q | k | v slices of the heads of this launch) and d_bias
 * [heads][N][N] ACCUMULATED (zero it first) over the windows.  scratch: null (d_bias by float atomics) or
 * srk_win_attention_bwd_padded_scratch bytes (per-window dS tiles + a reduction kernel, and a transposed copy of the bias for the
 * key-major pass: the fast path; fully written before it is read, needs no zeroing).  d_bias is added to whatever it holds.  Only
 * the q | k | v column blocks of heads 0 .. num_heads - 1 of rows 0 .. T - 1 are written (a wider CA holds another launch's heads);
 * shift_y < wh and shift_x < ww are independent; padded queries and the d k / d v of padded keys contribute nothing. */
size_t srk_win_attention_bwd_padded_scratch(int B, int Hp, int Wp, int wh, int ww, int num_heads);
int srk_win_attention_bwd_padded(const uint16_t* qkv, int ldq, int CA, const float* bias, const uint16_t* d_out, int ldo, uint16_t* d_qkv,
                                 float* d_bias, void* scratch, int B, int H, int W, int Hp, int Wp, int wh, int ww, int shift_y, int shift_x,
                                 int num_heads, float scale, srk_stream_t stream);
/* partial [samples][chunks][2][8 C8]: per 256-row chunk of a sample, sum_t p[t][c] and sum_t p[t][c] q[t][c] (fixed order; the caller
 * sums the chunks).  BatchNorm batch statistics (q = p), its backward sums (p = dz, q = x), the pooled mean (samples = B).
 * Every element of partial is written (it needs no zeroing); ldp, ldq >= 8 C8 are the caller's to keep (only their divisibility by 8
 * is checked). */
int64_t srk_chan_stats_chunks(int64_t rows_per_sample);
int srk_chan_stats(const uint16_t* p, int ldp, const uint16_t* q, int ldq, float* partial, int samples, int64_t rows_per_sample, int C8,
                   srk_stream_t stream);
/* nn.BatchNorm2d in training mode between two token passes (dat_arch.py:301-313, :464-476), one launch each:
 *   srk_bn_train_coeffs: the R partial rows (row_stride floats apart; sum x at + 0, sum x^2 at + ld; from srk_chan_stats or
 *     srk_spatial_gate_train what 0) summed in a fixed order -> coef [4][ld] = scale (gamma rstd), shift (beta - mean scale), mean, rstd over n values per channel; running_mean / running_var
 *     (or null) move in place by `momentum` with the unbiased variance; real_of[c] = index of channel c in the module's un-padded buffers,
 *     -1 for padding (null: identity).  Only columns 0..C-1 of each coefficient row are written; a channel whose variance comes out
 *     negative in fp32 is clamped at 0.
 *   srk_bn_train_bwd_coeffs: partial rows (sum dz, sum dz x) + the forward's coef -> coef [5][ld] = A, B, C of d x = A dz + B x + C,
 *     d gamma, d beta. */
/* out[o][i] = sum over r < R of in[o][r][i] (in: fp32 [outer][R][n] contiguous), rows added in a fixed order: the finishing sum of the
 * per-chunk partial rows the token passes above leave behind */
int srk_sum_rows_f32(const float* in, int outer, int R, int n, float* out, srk_stream_t stream);
int srk_bn_train_coeffs(const float* partial, int R, int row_stride, int ld, int C, float n, const float* gamma, const float* beta, float eps, float* coef,
                        float* running_mean, float* running_var, float momentum, const int* real_of, srk_stream_t stream);
int srk_bn_train_bwd_coeffs(const float* partial, int R, int row_stride, int ld, int C, float n, const float* fwd_coef, float* coef,
                            srk_stream_t stream);
/* nn.BatchNorm2d in EVAL mode inside a training step (frozen statistics), one launch each:
 *   srk_bn_frozen_coeffs: coef [4][ld] = scale (gamma rstd), shift (beta - mean scale), mean, rstd of channels 0..C-1 from the module's
 *     running buffers (real_of as above; padding channels all zero); gamma / beta in the padded layout.  Nothing is written but coef.
 *   srk_bn_frozen_bwd_coeffs: partial rows (sum dz, sum dz x) + that coef -> coef [5][ld] = A = scale, B = 0, C = 0,
 *     d gamma = rstd (sum dz x - mean sum dz), d beta = sum dz: the contract of srk_bn_train_bwd_coeffs. */
int srk_bn_frozen_coeffs(int ld, int C, const float* gamma, const float* beta, float eps, const float* running_mean, const float* running_var,
                         const int* real_of, float* coef, srk_stream_t stream);
int srk_bn_frozen_bwd_coeffs(const float* partial, int R, int row_stride, int ld, int C, const float* fwd_coef, float* coef, srk_stream_t stream);
/* out = act(x * scale[i][c] + shift[i][c]); i = row / rows_per_sample (rows_per_sample 0: one vector for all rows); act 1 = GELU.
 * x * scale + shift is one fused multiply-add.  For this and the three entry points below: scale / shift / A / B / C are contiguous
 * [samples][8 C8]; only the 8 C8 columns of the slice are read and written; the row strides must be >= 8 C8 (not checked beyond their
 * divisibility by 8); rows * C8 < 2^31. */
int srk_affine_act_bf16(const uint16_t* x, int ldx, const float* scale, const float* shift, uint16_t* out, int ldo, int64_t rows, int C8,
                        int rows_per_sample, int act, srk_stream_t stream);
/* out = dy * gelu'(x * scale[c] + shift[c]) */
int srk_dgelu_affine_bf16(const uint16_t* dy, int lddy, const uint16_t* x, int ldx, const float* scale, const float* shift, uint16_t* out,
                          int ldo, int64_t rows, int C8, srk_stream_t stream);
/* out (+)= A[i][c] p + B[i][c] q + C[i][c]   (null A / B: coefficient 1; null p / q: no such term; accumulate: out is read first).
 * Evaluated as ((old + A p) + B q) + C in fp32 with one bf16 rounding, so the one-term forms (copy, A p, old + p, old + C) are the
 * correctly rounded result; a -0 input is copied as +0. */
int srk_lincomb2_bf16(const uint16_t* p, int ldp, const uint16_t* q, int ldq, const float* A, const float* Bc, const float* Cc, uint16_t* out,
                      int ldo, int64_t rows, int C8, int rows_per_sample, int accumulate, srk_stream_t stream);
/* d a = dy * b, d b = dy * a  (SpatialGate's x1 * x2, dat_arch.py:54) */
int srk_mul_bwd_bf16(const uint16_t* dy, int lddy, const uint16_t* a, int lda, const uint16_t* b, int ldb, uint16_t* da, int ldda, uint16_t* db,
                     int lddb, int64_t rows, int C8, srk_stream_t stream);
/* depth-wise 3x3 (pad 1): partial [B][srk_dwconv3x3_wgrad_chunks(H)][10][8 C8]; rows 0..8 the taps' weight gradient, row 9 the bias gradient
 * of one band of 8 image rows.  Every element of partial is written (no zeroing); lddy, ldx >= 8 C8 (only divisibility by 8 is checked). */
int srk_dwconv3x3_wgrad_chunks(int H);
int srk_dwconv3x3_wgrad(const uint16_t* dy, int lddy, const uint16_t* x, int ldx, float* partial, int B, int H, int W, int C8,
                        srk_stream_t stream);
/* backward of srk_dual_gate_combine, out = a_chan * cgate[b][c] + a_tok * tgate[t]:  d_chan = d * cgate, d_tok = d * tgate,
 * dcg_partial [B][ceil(HW / 64)][CA] = chunk sums of d * a_chan  (gradient w.r.t. the post-sigmoid channel gate),
 * dsmap [B * HW] = (sum_c d * a_tok) * tgate (1 - tgate)   (gradient w.r.t. the PRE-sigmoid spatial map).
 * All bf16 operands contiguous [B * HW][CA] (no row stride), CA <= 256; dcg_partial and dsmap are fully written (no zeroing). */
int srk_dual_gate_bwd(const uint16_t* dcomb, const uint16_t* a_chan, const uint16_t* a_tok, const float* cgate, const float* tgate,
                      uint16_t* d_chan, uint16_t* d_tok, float* dcg_partial, float* dsmap, int B, int HW, int CA, srk_stream_t stream);
/* spatial_interaction in training (:318-323 / :475-480): y1 = W0 x + b0 (S <= 16), z = y1 * bn_scale + bn_shift, smap = w3 . gelu(z) + b3.
 *   what 0: partial [blocks][2][16]  = sums of y1, y1^2 over each 256-row block (BatchNorm batch statistics)
 *   what 1: partial [blocks][4][16]  = sums of dz, dz * y1, dsmap * gelu(z), dsmap (in slot 0) with dz = dsmap * w3 * gelu'(z)
 *   what 2: dy1 = cA * dz + cB * y1 + cC (the BatchNorm backward, coefficients from the caller); dx (+)= W0^T dy1;
 *           partial [blocks][16][C + 1] = the block's d W0 [s][c] (first 16 C floats) and d b0 [s] (last 16)
 * blocks = ceil(rows / 256); every element of partial is written, slots s >= S as 0 (no zeroing); C in {64, 128, 192, 256}; only the C
 * columns of dx are written; ldx, lddx >= C (only divisibility by 8 is checked). */
int srk_spatial_gate_train(int what, const uint16_t* x, int ldx, const float* W0, const float* b0, const float* bn_scale, const float* bn_shift,
                           const float* w3, const float* dsmap, const float* cA, const float* cB, const float* cC, uint16_t* dx, int lddx,
                           int accumulate, float* partial, int64_t rows, int C, int S, srk_stream_t stream);
/* LayerNorm (eps 1e-5) backward on bf16 rows (SpatialGate.norm): dx bf16 (columns C..CP_out-1 written as +0, columns >= CP_out not
 * written); partial [blocks][2][C] with the workgroups' d gamma / d beta sums (row m goes to block (m / 16) % blocks), blocks =
 * srk_rowln_bwd_blocks(rows) = min(1024, ceil(rows / 16)); every element of partial is written (no zeroing); CP_out <= 512.  The row
 * statistics are recomputed as the forward forms them (two passes: the variance from x - mean).  Columns C..CP_out-1 of x and dy are
 * never used (they may hold anything, NaN included). */
int64_t srk_rowln_bwd_blocks(int64_t rows);
int srk_rowln_bwd_bf16(const uint16_t* dy, int lddy, const uint16_t* x, int ldx, const float* gamma, uint16_t* dx, int lddx, float* partial,
                       int64_t rows, int C, int CP_out, srk_stream_t stream);
/* channel attention (:497-508): partial [B][heads][ceil(N / 256)][1088] = per chunk G[i][j] = sum_n x[n][32 h + i] y[n][32 h + j] (1024),
 * sum_n x[n][i]^2 (32), sum_n y[n][j]^2 (32); srk_chan_gram_floats = the partial's size in floats.  All 32 columns of every head are read
 * (the layout's padding must be finite; zero in the models); every element of partial is written (no zeroing). */
int64_t srk_chan_gram_floats(int B, int N, int num_heads);
int srk_chan_gram(const uint16_t* x, int ldx, const uint16_t* y, int ldy, float* partial, int B, int N, int num_heads, srk_stream_t stream);
/* out[n][32 h + i] (+)= sum_j M[b][h][i][j] src[n][32 h + j] + diag[b][h][i] src2[n][32 h + i]   (M fp32 [B][heads][32][32]; diag optional) */
int srk_chan_apply_mat(const float* M, const uint16_t* src, int ldsrc, const float* diag, const uint16_t* src2, int ldsrc2, uint16_t* out, int ldo,
                       int B, int N, int num_heads, int accumulate, srk_stream_t stream);

/* DAT training, the small functions between token passes as one launch each (csrc/dat_small.hip):
 *   srk_channel_interaction_fwd / _bwd: channel_interaction (dat_arch.py:315-321) on the pooled 1 x 1 map: pooled [B][ldp] = per-sample token
 *     sums in the head-padded channel order, pad_of[c] = padded position of real channel c; pm = pooled[pad_of] * inv_hw -> 1x1 conv W1 [S][C]
 *     -> BatchNorm2d over the BATCH (batch statistics; running buffers, if given, move as nn.BatchNorm2d's do) -> GELU -> 1x1 conv W2 [C][S]
 *     -> sigmoid -> cgate [B][CA] (padding 0); pm_out [B][C] is what the backward needs.  _bwd: d cgate [B][ldg] (head-padded) -> the six
 *     parameter gradients and dpool [B][CA] = d pm * inv_hw scattered back (padding 0).  One workgroup with both weight matrices and every
 *     [B][C] / [B][S] array in LDS: srk_channel_interaction_covered(B, C, S) says whether a shape fits (B > 1, S <= 64, 150 KB); SRK_E_SHAPE
 *     beyond (the caller keeps a torch path for larger batches).
 *   srk_chan_attn_matrix_fwd / _bwd: Adaptive_Channel_Attention's d x d matrix (:497-503) from the chunk partials of srk_chan_gram(q, k):
 *     gram [B][heads][1088] = their sum (G | sum q^2 | sum k^2), A [B][heads][32][32] = softmax_j(temperature_h G_ij / (|q_i| |k_j|)) over the
 *     dh real channels (norms clamped at 1e-12 as F.normalize; padding rows / columns 0).  _bwd: dpartial = chunk partials of
 *     srk_chan_gram(d out, v) (= d A) -> dG, dGt (its transpose), dsq2 / dsk2 [B][heads][32] (the diagonal coefficients of d q / d k through
 *     the norms, as srk_chan_apply_mat takes them), dtemp [B][heads] (sum over B = d temperature).
 *   What is read and written.  Channel interaction, trained and frozen alike: of pooled only the positions pad_of names are read (the
 *     others, and columns CA..ldp-1, may hold anything); every element of pm_out [B][C], cgate [B][CA] and dpool [B][CA] is written (the
 *     positions pad_of does not name receive +0); the six parameter gradients dW1 [S][C], db1 [S], dgamma [S], dbeta [S], dW2 [C][S],
 *     db2 [C] are OVERWRITTEN, not accumulated (the caller adds them to .grad).  The forms differ in the BatchNorm: the trained form
 *     normalises with the biased batch variance, moves running_mean / running_var (both given or both null, else SRK_E_SHAPE) by
 *     (1 - momentum) old + momentum new with the UNBIASED variance, and its backward carries the batch terms, so its db1 is a sum that is
 *     zero but for rounding; the frozen form reads the running buffers, writes none, and its db1 = sum d y.  The matrix kernels write
 *     every element of gram, A, dG, dGt, dsq2, dsk2 and dtemp, padding rows / columns (>= dh) +0; a channel whose sum of squares is
 *     at most 1e-24 is normalised by the clamp and gets dsq2 / dsk2 = 0.  The sums over chunks run in a fixed order (no atomics).
 *   SRK_E_NULL: a null pointer (the running buffers of the trained forward excepted); SRK_E_SHAPE: a (B, C, S) that is not covered, CA < C,
 *     ldp < CA, ldg < CA, exactly one running buffer null; for the matrix B, num_heads, nchunk < 1 or dh outside 1..32. */
int srk_channel_interaction_covered(int B, int C, int S);
int srk_channel_interaction_fwd(const float* pooled, int ldp, float inv_hw, const int* pad_of, const float* W1, const float* b1,
                                const float* gamma, const float* beta, float eps, const float* W2, const float* b2, float* running_mean,
                                float* running_var, float momentum, float* pm_out, float* cgate, int B, int C, int S, int CA,
                                srk_stream_t stream);
int srk_channel_interaction_bwd(const float* pm, const float* dcgate, int ldg, float inv_hw, const int* pad_of, const float* W1,
                                const float* b1, const float* gamma, const float* beta, float eps, const float* W2, const float* b2,
                                float* dW1, float* db1, float* dgamma, float* dbeta, float* dW2, float* db2, float* dpool, int B, int C, int S,
                                int CA, srk_stream_t stream);
/* srk_channel_interaction_frozen_fwd / _bwd: the same function with the BatchNorm in eval mode: normalised with running_mean / running_var
 * [S] (read only), no statistic over the batch, so B = 1 is valid (srk_channel_interaction_frozen_covered: B >= 1, S <= 64, 150 KB). */
int srk_channel_interaction_frozen_covered(int B, int C, int S);
int srk_channel_interaction_frozen_fwd(const float* pooled, int ldp, float inv_hw, const int* pad_of, const float* W1, const float* b1,
                                       const float* gamma, const float* beta, float eps, const float* W2, const float* b2,
                                       const float* running_mean, const float* running_var, float* pm_out, float* cgate, int B, int C, int S,
                                       int CA, srk_stream_t stream);
int srk_channel_interaction_frozen_bwd(const float* pm, const float* dcgate, int ldg, float inv_hw, const int* pad_of, const float* W1,
                                       const float* b1, const float* gamma, const float* beta, float eps, const float* W2, const float* b2,
                                       const float* running_mean, const float* running_var, float* dW1, float* db1, float* dgamma,
                                       float* dbeta, float* dW2, float* db2, float* dpool, int B, int C, int S, int CA, srk_stream_t stream);
int srk_chan_attn_matrix_fwd(const float* partial, int nchunk, const float* temperature, float* gram, float* A, int B, int num_heads, int dh,
                             srk_stream_t stream);
int srk_chan_attn_matrix_bwd(const float* dpartial, int nchunk, const float* gram, const float* A, const float* temperature, float* dG, float* dGt,
                             float* dsq2, float* dsk2, float* dtemp, int B, int num_heads, int dh, srk_stream_t stream);

/* ---- whole-model executor: SwinIR.forward / backward  (network_swinir.py:805-840) ------------------- */
enum { SRK_UPSAMPLER_PIXELSHUFFLE = 1,          /* classical SR           (network_swinir.py:740-745, :813-817) */
       SRK_UPSAMPLER_PIXELSHUFFLEDIRECT = 2,    /* lightweight SR         (:746-749, :818-822) */
       SRK_UPSAMPLER_NEAREST_CONV = 3,          /* real-world SR, x2 / x4 (:750-759, :823-831) */
       SRK_UPSAMPLER_NONE = 4 };                /* denoising / JPEG artefact reduction, upscale 1 (:760-762, :832-836) */
enum { SRK_RESI_1CONV = 0, SRK_RESI_3CONV = 1 };   /* RSTB / conv_after_body residual connection (:464-471, :728-736) */

typedef struct {
  int img_size;          /* constructor img_size // patch_size: only its relation to window_size matters (:193-196) */
  int in_chans;          /* 1 or 3 */
  int embed_dim;         /* C, <= 256 */
  int num_layers;        /* len(depths), <= 16 */
  int depths[16];
  int num_heads[16];     /* C / num_heads <= 32 */
  int window_size;       /* must be 8 */
  int hidden_dim;        /* int(C * mlp_ratio) */
  int upscale;
  int upsampler;         /* SRK_UPSAMPLER_* */
  float img_range;
  float mean[3];         /* (0.4488, 0.4371, 0.4040) for 3-channel input, 0 otherwise (:658-662) */
  float qk_scale;        /* <= 0: head_dim ** -0.5 */
  int resi_connection;   /* SRK_RESI_* */
  int ape;               /* constructor ape: != 0 -> parameter absolute_pos_embed [1][img_size^2][C] (first in the parameter table, as in
                            named_parameters()), added to the tokens after patch_embed.norm (network_swinir.py:678-689, :793-795); the
                            input must then have exactly img_size x img_size tokens, as in the reference */
  int use_checkpoint;    /* constructor use_checkpoint (network_swinir.py:397-405 wraps every block in torch.utils.checkpoint): != 0 ->
                            a training forward keeps, per block, only what cannot be recomputed cheaply (norm1 / norm2 outputs, the
                            residual rows, statistics); the attention output and the MLP's u / h = gelu(u) live in ONE shared set of
                            buffers and the backward pass re-runs the block's fused attention-forward and MLP-forward kernels to refill
                            them (same kernels, same inputs: gradients are bit-identical to use_checkpoint = 0; -250 MB per block at
                            cfg3 bs 32, + two forward launches per block in backward) */
} srk_swinir_config;

typedef struct srk_swinir_plan srk_swinir_plan;

/* Unsupported configurations return SRK_E_UNSUPPORTED with a message (no CPU fallback exists). */
int srk_swinir_plan_create(const srk_swinir_config* cfg, srk_swinir_plan** plan);
void srk_swinir_plan_destroy(srk_swinir_plan* plan);
/* Per-plan option values (names and values as srk_set_option): they apply to every later call on this plan (pack, workspace_bytes,
 * forward, forward_features, backward) and to nothing else.  Set them before the first srk_swinir_workspace_bytes query: some options
 * change the workspace layout.  get: *is_set = 1 when the plan carries the value, 0 when the process-wide value applies. */
int srk_swinir_plan_set_option(srk_swinir_plan* plan, const char* name, int value);
int srk_swinir_plan_get_option(const srk_swinir_plan* plan, const char* name, int* value, int* is_set);

/* Flat parameter buffer: fp32, every tensor in the reference's state_dict layout at a 64-float aligned
 * offset, in named_parameters() order. */
int64_t srk_swinir_param_floats(const srk_swinir_plan* plan);
int srk_swinir_param_count(const srk_swinir_plan* plan);
/* name: reference state_dict key; shape: up to 4 dims (ndim returned) */
int srk_swinir_param_info(const srk_swinir_plan* plan, int index, const char** name, int64_t* offset, int64_t* numel,
                          int* ndim, int64_t shape[4]);

/* Device-resident constant tables the plan needs (pack descriptors): size, then upload into caller memory. */
size_t srk_swinir_const_bytes(const srk_swinir_plan* plan);
int srk_swinir_const_init(srk_swinir_plan* plan, void* const_dev, srk_stream_t stream);

/* Packed (padded bf16 + fp32 side tables) weights: refresh after every parameter update. */
size_t srk_swinir_packed_bytes(const srk_swinir_plan* plan);
int srk_swinir_pack(srk_swinir_plan* plan, const float* params, void* packed, srk_stream_t stream);

/* Workspace for one forward (+ backward if training != 0) at batch B and (unpadded) input size H0 x W0. */
size_t srk_swinir_workspace_bytes(const srk_swinir_plan* plan, int B, int H0, int W0, int training);

/* x fp32 NCHW [B][in_chans][H0][W0] in [0,1]  ->  y fp32 NCHW [B][in_chans][H0*s][W0*s].
 * training != 0 keeps the activations the backward needs in `workspace`.  The one-step head (SRK_UPSAMPLER_PIXELSHUFFLEDIRECT) takes
 * upscale^2 * in_chans <= 64 (plan_create refuses more); past 16 it is inference-only: training != 0, and srk_swinir_backward,
 * return SRK_E_UNSUPPORTED before anything is launched.
 * drop_scale: null, or fp32 [n_blocks][2][B] per-sample DropPath factors (0 or 1/keep) for the
 * attention and MLP residual branches (timm DropPath in SwinTransformerBlock :276-277). */
int srk_swinir_forward(srk_swinir_plan* plan, const float* params, const void* packed, const float* x, float* y,
                       void* workspace, int B, int H0, int W0, int training, const float* drop_scale, srk_stream_t stream);

/* Backward in segments so the caller can overlap the gradient all-reduce of finished segments:
 * segment 0 = reconstruction tail + conv_after_body + final norm, 1..L = RSTB L-1..0, L+1 = patch-embed
 * norm + conv_first.  Segments must be run in increasing order after a training forward with the same
 * (B,H0,W0,workspace,drop_scale).  d_y fp32 NCHW like y.  grads: flat fp32 like params, ACCUMULATED.
 * After segment s, grads[begin,end) of srk_swinir_segment_range(s) are final. */
int srk_swinir_num_segments(const srk_swinir_plan* plan);
int srk_swinir_segment_range(const srk_swinir_plan* plan, int segment, int64_t* begin, int64_t* end);
int srk_swinir_backward(srk_swinir_plan* plan, const float* params, const void* packed, float* grads, const float* d_y,
                        void* workspace, int B, int H0, int W0, const float* drop_scale, int seg_begin, int seg_end,
                        srk_stream_t stream);

/* SwinIR.forward_features (network_swinir.py:790-803) as an inference entry of its own: f fp32 NCHW [B][embed_dim][H][W]
 * (what conv_first produced) -> patch_embed norm -> RSTBs -> final norm -> out fp32 NCHW [B][embed_dim][H][W].  H and W
 * must be multiples of window_size (the reference's window_partition needs the same).  workspace: as for a forward with
 * training == 0 at (B, H, W).  No gradient path (inference only). */
int srk_swinir_forward_features(srk_swinir_plan* plan, const float* params, const void* packed, const float* f, float* out,
                                void* workspace, int B, int H, int W, srk_stream_t stream);

/* Debug/parity access: byte offset and byte size of a named activation inside `workspace` for the
 * geometry of the last srk_swinir_workspace_bytes() query; returns SRK_E_STATE if unknown. */
int srk_swinir_workspace_lookup(const srk_swinir_plan* plan, const char* name, size_t* offset, size_t* bytes);

#ifdef __cplusplus
}
#endif
#endif /* SRK_H_ */
