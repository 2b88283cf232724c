// Internal launcher prototypes shared by api.hip and swinir.hip.
#pragma once
#include "common.h"
#include "gemm.h"
#include "pack.h"
#include "wgrad.h"

// attn_fused.hip: projection + attention in one kernel (classical width); SRK_NOT_COVERED -> run them separately
int srk_launch_qkv_attn_fwd(const bf16_t* xn, int lda, const bf16_t* Wt, const float* bias, float scale, bf16_t* qkv, const float* biasd,
                            bf16_t* ao, long long B_, int nH, int CA, int K, WinGeom geom, hipStream_t stream);
void srk_attn_fused_enable(int on);
int srk_attn_fused_mode();
// block_light.hip: one whole Swin block of the light width per launch (inference); SRK_NOT_COVERED when the shape is another
void srk_block_light_enable(int on);
int srk_block_light_enabled();
int srk_launch_swin_block_light(const float* x, float* y, bf16_t* yb, const float* n1w, const float* n1b, const float* n2w, const float* n2b,
                                const bf16_t* Wqkv, const bf16_t* Wproj, const bf16_t* W1, const bf16_t* W2, const float* bqkv,
                                const float* bproj, const float* b1, const float* b2, const float* biasd, float scale, int C, int CP, int HP,
                                int nH, int dh, int HID, long long B_, WinGeom geom, hipStream_t stream);
int srk_launch_attn_fwd(const bf16_t* qkv, const float* biasd, bf16_t* ao, long long B_, int nH, WinGeom geom, hipStream_t stream);
int srk_attn_bwd_slabs(long long B_, int nH, int* wpw_out);
int srk_launch_attn_bwd(const bf16_t* qkv, const float* biasd, const bf16_t* dao, bf16_t* dqkv, float* dbias_slab,
                        float* dtable, long long B_, int nH, WinGeom geom, float scale, hipStream_t stream);
int srk_launch_rpb_expand(const float* table, float* biasd, int nH, hipStream_t stream);
// attn_bwd_fused.hip: attention backward of one window per workgroup pass with q/k/v re-projected from xn1 and the output-projection
// dgrad folded in (classical width); SRK_NOT_COVERED -> dproj GEMM + srk_launch_attn_bwd on saved q/k/v
void srk_attn_bwd_fused_enable(int on);
int srk_attn_bwd_fused_enabled();
int srk_qkv_attn_bwd_slabs(long long B_, int nH, int CA, int K);    // d(bias) slabs it writes; 0 = not covered
int srk_launch_qkv_attn_bwd(const bf16_t* xn, int lda, const bf16_t* Wqkv, const float* bqkv, float scale, const bf16_t* g, int ldg,
                            const bf16_t* WprojT, const float* biasd, bf16_t* dqkv, float* slab, long long B_, int nH, int CA, int K,
                            WinGeom geom, hipStream_t stream);

int srk_launch_ln_fwd(const float* x, const float* gamma, const float* beta, bf16_t* yb, float* yf, float* mean,
                      float* rstd, int rows, int C, int CP, const WinGeom* geom, hipStream_t stream);
int srk_launch_ln_bwd(const bf16_t* dyb, const float* x, const float* mean, const float* rstd, const float* gamma,
                      float* gx, bf16_t* gxb, float* dgamma, float* dbeta, int rows, int C, int CP, const WinGeom* geom,
                      int dy_by_m, int stats_by_m, int out_by_m, int accumulate, const float* rowscale, int rows_per_sample,
                      hipStream_t stream);

int srk_launch_window_partition(const void* x, void* out, int B, int H, int W, int C, int ws, int elem_bytes, int reverse, hipStream_t stream);
int srk_launch_roll2d(const void* x, void* out, int B, int H, int W, int C, int sh, int sw, int elem_bytes, hipStream_t stream);
int srk_launch_pixel_shuffle(const void* x, void* out, int B, int C, int H, int W, int r, int elem_bytes, hipStream_t stream);
int srk_launch_shift_mask(float* mask, int H, int W, int ws, int shift, hipStream_t stream);
int srk_launch_rel_pos_index(long long* out, int ws, hipStream_t stream);
int srk_launch_img_prep(const float* x, float* out, int B, int Cimg, int H0, int W0, int H, int W, float range, const float* mean, hipStream_t stream);
int srk_launch_stem_conv(const float* in, const float* wgt, const float* bias, float* out, int B, int H, int W, int Cin, int C, int CP, hipStream_t stream);
int srk_launch_stem_wgrad(const float* in, const float* gy, float* dW, float* db, int B, int H, int W, int Cin, int C, int CP, hipStream_t stream);
int srk_launch_img_grad_prep(const float* dpred, float* gy, int B, int Cimg, int Hc, int Wc, int H, int W, int r, int CoP, float inv_range, hipStream_t stream);
int srk_launch_smallconv_dgrad(const float* gy, const float* wgt, bf16_t* dx, int B, int H, int W, int Cin, int CinP, int Co, int CoP, hipStream_t stream);
int srk_launch_smallconv_wgrad(const bf16_t* x, const float* gy, float* dW, float* db, int B, int H, int W, int Cin, int CinP, int Co, int CoP, hipStream_t stream);
// headconv_wide.hip: the same two gradients for a one-step head of 17 .. 64 output channels (CoP 32, 48 or 64; fp32-input MFMA), and the
// plan option that lets the SwinIR executor train through such a head
int srk_launch_widehead_dgrad(const float* gy, const float* wgt, bf16_t* dx, int B, int H, int W, int Cin, int CinP, int Co, int CoP, hipStream_t stream);
int srk_launch_widehead_wgrad(const bf16_t* x, const float* gy, float* dW, float* db, int B, int H, int W, int Cin, int CinP, int Co, int CoP, hipStream_t stream);
void srk_wide_head_train_enable(int on);
int srk_wide_head_train_enabled();
// workgroups per image of the PSNR partial pass (8192 elements each, at most 64)
inline int srk_batch_psnr_chunks(long long per_image) {
  const long long c = (per_image + 8191) / 8192;
  return (int)(c < 1 ? 1 : (c > 64 ? 64 : c));
}
int srk_launch_crop_u8(const unsigned char* pool, const long long* desc, float* out, int B, int patch, hipStream_t stream);
// dihedral.hip: the eight symmetries of the square on fp32 NCHW batches (arguments checked by srk_dihedral_f32)
int srk_launch_dihedral_f32(const float* in, float* out, const int* ops, int op_all, int B, int C, int H, int W, float alpha,
                            int accumulate, hipStream_t stream);
// resize.hip: antialiased bicubic resampling and the HR -> (LR, HR) training degradation (arguments checked by srk_resize_aa_f32 /
// srk_crop_degrade_u8)
int srk_launch_resize_aa_f32(const float* x, float* out, int planes, int H, int W, int Ho, int Wo, int quant_bits, hipStream_t stream);
int srk_launch_crop_degrade_u8(const unsigned char* pool, const long long* desc, float* lr_out, float* hr_out, int B, int P, int scale,
                               int quant_bits, hipStream_t stream);
// degrade.hip: the same two behind a per-sample Gaussian blur and with per-sample noise (arguments checked by srk_degrade_blind_f32 /
// srk_crop_degrade_blind_u8)
int srk_launch_degrade_blind_f32(const float* x, float* out, const long long* par, int B, int C, int H, int W, int scale, int quant_bits,
                                 hipStream_t stream);
int srk_launch_crop_degrade_blind_u8(const unsigned char* pool, const long long* desc, float* lr_out, float* hr_out, int B, int P, int scale,
                                     int quant_bits, hipStream_t stream);
// blur2d.hip: a per-sample ks x ks blur table as a correlation, and the training degradation behind it (arguments checked by
// srk_blur2d_f32 / srk_crop_degrade_psf_u8)
int srk_launch_blur2d_f32(const float* x, const float* psf, float* out, int B, int C, int H, int W, int ks, hipStream_t stream);
int srk_launch_crop_degrade_psf_u8(const unsigned char* pool, const long long* desc, const float* psf, int ks, float* lr_out, float* hr_out,
                                   int B, int P, int scale, int quant_bits, hipStream_t stream);
// jpeg.hip: the closed-form JPEG round trip at a per-sample quality (arguments checked by srk_jpeg_roundtrip_f32)
int srk_launch_jpeg_roundtrip_f32(const float* x, float* out, const int* quality, int B, int C, int H, int W, int subsample, short* coef_out,
                                  hipStream_t stream);
// restore.hip: the whole-image noise stage and the scale-1 training pairs (arguments checked by srk_noise_f32 / srk_crop_restore_u8)
int srk_launch_noise_f32(const float* x, float* out, const long long* par, int B, int C, int H, int W, int quant_bits, hipStream_t stream);
int srk_launch_crop_restore_u8(const unsigned char* pool, const long long* desc, float* clean_out, float* degraded_out, int B, int P,
                               int out_chans, int subsample, int quant_bits, hipStream_t stream);
// filter2d.hip: a signed per-sample ks x ks table as a correlation with a reflect-101 border, on a dense or ragged batch (arguments
// checked by srk_filter2d_f32)
int srk_launch_filter2d_f32(const float* x, const float* tab, float* out, const int* ext, int B, int C, int Hp, int Wp, int ks, int quant_bits,
                            hipStream_t stream);
// ragged.hip: the resize and the JPEG round trip at per-sample extents (arguments checked by srk_resize_aa_ragged_f32 /
// srk_jpeg_roundtrip_ragged_f32)
int srk_launch_resize_aa_ragged_f32(const float* x, const int* ext_in, float* out, const int* ext_out, int B, int C, int Hp, int Wp, int Hop,
                                    int Wop, int quant_bits, hipStream_t stream);
int srk_launch_jpeg_roundtrip_ragged_f32(const float* x, float* out, const int* quality, const int* ext, int B, int C, int Hp, int Wp,
                                         int subsample, hipStream_t stream);
// resize_modes.hip: the ragged resize with a rule per sample (arguments checked by srk_resize_ragged_mode_f32)
int srk_launch_resize_ragged_mode_f32(const float* x, const int* ext_in, float* out, const int* ext_out, const int* mode, int B, int C, int Hp,
                                      int Wp, int Hop, int Wop, int quant_bits, hipStream_t stream);
// usm.hip: the separable unsharp mask (arguments checked by srk_usm_sharpen_f32)
int srk_launch_usm_sharpen_f32(const float* x, const float* taps, float* out, float* work, int B, int C, int H, int W, int ks, float weight,
                               float threshold, hipStream_t stream);
// tile.hip: tiled inference (arguments checked by srk_tile_gather_f32 / srk_tile_merge_f32).  One axis of the tile grid: extent n,
// tile t (1 <= t <= n), stride s (1 <= s <= t), k = ceil((n - t) / s) + 1 tiles, origin o_i = min(i * s, n - t)
struct TileAxis { int n, t, s, k; };
inline TileAxis srk_tile_axis(int n, int t, int s) { return TileAxis{n, t, s, (n - t + s - 1) / s + 1}; }
inline int srk_tile_origin(const TileAxis& a, int i) { const long long o = (long long)i * a.s; return o < a.n - a.t ? (int)o : a.n - a.t; }
int srk_launch_tile_gather_f32(const float* x, float* tiles, int t0, int n, int planes, TileAxis ay, TileAxis ax, hipStream_t stream);
int srk_launch_tile_merge_f32(const float* tiles, float* out, int t0, int n, int planes, TileAxis ay, TileAxis ax, int mode,
                              hipStream_t stream);
// image_io.hip: interleaved 8- / 16-bit samples <-> planar fp32 (arguments checked by srk_image_unpack / srk_image_pack)
int srk_launch_image_unpack(const void* src, float* dst, float* alpha, int B, int H, int W, int in_chans, int bits, int out_chans,
                            hipStream_t stream);
int srk_launch_image_pack(const float* y, const float* alpha, void* dst, unsigned* counters, int B, int H, int W, int chans, int out_chans,
                          int bits, hipStream_t stream);
int srk_launch_batch_psnr(const float* pred, const float* target, float* partial, int B, long long per_image, float max_val,
                          float* psnr, float* psnr_sum, float* abs_sum, hipStream_t stream);
int srk_launch_zero_f32(float* p, long long n, hipStream_t stream);      // graph-safe zero fill (misc.hip)
int srk_launch_add_f32_bf16(float* a, const float* b, bf16_t* ab, long long n, hipStream_t stream);
int srk_launch_add_bf16_into_f32(float* a, const bf16_t* b, long long n, hipStream_t stream);
int srk_launch_cast_f32_bf16(const float* a, bf16_t* out, long long n, hipStream_t stream);
int srk_launch_ape_add(float* x, const float* ape, int B, int L, int C, int CP, hipStream_t stream);
int srk_launch_ape_grad(const float* gx, float* dape, int B, int L, int C, int CP, hipStream_t stream);
int srk_launch_dlrelu_bf16(bf16_t* g, const bf16_t* act, float slope, long long n, hipStream_t stream);
int srk_launch_nn2x_bf16(const bf16_t* in, bf16_t* out, int B, int h, int w, int C, hipStream_t stream);
int srk_launch_nn2x_sum_dlrelu(const bf16_t* g, const bf16_t* act, bf16_t* out, int B, int h, int w, int C, float slope, hipStream_t stream);
int srk_launch_nchw_tokens(const float* src, float* dst, int B, int C, int CP, int HW, int to_tokens, hipStream_t stream);
int srk_launch_l1_loss(const float* pred, const float* target, float* dpred, float* loss_sum, unsigned* nonfinite, long long n, float grad_scale, hipStream_t stream);
// loss.hip: pixel losses and the SSIM term with fixed-order sums (arguments checked by srk_pixel_loss_fwd_bwd / srk_ssim_loss_fwd_bwd)
// workgroups of the pixel-loss pass: 256 elements each, at most 2048 (then a grid-stride loop)
inline int srk_pixel_loss_blocks(long long n) {
  const long long b = (n + 255) / 256;
  return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}
int srk_launch_pixel_loss(const float* pred, const float* target, float* dpred, float* loss, unsigned* nonfinite, long long n, int kind,
                          float eps, float grad_scale, int accumulate, float* partial, hipStream_t stream);
int srk_launch_ssim_loss(const float* x, const float* y, float* partial, int B, int C, int H, int W, float data_range, float alpha, float* d_x,
                         int accumulate, float* ssim_mean, float* loss, hipStream_t stream);
// fft_loss.hip: the frequency loss (arguments checked by srk_fft_loss_fwd_bwd); ws holds srk_fft_loss_workspace_bytes(B, C, H, W) bytes
long long srk_fft_loss_workspace_bytes(int B, int C, int H, int W);
int srk_launch_fft_loss(const float* x, const float* y, float* ws, int B, int C, int H, int W, int ortho, float alpha, float* d_x,
                        int accumulate, float* value, float* loss, hipStream_t stream);
int srk_launch_sumsq(const float* g, long long n, float* out, hipStream_t stream);
int srk_launch_adamw(float* p, const float* g, float* m, float* v, long long n, const float* sumsq, const int* nonfinite, float max_norm, float grad_div, float lr, float beta1, float beta2, float eps, float wd, int step, hipStream_t stream);
int srk_launch_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, long long n, const float* sumsq, const int* nonfinite, float max_norm, float grad_div, float lr, float beta1, float beta2, float eps, float wd, int step, float ema_decay, hipStream_t stream);
// optim_multi.hip: the same two over lists of separate tensors, ceil(n_tensors / chunk) launches, tables by value in the kernel arguments
int srk_launch_multi_sumsq(const float* const* grads, const long long* numel, int n_tensors, float* out, hipStream_t stream);
int srk_launch_multi_adamw(float* const* p, const float* const* g, float* const* m, float* const* v, const long long* numel, int n_tensors, const float* sumsq, const int* nonfinite, const float* hyper, float max_norm, float grad_div, float lr, float beta1, float beta2, float eps, float wd, int step, hipStream_t stream);
int srk_launch_multi_adamw_ema(float* const* p, const float* const* g, float* const* m, float* const* v, float* const* e, const long long* numel, int n_tensors, const float* sumsq, const int* nonfinite, const float* hyper, float max_norm, float grad_div, float lr, float beta1, float beta2, float eps, float wd, int step, float ema_decay, hipStream_t stream);
int srk_launch_probe_trread(const bf16_t* in, bf16_t* out, hipStream_t stream);
int srk_launch_win256_attn_fwd(const bf16_t* qkv, int ldq, int CA, const float* bias, int table_rows, bf16_t* out, int ldo, int B, int H, int W, int wh, int ww, int sy, int sx, int nH, float scale, int overlap, hipStream_t stream);
int srk_launch_win_attn_fwd_padded(const bf16_t* qkv, int ldq, int CA, const float* bias, int table_rows, bf16_t* out, int ldo, int B, int H, int W, int Hp, int Wp, int wh, int ww, int sy, int sx, int nH, float scale, int overlap, hipStream_t stream);
// dat.hip: Gram partials of the channel attention on the matrix cores (also behind srk_chan_gram of dat_train.hip)
int srk_launch_chan_gram(const bf16_t* x, int ldx, const bf16_t* y, int ldy, float* partial, int B, int N, int nH, hipStream_t stream);
