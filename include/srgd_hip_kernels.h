/* libsrgd_hip - kernel-level C ABI: each hand-written gfx950 kernel family of the Real-SRGD hot path,
 * callable on raw device pointers.  The engine (srgd_hip.h) is built from exactly these launchers;
 * they are exported so that every operator can be parity-tested in isolation against the CPU oracle
 * (tests/test_kernels_gpu.py) and bound separately by a host that wants only one of them.
 *
 * Layout: activations are NHWC in the activation type selected by `is_bf16` (0: fp32, 1: bf16);
 * statistics, coefficients and weights handed in as fp32.  All pointers except `*_host` are device
 * pointers.  Calls are asynchronous on `stream` unless stated; return 0 or <0 (srgd_last_error()).
 */
#ifndef SRGD_HIP_KERNELS_H
#define SRGD_HIP_KERNELS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: only the entry points declared here are exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

/* Convolution as implicit GEMM on MFMA.  replaces: nn.Conv2d call sites of the U-Net - Block.proj
 * (model.py:246), res_conv (:271), to_qkv/to_out (:300,:303,:341,:342), Downsample (:106-110, kind 1:
 * pixel-unshuffle + 1x1 == 2x2/stride-2), PixelShuffleUpsample (:70-98, kind 2: 1x1 + SiLU + PixelShuffle),
 * and torch.cat on the skip path (:713,:716,:722: two channel-concatenated sources in0|in1).
 * weight_oihw_host / bias_host: PyTorch-layout fp32 on the HOST (packed + uploaded inside; this entry
 * point synchronises).  gn_partial: optional device [B][groups][nslots][2] receiving partial (sum, sum of squares)
 * of the output for a following GroupNorm.  nslots depends on the kernel the call selects (srgd_k_conv2d_timed reports it):
 * the generic kernel writes Hout*Wout/128 slots, the 3x3 fast paths one per contributing WAVE of a 256-pixel patch (4, or 8 per
 * 128-channel tile of a group that spans whole tiles).  Size the buffer for the largest:
 *     nslots_capacity = (Hout*Wout / 32) * max(1, (Cout / groups) / 64). */
int srgd_k_conv2d(const void* in0, const void* in1, int C0, int C1, int B, int Hin, int Win, int KS, int stride,
                  int pad, int kind, const float* weight_oihw_host, const float* bias_host, int Cout, void* out,
                  const void* residual, float* gn_partial, int groups, int is_bf16, void* stream);
/* Same, with implementation choice and timing: impl 0 = what the engine would pick, 1 = generic implicit-GEMM
 * kernel (conv_igemm.hip), 2 = the 3x3 bf16 halo/LDS-DMA kernel (conv3x3_bf16.hip; error if not eligible),
 * 3 = the pointwise bf16 streaming GEMM (conv1x1_bf16.hip; error if not eligible), 4 = the pointwise layer on the block-scaled
 * MX-fp8 matrix cores (conv1x1_mxfp8.hip, fp8 mode: the bf16 sources are quantised inside with srgd_k_quant_mxfp8's rule, the
 * weights per (output channel, tap, 32 input channels); C0, C1, Cout % 128 == 0; error if not eligible),
 * 5 = impl 2 with the PRODUCER's GroupNorm + SiLU applied while the input is staged (Block.forward model.py:250-259 between
 * two convolutions): conv(silu(gn_tail_a[b][c] * in0 + gn_tail_b[b][c])), zero padding applied after the activation; one source,
 * gn_tail_a / gn_tail_b = device fp32 [B][C0] in ONE allocation (shift behind scale), gn_tail_src must be NULL.
 * 6 / 7 = the split-operand kernels of SRGD_PRECISION_F16X3 (is_bf16 = 0: fp32 tensors; every product as three f16 MFMAs on (hi, lo)
 * operand pairs): 6 = the 3x3 halo-patch kernel (conv3x3_split.hip; conv3x3_bf16's shapes), 7 = the generic implicit GEMM
 * (conv_igemm.hip; C0, C1 % 32 == 0); 8 / 9 = the same two kernels with bf16 halves (numerics comparison only); 10 = the streaming
 * pointwise kernel of that mode (conv1x1_split.hip: 1x1 incl. two sources, 2x2 / stride-2 gather, + residual, SiLU + PixelShuffle;
 * C0, C1 % 32 == 0, Cout % 128 == 0, Hout * Wout % 256 == 0); 11 = impl 6 with the producer's GroupNorm + SiLU applied while the input
 * is staged, as impl 5 (gn_tail_a / gn_tail_b = device fp32 [B][C0], 16-byte aligned; one source; gn_tail_src NULL); 12 / 13 = impl
 * 6 / 11 on the 256-thread form of that kernel (two workgroups per CU) instead of the engine's default (512 threads, one per CU).
 * 14 / 15 = the two-MFMA prototype of SRGD_PRECISION_F16MX2 (conv3x3_mx2.hip: f16 leading term, both cross terms on MX-fp8 operands;
 * conv3x3_split's shapes), 15 with the producer's GroupNorm + SiLU applied while the input is staged (as impl 5: gn_tail_a / gn_tail_b in
 * ONE allocation, one source).
 * 16 / 17 = impl 6 / 11 with ONE f16 MFMA per product, the 3x3 convolution of SRGD_PRECISION_F16X1: conv(hi(x), hi(w s)) / s + bias on the
 * hi halves alone (conv3x3_split.hip's one-term instances; requirements as impl 6 / 11: is_bf16 = 0, conv3x3_split's shapes).
 * gn_tail_src (nullable, NHWC like out): out = silu(gn_tail_a[b][c] * gn_tail_src + gn_tail_b[b][c]) + conv(in) -
 * the second GroupNorm+SiLU of a ResnetBlock and its residual add folded into the 1x1 res_conv (model.py:250-259,:285);
 * gn_tail_a / gn_tail_b: device fp32 [B][Cout].  May alias out.
 * iters > 0: the launch is repeated `iters` times between two HIP events on `stream`, *avg_ms = mean duration.
 * *stats_slots (nullable) = slots per (sample, group) written to gn_partial - pass it to srgd_k_groupnorm_silu. */
int srgd_k_conv2d_timed(const void* in0, const void* in1, int C0, int C1, int B, int Hin, int Win, int KS, int stride,
                        int pad, int kind, const float* weight_oihw_host, const float* bias_host, int Cout, void* out,
                        const void* residual, float* gn_partial, int groups, int is_bf16, int impl, int iters,
                        float* avg_ms, int* stats_slots, const void* gn_tail_src, const float* gn_tail_a,
                        const float* gn_tail_b, void* stream);

/* bf16 NHWC [npix][C] -> OCP MX-fp8: q [npix][C] e4m3 bytes + s [npix][C/32] E8M0 bytes (x ~ q * 2^(s-127); one scale per 32
 * consecutive channels = floor(log2 max|x|) - 8, + 1 when the block maximum would exceed 448 after scaling; elements clamped to
 * +-448, round-to-nearest-even).  C % 32 == 0.
 * The activation format of the fp8 mode's 3x3 convolutions (SRGD_PRECISION_FP8). */
int srgd_k_quant_mxfp8(const void* x_bf16, void* q, void* s, int64_t npix, int C, void* stream);
/* 3x3 / stride 1 / pad 1 convolution on v_mfma_scale_f32_16x16x128_f8f6f4.  replaces: Block.proj (model.py:246) in fp8 mode.
 * in0 / in1: bf16 NHWC sources (channel concat; in1 nullable), quantised to MX-fp8 inside (srgd_k_quant_mxfp8); weights /
 * bias: PyTorch-layout fp32 on the HOST, quantised per (output channel, tap, 32 input channels).  C0, C1, Cout % 128 == 0,
 * H % 8 == 0, W % 32 == 0.  out: bf16 NHWC.  gn_partial / stats_slots as in srgd_k_conv2d_timed; iters > 0 times the
 * convolution kernel alone (*avg_ms).  Synchronises. */
int srgd_k_conv3x3_mxfp8(const void* in0, const void* in1, int C0, int C1, int B, int H, int W,
                         const float* weight_oihw_host, const float* bias_host, int Cout, void* out, float* gn_partial,
                         int groups, int iters, float* avg_ms, int* stats_slots, void* stream);

/* ---- test / probe interfaces of the MX-fp8 quantisation sites (tests/test_mxfp8_exact_gpu.py); the engine calls none of them.
 * Every q / out_q is [pixels][C] e4m3 bytes, every s / out_s [pixels][C/32] E8M0 bytes, of the bf16 tensor the same call stores
 * ("twin": identical to srgd_k_quant_mxfp8 of that tensor).
 *
 * y = silu(coefA[b][c] * x + coefB[b][c]) quantised straight to MX-fp8, no bf16 store in between (quant_mxfp8.hip's GroupNorm
 * variant: the input of the second 3x3 convolution of an fp8 ResnetBlock).  x: bf16 [B][hw][C]; coefA / coefB: device fp32 [B][C],
 * 16-byte aligned.  C % 32 == 0.  Asynchronous on `stream`. */
int srgd_k_gn_apply_silu_mxfp8(const void* x_bf16, void* q, void* s, const float* coefA, const float* coefB, int B, int hw,
                               int C, void* stream);
/* srgd_k_conv2d_timed without the timing, with the MX-fp8 twin of `out` (pixel-shuffle: of the shuffled [B][2H][2W][Cout/4] tensor).
 * Fails unless the selected kernel writes twins: impl 3 (conv1x1_bf16) or 4 (conv1x1_mxfp8).
 * ps0 > 0 (impl 3, one source, kind 0, stride 1, pad 0): the overlapping-window form in which the engine runs the 7x7 input
 * convolution - a KS x 1 kernel over C0 "channels" whose consecutive pixels lie ps0 elements apart in in0 ([B][Hin][Win][ps0]);
 * Wout is then given by the caller (Hout = Hin - KS + 1) and weight_oihw_host is [Cout][C0][KS][1].  ps0 = 0, Wout = 0 otherwise. */
int srgd_k_conv2d_twin(const void* in0, const void* in1, int C0, int C1, int B, int Hin, int Win, int KS, int stride,
                       int pad, int kind, const float* weight_oihw_host, const float* bias_host, int Cout, void* out,
                       const void* residual, float* gn_partial, int groups, int is_bf16, int impl, int* stats_slots,
                       const void* gn_tail_src, const float* gn_tail_a, const float* gn_tail_b, void* out_q, void* out_s,
                       int ps0, int Wout, void* stream);
/* srgd_k_conv3x3_mxfp8 with the MX-fp8 twin of `out`. */
int srgd_k_conv3x3_mxfp8_twin(const void* in0, const void* in1, int C0, int C1, int B, int H, int W,
                              const float* weight_oihw_host, const float* bias_host, int Cout, void* out, float* gn_partial,
                              int groups, int iters, float* avg_ms, int* stats_slots, void* out_q, void* out_s, void* stream);
/* srgd_k_groupnorm_silu (below) with the MX-fp8 twin of y; bf16 only, C % 32 == 0. */
int srgd_k_groupnorm_silu_twin(const void* x, void* y, const void* residual, const float* gn_partial, int B, int hw,
                               int C, int groups, const float* gamma, const float* beta, const float* scale_shift,
                               int nslots, int is_bf16, void* out_q, void* out_s, void* stream);

/* GroupNorm (from the conv's partial statistics) -> x*(scale+1)+shift -> SiLU (+ residual).
 * replaces: Block.forward after the conv (model.py:250-259) and the ResnetBlock residual add (:285).
 * gamma, beta: device [C]; scale_shift: device [B][2C] (scale | shift) or NULL; in place if y == x.
 * gn_partial: [B][groups][nslots][2] as written by the conv (nslots from srgd_k_conv2d_timed / srgd_k_conv3x3_mxfp8).
 * x must be that conv's output: with fp32 tensors, a group whose mean^2 exceeds 32 * (var + eps) takes its variance from x itself. */
int srgd_k_groupnorm_silu(const void* x, void* y, const void* residual, const float* gn_partial, int B, int hw,
                          int C, int groups, const float* gamma, const float* beta, const float* scale_shift,
                          int nslots, int is_bf16, void* stream);

/* RMSNorm over channels * g * sqrt(C) (+ residual).  replaces: RMSNorm.forward (model.py:206-207). */
int srgd_k_rmsnorm(const void* x, void* y, const void* residual, const float* g, int64_t npix, int C, int is_bf16,
                   void* stream);

/* qkv: [B,N,3*heads*32] -> out [B,N,heads*32].  replaces: LinearAttention.forward core (model.py:312-323)
 * and Attention.forward core + Attend (model.py:349-354). */
int srgd_k_linear_attention(const void* qkv, void* out, int B, int N, int heads, int is_bf16, void* stream);
int srgd_k_full_attention(const void* qkv, void* out, int B, int N, int heads, int is_bf16, void* stream);

/* The whole LinearAttention block plus its residual, fused (bf16, C = 128, 4 heads x 32, N % 128 == 0):
 * y = RMSNorm(to_out(linear_attention(to_qkv(RMSNorm(x))))) + x.   replaces: LinearAttention.forward
 * (model.py:306-324) and the `attn(x) + x` at model.py:703/:718.  x, y: device bf16 [B,N,C]; weights host fp32 in
 * PyTorch layout (to_qkv [384,C], norm.g [C], to_out.0.weight [C,128], to_out.0.bias [C], to_out.1.g [C]). */
int srgd_k_linattn_block_fused(const void* x, void* y, int B, int N, int C, const float* to_qkv_host,
                               const float* norm_g_host, const float* to_out_w_host, const float* to_out_b_host,
                               const float* out_g_host, void* stream);
/* The same call with the block's intermediates exposed for tests; every output below is optional (NULL: skipped).
 *   ctxn_out  device fp32 [B*4][32 d][32 e]: the normalised context * dim_head^-0.5 that the second kernel consumes
 *   rinv_out  device fp32 [B][N]: 1 / max(||x_n||, 1e-12)
 *   y_q, y_s  device bytes [B*N][C] and [B*N][C/32]: the MX-fp8 twin of y that fp8 mode writes alongside (both or neither)
 *   strip_out, tiles_per_wg_out  host ints: pixels per first-kernel workgroup and tiles per second-kernel workgroup of this launch */
int srgd_k_linattn_block_fused_probe(const void* x, void* y, int B, int N, int C, const float* to_qkv_host,
                                     const float* norm_g_host, const float* to_out_w_host, const float* to_out_b_host,
                                     const float* out_g_host, float* ctxn_out, float* rinv_out, void* y_q, void* y_s,
                                     int* strip_out, int* tiles_per_wg_out, void* stream);

/* f16x3 mode: a pointwise projection with an RMSNorm folded into its kernel (conv1x1_split.hip), fp32 NHWC tensors, N % 256 == 0.
 *   pre_norm_g_host  != NULL:  out = W . RMSNorm_g(x)                      replaces: self.norm(x) -> self.to_qkv (model.py:311-312, :348-349)
 *   post_norm_g_host != NULL:  out = RMSNorm_g(W . x + bias) + residual    replaces: LinearAttention.to_out (Conv2d, RMSNorm; model.py:300-303)
 *                              and the block's `attn(x) + x` (:703); Cout == 128, residual required.
 * RMSNorm_g(v) = v / max(||v||_2, 1e-12) * g * sqrt(C) over the channels of a pixel (model.py:201-207).  Weights [Cout][Cin], gains and
 * bias fp32 on the HOST (the gain of the pre-norm is folded into the weights before they are split); synchronises. */
int srgd_k_conv1x1_split_rms(const void* x, int Cin, int B, int N, const float* weight_oi_host, const float* bias_host, int Cout,
                             const float* pre_norm_g_host, const float* post_norm_g_host, const void* residual, void* out,
                             void* stream);

/* ---- read-only probes of the conditioning path and of gn_finalize (tests/test_cond_exact_gpu.py); the engine calls none of them.
 * Host code only: each makes the launches the engine makes, on the caller's buffers.  All return -1 with a message on a null argument.
 *
 * The two launchers of cond.hip.  Device pointers, fp32; synchronise.
 *   time_features: feat[r] = [x, sin(2 pi x w[0..half)), cos(2 pi x w[0..half))] for x = log_snr[r]; feat rows are 2 * half + 1 wide.
 *   linear_rows:   y[r][o] = act_out(sum_i W[o][i] * act_in(x[r][i]) + b[o]) + add[r * add_stride + o] for r < rows, o < out_f;
 *                  x rows x_stride apart, y rows y_stride apart; act 0: none, 1: erf-GELU on the output, 2: SiLU on the input;
 *                  b and add nullable; add_stride 0: one row of `add` for every r. */
int srgd_k_time_features(const float* log_snr, const float* w, int half, int rows, float* feat, void* stream);
int srgd_k_linear_rows(const float* x, int x_stride, const float* W, const float* b, float* y, int y_stride, int rows, int in_f,
                       int out_f, int act, const float* add, int add_stride, void* stream);
/* The conditioning table of n log-SNR values and K >= 1 labels, computed by the engine's own routine on a table of this call's own
 * (no table of the engine is touched, no record added to its profile): row i * (K + 1) + k carries the class embedding of class_ids_host[k], row i * (K + 1) + K
 * none (K = 1 with class_ids_host[0] < 0: no label, both rows alike).  table_host: [(K + 1) * n][ss_stride] fp32 on the HOST.
 * `engine` is a finalized srgd_engine.  Synchronises. */
int srgd_k_conditioning_table(void* engine, const float* log_snr_host, int n, const int32_t* class_ids_host, int K,
                              float* table_host, void* stream);
/* The columns of that table: *ss_stride = its row width, *n_blocks = the number of ResnetBlocks (both nullable); for 0 <= index <
 * n_blocks, in the order the engine registered them: the block's state-dict prefix (name, nullable), the column of its scale vector
 * (*ss_offset; its shift vector follows at *ss_offset + *Cout) and its width.  index < 0: only the two totals. */
int srgd_k_conditioning_layout(void* engine, int* ss_stride, int* n_blocks, int index, char* name, size_t name_cap, int* ss_offset,
                               int* Cout);
/* gn_finalize alone: coefA / coefB [B][C] (device) from partial [B][groups][nslots][2], gamma, beta [C] and - if ss_table is given -
 * the (scale | shift) vectors at column ss_offset of row ss_rows[b] + *step_ptr * step_mul of a table with rows ss_stride wide
 * (ss_rows: device [B]; step_ptr: device int, nullable).  No tensor is passed: the statistics are the accumulators' alone.
 * eps = 1e-5.  Synchronises. */
int srgd_k_gn_coefficients(const float* partial, int nslots, int B, int hw, int C, int groups, const float* gamma, const float* beta,
                           const float* ss_table, int ss_stride, int ss_offset, const int* ss_rows, const int* step_ptr,
                           int step_mul, float* coefA, float* coefB, void* stream);

/* The conditioning rows of one U-Net batch of a sampler step, as the step's own launch (launch_step_rows) writes them: `engine` has
 * a begun run (srgd_sampler_begin / _begin_images / srgd_edm_begin, with or without srgd_sampler_image_labels).  The batch is tiles
 * [first, first + nt) of the even (parity 0) or odd grid in one (nb == nt) or two (nb == 2 nt) passes; ev = evaluation of the step
 * (EDM: 0 at sigma_hat, 1 at sigma_next); pass1_null: the second pass takes the null row.  rows_host: nb ints on the HOST, each
 * (K + 1) * ev + (label slot | K); the step's share (K + 1) * evals * step is added on the device and is not part of them.  The launch
 * writes to a buffer of this call's own: nothing of the run changes.  Synchronises. */
int srgd_k_step_rows(void* engine, int parity, int nb, int nt, int first, int ev, int pass1_null, int32_t* rows_host, void* stream);

/* Counter-based Gaussian noise (Philox4x32-10 + Box-Muller) for n_streams noise streams in ONE launch: the batched counterpart of
 * srgd_randn (srgd_hip.h).  Stream k writes counts_host[k] floats at dst + offsets_host[k] from seeds_host[k], with its counter
 * starting at 0: bit for bit what srgd_randn writes for (counts_host[k], seeds_host[k], stream_id).  Offsets and counts need not be
 * multiples of 4; the slices must not overlap.  The three arrays are on the HOST (uploaded inside; synchronises).  A seeded
 * lock-step run (srgd_sampler_noise_seeds) draws its tile, ring and q-start noise through this kernel. */
int srgd_randn_streams(float* dst, const int64_t* offsets_host, const int64_t* counts_host, const uint64_t* seeds_host,
                       int n_streams, uint64_t stream_id, void* stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif
