/*
 * unipre3d_mambaops.h -- C-ABI of the two operators a Mamba block needs around its selective scan, forward and backward, for the
 * mamba3d and pcm backbones: the causal depthwise conv1d (+ SiLU) of `causal_conv1d`, and the fused residual-add + LayerNorm / RMSNorm
 * of mamba_ssm's `ops/triton/layernorm.py`.  gfx950, fp32 throughout.  Everything runs on the caller's stream; no allocation, no host
 * sync, no host read of device data, no float atomics: two calls on the same inputs give the same bits.
 *
 * Causal conv (u3d_cconv_*):
 *   pre[b,d,l] = bias[d] + sum_w weight[d,w] * x[b,d,l-(W-1)+w]   (x is 0 at negative steps),   out = pre, or pre * sigmoid(pre) (silu)
 *   x: element (b,d,l) at x[b * x_batch_stride + d * x_chan_stride + l] (strides in elements, so that a channel slice of a wider tensor
 *   is read in place); weight (D,W) contiguous, W in 2 .. 4; bias (D) or NULL; out, dout, dx (B,D,L) contiguous.
 *   One wave owns one (b,d) row and walks it in chunks of u3d_cconv_chunk_len(L) steps (64 lanes x 1 .. 4 steps, chosen from L), one
 *   step per lane and load; the W-1 earlier taps come from the neighbouring lanes, and across a chunk edge from the chunk before.
 *   u3d_cconv_bwd recomputes pre from x: dpre = dout * act'(pre);  dx[l] = sum_w weight[d,w] dpre[l+(W-1)-w];
 *   dweight[d,w] = sum_{b,l} x[b,d,l-(W-1)+w] dpre[b,d,l];  dbias[d] = sum_{b,l} dpre (written when bias and dbias are given).
 *   dweight / dbias are wave sums per (b,d) row in one fixed order, written as partials to scratch and summed over b in ascending order
 *   by a second launch.  scratch: u3d_cconv_bwd_scratch_bytes(B, D) bytes of device memory, 256-byte aligned, contents irrelevant.
 *
 * Add + norm (u3d_addnorm_*), on (M,N) contiguous rows, 1 <= N <= u3d_addnorm_max_n():
 *   r = x + residual (residual may be NULL: r = x)
 *   LayerNorm: mean = sum r / N; var = sum (r - mean)^2 / N (centred); y = (r - mean) * rstd * weight (+ bias), rstd = 1 / sqrt(var + eps)
 *   RMSNorm:   y = r * rstd * weight (+ bias), rstd = 1 / sqrt(sum r^2 / N + eps)
 *   u3d_addnorm_fwd: one launch, one wave per row, the row in registers; writes y, r_out (when not NULL), rstd (M) and, for LayerNorm,
 *   mean (M).
 *   u3d_addnorm_bwd: from dy, r (what the forward normalised), the saved mean / rstd and dres (the gradient arriving on r, or NULL):
 *   wdy = weight * dy, xhat = (r - mean) * rstd (RMSNorm: r * rstd);  dx = (wdy - xhat * mean(xhat * wdy) - mean(wdy)) * rstd (+ dres)
 *   (RMSNorm: without the mean(wdy) term);  dweight = sum_rows dy * xhat;  dbias = sum_rows dy (when dbias is not NULL).
 *   u3d_addnorm_bwd_waves(M) waves share the rows: wave g owns M / waves rows, one more when g < M % waves, contiguous and ascending in g.
 *   Each wave accumulates dweight / dbias over its rows in registers, in double, and writes one partial row; a second launch sums the
 *   partials in ascending wave order and rounds to fp32 once.  scratch: u3d_addnorm_bwd_scratch_bytes(M, N) bytes, 256-byte aligned, contents irrelevant.
 *
 * Returns 0 ok, 1 invalid argument, 2 unsupported shape (W outside 2 .. 4, N above the cap), 3 launch failure.
 */
#ifndef UNIPRE3D_MAMBAOPS_H
#define UNIPRE3D_MAMBAOPS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define U3D_MAMBAOPS_ABI_VERSION 1
#define U3D_CCONV_MAX_WIDTH 4
#define U3D_ADDNORM_MAX_N 1024
int u3d_mambaops_abi_version(void);
int u3d_cconv_chunk_len(int L);
size_t u3d_cconv_bwd_scratch_bytes(int B, int D);
int u3d_cconv_fwd(const float* x, const float* weight, const float* bias, float* out, int64_t x_batch_stride, int64_t x_chan_stride,
                  int B, int D, int L, int W, int silu, void* stream);
int u3d_cconv_bwd(const float* x, const float* weight, const float* bias, const float* dout, float* dx, float* dweight, float* dbias,
                  void* scratch, size_t scratch_bytes, int64_t x_batch_stride, int64_t x_chan_stride, int B, int D, int L, int W,
                  int silu, void* stream);
int u3d_addnorm_max_n(void);
int u3d_addnorm_bwd_waves(int M);
size_t u3d_addnorm_bwd_scratch_bytes(int M, int N);
int u3d_addnorm_fwd(const float* x, const float* residual, const float* weight, const float* bias, float* y, float* r_out, float* mean,
                    float* rstd, int M, int N, float eps, int is_rms, void* stream);
int u3d_addnorm_bwd(const float* dy, const float* dres, const float* r, const float* weight, const float* mean, const float* rstd,
                    float* dx, float* dweight, float* dbias, void* scratch, size_t scratch_bytes, int M, int N, int is_rms, void* stream);
#ifdef __cplusplus
}
#endif
#endif
