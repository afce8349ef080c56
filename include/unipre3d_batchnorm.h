/*
 * unipre3d_batchnorm.h -- C-ABI of the fused BatchNorm + activation + residual over point rows (nn.BatchNorm1d on a 2-D input followed
 * by ReLU or exact GELU, with the BasicBlock's residual add in front of the activation), forward and backward, fp32, gfx950.
 * Everything runs on the caller's stream, reads no device data on the host, uses no atomics and sums across workgroups in a fixed
 * order: two calls on the same inputs give the same bits and a forward + backward can be captured into a graph.
 *
 *   y = act(xhat gamma + beta [+ residual]),  xhat = (x - mean) invstd,  evaluated as (x - mean) (invstd gamma) + beta
 *
 * Shapes.  x, residual, y, dy, dx, dresidual are (N, C) fp32 with contiguous rows; they need 4-byte alignment only.  When C % 4 == 0
 * and every one of a call's row tensors is 16-byte aligned the kernels move 16 bytes per lane, otherwise 4.  gamma, beta, mean,
 * invstd, running_mean, running_var are (C) fp32; a null gamma is 1 and a null beta 0 (affine=False).  act: 0 none, 1 relu, 2 gelu
 * (erf form; no residual).  Each workgroup takes u3d_bn_row_chunk(C) rows; parts = ceil(N / chunk).
 *
 * A `block` is 1 + 2C doubles: the row count, then two per-channel sums.  A caller may add other processes' blocks between the sum
 * and the step that uses it (SyncBatchNorm).
 *
 *   u3d_bn_stats       partials (parts, 2C) f64 = per-chunk sum x | sum x^2.  Where nbt is not null it also advances
 *                      *nbt (num_batches_tracked) by one, so that the finalize that follows on the stream reads the advanced count.
 *   u3d_bn_sum         block = count | fixed-order sums of the partials; where not null, out_a (C) and out_b (C) get the two sums
 *                      in fp32 (the backward's dbeta and dgamma).
 *   u3d_bn_finalize    partials not null: the same sum into block first (count from the argument); null: block is read as it is.
 *                      mean_invstd (2C) = mean | 1 / sqrt(var_biased + eps), in f64 from the block.  Where not null, running_mean and
 *                      running_var move by `momentum` towards mean and the unbiased variance; momentum < 0 is the cumulative
 *                      average with factor 1 / *nbt (the advanced count).
 *   u3d_bn_apply       y from x (and residual, null: none).  eval == 0: mean / second = mean / invstd; eval != 0: running_mean /
 *                      running_var, folded with eps in the kernel's prologue.
 *   u3d_bn_bwd_reduce  partials (parts, 2C) f64 = per-chunk sum g | sum g xhat with g = dy act'(.): relu reads the mask y > 0 from the
 *                      saved output, gelu recomputes the pre-activation from x, none takes dy (y may be null for the last two).
 *   u3d_bn_bwd_apply   dx = gamma invstd (g - sum g / M - xhat sum(g xhat) / M) with M and the sums from `block`; block null (eval
 *                      mode): dx = g gamma invstd.  dresidual (null: not wanted) = g.  dx may be null when only dresidual is wanted.
 *
 * N >= 1, 1 <= C <= 1024.  Returns 0 ok, 1 invalid argument (a null or misaligned pointer: fp32 4 bytes, f64 and nbt 8), 2 unsupported
 * shape or mode, 3 launch failure.
 */
#ifndef UNIPRE3D_BATCHNORM_H
#define UNIPRE3D_BATCHNORM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define U3D_BN_ABI_VERSION 1
#define U3D_BN_MAX_CHANNELS 1024
#define U3D_BN_ACT_NONE 0
#define U3D_BN_ACT_RELU 1
#define U3D_BN_ACT_GELU 2
int u3d_bn_abi_version(void);
int u3d_bn_row_chunk(int C);
int u3d_bn_stats(const float* x, long long N, int C, long long* nbt, double* partials, void* stream);
int u3d_bn_sum(const double* partials, long long parts, int C, double count, double* block, float* out_a, float* out_b, void* stream);
int u3d_bn_finalize(const double* partials, long long parts, double count, double* block, int C, double eps, double momentum,
                    float* running_mean, float* running_var, const long long* nbt, float* mean_invstd, void* stream);
int u3d_bn_apply(const float* x, const float* residual, long long N, int C, int act, int eval, float eps, const float* mean,
                 const float* second, const float* gamma, const float* beta, float* y, void* stream);
int u3d_bn_bwd_reduce(const float* dy, const float* x, const float* y, long long N, int C, int act, int eval, float eps,
                      const float* mean, const float* second, const float* gamma, const float* beta, double* partials, void* stream);
int u3d_bn_bwd_apply(const float* dy, const float* x, const float* y, long long N, int C, int act, int eval, float eps,
                     const float* mean, const float* second, const float* gamma, const float* beta, const double* block, float* dx,
                     float* dresidual, void* stream);
#ifdef __cplusplus
}
#endif
#endif
