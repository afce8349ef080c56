/*
 * unipre3d_batchnorm_cf.h -- C-ABI of the fused BatchNorm + activation + residual (+ max over L) on channels-first tensors
 * (nn.BatchNorm1d on a (B, C, L) input followed by ReLU or exact GELU, with a residual add in front of the activation and, where
 * asked, the adaptive_max_pool1d(., 1) behind it: PointMLP's and PCM's ConvBNReLU1D / ConvBNReLURes1D / PreExtraction), forward and
 * backward, fp32, gfx950.  Everything runs on the caller's stream, reads no device data on the host, uses no atomics and sums across
 * workgroups in a fixed order: two calls on the same inputs give the same bits and a forward + backward can be captured into a graph.
 *
 *   y = act(xhat gamma + beta [+ residual]),  xhat = (x - mean) invstd,  evaluated as (x - mean) (invstd gamma) + beta
 *
 * Shapes.  x, residual, y, dy, dx, dresidual are contiguous (B, C, L) fp32; they need 4-byte alignment only.  When L % 4 == 0 and every
 * one of a call's (B, C, L) tensors is 16-byte aligned the kernels move 16 bytes per lane, otherwise 4.  gamma, beta, mean, invstd,
 * running_mean, running_var are (C) fp32; a null gamma is 1 and a null beta 0 (affine=False).  act: 0 none, 1 relu, 2 gelu (erf form;
 * no residual).  The count per channel is M = B L.
 *
 * The cross-workgroup sum, the mean / invstd, the running statistics and the SyncBatchNorm block are libunipre3d_batchnorm.so's
 * (u3d_bn_sum, u3d_bn_finalize with count = B L): `partials` and `block` have that library's layout.
 *
 * Pooled form.  pooled[b, c] = max over l of y[b, c, l] and arg[b, c] (int32) = the lowest l that attains it; no (B, C, L) tensor is
 * written.  S >= 1 is the storage of pooled / arg (and of dpooled): S == 1 is (B, C); S > 1 needs B % S == 0 and puts row b at element
 * ((b / S) C + c) S + b % S, a contiguous (B / S, C, S) tensor.  Non-finite inputs are outside the contract of the pooled form: a NaN
 * is not propagated and a row without a finite maximum has an unspecified arg (the backward never follows an arg outside [0, L)).
 *
 *   u3d_bncf_plan        host only: the dispatch class of a shape.  lanes_per_row (a power of two up to 64) lanes own one (b, c) row
 *                        at a time, vec (4 where `aligned` and L % 4 == 0, else 1) floats each, in ceil(ceil(L / vec) / lanes_per_row)
 *                        sweeps; a workgroup takes channel_tile channels x batch_chunk batch entries.  Null outputs are skipped.
 *                        Returns 0, or 2 for a shape out of range.
 *   u3d_bncf_parts       host only: ceil(B / batch_chunk), the rows of `partials`; 0 for a shape out of range.
 *   u3d_bncf_stats       partials (parts, 2C) f64 = per-part sum x | sum x^2, every element written exactly once.  Where nbt is not
 *                        null it also advances *nbt (num_batches_tracked) by one, as u3d_bn_stats does.
 *   u3d_bncf_apply       pooled null: y from x (and residual, null: none).  pooled not null: y must be null, arg not null.
 *                        eval == 0: mean / second = mean / invstd; eval != 0: running_mean / running_var, folded with eps.
 *   u3d_bncf_bwd_reduce  partials (parts, 2C) f64 = per-part sum g | sum g xhat with g = dy act'(.).  arg null (dense): dy and y are
 *                        (B, C, L); relu reads the mask y > 0, gelu recomputes the pre-activation from x, none takes dy (y may be null for
 *                        the last two).  arg not null (pooled): dy = dpooled, y = pooled, both in the S layout; g is dpooled act'(.) at
 *                        l = arg and 0 elsewhere, the relu mask is pooled > 0, and x is read at B C positions only.
 *   u3d_bncf_bwd_apply   dx = gamma invstd (g - sum g / M - xhat sum(g xhat) / M) with M and the sums from `block`; block null (eval
 *                        mode): dx = g gamma invstd.  dresidual (null: not wanted) = g.  dx may be null when only dresidual is wanted.
 *                        Pooled (arg not null): x is read once and every element of dx / dresidual is written once, the zeros included.
 *
 * B >= 1, 1 <= C <= 1024, L >= 1.  Returns 0 ok, 1 invalid argument (a null or misaligned pointer: fp32 and int32 4 bytes, f64 and nbt
 * 8; y and pooled both or neither given), 2 unsupported shape or mode, 3 launch failure.
 */
#ifndef UNIPRE3D_BATCHNORM_CF_H
#define UNIPRE3D_BATCHNORM_CF_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define U3D_BNCF_ABI_VERSION 1
#define U3D_BNCF_MAX_CHANNELS 1024
#define U3D_BNCF_ACT_NONE 0
#define U3D_BNCF_ACT_RELU 1
#define U3D_BNCF_ACT_GELU 2
int u3d_bncf_abi_version(void);
int u3d_bncf_plan(int C, int L, int aligned, int* lanes_per_row, int* channel_tile, int* batch_chunk, int* vec);
long long u3d_bncf_parts(long long B, int C, int L);
int u3d_bncf_stats(const float* x, long long B, int C, int L, long long* nbt, double* partials, void* stream);
int u3d_bncf_apply(const float* x, const float* residual, long long B, int C, int L, int act, int eval, float eps, const float* mean,
                   const float* second, const float* gamma, const float* beta, float* y, float* pooled, int* arg, long long S,
                   void* stream);
int u3d_bncf_bwd_reduce(const float* dy, const float* x, const float* y, const int* arg, long long B, int C, int L, int act, int eval,
                        float eps, const float* mean, const float* second, const float* gamma, const float* beta, long long S,
                        double* partials, void* stream);
int u3d_bncf_bwd_apply(const float* dy, const float* x, const float* y, const int* arg, long long B, int C, int L, int act, int eval,
                       float eps, const float* mean, const float* second, const float* gamma, const float* beta, const double* block,
                       long long S, float* dx, float* dresidual, void* stream);
#ifdef __cplusplus
}
#endif
#endif
