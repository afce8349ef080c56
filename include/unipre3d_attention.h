/*
 * unipre3d_attention.h -- C-ABI of the two operators the PTv3 backbone needs beyond torch and the sparse convolution:
 * variable-length packed-QKV attention (flash-attn's flash_attn_varlen_qkvpacked_func, non-causal) and torch_scatter's segment_csr.
 * gfx950, everything on the caller's stream, no host read of device data, no float atomics: two calls on the same inputs give the
 * same bits.
 *
 * Attention (fp16 in / out, fp32 scores, row max / row sum, P.V and gradient accumulation; v_mfma_f32_16x16x16_f16):
 *   qkv (T,3,H,D) fp16 contiguous, cu_seqlens (S+1) int32 ascending from 0, D == 16, 1 <= max_seqlen <= 1024.
 *   u3d_attn_varlen_fwd   out (T,H,D) fp16, lse (H,T) fp32 = log sum exp(softmax_scale * q.k) per row.  Every row of out / lse is
 *                         written: rows at or beyond cu_seqlens[S], and rows of a sequence beyond its first max_seqlen, as zeros
 *                         (such rows are not keys either).
 *   u3d_attn_varlen_bwd   dqkv (T,3,H,D) fp16 from dout (T,H,D) fp16, out and lse of the forward; P is recomputed from lse,
 *                         delta = rowsum(dout * out) in fp32.  dK / dV are summed over query blocks in a fixed order inside one
 *                         workgroup.  Rows outside the sequences are written as zeros.
 *   One (sequence, head) is one wave for max_seqlen <= 64 and one workgroup of 4 .. 16 waves above.
 *
 * segment_csr (fp32, src (N,C) row-major, indptr (M+1) int64 ascending, 0 <= indptr <= N):
 *   u3d_segment_csr_fwd   reduce 0 sum, 1 mean, 2 max, 3 min over rows indptr[m] .. indptr[m+1]-1 in ascending row order; an empty
 *                         segment gives 0 (arg -1).  arg (M,C) int64 (max / min only, else NULL): the lowest row that attains the
 *                         extremum; a NaN wins over every number and the lowest NaN row is the argument.
 *   u3d_segment_csr_bwd   dsrc (N,C): sum -> dout[m], mean -> dout[m] / count, max / min -> dout[m] at row arg[m,c], else 0; rows
 *                         outside [indptr[0], indptr[M]) get 0.  Every element is written once.
 *
 * Returns 0 ok, 1 invalid argument, 2 unsupported shape, 3 launch failure.
 */
#ifndef UNIPRE3D_ATTENTION_H
#define UNIPRE3D_ATTENTION_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define U3D_ATTN_ABI_VERSION 1
#define U3D_ATTN_MAX_SEQLEN 1024
int u3d_attn_abi_version(void);
int u3d_attn_varlen_fwd(const void* qkv, const int32_t* cu_seqlens, void* out, float* lse, int T, int S, int H, int D, int max_seqlen,
                        float softmax_scale, void* stream);
int u3d_attn_varlen_bwd(const void* qkv, const int32_t* cu_seqlens, const void* out, const void* dout, const float* lse, void* dqkv,
                        int T, int S, int H, int D, int max_seqlen, float softmax_scale, void* stream);
int u3d_segment_csr_fwd(const float* src, const int64_t* indptr, float* out, int64_t* arg, int N, int M, int C, int reduce,
                        void* stream);
int u3d_segment_csr_bwd(const float* dout, const int64_t* indptr, const int64_t* arg, float* dsrc, int N, int M, int C, int reduce,
                        void* stream);
#ifdef __cplusplus
}
#endif
#endif
