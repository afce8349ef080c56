/*
 * unipre3d_mha.h -- C-ABI of the dense multi-head attention of the transformer backbone (openpoints' PointTransformerEncoder:
 * Attention.forward's core, between the packed qkv Linear and proj), fused and in fp32.  gfx950, everything on the caller's stream, no
 * host read of device data, no synchronisation, no float atomics: two calls on the same inputs give the same bits, and a forward +
 * backward pair can be captured into a graph on one stream.
 *
 *   qkv  (B,N,3,H,D) fp32 contiguous: the output of nn.Linear(dim, 3 dim) as the reference views it (no permute copy).
 *   out  (B,N,H,D)   fp32: out[b,n,h] = softmax_m(softmax_scale * q[b,n,h] . k[b,m,h]) @ v[b,m,h], i.e. the (B,N,C) tensor proj reads.
 *   lse  (B,H,N)     fp32 = log sum_m exp(softmax_scale * q . k) per row.
 *   dout like out, dqkv like qkv.
 *   D == 64, H >= 1, B >= 1, 1 <= N <= 1024, softmax_scale > 0; non-causal, no mask, no dropout.
 *
 *   u3d_mha_fwd   v_mfma_f32_16x16x4_f32 (exact f32 fma chains) for q.k and P.V, online softmax over blocks of 64 keys; no N x N
 *                 tensor exists.  Every element of out and lse is written.
 *   u3d_mha_bwd   P is recomputed from lse, delta = rowsum(dout * out) in fp32; one grid over key blocks owns dK and dV (summed over
 *                 query blocks in ascending order), one over query blocks owns dQ.  Every element of dqkv is written.
 *
 * A null pointer, a pointer off a 16-byte boundary, B, N or H < 1 or a softmax_scale that is not a positive finite number returns 1
 * before anything is launched.  Returns 0 ok, 1 invalid argument, 2 unsupported shape (D != 64, N > 1024), 3 launch failure.
 */
#ifndef UNIPRE3D_MHA_H
#define UNIPRE3D_MHA_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define U3D_MHA_ABI_VERSION 1
#define U3D_MHA_MAX_SEQLEN 1024
#define U3D_MHA_HEAD_DIM 64
int u3d_mha_abi_version(void);
int u3d_mha_fwd(const float* qkv, float* out, float* lse, int B, int N, int H, int D, float softmax_scale, void* stream);
int u3d_mha_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                int B, int N, int H, int D, float softmax_scale, void* stream);
#ifdef __cplusplus
}
#endif
#endif
