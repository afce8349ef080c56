/*
 * unipre3d_lnp.h -- C-ABI of Mamba3D's local norm pooling (openpoints/models/Mamba3D/Mamba3D.py: GroupFeature's gathers, K_Norm and
 * K_Pool, the first half of every LNPBlock), fused and in fp32.  gfx950, everything on the caller's stream, no host read of device
 * data, no synchronisation, no float atomics: two calls on the same inputs give the same bits, and a forward + backward pair can be
 * captured into a graph on one stream.  No (B,G,K,.) float tensor is ever written.
 *
 *   x      (B,G,C) fp32, rows of C contiguous, batch element b at x + b * x_batch_stride (in floats, a multiple of 4, >= G*C): the
 *          reference's feat[:, 1:, :] view is passed as it lies.
 *   idx    (B,G,K) int32 row indices into the same batch element.  An index outside [0, G) is never dereferenced: it counts as the
 *          row itself (d = 0), in all three entry points.
 *   alpha, beta (2C) fp32: affine_alpha_feat and affine_beta_feat.
 *   out    (B,G,2C) fp32.  With d[b,g,k,c] = x[b,idx[b,g,k],c] - x[b,g,c], n = B G K C, mu = mean(d), s = sqrt(sum (d-mu)^2 / (n-1)),
 *          r = 1/(s+eps), v = alpha[c] d r + beta[c], p = softmax_k(v):  out[b,g,c] = sum_k p_k v_k  (c < C, the row maximum is
 *          subtracted before exp) and out[b,g,C+c] = alpha[C+c] x[b,g,c] + beta[C+c].
 *   lse    (B,G,C) fp32 = log sum_k exp(v_k).
 *   stats  4 floats: mu, s, r, r^2 / ((n-1) s) (0 where s == 0: the variance term of the backward is then taken as 0).
 *   ptr    (B,G+1) int32, ent (B,G*K) int32: the inverse neighbour lists.  Row j of batch element b is named by the entries
 *          ent[b, ptr[b,j] .. ptr[b,j+1]), each e = g K + k with idx[b,g,k] == j (after the rule above), in ascending e.
 *   dout like out, dx (B,G,C) contiguous, dalpha and dbeta (2C).
 *   scratch  u3d_lnp_scratch_bytes(B,G,K,C,backward) bytes, 16-byte aligned; the forward (backward = 0) and the backward (1) each
 *          write exactly that many bytes from its start: per-workgroup partial sums (f64 for mu, s and t = sum gu d; fp32 rows for
 *          dalpha and dbeta), which are then summed in a fixed order in f64.  It carries nothing from one call to the next.
 *
 *   u3d_lnp_neighbours  one workgroup per batch element: counts with integer LDS atomics, an exclusive scan, and every list filled
 *                       by one thread that walks idx in ascending (g,k) -- the order inside a list depends on no atomic.
 *   u3d_lnp_fwd         two launches: partial sums of d and d^2 (one wave per row, f64), then one wave per (b,g) row: every
 *                       workgroup sums the partials in the same order, the wave gathers its K neighbour rows twice (row maximum, then
 *                       exp) and writes out, lse; workgroup 0 writes stats.
 *   u3d_lnp_bwd         two launches: per row, v and p = exp(v - lse) are recomputed and t, dalpha, dbeta leave as per-workgroup
 *                       partials; then one wave per destination row gathers dx over its inverse list (and its own K neighbours),
 *                       while further workgroups of the same launch sum the dalpha / dbeta partials.
 *
 * B >= 1, 1 <= G <= 1024, 2 <= K <= 32, C a multiple of 4 and <= 512, B G <= 2^22, eps >= 0.  A null pointer, a pointer off a 16-byte
 * boundary, a dimension < 1, a bad stride or eps returns 1 before anything is launched; returns 0 ok, 1 invalid argument, 2 unsupported
 * shape, 3 launch failure.  u3d_lnp_scratch_bytes returns 0 for a shape the library does not take.
 */
#ifndef UNIPRE3D_LNP_H
#define UNIPRE3D_LNP_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define U3D_LNP_ABI_VERSION 1
#define U3D_LNP_MAX_GROUPS 1024
#define U3D_LNP_MAX_K 32
#define U3D_LNP_MAX_CHANNELS 512
int u3d_lnp_abi_version(void);
size_t u3d_lnp_scratch_bytes(int B, int G, int K, int C, int backward);
int u3d_lnp_neighbours(const int32_t* idx, int32_t* ptr, int32_t* ent, int B, int G, int K, void* stream);
int u3d_lnp_fwd(const float* x, long long x_batch_stride, const int32_t* idx, const float* alpha, const float* beta, float* out,
                float* lse, float* stats, void* scratch, int B, int G, int K, int C, float eps, void* stream);
int u3d_lnp_bwd(const float* x, long long x_batch_stride, const int32_t* idx, const int32_t* ptr, const int32_t* ent,
                const float* alpha, const float* beta, const float* out, const float* lse, const float* stats, const float* dout,
                float* dx, float* dalpha, float* dbeta, void* scratch, int B, int G, int K, int C, void* stream);
#ifdef __cplusplus
}
#endif
#endif
