/*
 * unipre3d_local_grouper.h -- C-ABI of the LocalGrouper of PointMLP (openpoints/models/backbone/pointmlp.py) and PCM
 * (openpoints/models/PCM/PointMLP_layers.py), the "geometric affine" block of every encoder stage: the gathers of the K neighbours'
 * features and coordinates, the subtraction of the group mean or of the anchor, the division by one standard deviation per batch element,
 * the affine and the cat with the anchor's feature, fused and in fp32.  gfx950, everything on the caller's stream, no host read of device
 * data, no synchronisation, no float atomics: two calls on the same inputs give the same bits, and a forward + backward pair can be captured
 * into a graph on one stream.  The only (B,S,K,.) float tensors are out and dout.
 *
 *   xyz     (B,N,3) fp32 contiguous.
 *   points  (B,N,D) fp32 read in place: element (b,j,c) at points + b * p_batch + j * p_point + c * p_chan (strides in floats), with
 *           (p_point, p_chan) = (D, 1) (rows contiguous) or (1, N) (the permute(0,2,1) view of a (B,D,N) tensor); p_batch >= N D.
 *   fps     (B,S) int32 anchors, or NULL for the identity (then S == N).  An entry outside [0, N) is never dereferenced: anchor s then
 *           counts as point s.  Duplicates are legal.
 *   idx     (B,S,K) int32 into [0, N).  An entry outside [0, N) is never dereferenced: it counts as the anchor fps[b,s] (so d = 0 with
 *           normalize = anchor), in every entry point.
 *   alpha, beta  (D + A) fp32, A = 3 with use_xyz and 0 without.
 *   normalize    0 none, 1 center, 2 anchor.
 *   out     (B,S,K,C) fp32, C = 2 D + A; channels_first = 0: that array contiguous; 1: stored as (B,S,C,K).  Per batch element b, with
 *           g[s,k,:] = cat(points[idx[s,k]], xyz[idx[s,k]]) (the xyz part only with use_xyz), m[s,:] = (sum_k g[s,k,:]) / K (center, the sum
 *           in ascending k) or cat(points[fps[s]], xyz[fps[s]]) (anchor), d = g - m, n = S K (D + A), mu = mean(d),
 *           s_b = sqrt(sum (d - mu)^2 / (n - 1)), r = 1 / (s_b + eps):  out[s,k,c] = alpha[c] d r + beta[c] for c < D + A (one fma), and
 *           out[s,k,D+A+c] = points[fps[s],c].  With normalize = none the first D + A channels are g itself.
 *   new_xyz (B,S,3) = xyz[fps].
 *   mean    (B,S,D+A) fp32 = m;  stats (B,4) fp32 = mu, s_b, r, r^2 / ((n-1) s_b) (0 where s_b == 0: the variance term of the backward is
 *           then taken as 0, where the reference's gradient is NaN).  With normalize = none neither is touched, nor alpha, beta, dalpha,
 *           dbeta and the forward's scratch (they may be NULL).
 *   lists   ptr (B,N+1), ent (B,S K): point j of batch element b is named by the entries ent[b, ptr[b,j] .. ptr[b,j+1]), each
 *           e = s K + k with idx[b,s,k] == j (after the rule above), in ascending e.  fptr (B,N+1), fent (B,S): the same for fps, e = s.
 *   dout    like out, in either layout (dout_channels_first);  dpoints (B,N,D) written through strides of the same two forms as points:
 *           dpoints[b,j,c] = sum over ent of gg[s,k,c] + sum over fent of (gm[s,c] + sum_k dout[s,k,D+A+c]), where gy = dout[..., :D+A],
 *           T_b = sum alpha gy d, gd = alpha gy r - r^2 T_b (d - mu) / ((n-1) s_b), gg = gd - mean_k gd (center) or gd (anchor, with
 *           gm = -sum_k gd), and gg = gy with normalize = none.  A point that no list names gets 0.  dalpha = sum gy d r, dbeta = sum gy.
 *           There is no gradient to xyz.
 *   scratch u3d_local_grouper_scratch_bytes(B,N,S,K,D,use_xyz,normalize,pass) bytes, 16-byte aligned, pass 0 forward, 1 backward,
 *           2 lists; each pass writes exactly that many bytes from its start (f64 per-workgroup partial sums of d, d^2 and T_b, fp32
 *           per-workgroup rows of dalpha and dbeta, the (B,S,.) helpers sum_k gy, sum_k d and sum_k dout[..., D+A:], the lists' cursors and
 *           unsorted entries) and carries nothing from one call to the next.  The unsorted entries are the one thing whose order depends on
 *           an atomic; nothing is computed from their order.
 *
 *   u3d_local_grouper_lists  two launches: one workgroup per batch element counts with integer atomics, scans, and drops every entry into
 *                            its list; then one wave per point ranks each list's entries, so the order inside a list is ascending and
 *                            depends on no atomic.
 *   u3d_local_grouper_fwd    two launches (one with normalize = none): m and the f64 partial sums of d and d^2, one wave per (b,s) row; then
 *                            one wave per row writes the row's K C outputs in storage order (every workgroup sums its batch element's
 *                            partials in the same order).
 *   u3d_local_grouper_bwd    two launches: per row, sum_k gy, sum_k d, sum_k ga, and the partials of T_b, dalpha and dbeta; then one wave per
 *                            point gathers dpoints over its two lists, while further workgroups of the same launch sum the dalpha / dbeta
 *                            partials in a fixed order in f64.
 *
 * B >= 1, 1 <= S <= N <= 16384, 2 <= K <= 64, D a multiple of 4 and <= 512, B S K < 2^24, B N < 2^24, eps >= 0.  A null pointer, a pointer off a 16-byte
 * boundary, a dimension < 1, a stride of neither form, a bad flag or eps returns 1 before anything is launched; returns 0 ok, 1 invalid
 * argument, 2 unsupported shape, 3 launch failure.  u3d_local_grouper_scratch_bytes returns 0 for a shape the library does not take.
 */
#ifndef UNIPRE3D_LOCAL_GROUPER_H
#define UNIPRE3D_LOCAL_GROUPER_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define U3D_LOCAL_GROUPER_ABI_VERSION 1
#define U3D_LOCAL_GROUPER_MAX_POINTS 16384
#define U3D_LOCAL_GROUPER_MAX_K 64
#define U3D_LOCAL_GROUPER_MAX_CHANNELS 512
int u3d_local_grouper_abi_version(void);
size_t u3d_local_grouper_scratch_bytes(int B, int N, int S, int K, int D, int use_xyz, int normalize, int pass);
int u3d_local_grouper_lists(const int32_t* fps, const int32_t* idx, int32_t* ptr, int32_t* ent, int32_t* fptr, int32_t* fent, void* scratch,
                            int B, int N, int S, int K, void* stream);
int u3d_local_grouper_fwd(const float* xyz, const float* points, long long p_batch, long long p_point, long long p_chan, const int32_t* fps,
                          const int32_t* idx, const float* alpha, const float* beta, float* out, float* new_xyz, float* mean, float* stats,
                          void* scratch, int B, int N, int S, int K, int D, int use_xyz, int normalize, int channels_first, float eps,
                          void* stream);
int u3d_local_grouper_bwd(const float* xyz, const float* points, long long p_batch, long long p_point, long long p_chan, const int32_t* fps,
                          const int32_t* idx, const int32_t* ptr, const int32_t* ent, const int32_t* fptr, const int32_t* fent,
                          const float* alpha, const float* mean, const float* stats, const float* dout, float* dpoints, long long g_batch,
                          long long g_point, long long g_chan, float* dalpha, float* dbeta, void* scratch, int B, int N, int S, int K, int D,
                          int use_xyz, int normalize, int dout_channels_first, void* stream);
#ifdef __cplusplus
}
#endif
#endif
