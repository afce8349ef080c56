/*
 * unipre3d_feature_propagation.h -- C-ABI of the decoder block of PointMLP (openpoints/models/backbone/pointmlp.py,
 * PointNetFeaturePropagation) and PCM (openpoints/models/PCM/PointMLP_layers.py): the search of the three nearest feature-carrying
 * points, the inverse-distance weights, the weighted gather of three rows per output and the cat with the skip features, in fp32.
 * gfx950, everything on the caller's stream, no host read of device data, no synchronisation, no float atomics: two calls on the same
 * inputs give the same bits, and a forward + backward pair can be captured into a graph on one stream.  Nothing of size (B,N,S) or
 * (B,N,3,D2) exists.
 *
 *   xyz1    (B,N,3) fp32 contiguous: the points to fill.      xyz2  (B,S,3) fp32 contiguous: the points that carry features.
 *   points1 (B,D1,N) fp32 contiguous, or NULL with D1 = 0.    points2  (B,D2,S) fp32 contiguous.
 *   idx     (B,N,3) int32, weight (B,N,3) fp32.  With S >= 3, per (b,n): the three smallest (d2, index) pairs over xyz2[b] in lexicographic
 *           order (ties go to the lower index; the contract of unipre3d_knn.h, whose u3d_knn with k = 3 returns the same idx bit for
 *           bit), d2 = (dx dx + dy dy) + dz dz with dx = xyz1.x - xyz2.x, every product and sum rounded on its own;
 *           r_j = 1 / (d2_j + 1e-8), w_j = r_j / ((r_0 + r_1) + r_2), IEEE divisions.  With S == 1: idx = (0,0,0), weight = (1,0,0).
 *   out     (B,D1+D2,N) fp32 contiguous.  out[b,c,n] = points1[b,c,n] for c < D1, and
 *           out[b,D1+c,n] = (w_0 p2[c,i_0] + w_1 p2[c,i_1]) + w_2 p2[c,i_2], p2 = points2[b], products and sums rounded on their own;
 *           with S == 1: out[b,D1+c,n] = points2[b,c,0].  An idx entry outside [0,S) (a caller's override) is never dereferenced: its term
 *           is 0, and it receives no gradient.
 *   lists   ptr (B,S+1), ent (B,3N) int32: support point s of batch element b is named by the entries ent[b, ptr[b,s] .. ptr[b,s+1]),
 *           each e = 3 n + j with idx[b,n,j] == s, in ascending e; ptr[b,0] = 0.  The entries whose idx lies outside [0,S) follow, in
 *           ascending e, in ent[b, ptr[b,S] .. 3N): every word of both arrays is written.
 *   dout    (B,D1+D2,N) fp32 contiguous.  dpoints2 (B,D2,S) fp32 contiguous: dpoints2[b,c,s] = sum over s's list, in its order, of
 *           weight[b,e] dout[b,D1+c,e/3]; the products are exact in f64, the sum runs in f64 and is rounded to fp32 once.  A support point
 *           no entry names gets 0.  The gradient to points1 is dout[:, :D1, :] itself: no kernel writes it.  There is no gradient to
 *           xyz1 and xyz2.
 *   scratch u3d_feature_propagation_scratch_bytes(B,N,S) bytes, 16-byte aligned, for u3d_feature_propagation_lists alone, which writes
 *           every one of them (the lists' S + 1 cursors per batch element and the 3N unsorted entries; the unsorted entries are the one
 *           thing whose order depends on an atomic, and nothing is computed from their order) and carries nothing to the next call.
 *
 *   u3d_feature_propagation_search  one launch: a lane per query, three uint64 keys (bits(d2) << 32) | index in registers, xyz2[b] staged
 *                                   through LDS in tiles of U3D_FEATURE_PROPAGATION_TILE points.
 *   u3d_feature_propagation_fwd     one launch: lanes along n, a workgroup per 256 queries and 16 output channels, the points1 half copied
 *                                   by the same launch.
 *   u3d_feature_propagation_lists   two launches: one workgroup per batch element counts with integer atomics, scans, and drops every
 *                                   entry into its list; then one wave per list ranks its entries, so the order inside a list is ascending
 *                                   and depends on no atomic.  (A list of L entries costs L^2 / 64 comparisons per lane: S == 1, where one
 *                                   list holds all 3N, is legal and slow.)
 *   u3d_feature_propagation_bwd     one launch: lanes along s, a workgroup per 256 support points and 8 channels; dout's 8 rows are staged in
 *                                   LDS 1024 queries at a time, and a lane takes from its list (ascending in n) the entries of that tile.
 *
 * B >= 1, 1 <= N <= 16384, S == 1 or 3 <= S <= 16384, 0 <= D1 <= 2048, 1 <= D2 <= 2048, B N < 2^24.  A null pointer (but points1 with
 * D1 == 0), a pointer off a 16-byte boundary or a dimension < 1 returns 1 before anything is launched; returns 0 ok, 1 invalid argument,
 * 2 unsupported shape, 3 launch failure.  u3d_feature_propagation_scratch_bytes returns 0 for a shape the library does not take.
 */
#ifndef UNIPRE3D_FEATURE_PROPAGATION_H
#define UNIPRE3D_FEATURE_PROPAGATION_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define U3D_FEATURE_PROPAGATION_ABI_VERSION 1
#define U3D_FEATURE_PROPAGATION_MAX_POINTS 16384
#define U3D_FEATURE_PROPAGATION_MAX_CHANNELS 2048
#define U3D_FEATURE_PROPAGATION_TILE 1024
int u3d_feature_propagation_abi_version(void);
size_t u3d_feature_propagation_scratch_bytes(int B, int N, int S);
int u3d_feature_propagation_search(const float* xyz1, const float* xyz2, int32_t* idx, float* weight, int B, int N, int S, void* stream);
int u3d_feature_propagation_lists(const int32_t* idx, int32_t* ptr, int32_t* ent, void* scratch, int B, int N, int S, void* stream);
int u3d_feature_propagation_fwd(const int32_t* idx, const float* weight, const float* points1, const float* points2, float* out, int B,
                                int N, int S, int D1, int D2, void* stream);
int u3d_feature_propagation_bwd(const int32_t* ptr, const int32_t* ent, const float* weight, const float* dout, float* dpoints2, int B,
                                int N, int S, int D1, int D2, void* stream);
#ifdef __cplusplus
}
#endif
#endif
