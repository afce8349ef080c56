/*
 * unipre3d_knn.h -- C-ABI of the MI355X (gfx950) k-nearest-neighbour search in 3-D (the groupers of Mamba3D, PCM and PointMLP).
 *
 * Stands in for `knn_cuda.KNN` (openpoints/models/Mamba3D/Mamba3D.py:16; not part of the reference tree) and for the reference's
 * distance-matrix + torch.topk forms (openpoints/models/PCM/PCM_utils.py:141-168, backbone/pointmlp.py:102-113,
 * layers/knn.py:7-61, layers/group.py:12-28).  fp32 data, int32 indices, contiguous row-major, raw DEVICE pointers and a HIP stream.
 * Returns 0 on success, 1 invalid argument, 3 launch failure.
 *
 *   u3d_knn(b, n, m, k, support (B,N,3), query (B,M,3), dist2 (B,M,k) or NULL, idx (B,M,k), stream)
 *        For every query the k support points of its own cloud with the smallest (d2, index) pairs in lexicographic order,
 *        ascending: equal distances go to the lower index, a duplicate of the query itself comes first at distance 0.
 *        d2 = (dx*dx + dy*dy) + dz*dz with dx = q.x - s.x (likewise y, z), every operation rounded on its own (no fused
 *        multiply-add): bit for bit what `((src - dst) ** 2).sum(-1)` gives.  d2 >= 0, so (bits(d2) << 32) | index is one uint64
 *        key with exactly that order; the selection runs on the key and yields k distinct in-range indices whatever the data.
 *        `dist2` receives the squared distances of the selected neighbours (NULL: not written).
 *        Invalid (1): a negative size, k < 1, k > n, k > U3D_KNN_MAX_K, a NULL mandatory pointer, b * ceil(m / 16) beyond 2^31 - 1.
 *        b == 0 or m == 0: 0 without a launch.  Inputs are assumed finite; for others only "k distinct in-range indices, every
 *        slot written" holds.
 *   u3d_knn_path(n, k)
 *        Host arithmetic only, no device is touched: 0 where u3d_knn would refuse (n, k), otherwise the number of LDS tiles
 *        (U3D_KNN_TILE support points each) the one kernel walks for a cloud of n points.  The launch and the query share one helper.
 */
#ifndef UNIPRE3D_KNN_H
#define UNIPRE3D_KNN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define U3D_KNN_MAX_K 64    /* one neighbour per lane of a wave; the largest k a backbone uses is 32 */
#define U3D_KNN_TILE 2048   /* support points per LDS tile (24 KB) */
#define U3D_KNN_QUERIES 16  /* queries per workgroup: sixteen waves, one query each */

int u3d_knn(int b, int n, int m, int k, const float* support, const float* query, float* dist2, int32_t* idx, void* stream);
int u3d_knn_path(int n, int k);

#ifdef __cplusplus
}
#endif
#endif
