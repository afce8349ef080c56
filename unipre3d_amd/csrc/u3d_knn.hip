// k-nearest-neighbour search in 3-D for gfx950 (include/unipre3d_knn.h); semantics restated on the CPU in tests/knn_ref.py.
//
// The reference's forms write a (B, M, N) distance matrix to HBM and run torch.topk over it.  Here nothing but the answer leaves
// the chip: a workgroup of sixteen waves stages the support cloud through LDS in tiles of KNN_TILE points (as three_nn_kernel does),
// every wave owns ONE query and walks the tile 64 candidates per step (lane l takes point j0 + l: three ds_read_b32 at a stride of
// three words, conflict-free).
//
// Selection runs on the uint64 key (bits(d2) << 32) | index with one key per lane, sorted across the wave: u3d_knn_core.h, shared
// with the offset-batched search of u3d_offsetops.hip.  There is no per-lane array: no scratch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unipre3d_knn.h"
#include "u3d_util.h"
#include "u3d_knn_core.h"

namespace {

using namespace u3d_util;
using namespace u3d_knn_core;

constexpr int KNN_Q = U3D_KNN_QUERIES;                               // queries per workgroup: one per wave
constexpr int KNN_THREADS = 64 * KNN_Q;
constexpr int KNN_TILE = U3D_KNN_TILE;

// 0: u3d_knn refuses (n, k); else the LDS tiles of a cloud of n points
inline int knn_tiles(int n, int k) {
  if (n < 1 || k < 1 || k > n || k > U3D_KNN_MAX_K) return 0;
  return (int)(((long long)n + KNN_TILE - 1) / KNN_TILE);
}

__global__ __launch_bounds__(KNN_THREADS) void knn_kernel(int n, int m, int k, int qblocks, const float* __restrict__ support,
                                                          const float* __restrict__ query, float* __restrict__ dist2,
                                                          int32_t* __restrict__ idx) {
  __shared__ float s_p[KNN_TILE * 3];
  const int bi = blockIdx.x / qblocks, qb = blockIdx.x - bi * qblocks;
  const uint32_t lane = lane_id();
  const int qi = qb * KNN_Q + (threadIdx.x >> 6);                    // this wave's query, if below m (wave-uniform)
  const bool live = qi < m;
  const float* q = query + ((size_t)bi * m + (live ? qi : 0)) * 3;
  const float qx = q[0], qy = q[1], qz = q[2];
  const float* sb = support + (size_t)bi * n * 3;
  uint64_t best = KEY_MAX;
  for (int t0 = 0; t0 < n; t0 += KNN_TILE) {
    const int cnt = min(KNN_TILE, n - t0);
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * 3; e += KNN_THREADS) s_p[e] = sb[(size_t)t0 * 3 + e];
    __syncthreads();
    if (live) best = knn_scan_tile(best, s_p, cnt, t0, k, lane, qx, qy, qz);   // (no barrier inside)
  }
  if (live && (int)lane < k) {
    const size_t o = ((size_t)bi * m + qi) * k + lane;
    idx[o] = (int32_t)(uint32_t)best;
    if (dist2) dist2[o] = __uint_as_float((uint32_t)(best >> 32));
  }
}

}  // namespace

extern "C" {

int u3d_knn_path(int n, int k) { return knn_tiles(n, k); }

int u3d_knn(int b, int n, int m, int k, const float* support, const float* query, float* dist2, int32_t* idx, void* stream) {
  if (b < 0 || n < 0 || m < 0) return 1;
  if (knn_tiles(n, k) == 0) return 1;
  if (b == 0 || m == 0) return 0;
  if (!support || !query || !idx) return 1;
  const long long qblocks = ((long long)m + KNN_Q - 1) / KNN_Q;
  if (qblocks * b > 2147483647ll || m > 2147483647 - KNN_Q) return 1;
  hipLaunchKernelGGL(knn_kernel, dim3((unsigned)(qblocks * b)), dim3(KNN_THREADS), 0, (hipStream_t)stream, n, m, k, (int)qblocks, support,
                     query, dist2, idx);
  return launched();
}

}  // extern "C"
