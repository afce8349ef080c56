// libunipre3d_feature_propagation.so: the decoder block of PointMLP and PCM (PointNetFeaturePropagation: three nearest support points,
// inverse-distance weights, weighted gather of three rows, cat with the skip features), fp32, gfx950, wave64.
// include/unipre3d_feature_propagation.h states what is computed; DESIGN.md section 7 the cut into kernels and the order of every sum.
//
// The search and the forward run one lane per query n, so idx, weight and the one write of `out` are contiguous along n; the backward runs
// one lane per support point s, which walks s's inverse list.  Every loop is bounded by a size argument and the launch shape: indices and
// list bounds read from memory are clamped before use, odd data (NaN, inf, a damaged override) changes values, never addresses or trip
// counts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "u3d_group.h"
#include "u3d_knn_core.h"
#include "u3d_util.h"
#include "unipre3d_feature_propagation.h"

namespace {

using u3d_util::bad_ptr;

constexpr int TILE = U3D_FEATURE_PROPAGATION_TILE;   // support points staged per pass of the search (12 KB of LDS)
constexpr int SEARCH_NT = 128;                       // queries per workgroup of the search
constexpr int FWD_NT = 256, FWD_CT = 16;             // forward: 256 queries x 16 output channels per workgroup
constexpr int BWD_NT = 256, BWD_CT = 8;              // backward: 256 support points x 8 channels per workgroup
constexpr int BWD_TILE = 1024;                       // ... and dout's 8 rows staged 1024 queries at a time (32 KB of LDS)
constexpr int LIST_NT = 1024, LIST_WAVES = 16;
constexpr int SORT_NT = 256, SORT_WAVES = 4;

// ---- search ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SEARCH_NT) void fp_search_kernel(const float* __restrict__ xyz1, const float* __restrict__ xyz2,
                                                              int32_t* __restrict__ idx, float* __restrict__ weight, int N, int S, int nblk) {
#pragma clang fp contract(off)
  __shared__ float s_p[3 * TILE];
  const size_t b = blockIdx.x / nblk;
  const int n = (int)(blockIdx.x % nblk) * SEARCH_NT + (int)threadIdx.x;
  const bool on = n < N;
  const float* q = xyz1 + (b * N + (on ? n : N - 1)) * 3;       // (idle lanes search for the last query and write nothing)
  const float qx = q[0], qy = q[1], qz = q[2];
  const float* sup = xyz2 + b * S * 3;
  uint64_t k0 = u3d_knn_core::KEY_MAX, k1 = u3d_knn_core::KEY_MAX, k2 = u3d_knn_core::KEY_MAX;
  for (int t0 = 0; t0 < S; t0 += TILE) {
    const int cnt = min(TILE, S - t0);
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * cnt; i += SEARCH_NT) s_p[i] = sup[(size_t)t0 * 3 + i];
    __syncthreads();
    for (int j = 0; j < cnt; ++j) {
      const float d = u3d_knn_core::knn_dist2(qx, qy, qz, s_p[3 * j], s_p[3 * j + 1], s_p[3 * j + 2]);
      const uint64_t key = ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)(t0 + j);
      const bool l0 = key < k0, l1 = key < k1, l2 = key < k2;
      k2 = l1 ? k1 : (l2 ? key : k2);
      k1 = l0 ? k0 : (l1 ? key : k1);
      k0 = l0 ? key : k0;
    }
  }
  if (!on) return;
  int32_t* irow = idx + (b * N + n) * 3;
  float* wrow = weight + (b * N + n) * 3;
  if (S < 3) {                                       // (S == 1: the reference's repeat)
    irow[0] = irow[1] = irow[2] = 0;
    wrow[0] = 1.f;
    wrow[1] = wrow[2] = 0.f;
    return;
  }
  const float r0 = 1.f / (__uint_as_float((uint32_t)(k0 >> 32)) + 1e-8f);
  const float r1 = 1.f / (__uint_as_float((uint32_t)(k1 >> 32)) + 1e-8f);
  const float r2 = 1.f / (__uint_as_float((uint32_t)(k2 >> 32)) + 1e-8f);
  const float norm = (r0 + r1) + r2;
  irow[0] = (int32_t)(uint32_t)k0;
  irow[1] = (int32_t)(uint32_t)k1;
  irow[2] = (int32_t)(uint32_t)k2;
  wrow[0] = r0 / norm;
  wrow[1] = r1 / norm;
  wrow[2] = r2 / norm;
}

// ---- forward --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(FWD_NT) void fp_fwd_kernel(const int32_t* __restrict__ idx, const float* __restrict__ weight,
                                                        const float* __restrict__ points1, const float* __restrict__ points2,
                                                        float* __restrict__ out, int N, int S, int D1, int D2, int nblk) {
#pragma clang fp contract(off)
  const size_t b = blockIdx.x / nblk;
  const int n = (int)(blockIdx.x % nblk) * FWD_NT + (int)threadIdx.x;
  if (n >= N) return;
  const int C = D1 + D2;
  const int c0 = (int)blockIdx.y * FWD_CT, c1 = min(c0 + FWD_CT, C);
  int i0 = 0, i1 = 0, i2 = 0;
  float w0 = 0.f, w1 = 0.f, w2 = 0.f;
  bool v0 = false, v1 = false, v2 = false;
  if (c1 > D1) {
    const int32_t* irow = idx + (b * N + n) * 3;
    const float* wrow = weight + (b * N + n) * 3;
    const int a0 = irow[0], a1 = irow[1], a2 = irow[2];
    v0 = (unsigned)a0 < (unsigned)S;
    v1 = (unsigned)a1 < (unsigned)S;
    v2 = (unsigned)a2 < (unsigned)S;
    i0 = v0 ? a0 : 0;
    i1 = v1 ? a1 : 0;
    i2 = v2 ? a2 : 0;
    w0 = wrow[0];
    w1 = wrow[1];
    w2 = wrow[2];
  }
  for (int c = c0; c < c1; ++c) {                    // (c is uniform over the workgroup)
    float v;
    if (c < D1) {
      v = points1[(b * D1 + c) * N + n];
    } else {
      const float* row = points2 + (b * D2 + (c - D1)) * S;
      const float t0 = v0 ? w0 * row[i0] : 0.f, t1 = v1 ? w1 * row[i1] : 0.f, t2 = v2 ? w2 * row[i2] : 0.f;
      v = (t0 + t1) + t2;                            // (S == 1: 1 p + 0 p + 0 p)
    }
    out[(b * C + c) * N + n] = v;
  }
}

// ---- inverse lists (u3d_group.h) ------------------------------------------------------------------------------------------------
// One workgroup per batch element.  List of entry e: the support point it names, or S, the overflow list of the entries that name none.
__global__ __launch_bounds__(LIST_NT) void fp_list_build_kernel(const int32_t* __restrict__ idx, int32_t* ptr, int32_t* cur, int32_t* tmp,
                                                                int N, int S) {
  __shared__ uint32_t wt[LIST_WAVES];
  const size_t b = blockIdx.x;
  const int n3 = 3 * N;
  const int32_t* idx_b = idx + b * n3;
  const auto target = [idx_b, S](int e) {
    const int v = idx_b[e];
    return ((unsigned)v < (unsigned)S) ? v : S;
  };
  u3d_group::build_lists<LIST_NT, LIST_WAVES, true>(target, n3, S, ptr + b * (S + 1), cur + b * (S + 1), tmp + b * n3, wt);
}

// One wave per list; list S ends at 3N.
__global__ __launch_bounds__(SORT_NT) void fp_list_sort_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ tmp,
                                                               int32_t* __restrict__ ent, int N, int S, long long rows) {
  const uint32_t lane = u3d_util::lane_id();
  const long long row = (long long)blockIdx.x * SORT_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long long b = row / (S + 1);
  const int s = (int)(row % (S + 1)), n3 = 3 * N;
  const int32_t* pb = ptr + b * (S + 1);
  const int p0 = max(0, min(pb[s], n3)), p1 = s < S ? max(p0, min(pb[s + 1], n3)) : n3;
  u3d_group::rank_list(tmp + b * n3, ent + b * n3, p0, p1, lane);
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
// Lanes along s.  A list is ascending in e = 3 n + j, so it is ascending in n: the workgroup stages dout's 8 rows in LDS in tiles of
// BWD_TILE queries, and every lane takes from its list the entries of the tile at hand, in list order.
__global__ __launch_bounds__(BWD_NT) void fp_bwd_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ ent,
                                                        const float* __restrict__ weight, const float* __restrict__ dout,
                                                        float* __restrict__ dpoints2, int N, int S, int D1, int D2, int sblk) {
  __shared__ float sh[BWD_CT * BWD_TILE];
  const size_t b = blockIdx.x / sblk;
  const int s = (int)(blockIdx.x % sblk) * BWD_NT + (int)threadIdx.x;
  const bool on = s < S;
  const int n3 = 3 * N;
  const int c0 = (int)blockIdx.y * BWD_CT, nc = min(BWD_CT, D2 - c0);
  const int32_t* pb = ptr + b * (S + 1);
  const int32_t* eb = ent + b * n3;
  const float* wb = weight + b * n3;
  const float* g = dout + (b * (D1 + D2) + D1 + c0) * N;
  int p = 0, p1 = 0;                                 // (a lane past S has an empty list and keeps the barriers uniform)
  if (on) {
    p = max(0, min(pb[s], n3));
    p1 = max(p, min(pb[s + 1], n3));
  }
  double acc[BWD_CT];
#pragma unroll
  for (int i = 0; i < BWD_CT; ++i) acc[i] = 0.0;
  for (int n0 = 0; n0 < N; n0 += BWD_TILE) {
    const int cnt = min(BWD_TILE, N - n0);
    __syncthreads();
    for (int c = 0; c < nc; ++c)
      for (int k = threadIdx.x; k < cnt; k += BWD_NT) sh[c * BWD_TILE + k] = g[(size_t)c * N + n0 + k];
    __syncthreads();
    while (p < p1) {                                 // at most one turn per entry of the list
      const unsigned e = (unsigned)eb[p];
      const unsigned n = e / 3u;
      if (e < (unsigned)n3 && n >= (unsigned)(n0 + cnt)) break;          // a later tile's
      ++p;
      if (e >= (unsigned)n3 || n < (unsigned)n0) continue;               // (a damaged list: not an entry, or out of order)
      const double w = (double)wb[e];
      const int k = (int)n - n0;
#pragma unroll
      for (int i = 0; i < BWD_CT; ++i)
        if (i < nc) acc[i] += w * (double)sh[i * BWD_TILE + k];          // (the product of two floats is exact in f64)
    }
  }
  if (!on) return;
#pragma unroll
  for (int i = 0; i < BWD_CT; ++i)
    if (i < nc) dpoints2[(b * D2 + c0 + i) * S + s] = (float)acc[i];
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
int plan(int B, int N, int S) {
  if (B < 1 || N < 1 || S < 1) return 1;
  if (N > U3D_FEATURE_PROPAGATION_MAX_POINTS || S > U3D_FEATURE_PROPAGATION_MAX_POINTS || S == 2) return 2;
  if ((long long)B * N >= (1ll << 24) || (long long)B * (S + 1) >= (1ll << 30)) return 2;      // (the second: block counts stay ints)
  return 0;
}
int plan_channels(int D1, int D2) {
  if (D1 < 0 || D2 < 1) return 1;
  return (D1 > U3D_FEATURE_PROPAGATION_MAX_CHANNELS || D2 > U3D_FEATURE_PROPAGATION_MAX_CHANNELS) ? 2 : 0;
}

}  // namespace

extern "C" {

int u3d_feature_propagation_abi_version(void) { return U3D_FEATURE_PROPAGATION_ABI_VERSION; }

size_t u3d_feature_propagation_scratch_bytes(int B, int N, int S) {
  if (plan(B, N, S)) return 0;
  return ((size_t)B * (S + 1) + (size_t)B * 3 * N) * sizeof(int32_t);
}

int u3d_feature_propagation_search(const float* xyz1, const float* xyz2, int32_t* idx, float* weight, int B, int N, int S, void* stream) {
  if (bad_ptr(xyz1) || bad_ptr(xyz2) || bad_ptr(idx) || bad_ptr(weight)) return 1;
  if (const int rc = plan(B, N, S)) return rc;
  const int nblk = u3d_util::blocks(N, SEARCH_NT);
  hipLaunchKernelGGL(fp_search_kernel, dim3(B * nblk), dim3(SEARCH_NT), 0, (hipStream_t)stream, xyz1, xyz2, idx, weight, N, S, nblk);
  return u3d_util::launched();
}

int u3d_feature_propagation_lists(const int32_t* idx, int32_t* ptr, int32_t* ent, void* scratch, int B, int N, int S, void* stream) {
  if (bad_ptr(idx) || bad_ptr(ptr) || bad_ptr(ent) || bad_ptr(scratch)) return 1;
  if (const int rc = plan(B, N, S)) return rc;
  int32_t* cur = static_cast<int32_t*>(scratch);
  int32_t* tmp = cur + (size_t)B * (S + 1);
  hipLaunchKernelGGL(fp_list_build_kernel, dim3(B), dim3(LIST_NT), 0, (hipStream_t)stream, idx, ptr, cur, tmp, N, S);
  if (const int rc = u3d_util::launched()) return rc;
  const long long rows = (long long)B * (S + 1);
  hipLaunchKernelGGL(fp_list_sort_kernel, dim3(u3d_util::blocks(rows, SORT_WAVES)), dim3(SORT_NT), 0, (hipStream_t)stream, ptr, tmp, ent, N, S,
                     rows);
  return u3d_util::launched();
}

int u3d_feature_propagation_fwd(const int32_t* idx, const float* weight, const float* points1, const float* points2, float* out, int B,
                                int N, int S, int D1, int D2, void* stream) {
  if (bad_ptr(idx) || bad_ptr(weight) || bad_ptr(points2) || bad_ptr(out)) return 1;
  if (const int rc = plan_channels(D1, D2)) return rc;
  if (D1 > 0 ? bad_ptr(points1) : (points1 != nullptr && !u3d_util::aligned16(points1))) return 1;
  if (const int rc = plan(B, N, S)) return rc;
  const int nblk = u3d_util::blocks(N, FWD_NT);
  hipLaunchKernelGGL(fp_fwd_kernel, dim3(B * nblk, u3d_util::blocks(D1 + D2, FWD_CT)), dim3(FWD_NT), 0, (hipStream_t)stream, idx, weight,
                     points1, points2, out, N, S, D1, D2, nblk);
  return u3d_util::launched();
}

int u3d_feature_propagation_bwd(const int32_t* ptr, const int32_t* ent, const float* weight, const float* dout, float* dpoints2, int B,
                                int N, int S, int D1, int D2, void* stream) {
  if (bad_ptr(ptr) || bad_ptr(ent) || bad_ptr(weight) || bad_ptr(dout) || bad_ptr(dpoints2)) return 1;
  if (const int rc = plan_channels(D1, D2)) return rc;
  if (const int rc = plan(B, N, S)) return rc;
  const int sblk = u3d_util::blocks(S, BWD_NT);
  hipLaunchKernelGGL(fp_bwd_kernel, dim3(B * sblk, u3d_util::blocks(D2, BWD_CT)), dim3(BWD_NT), 0, (hipStream_t)stream, ptr, ent, weight, dout,
                     dpoints2, N, S, D1, D2, sblk);
  return u3d_util::launched();
}

}  // extern "C"
