// What the libraries that work on neighbour tables share (internal, like u3d_knn_core.h: header-only, no shared object).  Included by
// u3d_lnp.hip and u3d_local_grouper.hip for the row helpers and the normalisation pieces, and by u3d_local_grouper.hip and
// u3d_feature_propagation.hip for the inverse lists; each keeps its own kernels, constants and launch shapes.
//
// Rows.  A wave owns a row of a (rows, K) table: lanes 0 .. K-1 hold the row's indices (load_neighbours) and hand them round with
// v_readlane (lane_value).  The sums a normalisation needs leave a workgroup in two steps, wave_sums_to_lds and block_sums_to_part,
// with a barrier of the caller's between them; norm_stats turns the totals into the four values both forward kernels store, and is
// the one place that fixes the bits of every normalised output.
//
// Inverse lists.  A table's entries e in [0, n) each name a target in [0, L); list t is the ascending run of the entries that name t,
// ent[ptr[t] .. ptr[t + 1]).  build_lists does it for one batch element with ONE workgroup in four phases -- zero the counts, count
// with integer atomics into ptr[t + 1], scan in place, drop every entry at an atomic cursor -- separated by a device-scope fence and
// a barrier, since each phase reads words that other threads' atomics wrote (hence also the agent-scope loads of the scan: they must
// not be hoisted over the barrier or served from a stale line).  The order inside a list is arbitrary after the drop; a second launch
// ranks every list with one wave (rank_list).  build_lists ends with the drop: a caller that goes on in the same kernel to read tmp,
// or to build a second table with the same cur and wt, puts __threadfence(); __syncthreads(); between the two itself.
// lnp_neighbours_kernel of u3d_lnp.hip is NOT a copy of this and stays apart: counts and starts in LDS (G <= 1024), no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "u3d_util.h"

namespace u3d_group {

// ---- rows -----------------------------------------------------------------------------------------------------------------------
// lane k < K: neighbour k of the row, an index outside [0, limit) replaced by `fallback`
__device__ __forceinline__ int load_neighbours(const int32_t* idx_row, int K, int fallback, int limit, uint32_t lane) {
  int j = fallback;
  if ((int)lane < K) {
    const int v = idx_row[lane];
    j = ((unsigned)v < (unsigned)limit) ? v : fallback;
  }
  return j;
}
__device__ __forceinline__ int lane_value(int v, int k) { return __builtin_amdgcn_readlane(v, k); }

// NS = 1 or 2 f64 sums (s2 is ignored with NS = 1) of a workgroup of WAVES waves: every wave's totals to sh[0 .. NS)[wave] ...
template <int WAVES, int NS>
__device__ __forceinline__ void wave_sums_to_lds(double s1, double s2, double (*sh)[WAVES], uint32_t lane, int wave) {
  s1 = u3d_util::wave_sum_f64(s1);
  if (NS > 1) s2 = u3d_util::wave_sum_f64(s2);
  if (lane == 0) {
    sh[0][wave] = s1;
    if (NS > 1) sh[1][wave] = s2;
  }
}
// ... and, after a barrier, the waves' totals added in wave order by thread 0 into part[at], part[at + 1] (a sum there is none of: 0).
// `at` keeps the caller's type (32-bit in u3d_lnp.hip, size_t in u3d_local_grouper.hip), so the address is formed inside the branch as before.
template <int WAVES, int NS, typename Index>
__device__ __forceinline__ void block_sums_to_part(const double (*sh)[WAVES], double* part, Index at) {
  if (threadIdx.x == 0) {
    double x[2] = {0.0, 0.0};
    for (int i = 0; i < WAVES; ++i) {
#pragma unroll
      for (int q = 0; q < NS; ++q) x[q] += sh[q][i];
    }
    part[at] = x[0];
    part[at + 1] = x[1];
  }
}

// (sum d, sum d^2, count, eps) -> mean, unbiased std, r = 1 / (std + eps) and r^2 / ((n - 1) std), the factor of the backward's t.
// Every thread gets r; thread 0 of the workgroup that is number blk == 0 among those that share the sums stores the four to stats4
// (the others do not pay for the fourth).
__device__ __forceinline__ float norm_stats(double S1, double S2, double n, float eps, unsigned blk, float* stats4) {
  const double var = n > 1.0 ? fmax((S2 - S1 * S1 / n) / (n - 1.0), 0.0) : 0.0;
  const float mu = (float)(S1 / n), sd = (float)sqrt(var);
  const float r = 1.f / (sd + eps);
  if (blk == 0 && threadIdx.x == 0) {
    stats4[0] = mu;
    stats4[1] = sd;
    stats4[2] = r;
    stats4[3] = sd > 0.f ? (float)((double)r * (double)r / ((n - 1.0) * (double)sd)) : 0.f;
  }
  return r;
}

// ---- inverse lists --------------------------------------------------------------------------------------------------------------
// One batch element's table by one workgroup of NT = 64 NW threads; target(e) in [0, L] is entry e's list, wt NW words of LDS.
// ptr_b[0 .. L] receives the starts (inclusive scan of the counts in ptr_b[1 ..]), tmp_b[0 .. n) the entries list by list, cur_b the
// cursors.  OVERFLOW: target L is the list of the entries that name nothing; it is not counted, starts at cur_b[L] = ptr_b[L] and
// ends at n.  Without it no entry has target L and cur_b has L words.
template <int NT, int NW, bool OVERFLOW, typename Target>
__device__ __forceinline__ void build_lists(Target target, int n, int L, int32_t* ptr_b, int32_t* cur_b, int32_t* tmp_b, uint32_t* wt) {
  static_assert(NT == 64 * NW, "one scan slot per wave");
  for (int j = threadIdx.x; j <= L; j += NT) ptr_b[j] = 0;
  __threadfence();
  __syncthreads();
  for (int e = threadIdx.x; e < n; e += NT) {
    const int t = target(e);
    if (!OVERFLOW || t < L) atomicAdd(&ptr_b[t + 1], 1);
  }
  __threadfence();
  __syncthreads();
  const int per = (L + 1 + NT - 1) / NT;
  const int lo = min((int)threadIdx.x * per, L + 1), hi = min(lo + per, L + 1);
  uint32_t sum = 0;
  for (int i = lo; i < hi; ++i) sum += (uint32_t)__hip_atomic_load(&ptr_b[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  uint32_t all;
  uint32_t run = u3d_util::block_excl_scan<NW>(sum, wt, all);
  for (int i = lo; i < hi; ++i) {
    run += (uint32_t)__hip_atomic_load(&ptr_b[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ptr_b[i] = (int32_t)run;
    if (OVERFLOW || i < L) cur_b[i] = (int32_t)run;
  }
  __threadfence();
  __syncthreads();
  for (int e = threadIdx.x; e < n; e += NT) {
    const int pos = atomicAdd(&cur_b[target(e)], 1);
    if ((unsigned)pos < (unsigned)n) tmp_b[pos] = e;
  }
}

// one list by one wave: its entries are distinct, entry x goes to the place (number of smaller entries)
__device__ __forceinline__ void rank_list(const int32_t* __restrict__ tmp, int32_t* __restrict__ dst, int p0, int p1, uint32_t lane) {
  for (int i0 = p0; i0 < p1; i0 += 64) {
    const int i = i0 + (int)lane;
    if (i < p1) {
      const int x = tmp[i];
      int rank = 0;
      for (int q = p0; q < p1; ++q) rank += tmp[q] < x ? 1 : 0;
      dst[p0 + rank] = x;
    }
  }
}

}  // namespace u3d_group
