// The selection core of the 3-D nearest-neighbour searches (internal, like u3d_keysort.h: header-only, no shared object).  Included by
// u3d_knn.hip (dense (B,N,3) clouds) and u3d_offsetops.hip (concatenated clouds with cumulative offsets); each keeps its own kernel,
// staging and launch shape and calls knn_scan_tile on the points it has staged in LDS.
//
// Selection.  A candidate is the uint64 key (bits(d2) << 32) | index: d2 >= 0, so unsigned order on the key IS the contract's
// lexicographic (d2, index) order, and keys are distinct.  A query's running answer is ONE key per lane, sorted ascending across
// the wave (lane i: the i-th smallest; KEY_MAX where there is none yet).  `thr`, the key in lane k - 1, is the bar: a ballot finds
// the step's candidates below it, and
//   * a few (<= KNN_MERGE_ABOVE: the usual case after the first steps) are inserted one by one with a wave-wide shift -- lane i
//     keeps its key if it is below x, else takes max(x, key of lane i - 1) -- after each of which the bar drops;
//   * many (the first step, where the bar is still KEY_MAX; clouds that arrive in order of falling distance) are handled at a fixed
//     price: the step's 64 keys are sorted across the wave (bitonic network, 21 exchanges) and merged into the list (the lane-wise
//     minimum of the list and the reversed candidates is the lower half of the 128 as a bitonic sequence; 6 exchanges sort it).
// Either way lanes 0..k-1 are the k smallest keys seen so far and the list is sorted; lanes k..63 hold overflow that never
// re-enters.  The answer is the k smallest keys of the points scanned whatever the order of arrival, so it does not depend on how
// points fall into lanes, steps or tiles, nor on which of the two routes a step took.
//
// Every loop is bounded by the count scanned and the launch shape: the insertion loop runs at most KNN_MERGE_ABOVE times per step
// (one per ballot bit) and leaves early when the ballot is used up; odd data (NaN, inf) changes keys, never trip counts.  There is
// no per-lane array: no scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace u3d_knn_core {

constexpr int KNN_MERGE_ABOVE = 8;   // more candidates below the bar than this: sort and merge the step (measured: DESIGN.md)
constexpr uint64_t KEY_MAX = ~0ull;                                  // above every key: no point has index 2^32 - 1

__device__ __forceinline__ uint64_t read_lane_u64(uint64_t v, int lane) {   // `lane` is wave-uniform
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
  return ((uint64_t)hi << 32) | lo;
}
// the key of lane - 1; lane 0 receives 0, which is below every key (wave_shr:1, bound_ctrl: a lane without a source reads 0)
__device__ __forceinline__ uint64_t lane_below_u64(uint64_t v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x138, 0xf, 0xf, true);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x138, 0xf, 0xf, true);
  return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ float knn_dist2(float qx, float qy, float qz, float sx, float sy, float sz) {
#pragma clang fp contract(off)   // every product and sum rounded on its own: ((q - s) ** 2).sum(-1)
  const float dx = qx - sx, dy = qy - sy, dz = qz - sz;
  return (dx * dx + dy * dy) + dz * dz;
}

// one exchange of a sorting network: lane and lane ^ S compare keys, the lane with bit S clear keeps the smaller iff `up`
template <int S>
__device__ __forceinline__ uint64_t lane_xor_u64(uint64_t v) {       // the key of lane ^ S: DPP where one control does it, else ds_bpermute
  constexpr int CTRL = S == 1 ? 0xB1 : S == 2 ? 0x4E : S == 8 ? 0x128 : 0;   // quad_perm [1,0,3,2] | quad_perm [2,3,0,1] | row_ror:8
  if (CTRL == 0) return __shfl_xor(v, S);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, CTRL, 0xf, 0xf, false);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), CTRL, 0xf, 0xf, false);
  return ((uint64_t)hi << 32) | lo;
}
template <int S>
__device__ __forceinline__ uint64_t exchange_u64(uint64_t v, uint32_t lane, bool up) {
  const uint64_t p = lane_xor_u64<S>(v);
  return ((p < v) == (((lane & S) == 0) == up)) ? p : v;
}
template <int SIZE>
__device__ __forceinline__ uint64_t bitonic_stage_u64(uint64_t v, uint32_t lane) {   // sorted runs of SIZE / 2 -> runs of SIZE, alternating
  const bool up = (lane & SIZE) == 0;                                                 // direction (SIZE = 64: all ascending)
  if (SIZE > 32) v = exchange_u64<32>(v, lane, up);
  if (SIZE > 16) v = exchange_u64<16>(v, lane, up);
  if (SIZE > 8) v = exchange_u64<8>(v, lane, up);
  if (SIZE > 4) v = exchange_u64<4>(v, lane, up);
  if (SIZE > 2) v = exchange_u64<2>(v, lane, up);
  return exchange_u64<1>(v, lane, up);
}
__device__ __forceinline__ uint64_t wave_sort_u64(uint64_t v, uint32_t lane) {        // the wave's 64 keys, ascending across lanes
  v = bitonic_stage_u64<2>(v, lane);
  v = bitonic_stage_u64<4>(v, lane);
  v = bitonic_stage_u64<8>(v, lane);
  v = bitonic_stage_u64<16>(v, lane);
  v = bitonic_stage_u64<32>(v, lane);
  return bitonic_stage_u64<64>(v, lane);
}
// the 64 smallest of two ascending lists, ascending
__device__ __forceinline__ uint64_t wave_merge_u64(uint64_t a, uint64_t b, uint32_t lane) {
  const uint64_t r = __shfl(b, 63 - (int)lane);
  return bitonic_stage_u64<64>(r < a ? r : a, lane);
}

// one query over `cnt` >= 1 staged points (s_p: xyz triples in LDS; the first has global index t0): returns the updated sorted list
__device__ __forceinline__ uint64_t knn_scan_tile(uint64_t best, const float* s_p, int cnt, int t0, int k, uint32_t lane, float qx, float qy,
                                                  float qz) {
  uint64_t thr = read_lane_u64(best, k - 1);
  for (int j0 = 0; j0 < cnt; j0 += 64) {
    const int j = j0 + (int)lane;
    const bool in = j < cnt;
    const int jr = in ? j : 0;                                       // (cnt >= 1: a valid LDS address for the idle lanes)
    const float d = knn_dist2(qx, qy, qz, s_p[jr * 3], s_p[jr * 3 + 1], s_p[jr * 3 + 2]);
    const uint64_t key = in ? ((uint64_t)__float_as_uint(d) << 32) | (uint32_t)(t0 + j) : KEY_MAX;
    uint64_t todo = __ballot(key < thr);
    if (__popcll(todo) > KNN_MERGE_ABOVE) {                          // (wave-uniform)
      best = wave_merge_u64(best, wave_sort_u64(key, lane), lane);
      thr = read_lane_u64(best, k - 1);
      continue;
    }
    for (int t = 0; t < KNN_MERGE_ABOVE; ++t) {                      // at most one turn per ballot bit
      if (todo == 0) break;
      const int src = __builtin_ctzll(todo);
      todo &= todo - 1;
      const uint64_t x = read_lane_u64(key, src);
      if (x < thr) {                                                 // (wave-uniform; the bar may have dropped since the ballot)
        const uint64_t below = lane_below_u64(best);
        best = best > x ? (below > x ? below : x) : best;
        thr = read_lane_u64(best, k - 1);
      }
    }
  }
  return best;
}

}  // namespace u3d_knn_core
