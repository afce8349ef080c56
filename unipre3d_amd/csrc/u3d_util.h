// Helpers every HIP library of the package used to carry a copy of (internal, like u3d_common.h: not part of any public boundary).
// The host part is plain C++17 (the torch binding includes it under g++); the device part needs hipcc.  Each library keeps its own
// NT / ITEMS / TILE constants -- those are tuning -- and passes what a helper needs of them as a template argument.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define U3D_UTIL_HD __host__ __device__
#else
#include <hip/hip_runtime_api.h>
#define U3D_UTIL_HD
#endif
#include <stddef.h>
#include <stdint.h>

namespace u3d_util {

inline size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }
inline int launched() { return hipGetLastError() == hipSuccess ? 0 : 3; }
U3D_UTIL_HD inline int blocks(long long n, int per) { return (int)((n + per - 1) / per); }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
inline bool bad_ptr(const void* p) { return p == nullptr || !aligned16(p); }      // what an entry point refuses for a required buffer
// steps a lane owns in one 64-lane pass over a row of length L (the selective scan's passes, the causal conv's chunks)
inline int steps_per_lane(int L) { return L <= 64 ? 1 : L <= 128 ? 2 : L <= 192 ? 3 : 4; }

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t lane_id() { return __lane_id(); }

template <int NW>
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t x, uint32_t* wt, uint32_t& all) {   // 64 NW threads, wt: NW words of LDS
  const uint32_t lane = lane_id();
  const int wave = threadIdx.x >> 6;
  uint32_t inc = x;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)inc, o);
    if ((int)lane >= o) inc += u;
  }
  if (lane == 63) wt[wave] = inc;
  __syncthreads();
  uint32_t before = 0;
  all = 0;
  for (int w = 0; w < NW; ++w) { if (w < wave) before += wt[w]; all += wt[w]; }
  __syncthreads();
  return before + inc - x;
}

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_f(float old, float v) {   // lanes without a source (or outside ROW_MASK) keep `old`
  return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
template <int LANE>
__device__ __forceinline__ float lane_f(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), LANE)); }
__device__ __forceinline__ float wave_sum(float v) {              // the sum of the 64 lanes, in one fixed order, in every lane
  v += dpp_f<0x111, 0xf>(0.f, v);   // row_shr:1
  v += dpp_f<0x112, 0xf>(0.f, v);   // row_shr:2
  v += dpp_f<0x114, 0xf>(0.f, v);   // row_shr:4
  v += dpp_f<0x118, 0xf>(0.f, v);   // row_shr:8
  v += dpp_f<0x142, 0xa>(0.f, v);   // row_bcast:15 into rows 1 and 3
  v += dpp_f<0x143, 0xc>(0.f, v);   // row_bcast:31 into rows 2 and 3
  return lane_f<63>(v);
}
__device__ __forceinline__ double wave_sum_f64(double v) {       // one fixed order; the total in every lane
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
// sum of the NT threads' `mine` in a fixed tree, in every thread (sh: NT doubles of LDS)
template <int NT>
__device__ __forceinline__ double block_tree_sum(double mine, double* sh) {
  sh[threadIdx.x] = mine;
  __syncthreads();
  for (int o = NT / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  const double total = sh[0];
  __syncthreads();
  return total;
}
__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }
#endif

}  // namespace u3d_util
