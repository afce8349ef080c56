// Scene-level PointFusion: compaction, FNV grid sampling and the NCHW feature gather on the device; see
// include/unipre3d_pointfusion.h.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include <algorithm>

#include "unipre3d_pointfusion.h"
#include "u3d_keysort.h"

namespace {

using namespace u3d_util;

constexpr int NT = 256;              // threads per workgroup (four waves)
constexpr int NW = NT / 64;
constexpr int ITEMS = 16;            // rounds of NT elements per tile
constexpr int TILE = NT * ITEMS;     // elements per workgroup in the tiled passes
constexpr int SCAN_NT = 1024;        // the one-workgroup exclusive scan

// passes of the 8-bit LSD sort: eight over the 64-bit key, then enough over the set index to order sets (0 for one set)
inline int set_passes(int S) { int q = 0; while (q < 4 && (1ll << (8 * q)) < S) ++q; return q; }
inline int final_buffer(int S) { return (8 + set_passes(S)) & 1; }

struct Scratch {   // carved out of the caller's buffer; every array sized for n_max points
  unsigned long long* keys[2];
  uint32_t* vals[2];
  uint32_t* rank;     // voxel (global rank) of each sorted position
  uint32_t* starts;   // first sorted position of each voxel; starts[M] = n
  uint32_t* hist;     // 256 digit counts per tile (also the tiles' flag counts)
  int32_t* setmax;    // largest voxel count of each set
};

size_t carve(void* base, int n_max, int S, Scratch* s) {
  const size_t n = (size_t)(n_max > 0 ? n_max : 1);
  const size_t nb = (size_t)blocks((long long)n, TILE);
  Carver c{(char*)base};
  Scratch t;
  t.keys[0] = c.take<unsigned long long>(n * 8);
  t.keys[1] = c.take<unsigned long long>(n * 8);
  t.vals[0] = c.take<uint32_t>(n * 4);
  t.vals[1] = c.take<uint32_t>(n * 4);
  t.rank = c.take<uint32_t>(n * 4);
  t.starts = c.take<uint32_t>((n + 1) * 4);
  t.hist = c.take<uint32_t>((nb + 1) * 256 * 4);   // + the 256 digit totals of a radix pass
  t.setmax = c.take<int32_t>((size_t)(S > 0 ? S : 1) * 4);
  if (s) *s = t;
  return c.off;
}

// set of point i: the largest s with off[s] <= i (empty sets are skipped over)
__device__ __forceinline__ int set_of(const int32_t* __restrict__ off, int S, uint32_t i) {
  if (S <= 1) return 0;
  int lo = 0, hi = S - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if ((uint32_t)off[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}
__device__ __forceinline__ uint32_t set_begin(const int32_t* __restrict__ off, int S, int s) { return S <= 1 ? 0u : (uint32_t)off[s]; }

// float <-> int with the same order (atomicMin / atomicMax on the int)
__device__ __forceinline__ int f2o(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
__device__ __forceinline__ float o2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

// numpy's float -> int64 (x86 conversion): exact for every float whose floor fits, |f| < 2^63 (the largest such fp32 is
// 2^63 - 2^39); NaN and everything else give INT64_MIN (so does -2^63 itself, which fits)
__device__ __forceinline__ long long floor_i64(float x) {
  const float f = floorf(x);
  return fabsf(f) < 0x1p63f ? (long long)f : LLONG_MIN;
}

// grid coordinate of one axis exactly as the reference's numpy 1.26 computes it, with a correctly rounded fp32 division:
//   origin 0 (min_coord given):  floor((c - m) / gs), the subtraction in fp32
//   origin 1 (min_coord=None):   floor(c / gs) - floor(m / gs), m the set's own minimum.  The reference subtracts the minimum of
//                                the floors; floor and the division by gs > 0 are monotone, so that is the floor of the minimum.
//                                (the difference wraps as numpy's int64 does)
__device__ __forceinline__ long long grid_axis(int origin, float c, float m, float gs) {
  if (origin == 0) return floor_i64(__fdiv_rn(__fsub_rn(c, m), gs));
  return (long long)((unsigned long long)floor_i64(__fdiv_rn(c, gs)) - (unsigned long long)floor_i64(__fdiv_rn(m, gs)));
}

__device__ __forceinline__ unsigned long long fnv_key(long long g0, long long g1, long long g2) {
  unsigned long long h = 0xcbf29ce484222325ull;
  h *= 0x100000001b3ull; h ^= (unsigned long long)g0;   // multiply, then xor: the reference's loop (not FNV-1a's order)
  h *= 0x100000001b3ull; h ^= (unsigned long long)g1;
  h *= 0x100000001b3ull; h ^= (unsigned long long)g2;
  return h;
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {   // splitmix64 finaliser
  z += 0x9e3779b97f4a7c15ull;
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}

// ---- min / max corner ------------------------------------------------------------------------------------------------------
__global__ void minmax_init_kernel(int S, int* __restrict__ mm) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < 6 * S) mm[t] = (t % 6) < 3 ? INT_MAX : INT_MIN;
}

__global__ __launch_bounds__(NT) void minmax_reduce_kernel(int n, int S, const int32_t* __restrict__ off, const float* __restrict__ coord,
                                                           int* __restrict__ mm) {
  const int s = blockIdx.y;
  const uint32_t b = S <= 1 ? 0u : (uint32_t)off[s], e = S <= 1 ? (uint32_t)n : (uint32_t)off[s + 1];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (uint32_t i = b + blockIdx.x * NT + threadIdx.x; i < e; i += gridDim.x * NT)
    for (int a = 0; a < 3; ++a) {
      const float c = coord[(size_t)i * 3 + a];
      lo[a] = fminf(lo[a], c);
      hi[a] = fmaxf(hi[a], c);
    }
  __shared__ float red[NW][6];
  for (int a = 0; a < 3; ++a)
    for (int o = 32; o > 0; o >>= 1) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], o));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o));
    }
  const int wave = threadIdx.x >> 6;
  if (lane_id() == 0)
    for (int a = 0; a < 3; ++a) { red[wave][a] = lo[a]; red[wave][3 + a] = hi[a]; }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int a = threadIdx.x;
    float v = red[0][a];
    for (int w = 1; w < NW; ++w) v = a < 3 ? fminf(v, red[w][a]) : fmaxf(v, red[w][a]);
    if (b < e) {
      if (a < 3) atomicMin(&mm[s * 6 + a], f2o(v)); else atomicMax(&mm[s * 6 + a], f2o(v));
    }
  }
}

__global__ void minmax_decode_kernel(int S, int* __restrict__ mm) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < 6 * S) reinterpret_cast<float*>(mm)[t] = o2f(mm[t]);
}

// ---- the two uses of the flag ranking (flag_count_kernel -> scan_kernel -> flag_apply_kernel, u3d_keysort.h) -----------------------
struct CompactOp {   // keep pixel i: w != 0 (NaN is valid, as torch's .bool()) and the inclusive box
  const float* uc4; const float* box; float* coord_out; int32_t* src_out;
  __device__ bool flag(uint32_t i) const {
    const float4 u = reinterpret_cast<const float4*>(uc4)[i];
    return u.w != 0.f && u.x >= box[0] && u.x <= box[3] && u.y >= box[1] && u.y <= box[4] && u.z >= box[2] && u.z <= box[5];
  }
  __device__ void emit(uint32_t i, uint32_t r, bool f) const {
    if (!f) return;
    const float4 u = reinterpret_cast<const float4*>(uc4)[i];
    coord_out[(size_t)r * 3 + 0] = u.x; coord_out[(size_t)r * 3 + 1] = u.y; coord_out[(size_t)r * 3 + 2] = u.z;
    src_out[r] = (int32_t)i;
  }
};

struct HeadOp {      // segment heads of the sorted (set, key) sequence; rank = voxel of each sorted position
  const unsigned long long* keys; const uint32_t* vals; const int32_t* off; int S; uint32_t* rank; uint32_t* starts;
  __device__ bool flag(uint32_t i) const {
    return i == 0 || keys[i] != keys[i - 1] || set_of(off, S, vals[i]) != set_of(off, S, vals[i - 1]);
  }
  __device__ void emit(uint32_t i, uint32_t r, bool f) const {
    rank[i] = f ? r : r - 1u;   // r = heads before i: a non-head belongs to the previous head's voxel
    if (f) starts[r] = i;
  }
};

// ---- keys and the stable LSD radix sort of (set, key, index) -------------------------------------------------------------
__global__ __launch_bounds__(NT) void key_kernel(int n_fixed, const int32_t* __restrict__ n_dev, int S, const int32_t* __restrict__ off,
                                                 const float* __restrict__ coord, const float* __restrict__ minc, int ms, int origin,
                                                 float gs, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  const uint32_t n = n_fixed >= 0 ? (uint32_t)n_fixed : (uint32_t)*n_dev;
  const uint32_t i = blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const float* m = minc + (size_t)set_of(off, S, i) * ms;
  const float* c = coord + (size_t)i * 3;
  keys[i] = fnv_key(grid_axis(origin, c[0], m[0], gs), grid_axis(origin, c[1], m[1], gs), grid_axis(origin, c[2], m[2], gs));
  vals[i] = i;
}

__device__ __forceinline__ uint32_t digit_of(int pass, unsigned long long k, uint32_t v, const int32_t* off, int S) {
  return pass < 8 ? (uint32_t)(k >> (8 * pass)) & 255u : ((uint32_t)set_of(off, S, v) >> (8 * (pass - 8))) & 255u;
}

__global__ __launch_bounds__(NT) void radix_hist_kernel(int pass, const int32_t* __restrict__ n_dev, int nb, const int32_t* __restrict__ off,
                                                        int S, const unsigned long long* __restrict__ kin, const uint32_t* __restrict__ vin,
                                                        uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  const uint32_t n = (uint32_t)*n_dev;
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * (uint32_t)TILE;
  for (int r = 0; r < ITEMS; ++r) {
    const uint32_t i = base + r * NT + threadIdx.x;
    if (i < n) atomicAdd(&h[digit_of(pass, kin[i], vin[i], off, S)], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];   // digit-major: one exclusive scan gives every (digit, tile) its base
}

// Stable scatter of one tile: rounds of NT elements ranked with the ballot multi-split (element order = round, wave, lane);
// the per-wave digit counts become destinations through one prefix over the waves (the block radix sort of u3d_sort.hip, over HBM).
__global__ __launch_bounds__(NT) void radix_scatter_kernel(int pass, const int32_t* __restrict__ n_dev, int nb,
                                                           const int32_t* __restrict__ off, int S, const uint32_t* __restrict__ hist,
                                                           const unsigned long long* __restrict__ kin, const uint32_t* __restrict__ vin,
                                                           unsigned long long* __restrict__ kout, uint32_t* __restrict__ vout) {
  __shared__ RadixLds<NW> lds;
  const uint32_t n = (uint32_t)*n_dev;
  const uint32_t base = blockIdx.x * (uint32_t)TILE;
  if (base >= n) return;
  radix_bases<NW>(lds, hist, hist + (size_t)nb * 256, nb);
  for (int r = 0; r < ITEMS; ++r) {
    radix_round_begin<NW>(lds);
    const uint32_t i = base + r * NT + threadIdx.x;
    const bool valid = i < n;
    unsigned long long k = 0; uint32_t v = 0, digit = 0;
    if (valid) { k = kin[i]; v = vin[i]; digit = digit_of(pass, k, v, off, S); }
    const uint32_t dst = radix_round_dst<NW>(lds, valid, digit);
    if (valid) {
      kout[dst] = k;
      vout[dst] = v;
    }
    __syncthreads();
  }
}

// ---- voxels ------------------------------------------------------------------------------------------------------------------
__global__ void setup_kernel(int n_fixed, int32_t* __restrict__ meta, int S, int32_t* __restrict__ setmax) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) {
    if (n_fixed >= 0) meta[0] = n_fixed;
    meta[1] = 0; meta[2] = 0; meta[3] = 0;
  }
  if (t < S) setmax[t] = 0;
}

// starts[M] = n; voxel_offsets[s] = voxel of the first point of set s (M past the last point)
__global__ void finish_kernel(const int32_t* __restrict__ meta, int S, const int32_t* __restrict__ off, const uint32_t* __restrict__ rank,
                              uint32_t* __restrict__ starts, int32_t* __restrict__ voxel_off) {
  const int n = meta[0], M = meta[1];
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) starts[M] = (uint32_t)n;
  if (t <= S) {
    const int b = t == S ? n : (int)set_begin(off, S, t);
    voxel_off[t] = b < n ? (int)rank[b] : M;
  }
}

__global__ __launch_bounds__(NT) void count_max_kernel(int32_t* __restrict__ meta, int S, const int32_t* __restrict__ off,
                                                       const uint32_t* __restrict__ starts, const uint32_t* __restrict__ vals,
                                                       int32_t* __restrict__ setmax) {
  const int M = meta[1];
  const int v = blockIdx.x * NT + threadIdx.x;
  const bool valid = v < M;
  int c = 0, s = 0;
  if (valid) { c = (int)(starts[v + 1] - starts[v]); s = set_of(off, S, vals[starts[v]]); }
  // one atomic per wave when the wave's voxels share a set (nearly always), per lane otherwise
  const int s0 = __shfl(s, 0);
  const unsigned long long act = __ballot(valid);
  const bool uniform = __ballot(valid && s != s0) == 0ull;
  if (uniform) {
    int m = c;
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
    if (lane_id() == 0 && act) { atomicMax(&setmax[s0], m); atomicMax(&meta[2], m); }
  } else if (valid) {
    atomicMax(&setmax[s], c);
    atomicMax(&meta[2], c);
  }
}

__global__ __launch_bounds__(NT) void pick_kernel(int M, int S, const int32_t* __restrict__ off, const int32_t* __restrict__ voxel_off,
                                                  const float* __restrict__ coord, const float* __restrict__ minc, int ms, int origin,
                                                  float gs, int mode, int part, const int64_t* __restrict__ draws, unsigned long long seed,
                                                  const int32_t* __restrict__ src_map, const uint32_t* __restrict__ starts,
                                                  const uint32_t* __restrict__ vals, const int32_t* __restrict__ setmax,
                                                  int64_t* __restrict__ out_index, float* __restrict__ out_coord,
                                                  int64_t* __restrict__ out_grid, int32_t* __restrict__ out_src) {
  const int v = blockIdx.x * NT + threadIdx.x;
  if (v >= M) return;
  const uint32_t st = starts[v], cnt = starts[v + 1] - st;
  const int s = set_of(off, S, vals[st]);
  unsigned long long r;
  if (mode == 1) r = (unsigned long long)(unsigned)part;
  else if (draws) r = (unsigned long long)draws[v];   // the reference's randint(0, count.max()) draw, replayed
  else r = mix64(seed ^ mix64((unsigned long long)(v - voxel_off[s]))) % (unsigned long long)max(setmax[s], 1);
  const uint32_t idx = vals[st + (uint32_t)(r % cnt)];
  out_index[v] = (int64_t)(idx - set_begin(off, S, s));
  const float* c = coord + (size_t)idx * 3;
  const float* m = minc + (size_t)s * ms;
  for (int a = 0; a < 3; ++a) {
    out_coord[(size_t)v * 3 + a] = c[a];
    out_grid[(size_t)v * 3 + a] = grid_axis(origin, c[a], m[a], gs);
  }
  if (out_src) out_src[v] = src_map ? src_map[idx] : (int32_t)idx;
}

__global__ __launch_bounds__(NT) void inverse_kernel(int n, int S, const int32_t* __restrict__ off, const int32_t* __restrict__ voxel_off,
                                                     const uint32_t* __restrict__ vals, const uint32_t* __restrict__ rank,
                                                     int64_t* __restrict__ inverse) {
  const uint32_t i = blockIdx.x * NT + threadIdx.x;
  if (i >= (uint32_t)n) return;
  const uint32_t p = vals[i];
  const int s = set_of(off, S, p);
  inverse[p] = (int64_t)rank[i] - voxel_off[s];
}

// ---- features --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void gather_fwd_kernel(int M, int C, int HW, const float* __restrict__ feat, const int32_t* __restrict__ src,
                                                        float* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * NT + threadIdx.x;
  if (e >= (size_t)M * C) return;
  const int v = (int)(e / C), c = (int)(e - (size_t)v * C);
  const int p = src[v];
  const int view = p / HW, hw = p - view * HW;
  out[e] = feat[((size_t)view * C + c) * HW + hw];
}

__global__ __launch_bounds__(NT) void pixel_map_kernel(int M, const int32_t* __restrict__ src, int32_t* __restrict__ map) {
  const int v = blockIdx.x * NT + threadIdx.x;
  if (v < M) map[src[v]] = v;   // a voxel picks one point and a point lies in one voxel: each pixel is named at most once
}

// gather form: workgroups walk (view, channel) planes; every gradient element is written once
__global__ __launch_bounds__(NT) void gather_bwd_kernel(int V, int C, int HW, const float* __restrict__ g, const int32_t* __restrict__ map,
                                                        float* __restrict__ grad) {
  const int planes = V * C;
  for (int pl = blockIdx.y; pl < planes; pl += gridDim.y) {
    const int view = pl / C, c = pl - view * C;
    const int32_t* mp = map + (size_t)view * HW;
    float* o = grad + (size_t)pl * HW;
    for (int hw = blockIdx.x * NT + threadIdx.x; hw < HW; hw += gridDim.x * NT) {
      const int m = mp[hw];
      o[hw] = m >= 0 ? g[(size_t)m * C + c] : 0.f;
    }
  }
}

}  // namespace

extern "C" {

int u3d_pointfusion_abi_version(void) { return U3D_POINTFUSION_ABI_VERSION; }

size_t u3d_pointfusion_scratch_bytes(int n_max, int n_sets) {
  if (n_max < 0 || n_sets < 1) return 0;
  return carve(nullptr, n_max, n_sets, nullptr);
}

int u3d_pointfusion_minmax(int n, int n_sets, const int32_t* set_offsets, const float* coord, float* minmax, void* stream) {
  if (n < 0 || n_sets < 1 || !minmax || (n > 0 && !coord) || (n_sets > 1 && !set_offsets)) return 1;
  if (n_sets > 65535) return 2;
  hipStream_t st = (hipStream_t)stream;
  int* mm = reinterpret_cast<int*>(minmax);
  minmax_init_kernel<<<blocks(6ll * n_sets, NT), NT, 0, st>>>(n_sets, mm);
  if (n > 0) {
    const int gx = n_sets > 1 ? 64 : std::min(blocks(n, NT * 8), 1024);
    minmax_reduce_kernel<<<dim3(std::max(gx, 1), n_sets), NT, 0, st>>>(n, n_sets, set_offsets, coord, mm);
  }
  minmax_decode_kernel<<<blocks(6ll * n_sets, NT), NT, 0, st>>>(n_sets, mm);
  return launched();
}

int u3d_pointfusion_compact(int P, const float* uc4, const float* box, float* coord_out, int32_t* src_out, int32_t* meta, void* scratch,
                            void* stream) {
  if (P < 0 || !meta || !scratch || (P > 0 && (!uc4 || !box || !coord_out || !src_out))) return 1;
  hipStream_t st = (hipStream_t)stream;
  Scratch s;
  carve(scratch, P, 1, &s);
  if (P == 0) {
    (void)hipMemsetAsync(meta, 0, 4 * sizeof(int32_t), st);
    return launched();
  }
  const int nb = blocks(P, TILE);
  CompactOp op{uc4, box, coord_out, src_out};
  flag_count_kernel<NT, ITEMS, CompactOp><<<nb, NT, 0, st>>>(op, P, nullptr, s.hist);
  scan_kernel<SCAN_NT><<<1, SCAN_NT, 0, st>>>(nb, s.hist, meta);
  flag_apply_kernel<NT, ITEMS, CompactOp><<<nb, NT, 0, st>>>(op, P, nullptr, s.hist);
  return launched();
}

int u3d_pointfusion_voxelize(int n_max, int n, int n_sets, const int32_t* set_offsets, const float* coord, const float* min_coord,
                             int min_stride, int origin, float grid_size, int32_t* meta, int32_t* voxel_offsets, void* scratch,
                             void* stream) {
  if (origin != 0 && origin != 1) return 1;
  if (n_max < 0 || n > n_max || n_sets < 1 || !meta || !voxel_offsets || !scratch || (n_sets > 1 && !set_offsets)) return 1;
  if (n_max > 0 && (!coord || !min_coord || min_stride < 3)) return 1;
  if (!(grid_size > 0.f)) return 1;
  hipStream_t st = (hipStream_t)stream;
  Scratch s;
  carve(scratch, n_max, n_sets, &s);
  setup_kernel<<<blocks(n_sets + 1, NT), NT, 0, st>>>(n, meta, n_sets, s.setmax);
  if (n_max > 0) {
    const int nb = blocks(n_max, TILE);
    key_kernel<<<blocks(n_max, NT), NT, 0, st>>>(-1, meta, n_sets, set_offsets, coord, min_coord, min_stride, origin, grid_size, s.keys[0],
                                                        s.vals[0]);
    const int passes = 8 + set_passes(n_sets);
    for (int p = 0; p < passes; ++p) {
      const int a = p & 1;
      radix_hist_kernel<<<nb, NT, 0, st>>>(p, meta, nb, set_offsets, n_sets, s.keys[a], s.vals[a], s.hist);
      digit_scan_kernel<NT><<<256, NT, 0, st>>>(nb, s.hist);
      radix_scatter_kernel<<<nb, NT, 0, st>>>(p, meta, nb, set_offsets, n_sets, s.hist, s.keys[a], s.vals[a], s.keys[a ^ 1], s.vals[a ^ 1]);
    }
    const int fb = final_buffer(n_sets);
    HeadOp op{s.keys[fb], s.vals[fb], set_offsets, n_sets, s.rank, s.starts};
    flag_count_kernel<NT, ITEMS, HeadOp><<<nb, NT, 0, st>>>(op, -1, meta, s.hist);
    scan_kernel<SCAN_NT><<<1, SCAN_NT, 0, st>>>(nb, s.hist, meta + 1);
    flag_apply_kernel<NT, ITEMS, HeadOp><<<nb, NT, 0, st>>>(op, -1, meta, s.hist);
    finish_kernel<<<blocks(n_sets + 1, NT), NT, 0, st>>>(meta, n_sets, set_offsets, s.rank, s.starts, voxel_offsets);
    count_max_kernel<<<blocks(n_max, NT), NT, 0, st>>>(meta, n_sets, set_offsets, s.starts, s.vals[fb], s.setmax);
  } else {
    (void)hipMemsetAsync(voxel_offsets, 0, (size_t)(n_sets + 1) * sizeof(int32_t), st);
  }
  return launched();
}

int u3d_pointfusion_pick(int M, int n_max, int n_sets, const int32_t* set_offsets, const int32_t* voxel_offsets, const float* coord,
                         const float* min_coord, int min_stride, int origin, float grid_size, int mode, int part, const int64_t* draws,
                         uint64_t seed, const int32_t* src_map, int64_t* out_index, float* out_coord, int64_t* out_grid, int32_t* out_src,
                         const void* scratch, void* stream) {
  if (origin != 0 && origin != 1) return 1;
  if (M < 0 || M > n_max || n_sets < 1 || (mode != 0 && mode != 1) || part < 0 || (n_sets > 1 && !set_offsets)) return 1;
  if (M == 0) return 0;
  if (!voxel_offsets || !coord || !min_coord || min_stride < 3 || !out_index || !out_coord || !out_grid || !scratch) return 1;
  Scratch s;
  carve(const_cast<void*>(scratch), n_max, n_sets, &s);
  const int fb = final_buffer(n_sets);
  pick_kernel<<<blocks(M, NT), NT, 0, (hipStream_t)stream>>>(M, n_sets, set_offsets, voxel_offsets, coord, min_coord, min_stride, origin,
                                                             grid_size, mode, part, draws, (unsigned long long)seed, src_map, s.starts, s.vals[fb],
                                                             s.setmax, out_index, out_coord, out_grid, out_src);
  return launched();
}

int u3d_pointfusion_inverse(int n, int n_max, int n_sets, const int32_t* set_offsets, const int32_t* voxel_offsets, int64_t* inverse,
                            const void* scratch, void* stream) {
  if (n < 0 || n > n_max || n_sets < 1 || (n_sets > 1 && !set_offsets)) return 1;
  if (n == 0) return 0;
  if (!voxel_offsets || !inverse || !scratch) return 1;
  Scratch s;
  carve(const_cast<void*>(scratch), n_max, n_sets, &s);
  inverse_kernel<<<blocks(n, NT), NT, 0, (hipStream_t)stream>>>(n, n_sets, set_offsets, voxel_offsets, s.vals[final_buffer(n_sets)], s.rank,
                                                                inverse);
  return launched();
}

int u3d_pointfusion_gather_forward(int M, int C, int HW, const float* feat, const int32_t* src, float* out, void* stream) {
  if (M < 0 || C < 0 || HW < 0) return 1;
  if ((long long)M * C == 0) return 0;
  if (!feat || !src || !out) return 1;
  gather_fwd_kernel<<<blocks((long long)M * C, NT), NT, 0, (hipStream_t)stream>>>(M, C, HW, feat, src, out);
  return launched();
}

int u3d_pointfusion_gather_backward(int V, int C, int HW, int M, const float* grad_out, const int32_t* src, int32_t* pixel_map,
                                    float* grad_feat, void* stream) {
  if (V < 0 || C < 0 || HW < 0 || M < 0 || (long long)V * HW >= (1ll << 31)) return 1;
  if ((long long)V * C * HW == 0) return 0;
  if (!pixel_map || !grad_feat || (M > 0 && (!grad_out || !src))) return 1;
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(pixel_map, 0xff, (size_t)V * HW * sizeof(int32_t), st);   // -1: no voxel picked the pixel
  if (M > 0) pixel_map_kernel<<<blocks(M, NT), NT, 0, st>>>(M, src, pixel_map);
  const int gx = std::min(blocks(HW, NT), 64);
  gather_bwd_kernel<<<dim3(gx, std::min(V * C, 65535)), NT, 0, st>>>(V, C, HW, grad_out, pixel_map, grad_feat);
  return launched();
}

}  // extern "C"
