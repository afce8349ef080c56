// Offset-batched ("ragged") point operators for gfx950 (include/unipre3d_offsetops.h); semantics restated on the CPU in
// tests/offsetops_ref.py.  Clouds are concatenated, (n,3) with the cumulative ends of the b clouds in `offset`.
//
// kNN.  The launch shape of u3d_knn: sixteen waves, one query each, the support staged through LDS in tiles of KNN_TILE points, and
// the selection of u3d_knn_core.h.  What is new is the range: every wave finds its query's segment (a linear walk of new_offset
// with scalar loads: b is a batch size) and its support range [start, end); the workgroup stages the UNION of its waves' ranges, and
// each wave hands knn_scan_tile the part of the staged tile inside its own range.  A workgroup whose sixteen queries share a
// segment stages exactly that segment; one that straddles a boundary stages both segments and each wave skips the other's tiles.
// The selection does not depend on arrival order (u3d_knn_core.h), so the answer is the one of a per-segment dense search.
//
// Ball query.  One wave per query walks its range 64 points per step straight from global memory; a ballot and the popcount of the
// lower lanes rank the step's hits in index order, and the walk ends once nsample hits are found.
//
// Index-addressed operators.  Lanes run along c.  Outputs with ONE owner per element (gathers, the interpolation and aggregation
// sums, grad_in1, grad_position, grad_weight) are computed in registers and stored once, 16 bytes per lane where c % 4 == 0 and
// the pointers allow it, one float per lane otherwise.  Outputs addressed through idx (grad_in of group, grad_input of interpolate
// and aggregate, grad_in2) are zero-filled and summed with atomicAdd(float*) -- global_atomic_add_f32 under -munsafe-fp-atomics --
// one float per lane, consecutive lanes on consecutive channels, so that a wave-instruction adds contiguous bytes of a row.
// An index outside its tensor is never used as an address: see the header for what each operator does instead.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <initializer_list>

#include "unipre3d_knn.h"
#include "unipre3d_offsetops.h"
#include "u3d_util.h"
#include "u3d_knn_core.h"

namespace {

using namespace u3d_util;
using namespace u3d_knn_core;

constexpr int KNN_Q = U3D_KNN_QUERIES;                               // queries per workgroup: one per wave
constexpr int KNN_THREADS = 64 * KNN_Q;
constexpr int KNN_TILE = U3D_KNN_TILE;
constexpr int MAX_K = U3D_KNN_MAX_K;
constexpr int BQ_WAVES = 4;                                          // ball query: queries (waves) per workgroup
constexpr int NT = 256;                                              // the elementwise kernels' workgroup
constexpr float FILL_D2 = 1e10f;
constexpr long long MAX_BLOCKS = 2147483647ll;
constexpr int MAX_N = 2147483647 - KNN_TILE;                         // the searches step a 32-bit row counter by up to one tile past n

// the support range of query row qi (wave-uniform): clamped to [0, n], empty as start == end
__device__ __forceinline__ void segment_range(int qi, int b, int n, const int32_t* __restrict__ offset, const int32_t* __restrict__ new_offset,
                                              int& start, int& end) {
  int s = 0;
  while (s < b && qi >= new_offset[s]) ++s;
  start = end = 0;
  if (s < b) {
    start = s == 0 ? 0 : offset[s - 1];
    end = offset[s];
    start = min(max(start, 0), n);
    end = min(max(end, 0), n);
    if (end < start) end = start;
  }
}

__global__ __launch_bounds__(KNN_THREADS) void offset_knn_kernel(int b, int n, int m, int k, const float* __restrict__ xyz,
                                                                 const float* __restrict__ new_xyz, const int32_t* __restrict__ offset,
                                                                 const int32_t* __restrict__ new_offset, float* __restrict__ dist2,
                                                                 int32_t* __restrict__ idx) {
  __shared__ float s_p[KNN_TILE * 3];
  __shared__ int s_rng[2 * KNN_Q];
  const uint32_t lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long qi = (long long)blockIdx.x * KNN_Q + wave;         // this wave's query, if below m (wave-uniform)
  const bool live = qi < m;
  int start = 0, end = 0;
  if (live) segment_range((int)qi, b, n, offset, new_offset, start, end);
  if (lane == 0) { s_rng[2 * wave] = start; s_rng[2 * wave + 1] = end; }
  const float* q = new_xyz + (size_t)(live ? qi : 0) * 3;
  const float qx = q[0], qy = q[1], qz = q[2];
  __syncthreads();
  int lo = n, hi = 0;                                                // the union of the non-empty ranges (block-uniform)
  for (int w = 0; w < KNN_Q; ++w) {
    const int a = s_rng[2 * w], e = s_rng[2 * w + 1];
    if (a < e) { lo = min(lo, a); hi = max(hi, e); }
  }
  uint64_t best = KEY_MAX;
  for (int t0 = lo; t0 < hi; t0 += KNN_TILE) {                       // 0 <= lo, hi <= n: the staging reads stay inside xyz
    const int cnt = min(KNN_TILE, hi - t0);
    __syncthreads();
    for (int e = threadIdx.x; e < cnt * 3; e += KNN_THREADS) s_p[e] = xyz[(size_t)t0 * 3 + e];
    __syncthreads();
    const int a = max(start, t0), z = min(end, t0 + cnt);            // this wave's part of the tile
    if (a < z) best = knn_scan_tile(best, s_p + (a - t0) * 3, z - a, a, k, lane, qx, qy, qz);   // (no barrier inside)
  }
  if (live && (int)lane < k) {
    const size_t o = (size_t)qi * k + lane;
    const bool found = best != KEY_MAX;
    idx[o] = found ? (int32_t)(uint32_t)best : (start < end ? start : -1);
    if (dist2) dist2[o] = found ? __uint_as_float((uint32_t)(best >> 32)) : FILL_D2;
  }
}

__global__ __launch_bounds__(64 * BQ_WAVES) void offset_ballquery_kernel(int b, int n, int m, float r2, int nsample,
                                                                         const float* __restrict__ xyz, const float* __restrict__ new_xyz,
                                                                         const int32_t* __restrict__ offset,
                                                                         const int32_t* __restrict__ new_offset, int32_t* __restrict__ idx) {
  const uint32_t lane = lane_id();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long qi = (long long)blockIdx.x * BQ_WAVES + wave;
  if (qi >= m) return;                                               // (wave-uniform; the kernel has no barrier)
  int start, end;
  segment_range((int)qi, b, n, offset, new_offset, start, end);
  const float qx = new_xyz[(size_t)qi * 3], qy = new_xyz[(size_t)qi * 3 + 1], qz = new_xyz[(size_t)qi * 3 + 2];
  int32_t* out = idx + (size_t)qi * nsample;
  int cnt = 0, first = 0;
  for (int j0 = start; j0 < end && cnt < nsample; j0 += 64) {
    const int j = j0 + (int)lane;                                    // (n <= MAX_N: no wrap)
    const bool in = j < end;
    const size_t jr = (size_t)(in ? j : start) * 3;                  // (start < end here: a valid row for the idle lanes)
    const bool hit = in && knn_dist2(qx, qy, qz, xyz[jr], xyz[jr + 1], xyz[jr + 2]) < r2;
    const uint64_t hits = __ballot(hit);
    if (hits == 0) continue;
    if (cnt == 0) first = j0 + __builtin_ctzll(hits);
    const int rank = cnt + __popcll(hits & ((1ull << lane) - 1));
    if (hit && rank < nsample) out[rank] = j;
    cnt += __popcll(hits);
  }
  if ((int)lane >= cnt && (int)lane < nsample) out[lane] = first;    // nsample <= 64: one lane per slot; no hit: 0
}

// ---- index-addressed operators: V floats per lane along c (4: 16-byte accesses; 1: any c, any alignment)
template <int V> struct Vec;
template <> struct Vec<4> { typedef float4 T; };
template <> struct Vec<1> { typedef float T; };
template <int V> __device__ __forceinline__ void ld(const float* p, float (&r)[V]) {
  const typename Vec<V>::T v = *reinterpret_cast<const typename Vec<V>::T*>(p);
  __builtin_memcpy(r, &v, sizeof(v));
}
template <int V> __device__ __forceinline__ void st(float* p, const float (&r)[V]) {
  typename Vec<V>::T v;
  __builtin_memcpy(&v, r, sizeof(v));
  *reinterpret_cast<typename Vec<V>::T*>(p) = v;
}
__device__ __forceinline__ bool inside(int32_t i, int rows) { return (uint32_t)i < (uint32_t)rows; }
__device__ __forceinline__ long long flat_id() { return (long long)blockIdx.x * NT + threadIdx.x; }

// out[r, :] = input[idx[r], :] (0 where idx[r] is outside) -- rows = m * nsample
template <int V>
__global__ __launch_bounds__(NT) void group_fwd_kernel(long long rows, int c, int n, const float* __restrict__ input,
                                                       const int32_t* __restrict__ idx, float* __restrict__ out) {
  const int cv = c / V;
  const long long t = flat_id();
  if (t >= rows * cv) return;
  const long long r = t / cv;
  const int col = (int)(t - r * cv) * V;
  const int32_t id = idx[r];
  float v[V] = {};
  if (inside(id, n)) ld<V>(input + (size_t)id * c + col, v);
  st<V>(out + (size_t)r * c + col, v);
}

// dst[idx[r], ch] += sign * src[r, ch] -- one float per lane
__global__ __launch_bounds__(NT) void scatter_add_kernel(long long rows, int c, int n, float sign, const float* __restrict__ src,
                                                         const int32_t* __restrict__ idx, float* __restrict__ dst) {
  const long long t = flat_id();
  if (t >= rows * c) return;
  const long long r = t / c;
  const int ch = (int)(t - r * c);
  const int32_t id = idx[r];
  if (inside(id, n)) atomicAdd(dst + (size_t)id * c + ch, sign * src[t]);
}

template <int V>
__global__ __launch_bounds__(NT) void interp_fwd_kernel(int n_out, int c, int k, int m_in, const float* __restrict__ input,
                                                        const int32_t* __restrict__ idx, const float* __restrict__ weight,
                                                        float* __restrict__ out) {
  const int cv = c / V;
  const long long t = flat_id();
  if (t >= (long long)n_out * cv) return;
  const long long i = t / cv;
  const int col = (int)(t - i * cv) * V;
  float acc[V] = {};
  for (int j = 0; j < k; ++j) {
    const int32_t id = idx[i * k + j];
    if (!inside(id, m_in)) continue;
    const float w = weight[i * k + j];
    float v[V];
    ld<V>(input + (size_t)id * c + col, v);
#pragma unroll
    for (int u = 0; u < V; ++u) acc[u] += v[u] * w;
  }
  st<V>(out + (size_t)i * c + col, acc);
}

// grad_input[idx[i,j], ch] += grad_out[i, ch] * weight[i,j]
__global__ __launch_bounds__(NT) void interp_bwd_kernel(long long rows, int c, int k, int m_in, const float* __restrict__ grad_out,
                                                        const int32_t* __restrict__ idx, const float* __restrict__ weight,
                                                        float* __restrict__ grad_input) {
  const long long t = flat_id();
  if (t >= rows * c) return;
  const long long r = t / c;                                         // r = i * k + j
  const int ch = (int)(t - r * c);
  const int32_t id = idx[r];
  if (inside(id, m_in)) atomicAdd(grad_input + (size_t)id * c + ch, grad_out[(size_t)(r / k) * c + ch] * weight[r]);
}

template <int V>
__global__ __launch_bounds__(NT) void subtract_fwd_kernel(long long rows, int nsample, int c, int n, const float* __restrict__ in1,
                                                          const float* __restrict__ in2, const int32_t* __restrict__ idx,
                                                          float* __restrict__ out) {
  const int cv = c / V;
  const long long t = flat_id();
  if (t >= rows * cv) return;
  const long long r = t / cv;                                        // r = i * nsample + s
  const int col = (int)(t - r * cv) * V;
  const int32_t id = idx[r];
  float a[V], v[V] = {};
  ld<V>(in1 + (size_t)(r / nsample) * c + col, a);
  if (inside(id, n)) ld<V>(in2 + (size_t)id * c + col, v);
#pragma unroll
  for (int u = 0; u < V; ++u) a[u] -= v[u];
  st<V>(out + (size_t)r * c + col, a);
}

// grad_in1[i, ch] = sum_s grad_out[i, s, ch] in registers; grad_in2[idx[i,s], ch] -= grad_out[i, s, ch]
__global__ __launch_bounds__(NT) void subtract_bwd_kernel(int n, int nsample, int c, const int32_t* __restrict__ idx,
                                                          const float* __restrict__ grad_out, float* __restrict__ grad_in1,
                                                          float* __restrict__ grad_in2) {
  const long long t = flat_id();
  if (t >= (long long)n * c) return;
  const long long i = t / c;
  const int ch = (int)(t - i * c);
  float acc = 0.f;
  for (int s = 0; s < nsample; ++s) {
    const float g = grad_out[((size_t)i * nsample + s) * c + ch];
    acc += g;
    const int32_t id = idx[i * nsample + s];
    if (inside(id, n)) atomicAdd(grad_in2 + (size_t)id * c + ch, -g);
  }
  grad_in1[t] = acc;
}

template <int V>
__global__ __launch_bounds__(NT) void aggregate_fwd_kernel(int n, int nsample, int c, int w_c, const float* __restrict__ input,
                                                           const float* __restrict__ position, const float* __restrict__ weight,
                                                           const int32_t* __restrict__ idx, float* __restrict__ out) {
  const int cv = c / V;
  const long long t = flat_id();
  if (t >= (long long)n * cv) return;
  const long long i = t / cv;
  const int col = (int)(t - i * cv) * V;
  int wc[V];
#pragma unroll
  for (int u = 0; u < V; ++u) wc[u] = (col + u) % w_c;
  float acc[V] = {};
  for (int s = 0; s < nsample; ++s) {
    const size_t r = (size_t)i * nsample + s;
    const int32_t id = idx[r];
    if (!inside(id, n)) continue;
    float v[V], p[V];
    ld<V>(input + (size_t)id * c + col, v);
    ld<V>(position + r * c + col, p);
#pragma unroll
    for (int u = 0; u < V; ++u) acc[u] += (v[u] + p[u]) * weight[r * w_c + wc[u]];
  }
  st<V>(out + (size_t)i * c + col, acc);
}

// grad_position[i,s,ch] = g[i,ch] * w[i,s,ch % w_c]; grad_input[idx[i,s], ch] += the same
__global__ __launch_bounds__(NT) void aggregate_bwd_kernel(long long rows, int nsample, int c, int w_c, int n,
                                                           const float* __restrict__ weight, const int32_t* __restrict__ idx,
                                                           const float* __restrict__ grad_out, float* __restrict__ grad_input,
                                                           float* __restrict__ grad_position) {
  const long long t = flat_id();
  if (t >= rows * c) return;
  const long long r = t / c;                                         // r = i * nsample + s
  const int ch = (int)(t - r * c);
  const int32_t id = idx[r];
  float gw = 0.f;
  if (inside(id, n)) {
    gw = grad_out[(size_t)(r / nsample) * c + ch] * weight[(size_t)r * w_c + ch % w_c];
    atomicAdd(grad_input + (size_t)id * c + ch, gw);
  }
  grad_position[t] = gw;
}

// grad_weight[i,s,wc] = sum over ch = wc, wc + w_c, ... of g[i,ch] * (input[idx[i,s],ch] + position[i,s,ch])
__global__ __launch_bounds__(NT) void aggregate_bwd_weight_kernel(long long rows, int nsample, int c, int w_c, int n,
                                                                  const float* __restrict__ input, const float* __restrict__ position,
                                                                  const int32_t* __restrict__ idx, const float* __restrict__ grad_out,
                                                                  float* __restrict__ grad_weight) {
  const long long t = flat_id();
  if (t >= rows * w_c) return;
  const long long r = t / w_c;
  const int wc = (int)(t - r * w_c);
  const int32_t id = idx[r];
  float acc = 0.f;
  if (inside(id, n)) {
    const float* g = grad_out + (size_t)(r / nsample) * c;
    const float* v = input + (size_t)id * c;
    const float* p = position + (size_t)r * c;
    for (int ch = wc; ch < c; ch += w_c) acc += g[ch] * (v[ch] + p[ch]);
  }
  grad_weight[t] = acc;
}

// ---- host side
inline bool grid_for(long long work, unsigned& grid) {               // work >= 1 threads in workgroups of NT
  const long long g = (work + NT - 1) / NT;
  grid = (unsigned)g;
  return g <= MAX_BLOCKS;
}
inline bool vec4(int c, std::initializer_list<const void*> ptrs) {
  if (c % 4 != 0) return false;
  for (const void* p : ptrs) if (!aligned16(p)) return false;
  return true;
}
inline bool zero_fill(float* p, long long count, hipStream_t st) {
  return hipMemsetAsync(p, 0, (size_t)count * sizeof(float), st) == hipSuccess;
}

}  // namespace

extern "C" {

int u3d_offset_knn(int b, int n, int m, int k, const float* xyz, const float* new_xyz, const int32_t* offset, const int32_t* new_offset,
                   float* dist2, int32_t* idx, void* stream) {
  if (b < 0 || n < 0 || m < 0 || k < 1 || k > MAX_K || n > MAX_N) return 1;
  if (b == 0 || m == 0) return 0;
  if (!new_xyz || !offset || !new_offset || !idx || (n > 0 && !xyz)) return 1;
  const long long qblocks = ((long long)m + KNN_Q - 1) / KNN_Q;
  hipLaunchKernelGGL(offset_knn_kernel, dim3((unsigned)qblocks), dim3(KNN_THREADS), 0, (hipStream_t)stream, b, n, m, k, xyz, new_xyz, offset,
                     new_offset, dist2, idx);
  return launched();
}

int u3d_offset_ballquery(int b, int n, int m, float radius, int nsample, const float* xyz, const float* new_xyz, const int32_t* offset,
                         const int32_t* new_offset, int32_t* idx, void* stream) {
  if (b < 0 || n < 0 || m < 0 || nsample < 1 || nsample > MAX_K || n > MAX_N) return 1;
  if (b == 0 || m == 0) return 0;
  if (!new_xyz || !offset || !new_offset || !idx || (n > 0 && !xyz)) return 1;
  const long long blocks = ((long long)m + BQ_WAVES - 1) / BQ_WAVES;
  hipLaunchKernelGGL(offset_ballquery_kernel, dim3((unsigned)blocks), dim3(64 * BQ_WAVES), 0, (hipStream_t)stream, b, n, m, radius * radius,
                     nsample, xyz, new_xyz, offset, new_offset, idx);
  return launched();
}

int u3d_offset_group_forward(int m, int nsample, int c, int n, const float* input, const int32_t* idx, float* out, void* stream) {
  if (m < 0 || nsample < 0 || c < 0 || n < 0) return 1;
  const long long rows = (long long)m * nsample;
  if (rows == 0 || c == 0) return 0;
  if (!idx || !out || (n > 0 && !input)) return 1;
  const bool v4 = vec4(c, {input, out});
  unsigned grid;
  if (!grid_for(rows * (v4 ? c / 4 : c), grid)) return 1;
  if (v4) hipLaunchKernelGGL(group_fwd_kernel<4>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, rows, c, n, input, idx, out);
  else hipLaunchKernelGGL(group_fwd_kernel<1>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, rows, c, n, input, idx, out);
  return launched();
}

int u3d_offset_group_backward(int m, int nsample, int c, int n, const float* grad_out, const int32_t* idx, float* grad_in, void* stream) {
  if (m < 0 || nsample < 0 || c < 0 || n < 0) return 1;
  const long long rows = (long long)m * nsample;
  if (rows == 0 || c == 0 || n == 0) return 0;
  if (!grad_out || !idx || !grad_in) return 1;
  unsigned grid;
  if (!grid_for(rows * c, grid)) return 1;
  if (!zero_fill(grad_in, (long long)n * c, (hipStream_t)stream)) return 3;
  hipLaunchKernelGGL(scatter_add_kernel, dim3(grid), dim3(NT), 0, (hipStream_t)stream, rows, c, n, 1.f, grad_out, idx, grad_in);
  return launched();
}

int u3d_offset_interpolate_forward(int n_out, int c, int k, int m_in, const float* input, const int32_t* idx, const float* weight,
                                   float* out, void* stream) {
  if (n_out < 0 || c < 0 || k < 0 || m_in < 0) return 1;
  if (n_out == 0 || c == 0) return 0;
  if (!out || (k > 0 && (!idx || !weight)) || (k > 0 && m_in > 0 && !input)) return 1;
  const bool v4 = vec4(c, {input, out});
  unsigned grid;
  if (!grid_for((long long)n_out * (v4 ? c / 4 : c), grid)) return 1;
  if (v4) hipLaunchKernelGGL(interp_fwd_kernel<4>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, n_out, c, k, m_in, input, idx, weight, out);
  else hipLaunchKernelGGL(interp_fwd_kernel<1>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, n_out, c, k, m_in, input, idx, weight, out);
  return launched();
}

int u3d_offset_interpolate_backward(int n_out, int c, int k, int m_in, const float* grad_out, const int32_t* idx, const float* weight,
                                    float* grad_input, void* stream) {
  if (n_out < 0 || c < 0 || k < 0 || m_in < 0) return 1;
  const long long rows = (long long)n_out * k;
  if (rows == 0 || c == 0 || m_in == 0) return 0;
  if (!grad_out || !idx || !weight || !grad_input) return 1;
  unsigned grid;
  if (!grid_for(rows * c, grid)) return 1;
  if (!zero_fill(grad_input, (long long)m_in * c, (hipStream_t)stream)) return 3;
  hipLaunchKernelGGL(interp_bwd_kernel, dim3(grid), dim3(NT), 0, (hipStream_t)stream, rows, c, k, m_in, grad_out, idx, weight, grad_input);
  return launched();
}

int u3d_offset_subtract_forward(int n, int nsample, int c, const float* in1, const float* in2, const int32_t* idx, float* out,
                                void* stream) {
  if (n < 0 || nsample < 0 || c < 0) return 1;
  const long long rows = (long long)n * nsample;
  if (rows == 0 || c == 0) return 0;
  if (!in1 || !in2 || !idx || !out) return 1;
  const bool v4 = vec4(c, {in1, in2, out});
  unsigned grid;
  if (!grid_for(rows * (v4 ? c / 4 : c), grid)) return 1;
  if (v4) hipLaunchKernelGGL(subtract_fwd_kernel<4>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, rows, nsample, c, n, in1, in2, idx, out);
  else hipLaunchKernelGGL(subtract_fwd_kernel<1>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, rows, nsample, c, n, in1, in2, idx, out);
  return launched();
}

int u3d_offset_subtract_backward(int n, int nsample, int c, const int32_t* idx, const float* grad_out, float* grad_in1, float* grad_in2,
                                 void* stream) {
  if (n < 0 || nsample < 0 || c < 0) return 1;
  if (n == 0 || c == 0) return 0;
  if (!grad_in1 || !grad_in2 || (nsample > 0 && (!idx || !grad_out))) return 1;
  unsigned grid;
  if (!grid_for((long long)n * c, grid)) return 1;
  if (!zero_fill(grad_in2, (long long)n * c, (hipStream_t)stream)) return 3;
  hipLaunchKernelGGL(subtract_bwd_kernel, dim3(grid), dim3(NT), 0, (hipStream_t)stream, n, nsample, c, idx, grad_out, grad_in1, grad_in2);
  return launched();
}

int u3d_offset_aggregate_forward(int n, int nsample, int c, int w_c, const float* input, const float* position, const float* weight,
                                 const int32_t* idx, float* out, void* stream) {
  if (n < 0 || nsample < 0 || c < 0 || w_c < 1 || c % w_c != 0) return 1;
  if (n == 0 || c == 0) return 0;
  if (!input || !out || (nsample > 0 && (!position || !weight || !idx))) return 1;
  const bool v4 = vec4(c, {input, position, out});
  unsigned grid;
  if (!grid_for((long long)n * (v4 ? c / 4 : c), grid)) return 1;
  if (v4) hipLaunchKernelGGL(aggregate_fwd_kernel<4>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, n, nsample, c, w_c, input, position, weight,
                             idx, out);
  else hipLaunchKernelGGL(aggregate_fwd_kernel<1>, dim3(grid), dim3(NT), 0, (hipStream_t)stream, n, nsample, c, w_c, input, position, weight,
                          idx, out);
  return launched();
}

int u3d_offset_aggregate_backward(int n, int nsample, int c, int w_c, const float* input, const float* position, const float* weight,
                                  const int32_t* idx, const float* grad_out, float* grad_input, float* grad_position, float* grad_weight,
                                  void* stream) {
  if (n < 0 || nsample < 0 || c < 0 || w_c < 1 || c % w_c != 0) return 1;
  if (n == 0 || c == 0) return 0;
  if (!grad_input) return 1;
  const long long rows = (long long)n * nsample;
  if (rows > 0 && (!input || !position || !weight || !idx || !grad_out || !grad_position || !grad_weight)) return 1;
  unsigned grid, grid_w;
  if (rows > 0 && (!grid_for(rows * c, grid) || !grid_for(rows * w_c, grid_w))) return 1;
  if (!zero_fill(grad_input, (long long)n * c, (hipStream_t)stream)) return 3;
  if (rows == 0) return 0;
  hipLaunchKernelGGL(aggregate_bwd_kernel, dim3(grid), dim3(NT), 0, (hipStream_t)stream, rows, nsample, c, w_c, n, weight, idx, grad_out,
                     grad_input, grad_position);
  hipLaunchKernelGGL(aggregate_bwd_weight_kernel, dim3(grid_w), dim3(NT), 0, (hipStream_t)stream, rows, nsample, c, w_c, n, input, position,
                     idx, grad_out, grad_weight);
  return launched();
}

}  // extern "C"
