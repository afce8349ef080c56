// libunipre3d_batchnorm.so: BatchNorm1d over (N, C) point rows fused with its activation and the residual add, forward and backward
// (include/unipre3d_batchnorm.h).  Lanes run along the channels; a workgroup takes row_chunk(C) rows, so a chunk starts at channel 0.
// The sums are f64 per chunk, combined through LDS and then across chunks in a fixed order: no atomics, same bits every run.
// The f32 arithmetic is written out without contraction so that tests/batchnorm_ref.py can restate it operation by operation.
#include "unipre3d_batchnorm.h"

#include <hip/hip_runtime.h>
#include <math.h>

#include <initializer_list>

#include "u3d_util.h"

#pragma clang fp contract(off)

using namespace u3d_util;

namespace {

constexpr int NT = 256;                       // threads per workgroup
constexpr int MAXC = U3D_BN_MAX_CHANNELS;
constexpr int CHUNK_FLOATS = 4096;            // a workgroup's share of a (N, C) tensor, at least MIN_ROWS rows
constexpr int MIN_ROWS = 32;

inline int row_chunk(int C) { return CHUNK_FLOATS / C < MIN_ROWS ? MIN_ROWS : CHUNK_FLOATS / C; }
inline bool ok4(const void* p) { return p != nullptr && ((uintptr_t)p & 3u) == 0; }
inline bool opt4(const void* p) { return ((uintptr_t)p & 3u) == 0; }
inline bool ok8(const void* p) { return p != nullptr && ((uintptr_t)p & 7u) == 0; }
inline bool opt8(const void* p) { return ((uintptr_t)p & 7u) == 0; }

template <int V>
__device__ __forceinline__ void ld(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = *p;
  }
}
template <int V>
__device__ __forceinline__ void st(float* p, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

// sm: mean [C] | invstd [C] | invstd gamma [C] | beta [C]
__device__ __forceinline__ void load_fold(float* sm, int C, int eval, float eps, const float* mean, const float* second, const float* gamma,
                                          const float* beta) {
  for (int c = threadIdx.x; c < C; c += NT) {
    const float is = eval ? 1.f / sqrtf(second[c] + eps) : second[c];
    sm[c] = mean[c];
    sm[C + c] = is;
    sm[2 * C + c] = is * (gamma ? gamma[c] : 1.f);
    sm[3 * C + c] = beta ? beta[c] : 0.f;
  }
}

template <int ACT>
__device__ __forceinline__ float act_fwd(float z) {
  if constexpr (ACT == U3D_BN_ACT_RELU) return z > 0.f ? z : 0.f;
  if constexpr (ACT == U3D_BN_ACT_GELU) return (0.5f * z) * (1.f + erff(z * 0.70710678118654752440f));
  return z;
}
// g = dy act'(.)
template <int ACT>
__device__ __forceinline__ float act_bwd(float dy, float x, float y, float mean, float a, float beta) {
  if constexpr (ACT == U3D_BN_ACT_RELU) return y > 0.f ? dy : 0.f;
  if constexpr (ACT == U3D_BN_ACT_GELU) {
    const float z = (x - mean) * a + beta;
    const float cdf = 0.5f * (1.f + erff(z * 0.70710678118654752440f));
    const float pdf = expf((-0.5f * z) * z) * 0.39894228040143267794f;
    return dy * (cdf + z * pdf);
  }
  return dy;
}

// The chunk's per-channel f64 sums of the two values f gives per element -> partials[blockIdx.x] = sum a [C] | sum b [C].
// Threads tile the chunk as (row lane, column unit of V channels); the row lanes of a column are added in ascending order.
template <int V, class F>
__device__ __forceinline__ void chunk_sums(F f, long long N, int C, int chunk, double* partials, double* sh) {
  const int cols = C / V;
  const long long r0 = (long long)blockIdx.x * chunk;
  const int rows = (int)(N - r0 < chunk ? N - r0 : chunk);
  const int cpp = cols < NT ? cols : NT;      // column units per pass
  const int RP = NT / cpp;                    // row lanes
  const int t = threadIdx.x, cu_in = t % cpp, rl = t / cpp;
  double* out = partials + (size_t)blockIdx.x * 2 * C;
  for (int cu0 = 0; cu0 < cols; cu0 += cpp) {
    const int cu = cu0 + cu_in;
    double s1[V], s2[V];
#pragma unroll
    for (int j = 0; j < V; ++j) s1[j] = s2[j] = 0.0;
    if (rl < RP && cu < cols) {
#pragma unroll 4
      for (int r = rl; r < rows; r += RP) {
        double a[V], b[V];
        f((size_t)(r0 + r) * C + (size_t)cu * V, cu * V, a, b);
#pragma unroll
        for (int j = 0; j < V; ++j) { s1[j] += a[j]; s2[j] += b[j]; }
      }
    }
    if (rl < RP) {
#pragma unroll
      for (int j = 0; j < V; ++j) {
        sh[(rl * cpp + cu_in) * V + j] = s1[j];
        sh[NT * V + (rl * cpp + cu_in) * V + j] = s2[j];
      }
    }
    __syncthreads();
    const int nout = (cols - cu0 < cpp ? cols - cu0 : cpp) * V;
    for (int u = t; u < nout; u += NT) {
      double a = 0.0, b = 0.0;
      for (int q = 0; q < RP; ++q) { a += sh[q * cpp * V + u]; b += sh[NT * V + q * cpp * V + u]; }
      out[cu0 * V + u] = a;
      out[C + cu0 * V + u] = b;
    }
    __syncthreads();
  }
}

template <int V>
__global__ __launch_bounds__(NT) void stats_kernel(const float* __restrict__ x, long long N, int C, int chunk, long long* nbt,
                                                   double* __restrict__ partials) {
  __shared__ double sh[2 * NT * V];
  if (nbt != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *nbt += 1;
  chunk_sums<V>([&](size_t at, int, double (&a)[V], double (&b)[V]) {
    float v[V];
    ld<V>(x + at, v);
#pragma unroll
    for (int j = 0; j < V; ++j) { a[j] = (double)v[j]; b[j] = a[j] * a[j]; }
  }, N, C, chunk, partials, sh);
}

template <int V, int ACT>
__global__ __launch_bounds__(NT) void bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y,
                                                        long long N, int C, int chunk, int eval, float eps, const float* mean,
                                                        const float* second, const float* gamma, const float* beta,
                                                        double* __restrict__ partials) {
  __shared__ double sh[2 * NT * V];
  __shared__ __align__(16) float sm[4 * MAXC];
  load_fold(sm, C, eval, eps, mean, second, gamma, beta);
  __syncthreads();
  chunk_sums<V>([&](size_t at, int c, double (&a)[V], double (&b)[V]) {
    float dv[V], xv[V], yv[V];
    ld<V>(dy + at, dv);
    ld<V>(x + at, xv);
    if constexpr (ACT == U3D_BN_ACT_RELU) ld<V>(y + at, yv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float g = act_bwd<ACT>(dv[j], xv[j], ACT == U3D_BN_ACT_RELU ? yv[j] : 0.f, sm[c + j], sm[2 * C + c + j], sm[3 * C + c + j]);
      const float xhat = (xv[j] - sm[c + j]) * sm[C + c + j];
      a[j] = (double)g;
      b[j] = (double)g * (double)xhat;
    }
  }, N, C, chunk, partials, sh);
}

// Adds the partials per column in a fixed order and, where asked, derives what follows from the block.  A workgroup takes SUM_COLS
// columns; SUM_SLOTS slots of threads walk the chunks SUM_SLOTS apart with SUM_U independent accumulators each (the loads of one step
// are all in flight together: the chain is parts / 512 steps long, not parts), then a pairwise sum per thread and a tree over the slots.
// partials null: the block is taken as it stands (it may hold other processes' rows too).
constexpr int SUM_COLS = 16, SUM_SLOTS = 64, SUM_U = 8, SUM_NT = SUM_COLS * SUM_SLOTS;
__global__ __launch_bounds__(SUM_NT) void sum_kernel(const double* __restrict__ partials, long long parts, int C, double count, double* block,
                                                     float* out_a, float* out_b, double eps, double momentum, float* run_mean, float* run_var,
                                                     const long long* nbt, float* mean_invstd) {
  __shared__ double sh[2][SUM_SLOTS][SUM_COLS];
  const int slot = threadIdx.x / SUM_COLS, col = threadIdx.x % SUM_COLS, c = blockIdx.x * SUM_COLS + col;
  if (partials != nullptr) {
    double a[SUM_U], b[SUM_U];
#pragma unroll
    for (int k = 0; k < SUM_U; ++k) a[k] = b[k] = 0.0;
    if (c < C)
      for (long long p0 = slot; p0 < parts; p0 += SUM_SLOTS * SUM_U) {
#pragma unroll
        for (int k = 0; k < SUM_U; ++k) {                       // a chunk past the end is read as the last one and added as zero
          const long long p = p0 + (long long)k * SUM_SLOTS, q = p < parts ? p : parts - 1;
          const double v1 = partials[(size_t)q * 2 * C + c], v2 = partials[(size_t)q * 2 * C + C + c];
          a[k] += p < parts ? v1 : 0.0;
          b[k] += p < parts ? v2 : 0.0;
        }
      }
    sh[0][slot][col] = ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]));
    sh[1][slot][col] = ((b[0] + b[1]) + (b[2] + b[3])) + ((b[4] + b[5]) + (b[6] + b[7]));
    __syncthreads();
    for (int o = SUM_SLOTS / 2; o > 0; o >>= 1) {
      if (slot < o) {
        sh[0][slot][col] += sh[0][slot + o][col];
        sh[1][slot][col] += sh[1][slot + o][col];
      }
      __syncthreads();
    }
  }
  if (slot != 0 || c >= C) return;
  double M, S1, S2;
  if (partials != nullptr) {
    M = count;
    S1 = sh[0][0][col];
    S2 = sh[1][0][col];
    if (c == 0) block[0] = M;
    block[1 + c] = S1;
    block[1 + C + c] = S2;
  } else {
    M = block[0];
    S1 = block[1 + c];
    S2 = block[1 + C + c];
  }
  if (out_a != nullptr) out_a[c] = (float)S1;
  if (out_b != nullptr) out_b[c] = (float)S2;
  if (mean_invstd == nullptr) return;
  const double mean = S1 / M;
  double var = S2 / M - mean * mean;
  if (!(var > 0.0)) var = 0.0;
  mean_invstd[c] = (float)mean;
  mean_invstd[C + c] = (float)(1.0 / sqrt(var + eps));
  const double f = momentum < 0.0 ? 1.0 / (double)(nbt != nullptr ? *nbt : 1) : momentum;
  if (run_mean != nullptr) run_mean[c] = (float)((1.0 - f) * (double)run_mean[c] + f * mean);
  if (run_var != nullptr) run_var[c] = (float)((1.0 - f) * (double)run_var[c] + f * (M > 1.0 ? var * (M / (M - 1.0)) : var));
}

template <int V, int ACT, bool RES>
__global__ __launch_bounds__(NT) void apply_kernel(const float* __restrict__ x, const float* __restrict__ res, long long N, int C, int chunk,
                                                   int eval, float eps, const float* mean, const float* second, const float* gamma,
                                                   const float* beta, float* __restrict__ y) {
  __shared__ __align__(16) float sm[4 * MAXC];
  load_fold(sm, C, eval, eps, mean, second, gamma, beta);
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * chunk;
  const int rows = (int)(N - r0 < chunk ? N - r0 : chunk);
  const size_t base = (size_t)r0 * C;
  const int n = rows * C / V, step = (NT * V) % C;
  int c = (threadIdx.x * V) % C;
  for (int i = threadIdx.x; i < n; i += NT) {
    float xv[V], rv[V], out[V];
    ld<V>(x + base + (size_t)i * V, xv);
    if constexpr (RES) ld<V>(res + base + (size_t)i * V, rv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      float z = (xv[j] - sm[c + j]) * sm[2 * C + c + j] + sm[3 * C + c + j];
      if constexpr (RES) z = z + rv[j];
      out[j] = act_fwd<ACT>(z);
    }
    st<V>(y + base + (size_t)i * V, out);
    c += step;
    if (c >= C) c -= C;
  }
}

// sm: the fold | sum g / M [C] | sum(g xhat) / M [C]
template <int V, int ACT>
__global__ __launch_bounds__(NT) void bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y,
                                                       long long N, int C, int chunk, int eval, float eps, const float* mean,
                                                       const float* second, const float* gamma, const float* beta,
                                                       const double* __restrict__ block, float* __restrict__ dx, float* __restrict__ dres) {
  __shared__ __align__(16) float sm[6 * MAXC];
  load_fold(sm, C, eval, eps, mean, second, gamma, beta);
  if (block != nullptr) {
    const double M = block[0];
    for (int c = threadIdx.x; c < C; c += NT) {
      sm[4 * C + c] = (float)(block[1 + c] / M);
      sm[5 * C + c] = (float)(block[1 + C + c] / M);
    }
  }
  __syncthreads();
  const long long r0 = (long long)blockIdx.x * chunk;
  const int rows = (int)(N - r0 < chunk ? N - r0 : chunk);
  const size_t base = (size_t)r0 * C;
  const int n = rows * C / V, step = (NT * V) % C;
  int c = (threadIdx.x * V) % C;
  for (int i = threadIdx.x; i < n; i += NT) {
    const size_t at = base + (size_t)i * V;
    float dv[V], xv[V], yv[V], gv[V], out[V];
    ld<V>(dy + at, dv);
    ld<V>(x + at, xv);
    if constexpr (ACT == U3D_BN_ACT_RELU) ld<V>(y + at, yv);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      const float g = act_bwd<ACT>(dv[j], xv[j], ACT == U3D_BN_ACT_RELU ? yv[j] : 0.f, sm[c + j], sm[2 * C + c + j], sm[3 * C + c + j]);
      gv[j] = g;
      if (block != nullptr) {
        const float xhat = (xv[j] - sm[c + j]) * sm[C + c + j];
        out[j] = sm[2 * C + c + j] * ((g - sm[4 * C + c + j]) - xhat * sm[5 * C + c + j]);
      } else {
        out[j] = g * sm[2 * C + c + j];
      }
    }
    if (dx != nullptr) st<V>(dx + at, out);
    if (dres != nullptr) st<V>(dres + at, gv);
    c += step;
    if (c >= C) c -= C;
  }
}

inline bool shape_ok(long long N, int C, long long& parts) {
  if (N < 1 || C < 1 || C > MAXC) return false;
  parts = (N + row_chunk(C) - 1) / row_chunk(C);
  return parts <= 0x7fffffffLL;
}
inline bool wide(int C, std::initializer_list<const void*> rows) {      // 16 bytes per lane: C % 4 == 0 and every row tensor aligned to 16
  if (C % 4) return false;
  for (const void* p : rows) if (!aligned16(p)) return false;             // (a null pointer counts as aligned)
  return true;
}

}  // namespace

extern "C" {

int u3d_bn_abi_version(void) { return U3D_BN_ABI_VERSION; }

int u3d_bn_row_chunk(int C) { return C < 1 || C > MAXC ? 0 : row_chunk(C); }

int u3d_bn_stats(const float* x, long long N, int C, long long* nbt, double* partials, void* stream) {
  long long parts;
  if (!ok4(x) || !opt8(nbt) || !ok8(partials) || N < 1 || C < 1) return 1;
  if (!shape_ok(N, C, parts)) return 2;
  hipStream_t s = (hipStream_t)stream;
  if (wide(C, {x})) stats_kernel<4><<<(unsigned)parts, NT, 0, s>>>(x, N, C, row_chunk(C), nbt, partials);
  else stats_kernel<1><<<(unsigned)parts, NT, 0, s>>>(x, N, C, row_chunk(C), nbt, partials);
  return launched();
}

int u3d_bn_sum(const double* partials, long long parts, int C, double count, double* block, float* out_a, float* out_b, void* stream) {
  if (!ok8(partials) || !ok8(block) || !opt4(out_a) || !opt4(out_b) || parts < 1 || C < 1) return 1;
  if (C > MAXC) return 2;
  sum_kernel<<<blocks(C, SUM_COLS), SUM_NT, 0, (hipStream_t)stream>>>(partials, parts, C, count, block, out_a, out_b, 0.0, 0.0, nullptr, nullptr, nullptr,
                                                           nullptr);
  return launched();
}

int u3d_bn_finalize(const double* partials, long long parts, double count, double* block, int C, double eps, double momentum,
                    float* running_mean, float* running_var, const long long* nbt, float* mean_invstd, void* stream) {
  if (!opt8(partials) || !ok8(block) || !opt4(running_mean) || !opt4(running_var) || !opt8(nbt) || !ok4(mean_invstd) || C < 1 ||
      (partials != nullptr && parts < 1))
    return 1;
  if (C > MAXC) return 2;
  sum_kernel<<<blocks(C, SUM_COLS), SUM_NT, 0, (hipStream_t)stream>>>(partials, parts, C, count, block, nullptr, nullptr, eps, momentum,
                                                           running_mean, running_var, nbt, mean_invstd);
  return launched();
}

#define U3D_BN_APPLY(V)                                                                                                                  \
  do {                                                                                                                                   \
    if (act == U3D_BN_ACT_GELU) apply_kernel<V, U3D_BN_ACT_GELU, false><<<g, NT, 0, s>>>(x, residual, N, C, ch, eval, eps, mean, second, gamma, beta, y); \
    else if (act == U3D_BN_ACT_RELU && residual) apply_kernel<V, U3D_BN_ACT_RELU, true><<<g, NT, 0, s>>>(x, residual, N, C, ch, eval, eps, mean, second, gamma, beta, y); \
    else if (act == U3D_BN_ACT_RELU) apply_kernel<V, U3D_BN_ACT_RELU, false><<<g, NT, 0, s>>>(x, residual, N, C, ch, eval, eps, mean, second, gamma, beta, y); \
    else if (residual) apply_kernel<V, U3D_BN_ACT_NONE, true><<<g, NT, 0, s>>>(x, residual, N, C, ch, eval, eps, mean, second, gamma, beta, y); \
    else apply_kernel<V, U3D_BN_ACT_NONE, false><<<g, NT, 0, s>>>(x, residual, N, C, ch, eval, eps, mean, second, gamma, beta, y);      \
  } while (0)

int u3d_bn_apply(const float* x, const float* residual, long long N, int C, int act, int eval, float eps, const float* mean,
                 const float* second, const float* gamma, const float* beta, float* y, void* stream) {
  long long parts;
  if (!ok4(x) || !opt4(residual) || !ok4(mean) || !ok4(second) || !opt4(gamma) || !opt4(beta) || !ok4(y) || N < 1 || C < 1) return 1;
  if (!shape_ok(N, C, parts) || act < 0 || act > 2 || (act == U3D_BN_ACT_GELU && residual != nullptr)) return 2;
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = (unsigned)parts;
  const int ch = row_chunk(C);
  if (wide(C, {x, residual, y})) U3D_BN_APPLY(4);
  else U3D_BN_APPLY(1);
  return launched();
}

#define U3D_BN_BWD(KERNEL, V, ...)                                                                        \
  do {                                                                                                    \
    if (act == U3D_BN_ACT_GELU) KERNEL<V, U3D_BN_ACT_GELU><<<g, NT, 0, s>>>(__VA_ARGS__);                  \
    else if (act == U3D_BN_ACT_RELU) KERNEL<V, U3D_BN_ACT_RELU><<<g, NT, 0, s>>>(__VA_ARGS__);             \
    else KERNEL<V, U3D_BN_ACT_NONE><<<g, NT, 0, s>>>(__VA_ARGS__);                                         \
  } while (0)

int u3d_bn_bwd_reduce(const float* dy, const float* x, const float* y, long long N, int C, int act, int eval, float eps,
                      const float* mean, const float* second, const float* gamma, const float* beta, double* partials, void* stream) {
  long long parts;
  if (!ok4(dy) || !ok4(x) || !opt4(y) || !ok4(mean) || !ok4(second) || !opt4(gamma) || !opt4(beta) || !ok8(partials) || N < 1 || C < 1)
    return 1;
  if (act == U3D_BN_ACT_RELU && y == nullptr) return 1;
  if (!shape_ok(N, C, parts) || act < 0 || act > 2) return 2;
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = (unsigned)parts;
  const int ch = row_chunk(C);
  if (act != U3D_BN_ACT_RELU) y = nullptr;
  if (wide(C, {dy, x, y})) U3D_BN_BWD(bwd_reduce_kernel, 4, dy, x, y, N, C, ch, eval, eps, mean, second, gamma, beta, partials);
  else U3D_BN_BWD(bwd_reduce_kernel, 1, dy, x, y, N, C, ch, eval, eps, mean, second, gamma, beta, partials);
  return launched();
}

int u3d_bn_bwd_apply(const float* dy, const float* x, const float* y, long long N, int C, int act, int eval, float eps,
                     const float* mean, const float* second, const float* gamma, const float* beta, const double* block, float* dx,
                     float* dresidual, void* stream) {
  long long parts;
  if (!ok4(dy) || !ok4(x) || !opt4(y) || !ok4(mean) || !ok4(second) || !opt4(gamma) || !opt4(beta) || !opt8(block) || !opt4(dx) ||
      !opt4(dresidual) || (dx == nullptr && dresidual == nullptr) || N < 1 || C < 1)
    return 1;
  if (act == U3D_BN_ACT_RELU && y == nullptr) return 1;
  if (!shape_ok(N, C, parts) || act < 0 || act > 2 || (act == U3D_BN_ACT_GELU && dresidual != nullptr)) return 2;
  hipStream_t s = (hipStream_t)stream;
  const unsigned g = (unsigned)parts;
  const int ch = row_chunk(C);
  if (act != U3D_BN_ACT_RELU) y = nullptr;
  if (wide(C, {dy, x, y, dx, dresidual}))
    U3D_BN_BWD(bwd_apply_kernel, 4, dy, x, y, N, C, ch, eval, eps, mean, second, gamma, beta, block, dx, dresidual);
  else
    U3D_BN_BWD(bwd_apply_kernel, 1, dy, x, y, N, C, ch, eval, eps, mean, second, gamma, beta, block, dx, dresidual);
  return launched();
}

}  // extern "C"
