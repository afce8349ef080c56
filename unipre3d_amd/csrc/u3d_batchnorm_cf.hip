// libunipre3d_batchnorm_cf.so: BatchNorm1d over channels-first (B, C, L) tensors fused with its activation, the residual add and,
// where asked, the max over L that follows (include/unipre3d_batchnorm_cf.h).  A (b, c) row is L contiguous floats.  A power-of-two
// group of G lanes owns one row at a time; a workgroup of 256 threads holds 256 / G row slots = channel_tile channels x batch lanes,
// and a slot keeps its channel while it walks a chunk of batch entries, so the f64 sums stay in registers and meet once per
// workgroup: a butterfly over the group's lanes, then the batch lanes through LDS in ascending order.  No atomics, same bits every
// run.  The row max / argmax of the pooled form is the same butterfly over (value, index), ties to the lower index.
// The f32 arithmetic is written out without contraction so that tests/batchnorm_cf_ref.py can restate it operation by operation.
#include "unipre3d_batchnorm_cf.h"

#include <hip/hip_runtime.h>
#include <math.h>

#include <initializer_list>
#include <type_traits>

#include "u3d_util.h"

#pragma clang fp contract(off)

using namespace u3d_util;

namespace {

constexpr int NT = 256;                       // threads per workgroup
constexpr int MAXC = U3D_BNCF_MAX_CHANNELS;
constexpr int MAXG = 64;                      // a lane group never leaves its wave
constexpr int CHUNK_FLOATS = 8192;            // batch_chunk = CHUNK_FLOATS / (min(C, 32) L), at least 1, at most MAX_CHUNK
constexpr int MAX_CHUNK = 4096;

struct Plan {
  int G, CT, BS, BC, V;                       // lanes per row, channel tile, batch lanes, batch chunk, floats per lane
};

inline int batch_chunk(int C, int L) {
  const long long per = (long long)(C < 32 ? C : 32) * L;
  const long long bc = CHUNK_FLOATS / per;
  return bc < 1 ? 1 : bc > MAX_CHUNK ? MAX_CHUNK : (int)bc;
}
inline Plan make_plan(int C, int L, bool wide) {
  Plan p;
  p.V = wide ? 4 : 1;
  const int units = (L + p.V - 1) / p.V;
  p.G = 1;
  while (p.G < units && p.G < MAXG) p.G <<= 1;
  const int R = NT / p.G;
  p.CT = C < R ? C : R;
  p.BS = R / p.CT;
  p.BC = batch_chunk(C, L);
  return p;
}

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

template <int ACT>
__device__ __forceinline__ float act_fwd(float z) {
  if constexpr (ACT == U3D_BNCF_ACT_RELU) return z > 0.f ? z : 0.f;
  if constexpr (ACT == U3D_BNCF_ACT_GELU) return (0.5f * z) * (1.f + erff(z * 0.70710678118654752440f));
  return z;
}
// g = dy act'(.): relu from the output's mask, gelu from the pre-activation z
template <int ACT>
__device__ __forceinline__ float act_bwd(float dy, float z, float y) {
  if constexpr (ACT == U3D_BNCF_ACT_RELU) return y > 0.f ? dy : 0.f;
  if constexpr (ACT == U3D_BNCF_ACT_GELU) {
    const float cdf = 0.5f * (1.f + erff(z * 0.70710678118654752440f));
    const float pdf = expf((-0.5f * z) * z) * 0.39894228040143267794f;
    return dy * (cdf + z * pdf);
  }
  return dy;
}

// What a thread is in its workgroup: lane gl of a group of G, row slot (channel c, batch lane bs).  Slots past CT * BS and channels
// past C own nothing (live == false) but still walk every loop, so that the cross-lane steps see whole waves.
struct Slot {
  int gl, c, bs;
  bool live;
  long long b0, b1;                           // the workgroup's batch entries [b0, b1)
  int iters;                                  // steps of the batch loop, the same for every thread
};
__device__ __forceinline__ Slot slot_of(const Plan& p, long long B, int C) {
  Slot s;
  const int rs = threadIdx.x / p.G;
  s.gl = threadIdx.x % p.G;
  const int ci = rs % p.CT;
  s.bs = rs / p.CT;
  s.c = blockIdx.y * p.CT + ci;
  s.live = s.bs < p.BS && s.c < C;
  if (!s.live) s.c = 0;
  s.b0 = (long long)blockIdx.x * p.BC;
  s.b1 = s.b0 + p.BC < B ? s.b0 + p.BC : B;
  s.iters = (int)((s.b1 - s.b0 + p.BS - 1) / p.BS);
  return s;
}

// mean, invstd, invstd gamma, beta of a channel
struct Fold {
  float mean, is, a, beta;
};
__device__ __forceinline__ Fold fold_of(int c, int eval, float eps, const float* mean, const float* second, const float* gamma,
                                        const float* beta) {
  Fold f;
  f.is = eval ? 1.f / sqrtf(second[c] + eps) : second[c];
  f.mean = mean[c];
  f.a = f.is * (gamma ? gamma[c] : 1.f);
  f.beta = beta ? beta[c] : 0.f;
  return f;
}

// A workgroup's f64 sums of (s1, s2) per channel -> partials[blockIdx.x] = sum a [C] | sum b [C], its channel tile's slice.
__device__ __forceinline__ void meet(const Plan& p, const Slot& s, double s1, double s2, int C, double* partials, double (*sh)[NT]) {
  for (int o = p.G >> 1; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  const int rs = threadIdx.x / p.G;
  if (s.gl == 0) { sh[0][rs] = s1; sh[1][rs] = s2; }
  __syncthreads();
  const int t = threadIdx.x, c = blockIdx.y * p.CT + t;
  if (t < p.CT && c < C) {
    double a = 0.0, b = 0.0;
    for (int q = 0; q < p.BS; ++q) { a += sh[0][q * p.CT + t]; b += sh[1][q * p.CT + t]; }
    double* out = partials + (size_t)blockIdx.x * 2 * C;
    out[c] = a;
    out[C + c] = b;
  }
}

template <int V>
__global__ __launch_bounds__(NT) void stats_kernel(const float* __restrict__ x, long long B, int C, int L, Plan p, long long* nbt,
                                                   double* __restrict__ partials) {
  __shared__ double sh[2][NT];
  if (nbt != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *nbt += 1;
  const Slot s = slot_of(p, B, C);
  double s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < s.iters; ++i) {
    const long long b = s.b0 + (long long)i * p.BS + s.bs;
    if (!s.live || b >= s.b1) continue;
    const float* row = x + ((size_t)b * C + s.c) * L;
    for (int l = s.gl * V; l < L; l += p.G * V) {
      float v[V];
      ld<V>(row + l, v);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const double d = (double)v[j];
        s1 += d;
        s2 += d * d;
      }
    }
  }
  meet(p, s, s1, s2, C, partials, sh);
}

// Dense form: y (B, C, L).  Pooled form: pooled / arg in the S layout, nothing of (B, C, L) written.
template <int V, int ACT, bool RES, bool POOL>
__global__ __launch_bounds__(NT) void apply_kernel(const float* __restrict__ x, const float* __restrict__ res, long long B, int C, int L,
                                                   Plan p, int eval, float eps, const float* mean, const float* second,
                                                   const float* gamma, const float* beta, float* __restrict__ y,
                                                   float* __restrict__ pooled, int* __restrict__ arg, long long S) {
  const Slot s = slot_of(p, B, C);
  const Fold f = fold_of(s.c, eval, eps, mean, second, gamma, beta);
  for (int i = 0; i < s.iters; ++i) {
    const long long b = s.b0 + (long long)i * p.BS + s.bs;
    const bool on = s.live && b < s.b1;
    const size_t at = on ? ((size_t)b * C + s.c) * L : 0;
    float best = -INFINITY;
    int where = 0x7fffffff;
    if (on) {
      for (int l = s.gl * V; l < L; l += p.G * V) {
        float xv[V], rv[V], out[V];
        ld<V>(x + at + l, xv);
        if constexpr (RES) ld<V>(res + at + l, rv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
          float z = (xv[j] - f.mean) * f.a + f.beta;
          if constexpr (RES) z = z + rv[j];
          out[j] = act_fwd<ACT>(z);
          if constexpr (POOL) {
            if (out[j] > best) { best = out[j]; where = l + j; }
          }
        }
        if constexpr (!POOL) st<V>(y + at + l, out);
      }
    }
    if constexpr (POOL) {
      for (int o = p.G >> 1; o > 0; o >>= 1) {
        const float ob = __shfl_xor(best, o);
        const int ow = __shfl_xor(where, o);
        if (ob > best || (ob == best && ow < where)) { best = ob; where = ow; }
      }
      if (on && s.gl == 0) {
        const size_t to = ((size_t)(b / S) * C + s.c) * S + (size_t)(b % S);
        pooled[to] = best;
        arg[to] = where;
      }
    }
  }
}

template <int V, int ACT>
__global__ __launch_bounds__(NT) void bwd_reduce_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y,
                                                        long long B, int C, int L, Plan p, int eval, float eps, const float* mean,
                                                        const float* second, const float* gamma, const float* beta,
                                                        double* __restrict__ partials) {
  __shared__ double sh[2][NT];
  const Slot s = slot_of(p, B, C);
  const Fold f = fold_of(s.c, eval, eps, mean, second, gamma, beta);
  double s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < s.iters; ++i) {
    const long long b = s.b0 + (long long)i * p.BS + s.bs;
    if (!s.live || b >= s.b1) continue;
    const size_t at = ((size_t)b * C + s.c) * L;
    for (int l = s.gl * V; l < L; l += p.G * V) {
      float dv[V], xv[V], yv[V];
      ld<V>(dy + at + l, dv);
      ld<V>(x + at + l, xv);
      if constexpr (ACT == U3D_BNCF_ACT_RELU) ld<V>(y + at + l, yv);
#pragma unroll
      for (int j = 0; j < V; ++j) {
        const float z = ACT == U3D_BNCF_ACT_GELU ? (xv[j] - f.mean) * f.a + f.beta : 0.f;
        const float g = act_bwd<ACT>(dv[j], z, ACT == U3D_BNCF_ACT_RELU ? yv[j] : 0.f);
        const float xhat = (xv[j] - f.mean) * f.is;
        s1 += (double)g;
        s2 += (double)g * (double)xhat;
      }
    }
  }
  meet(p, s, s1, s2, C, partials, sh);
}

// g of the pooled form at (b, c): dpooled act'(.) at l = arg, read from x at that one position
template <int ACT>
__device__ __forceinline__ float pooled_g(const float* dpooled, const float* pooled, size_t to, float xa, const Fold& f) {
  const float z = ACT == U3D_BNCF_ACT_GELU ? (xa - f.mean) * f.a + f.beta : 0.f;
  return act_bwd<ACT>(dpooled[to], z, ACT == U3D_BNCF_ACT_RELU ? pooled[to] : 0.f);
}

// Pooled form: one thread per channel walks the chunk's batch entries in ascending order; x is read at B C positions only.
template <int ACT>
__global__ __launch_bounds__(NT) void bwd_reduce_pooled_kernel(const float* __restrict__ dpooled, const float* __restrict__ x,
                                                               const float* __restrict__ pooled, const int* __restrict__ arg, long long B,
                                                               int C, int L, int BC, long long S, int eval, float eps, const float* mean,
                                                               const float* second, const float* gamma, const float* beta,
                                                               double* __restrict__ partials) {
  const int c = blockIdx.y * NT + threadIdx.x;
  if (c >= C) return;
  const Fold f = fold_of(c, eval, eps, mean, second, gamma, beta);
  const long long b0 = (long long)blockIdx.x * BC, b1 = b0 + BC < B ? b0 + BC : B;
  double s1 = 0.0, s2 = 0.0;
  for (long long b = b0; b < b1; ++b) {
    const size_t to = ((size_t)(b / S) * C + c) * S + (size_t)(b % S);
    int l = arg[to];
    l = l < 0 ? 0 : l >= L ? L - 1 : l;                       // (an index outside the row is the caller's error; it is not followed)
    const float xa = x[((size_t)b * C + c) * L + l];
    const float g = pooled_g<ACT>(dpooled, pooled, to, xa, f);
    const float xhat = (xa - f.mean) * f.is;
    s1 += (double)g;
    s2 += (double)g * (double)xhat;
  }
  double* out = partials + (size_t)blockIdx.x * 2 * C;
  out[c] = s1;
  out[C + c] = s2;
}

// Dense form: dy, y (B, C, L).  Pooled form (POOL): dy = dpooled, y = pooled, arg in the S layout; g is zero off l = arg and every
// element of dx / dresidual is written once, the zeros included.
template <int V, bool POOL, int ACT>
__global__ __launch_bounds__(NT) void bwd_apply_kernel(const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ y,
                                                       const int* __restrict__ arg, long long B, int C, int L, Plan p, int eval, float eps,
                                                       const float* mean, const float* second, const float* gamma, const float* beta,
                                                       const double* __restrict__ block, long long S, float* __restrict__ dx,
                                                       float* __restrict__ dres) {
  const Slot s = slot_of(p, B, C);
  const Fold f = fold_of(s.c, eval, eps, mean, second, gamma, beta);
  float sb = 0.f, sd = 0.f;
  if (block != nullptr) {
    const double M = block[0];
    sb = (float)(block[1 + s.c] / M);
    sd = (float)(block[1 + C + s.c] / M);
  }
  for (int i = 0; i < s.iters; ++i) {
    const long long b = s.b0 + (long long)i * p.BS + s.bs;
    if (!s.live || b >= s.b1) continue;
    const size_t at = ((size_t)b * C + s.c) * L;
    float gp = 0.f;
    int la = -1;
    if constexpr (POOL) {
      const size_t to = ((size_t)(b / S) * C + s.c) * S + (size_t)(b % S);
      la = arg[to];
      la = la < 0 ? 0 : la >= L ? L - 1 : la;
      gp = pooled_g<ACT>(dy, y, to, x[at + la], f);
    }
    for (int l = s.gl * V; l < L; l += p.G * V) {
      float dv[V], xv[V], yv[V], gv[V], out[V];
      ld<V>(x + at + l, xv);
      if constexpr (!POOL) {
        ld<V>(dy + at + l, dv);
        if constexpr (ACT == U3D_BNCF_ACT_RELU) ld<V>(y + at + l, yv);
      }
#pragma unroll
      for (int j = 0; j < V; ++j) {
        float g;
        if constexpr (POOL) {
          g = l + j == la ? gp : 0.f;
        } else {
          const float z = ACT == U3D_BNCF_ACT_GELU ? (xv[j] - f.mean) * f.a + f.beta : 0.f;
          g = act_bwd<ACT>(dv[j], z, ACT == U3D_BNCF_ACT_RELU ? yv[j] : 0.f);
        }
        gv[j] = g;
        if (block != nullptr) {
          const float xhat = (xv[j] - f.mean) * f.is;
          out[j] = f.a * ((g - sb) - xhat * sd);
        } else {
          out[j] = g * f.a;
        }
      }
      if (dx != nullptr) st<V>(dx + at + l, out);
      if (dres != nullptr) st<V>(dres + at + l, gv);
    }
  }
}

inline bool shape_ok(long long B, int C, int L, long long& parts) {
  if (B < 1 || C < 1 || C > MAXC || L < 1) return false;
  const int bc = batch_chunk(C, L);
  parts = (B + bc - 1) / bc;
  return parts <= 0x7fffffffLL;
}
inline bool wide(int L, std::initializer_list<const void*> rows) {       // 16 bytes per lane: L % 4 == 0 and every row tensor aligned to 16
  if (L % 4) return false;
  for (const void* p : rows) if (!aligned16(p)) return false;            // (a null pointer counts as aligned)
  return true;
}
// f(the activation as a constant)
template <class F>
inline void with_act(int act, F f) {
  if (act == U3D_BNCF_ACT_GELU) f(std::integral_constant<int, U3D_BNCF_ACT_GELU>{});
  else if (act == U3D_BNCF_ACT_RELU) f(std::integral_constant<int, U3D_BNCF_ACT_RELU>{});
  else f(std::integral_constant<int, U3D_BNCF_ACT_NONE>{});
}
inline dim3 grid_of(const Plan& p, long long parts, int C) { return dim3((unsigned)parts, (unsigned)((C + p.CT - 1) / p.CT), 1); }

}  // namespace

extern "C" {

int u3d_bncf_abi_version(void) { return U3D_BNCF_ABI_VERSION; }

int u3d_bncf_plan(int C, int L, int aligned, int* lanes_per_row, int* channel_tile, int* batch_chunk_out, int* vec) {
  if (C < 1 || C > MAXC || L < 1) return 2;
  const Plan p = make_plan(C, L, aligned != 0 && L % 4 == 0);
  if (lanes_per_row) *lanes_per_row = p.G;
  if (channel_tile) *channel_tile = p.CT;
  if (batch_chunk_out) *batch_chunk_out = p.BC;
  if (vec) *vec = p.V;
  return 0;
}

long long u3d_bncf_parts(long long B, int C, int L) {
  long long parts;
  return shape_ok(B, C, L, parts) ? parts : 0;
}

int u3d_bncf_stats(const float* x, long long B, int C, int L, long long* nbt, double* partials, void* stream) {
  long long parts;
  if (!ok4(x) || !opt8(nbt) || !ok8(partials) || B < 1 || C < 1 || L < 1) return 1;
  if (!shape_ok(B, C, L, parts)) return 2;
  hipStream_t s = (hipStream_t)stream;
  const bool w = wide(L, {x});
  const Plan p = make_plan(C, L, w);
  const dim3 g = grid_of(p, parts, C);
  if (w) stats_kernel<4><<<g, NT, 0, s>>>(x, B, C, L, p, nbt, partials);
  else stats_kernel<1><<<g, NT, 0, s>>>(x, B, C, L, p, nbt, partials);
  return launched();
}

int u3d_bncf_apply(const float* x, const float* residual, long long B, int C, int L, int act, int eval, float eps, const float* mean,
                   const float* second, const float* gamma, const float* beta, float* y, float* pooled, int* arg, long long S,
                   void* stream) {
  long long parts;
  if (!ok4(x) || !opt4(residual) || !ok4(mean) || !ok4(second) || !opt4(gamma) || !opt4(beta) || !opt4(y) || !opt4(pooled) || !opt4(arg) ||
      B < 1 || C < 1 || L < 1)
    return 1;
  if ((pooled == nullptr) == (y == nullptr) || (pooled != nullptr) != (arg != nullptr)) return 1;      // y alone, or pooled and arg
  if (!shape_ok(B, C, L, parts) || act < 0 || act > 2 || (act == U3D_BNCF_ACT_GELU && residual != nullptr)) return 2;
  if (pooled != nullptr && (S < 1 || B % S != 0)) return 2;
  hipStream_t s = (hipStream_t)stream;
  const bool w = wide(L, {x, residual, y});
  const Plan p = make_plan(C, L, w);
  const dim3 g = grid_of(p, parts, C);
  auto go = [&](auto V, auto POOL) {
    with_act(act, [&](auto A) {
      constexpr int v = decltype(V)::value, a = decltype(A)::value;
      constexpr bool pool = decltype(POOL)::value;
      if (residual != nullptr) {
        if constexpr (a != U3D_BNCF_ACT_GELU)
          apply_kernel<v, a, true, pool><<<g, NT, 0, s>>>(x, residual, B, C, L, p, eval, eps, mean, second, gamma, beta, y, pooled, arg, S);
      } else {
        apply_kernel<v, a, false, pool><<<g, NT, 0, s>>>(x, residual, B, C, L, p, eval, eps, mean, second, gamma, beta, y, pooled, arg, S);
      }
    });
  };
  using one = std::integral_constant<int, 1>;
  using four = std::integral_constant<int, 4>;
  if (pooled != nullptr) w ? go(four{}, std::true_type{}) : go(one{}, std::true_type{});
  else w ? go(four{}, std::false_type{}) : go(one{}, std::false_type{});
  return launched();
}

int u3d_bncf_bwd_reduce(const float* dy, const float* x, const float* y, const int* arg, long long B, int C, int L, int act, int eval,
                        float eps, const float* mean, const float* second, const float* gamma, const float* beta, long long S,
                        double* partials, void* stream) {
  long long parts;
  if (!ok4(dy) || !ok4(x) || !opt4(y) || !opt4(arg) || !ok4(mean) || !ok4(second) || !opt4(gamma) || !opt4(beta) || !ok8(partials) ||
      B < 1 || C < 1 || L < 1)
    return 1;
  if (act == U3D_BNCF_ACT_RELU && y == nullptr) return 1;
  if (!shape_ok(B, C, L, parts) || act < 0 || act > 2) return 2;
  if (arg != nullptr && (S < 1 || B % S != 0)) return 2;
  hipStream_t s = (hipStream_t)stream;
  if (act != U3D_BNCF_ACT_RELU) y = nullptr;
  if (arg != nullptr) {
    const dim3 g((unsigned)parts, (unsigned)((C + NT - 1) / NT), 1);
    const int bc = batch_chunk(C, L);
    with_act(act, [&](auto A) {
      bwd_reduce_pooled_kernel<decltype(A)::value><<<g, NT, 0, s>>>(dy, x, y, arg, B, C, L, bc, S, eval, eps, mean, second, gamma, beta, partials);
    });
    return launched();
  }
  const bool w = wide(L, {dy, x, y});
  const Plan p = make_plan(C, L, w);
  const dim3 g = grid_of(p, parts, C);
  with_act(act, [&](auto A) {
    constexpr int a = decltype(A)::value;
    if (w) bwd_reduce_kernel<4, a><<<g, NT, 0, s>>>(dy, x, y, B, C, L, p, eval, eps, mean, second, gamma, beta, partials);
    else bwd_reduce_kernel<1, a><<<g, NT, 0, s>>>(dy, x, y, B, C, L, p, eval, eps, mean, second, gamma, beta, partials);
  });
  return launched();
}

int u3d_bncf_bwd_apply(const float* dy, const float* x, const float* y, const int* arg, long long B, int C, int L, int act, int eval,
                       float eps, const float* mean, const float* second, const float* gamma, const float* beta, const double* block,
                       long long S, float* dx, float* dresidual, void* stream) {
  long long parts;
  if (!ok4(dy) || !ok4(x) || !opt4(y) || !opt4(arg) || !ok4(mean) || !ok4(second) || !opt4(gamma) || !opt4(beta) || !opt8(block) ||
      !opt4(dx) || !opt4(dresidual) || (dx == nullptr && dresidual == nullptr) || B < 1 || C < 1 || L < 1)
    return 1;
  if (act == U3D_BNCF_ACT_RELU && y == nullptr) return 1;
  if (!shape_ok(B, C, L, parts) || act < 0 || act > 2 || (act == U3D_BNCF_ACT_GELU && dresidual != nullptr)) return 2;
  if (arg != nullptr && (S < 1 || B % S != 0)) return 2;
  hipStream_t s = (hipStream_t)stream;
  if (act != U3D_BNCF_ACT_RELU) y = nullptr;
  const bool pool = arg != nullptr;
  const bool w = pool ? wide(L, {x, dx, dresidual}) : wide(L, {dy, x, y, dx, dresidual});
  const Plan p = make_plan(C, L, w);
  const dim3 g = grid_of(p, parts, C);
  auto go = [&](auto V, auto POOL) {
    with_act(act, [&](auto A) {
      bwd_apply_kernel<decltype(V)::value, decltype(POOL)::value, decltype(A)::value><<<g, NT, 0, s>>>(
          dy, x, y, arg, B, C, L, p, eval, eps, mean, second, gamma, beta, block, S, dx, dresidual);
    });
  };
  using one = std::integral_constant<int, 1>;
  using four = std::integral_constant<int, 4>;
  if (pool) w ? go(four{}, std::true_type{}) : go(one{}, std::true_type{});
  else w ? go(four{}, std::false_type{}) : go(one{}, std::false_type{});
  return launched();
}

}  // extern "C"
