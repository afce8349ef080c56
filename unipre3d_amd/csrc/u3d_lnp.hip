// libunipre3d_lnp.so: Mamba3D's local norm pooling (GroupFeature's gathers + K_Norm + K_Pool), fp32, gfx950, wave64.
// include/unipre3d_lnp.h states what is computed; DESIGN.md section 7 the cut into kernels and the order of every reduction.
//
// One wave owns one (b, g) row.  A lane owns the float4 channel groups lane and lane + 64 (C <= 512), so a row of C = 384 is one
// 1536-byte coalesced load and the K neighbour rows of a wave are K independent loads.  Neighbour indices are loaded once by lanes
// 0 .. K-1 and handed round with v_readlane while every lane is active; the channel predicate is applied inside.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "u3d_group.h"
#include "u3d_util.h"
#include "unipre3d_lnp.h"

namespace {

using u3d_group::lane_value;
using u3d_group::load_neighbours;      // (idx_row, K, g, G, lane): lane k < K has neighbour k of row g, g itself where idx is outside [0, G)
using u3d_util::bad_ptr;
using u3d_util::block_tree_sum;

constexpr int SLOTS = 2;                         // float4 groups per lane
constexpr int ROW_NT = 256, ROW_WAVES = 4;       // stats / forward / dx kernels: four rows per workgroup
constexpr int STAT_MAX_WG = 256;                 // partials of (sum d, sum d^2): one double2 per workgroup
constexpr int BWD_NT = 512, BWD_WAVES = 8;       // partial kernel of the backward: eight rows per workgroup pass
constexpr int BWD_MAX_WG = 512;                  // partials of t and of the 4C parameter sums
constexpr int NB_NT = 256;
constexpr int PR_Q = 16, PR_GROUPS = 16;         // parameter reduce: 16 float4 columns x 16 groups of partial rows per workgroup

struct F4 { float v[4]; };
__device__ __forceinline__ F4 ld4(const float* p) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  return {{t.x, t.y, t.z, t.w}};
}
__device__ __forceinline__ void st4(float* p, const F4& a) { *reinterpret_cast<float4*>(p) = make_float4(a.v[0], a.v[1], a.v[2], a.v[3]); }
__device__ __forceinline__ F4 splat(float a) { return {{a, a, a, a}}; }

// ---- inverse neighbour lists ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NB_NT) void lnp_neighbours_kernel(const int32_t* __restrict__ idx, int32_t* __restrict__ ptr,
                                                                int32_t* __restrict__ ent, int G, int K) {
  __shared__ int cnt[U3D_LNP_MAX_GROUPS];
  __shared__ int start[U3D_LNP_MAX_GROUPS + 1];
  const int n = G * K;
  const int32_t* ib = idx + (size_t)blockIdx.x * n;
  int32_t* eb = ent + (size_t)blockIdx.x * n;
  for (int j = threadIdx.x; j < G; j += NB_NT) cnt[j] = 0;
  __syncthreads();
  for (int e = threadIdx.x; e < n; e += NB_NT) {
    const int v = ib[e];
    atomicAdd(&cnt[((unsigned)v < (unsigned)G) ? v : e / K], 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int j = 0; j < G; ++j) { start[j] = run; run += cnt[j]; }
    start[G] = run;
  }
  __syncthreads();
  for (int j = threadIdx.x; j <= G; j += NB_NT) ptr[(size_t)blockIdx.x * (G + 1) + j] = start[j];
  // every list by one thread, walking idx in ascending e = g K + k (the lanes of a wave read the same word)
  for (int j = threadIdx.x; j < G; j += NB_NT) {
    int pos = start[j];
    const int end = start[j + 1];
    for (int e = 0; e < n && pos < end; ++e) {
      const int v = ib[e];
      if ((((unsigned)v < (unsigned)G) ? v : e / K) == j) eb[pos++] = e;
    }
  }
}

// ---- forward --------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(ROW_NT) void lnp_stats_kernel(const float* __restrict__ x, long long xs, const int32_t* __restrict__ idx,
                                                           double* __restrict__ part, int G, int K, int C, long long rows, int nwg) {
  __shared__ double sh[2][ROW_WAVES];
  const uint32_t lane = u3d_util::lane_id();
  const int wave = threadIdx.x >> 6, C4 = C >> 2;
  double s1 = 0.0, s2 = 0.0;
  for (long long row = (long long)blockIdx.x * ROW_WAVES + wave; row < rows; row += (long long)nwg * ROW_WAVES) {
    const int g = (int)(row % G);
    const float* xb = x + (row / G) * xs;
    const int jn = load_neighbours(idx + row * K, K, g, G, lane);
    F4 xc[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int c4 = lane + 64 * s;
      xc[s] = c4 < C4 ? ld4(xb + (size_t)g * C + 4 * c4) : splat(0.f);
    }
    for (int k = 0; k < K; ++k) {
      const float* xn = xb + (size_t)lane_value(jn, k) * C;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const int c4 = lane + 64 * s;
        if (c4 < C4) {
          const F4 a = ld4(xn + 4 * c4);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const double d = (double)(a.v[i] - xc[s].v[i]);
            s1 += d;
            s2 += d * d;
          }
        }
      }
    }
  }
  u3d_group::wave_sums_to_lds<ROW_WAVES, 2>(s1, s2, sh, lane, wave);
  __syncthreads();
  u3d_group::block_sums_to_part<ROW_WAVES, 2>(sh, part, 2 * blockIdx.x);
}

__global__ __launch_bounds__(ROW_NT) void lnp_fwd_kernel(const float* __restrict__ x, long long xs, const int32_t* __restrict__ idx,
                                                         const float* __restrict__ alpha, const float* __restrict__ beta,
                                                         float* __restrict__ out, float* __restrict__ lse, float* __restrict__ stats,
                                                         const double* __restrict__ part, int G, int K, int C, long long rows, int nstat,
                                                         double n, float eps) {
  __shared__ double sh[ROW_NT];
  // every workgroup sums the same partials in the same tree: mu, s and r have the same bits everywhere
  const bool has = (int)threadIdx.x < nstat;
  const double S1 = block_tree_sum<ROW_NT>(has ? part[2 * threadIdx.x] : 0.0, sh);
  const double S2 = block_tree_sum<ROW_NT>(has ? part[2 * threadIdx.x + 1] : 0.0, sh);
  const float r = u3d_group::norm_stats(S1, S2, n, eps, blockIdx.x, stats);
  const uint32_t lane = u3d_util::lane_id();
  const int wave = threadIdx.x >> 6, C4 = C >> 2;
  const long long row = (long long)blockIdx.x * ROW_WAVES + wave;
  if (row >= rows) return;
  const int g = (int)(row % G);
  const float* xb = x + (row / G) * xs;
  const int jn = load_neighbours(idx + row * K, K, g, G, lane);
  F4 xc[SLOTS], al[SLOTS], be[SLOTS], m[SLOTS], l[SLOTS], acc[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int c4 = lane + 64 * s;
    const bool on = c4 < C4;
    xc[s] = on ? ld4(xb + (size_t)g * C + 4 * c4) : splat(0.f);
    al[s] = on ? ld4(alpha + 4 * c4) : splat(0.f);
    be[s] = on ? ld4(beta + 4 * c4) : splat(0.f);
    m[s] = splat(-INFINITY);
    l[s] = splat(0.f);
    acc[s] = splat(0.f);
  }
  for (int k = 0; k < K; ++k) {
    const float* xn = xb + (size_t)lane_value(jn, k) * C;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int c4 = lane + 64 * s;
      if (c4 < C4) {
        const F4 a = ld4(xn + 4 * c4);
#pragma unroll
        for (int i = 0; i < 4; ++i) m[s].v[i] = fmaxf(m[s].v[i], fmaf(al[s].v[i], (a.v[i] - xc[s].v[i]) * r, be[s].v[i]));
      }
    }
  }
  for (int k = 0; k < K; ++k) {
    const float* xn = xb + (size_t)lane_value(jn, k) * C;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int c4 = lane + 64 * s;
      if (c4 < C4) {
        const F4 a = ld4(xn + 4 * c4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v = fmaf(al[s].v[i], (a.v[i] - xc[s].v[i]) * r, be[s].v[i]);
          const float e = expf(v - m[s].v[i]);
          l[s].v[i] += e;
          acc[s].v[i] = fmaf(e, v, acc[s].v[i]);
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int c4 = lane + 64 * s;
    if (c4 < C4) {
      F4 o, ls, up;
      const F4 ah = ld4(alpha + C + 4 * c4), bh = ld4(beta + C + 4 * c4);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        o.v[i] = acc[s].v[i] / l[s].v[i];
        ls.v[i] = m[s].v[i] + logf(l[s].v[i]);
        up.v[i] = fmaf(ah.v[i], xc[s].v[i], bh.v[i]);
      }
      st4(out + (size_t)row * 2 * C + 4 * c4, o);
      st4(out + (size_t)row * 2 * C + C + 4 * c4, up);
      st4(lse + (size_t)row * C + 4 * c4, ls);
    }
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
// gv = g1 p ((v - out) + 1) for one element; u = d r
__device__ __forceinline__ float grad_v(float al, float be, float u, float ls, float o, float g1) {
  const float v = fmaf(al, u, be);
  return g1 * expf(v - ls) * ((v - o) + 1.f);
}

__global__ __launch_bounds__(BWD_NT) void lnp_bwd_partial_kernel(const float* __restrict__ x, long long xs, const int32_t* __restrict__ idx,
                                                                 const float* __restrict__ alpha, const float* __restrict__ beta,
                                                                 const float* __restrict__ out, const float* __restrict__ lse,
                                                                 const float* __restrict__ stats, const float* __restrict__ dout,
                                                                 double* __restrict__ tpart, float* __restrict__ ppart, int G, int K, int C,
                                                                 long long rows, int nwg) {
  __shared__ float shp[4 * U3D_LNP_MAX_CHANNELS];      // [dalpha lower | dbeta lower | dalpha upper | dbeta upper], C each
  __shared__ double sht[1][BWD_WAVES];
  const uint32_t lane = u3d_util::lane_id();
  const int wave = threadIdx.x >> 6, C4 = C >> 2;
  const float r = stats[2];
  F4 al[SLOTS], be[SLOTS], da[SLOTS], db[SLOTS], dah[SLOTS], dbh[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int c4 = lane + 64 * s;
    al[s] = c4 < C4 ? ld4(alpha + 4 * c4) : splat(0.f);
    be[s] = c4 < C4 ? ld4(beta + 4 * c4) : splat(0.f);
    da[s] = db[s] = dah[s] = dbh[s] = splat(0.f);
  }
  double t = 0.0;
  for (long long row = (long long)blockIdx.x * BWD_WAVES + wave; row < rows; row += (long long)nwg * BWD_WAVES) {
    const int g = (int)(row % G);
    const float* xb = x + (row / G) * xs;
    const int jn = load_neighbours(idx + row * K, K, g, G, lane);
    F4 xc[SLOTS], o[SLOTS], ls[SLOTS], g1[SLOTS];
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int c4 = lane + 64 * s;
      const bool on = c4 < C4;
      xc[s] = on ? ld4(xb + (size_t)g * C + 4 * c4) : splat(0.f);
      o[s] = on ? ld4(out + (size_t)row * 2 * C + 4 * c4) : splat(0.f);
      ls[s] = on ? ld4(lse + (size_t)row * C + 4 * c4) : splat(0.f);
      g1[s] = on ? ld4(dout + (size_t)row * 2 * C + 4 * c4) : splat(0.f);
      if (on) {
        const F4 g2 = ld4(dout + (size_t)row * 2 * C + C + 4 * c4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          dah[s].v[i] = fmaf(g2.v[i], xc[s].v[i], dah[s].v[i]);
          dbh[s].v[i] += g2.v[i];
        }
      }
    }
    for (int k = 0; k < K; ++k) {
      const float* xn = xb + (size_t)lane_value(jn, k) * C;
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const int c4 = lane + 64 * s;
        if (c4 < C4) {
          const F4 a = ld4(xn + 4 * c4);
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float d = a.v[i] - xc[s].v[i], u = d * r;
            const float gv = grad_v(al[s].v[i], be[s].v[i], u, ls[s].v[i], o[s].v[i], g1[s].v[i]);
            da[s].v[i] = fmaf(gv, u, da[s].v[i]);
            db[s].v[i] += gv;
            t += (double)((gv * al[s].v[i]) * d);
          }
        }
      }
    }
  }
  u3d_group::wave_sums_to_lds<BWD_WAVES, 1>(t, 0.0, sht, lane, wave);
  // the eight waves' rows, added in wave order
  for (int w = 0; w < BWD_WAVES; ++w) {
    if (wave == w) {
#pragma unroll
      for (int s = 0; s < SLOTS; ++s) {
        const int c4 = lane + 64 * s;
        if (c4 < C4) {
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int c = 4 * c4 + i;
            if (w == 0) {
              shp[c] = da[s].v[i]; shp[C + c] = db[s].v[i]; shp[2 * C + c] = dah[s].v[i]; shp[3 * C + c] = dbh[s].v[i];
            } else {
              shp[c] += da[s].v[i]; shp[C + c] += db[s].v[i]; shp[2 * C + c] += dah[s].v[i]; shp[3 * C + c] += dbh[s].v[i];
            }
          }
        }
      }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < 4 * C; i += BWD_NT) ppart[(size_t)blockIdx.x * 4 * C + i] = shp[i];
  u3d_group::block_sums_to_part<BWD_WAVES, 1>(sht, tpart, 2 * blockIdx.x);      // (t, 0)
}

__global__ __launch_bounds__(ROW_NT) void lnp_bwd_dx_kernel(const float* __restrict__ x, long long xs, const int32_t* __restrict__ idx,
                                                            const int32_t* __restrict__ ptr, const int32_t* __restrict__ ent,
                                                            const float* __restrict__ alpha, const float* __restrict__ beta,
                                                            const float* __restrict__ out, const float* __restrict__ lse,
                                                            const float* __restrict__ stats, const float* __restrict__ dout,
                                                            const double* __restrict__ tpart, const float* __restrict__ ppart,
                                                            float* __restrict__ dx, float* __restrict__ dalpha, float* __restrict__ dbeta,
                                                            int G, int K, int C, long long rows, int nwg, int dx_blocks) {
  __shared__ double sh[ROW_NT * 4];
  const int C4 = C >> 2;
  if ((int)blockIdx.x >= dx_blocks) {
    // dalpha / dbeta: column q of the (nwg, C float4) partial array, 16 groups of rows in f64, then the groups in order
    const int ql = threadIdx.x % PR_Q, grp = threadIdx.x / PR_Q;
    const int q = ((int)blockIdx.x - dx_blocks) * PR_Q + ql;        // float4 column of [dalpha lo | dbeta lo | dalpha hi | dbeta hi]
    double a[4] = {0.0, 0.0, 0.0, 0.0};
    if (q < C) {
      for (int w = grp; w < nwg; w += PR_GROUPS) {
        const F4 p = ld4(ppart + (size_t)w * 4 * C + 4 * q);
#pragma unroll
        for (int i = 0; i < 4; ++i) a[i] += (double)p.v[i];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) sh[4 * threadIdx.x + i] = a[i];
    __syncthreads();
    if (grp == 0 && q < C) {
      F4 res;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double tot = 0.0;
        for (int gq = 0; gq < PR_GROUPS; ++gq) tot += sh[4 * (gq * PR_Q + ql) + i];
        res.v[i] = (float)tot;
      }
      const int section = q / C4, c = 4 * (q % C4);
      float* dst = (section & 1) ? dbeta : dalpha;
      st4(dst + (section >> 1) * C + c, res);
    }
    return;
  }
  double mine = 0.0;
  for (int i = threadIdx.x; i < nwg; i += ROW_NT) mine += tpart[2 * i];
  const double t = block_tree_sum<ROW_NT>(mine, sh);
  const float mu = stats[0], r = stats[2], coef = (float)(t * (double)stats[3]);
  const uint32_t lane = u3d_util::lane_id();
  const int wave = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * ROW_WAVES + wave;
  if (row >= rows) return;
  const long long b = row / G;
  const int j = (int)(row % G);
  const float* xb = x + b * xs;
  const size_t rb = (size_t)b * G;
  F4 xj[SLOTS], al[SLOTS], be[SLOTS], acc[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int c4 = lane + 64 * s;
    const bool on = c4 < C4;
    xj[s] = on ? ld4(xb + (size_t)j * C + 4 * c4) : splat(0.f);
    al[s] = on ? ld4(alpha + 4 * c4) : splat(0.f);
    be[s] = on ? ld4(beta + 4 * c4) : splat(0.f);
    acc[s] = splat(0.f);
  }
  // rows that name j as a neighbour: d = x[j] - x[g], with row g's out, lse and dout
  const int n = G * K;
  const int32_t* pb = ptr + b * (G + 1);
  const int32_t* eb = ent + b * n;
  const int e0 = max(0, min(pb[j], n)), e1 = max(e0, min(pb[j + 1], n));
#pragma unroll 2
  for (int e = e0; e < e1; ++e) {
    const unsigned ev = (unsigned)eb[e] / (unsigned)K;
    const int g = ev < (unsigned)G ? (int)ev : j;
    const float* xg = xb + (size_t)g * C;
    const float* og = out + (rb + g) * 2 * C;
    const float* lg = lse + (rb + g) * C;
    const float* dg = dout + (rb + g) * 2 * C;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int c4 = lane + 64 * s;
      if (c4 < C4) {
        const F4 a = ld4(xg + 4 * c4), o = ld4(og + 4 * c4), ls = ld4(lg + 4 * c4), g1 = ld4(dg + 4 * c4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float d = xj[s].v[i] - a.v[i];
          const float gv = grad_v(al[s].v[i], be[s].v[i], d * r, ls.v[i], o.v[i], g1.v[i]);
          acc[s].v[i] += fmaf(gv * al[s].v[i], r, -(coef * (d - mu)));
        }
      }
    }
  }
  // minus row j's own K terms
  const int jn = load_neighbours(idx + row * K, K, j, G, lane);
  F4 o[SLOTS], ls[SLOTS], g1[SLOTS];
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int c4 = lane + 64 * s;
    const bool on = c4 < C4;
    o[s] = on ? ld4(out + (size_t)row * 2 * C + 4 * c4) : splat(0.f);
    ls[s] = on ? ld4(lse + (size_t)row * C + 4 * c4) : splat(0.f);
    g1[s] = on ? ld4(dout + (size_t)row * 2 * C + 4 * c4) : splat(0.f);
  }
  for (int k = 0; k < K; ++k) {
    const float* xn = xb + (size_t)lane_value(jn, k) * C;
#pragma unroll
    for (int s = 0; s < SLOTS; ++s) {
      const int c4 = lane + 64 * s;
      if (c4 < C4) {
        const F4 a = ld4(xn + 4 * c4);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float d = a.v[i] - xj[s].v[i];
          const float gv = grad_v(al[s].v[i], be[s].v[i], d * r, ls[s].v[i], o[s].v[i], g1[s].v[i]);
          acc[s].v[i] -= fmaf(gv * al[s].v[i], r, -(coef * (d - mu)));
        }
      }
    }
  }
#pragma unroll
  for (int s = 0; s < SLOTS; ++s) {
    const int c4 = lane + 64 * s;
    if (c4 < C4) {
      const F4 ah = ld4(alpha + C + 4 * c4), g2 = ld4(dout + (size_t)row * 2 * C + C + 4 * c4);
      F4 res;
#pragma unroll
      for (int i = 0; i < 4; ++i) res.v[i] = fmaf(ah.v[i], g2.v[i], acc[s].v[i]);
      st4(dx + (size_t)row * C + 4 * c4, res);
    }
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct Plan {
  long long rows;
  int stat_wg, bwd_wg, row_blocks, param_blocks;
};

int plan(int B, int G, int K, int C, Plan& p) {
  if (B < 1 || G < 1 || K < 1 || C < 1) return 1;
  if (G > U3D_LNP_MAX_GROUPS || K < 2 || K > U3D_LNP_MAX_K || (C & 3) || C > U3D_LNP_MAX_CHANNELS) return 2;
  p.rows = (long long)B * G;
  if (p.rows > (1ll << 22)) return 2;
  p.row_blocks = u3d_util::blocks(p.rows, ROW_WAVES);
  p.stat_wg = p.row_blocks < STAT_MAX_WG ? p.row_blocks : STAT_MAX_WG;
  const int bw = u3d_util::blocks(p.rows, BWD_WAVES);
  p.bwd_wg = bw < BWD_MAX_WG ? bw : BWD_MAX_WG;
  p.param_blocks = u3d_util::blocks(C, PR_Q);
  return 0;
}

size_t fwd_scratch(const Plan& p) { return (size_t)p.stat_wg * 2 * sizeof(double); }
size_t bwd_scratch(const Plan& p, int C) { return (size_t)p.bwd_wg * (2 * sizeof(double) + (size_t)4 * C * sizeof(float)); }

}  // namespace

extern "C" {

int u3d_lnp_abi_version(void) { return U3D_LNP_ABI_VERSION; }

size_t u3d_lnp_scratch_bytes(int B, int G, int K, int C, int backward) {
  Plan p;
  if (plan(B, G, K, C, p)) return 0;
  return backward ? bwd_scratch(p, C) : fwd_scratch(p);
}

int u3d_lnp_neighbours(const int32_t* idx, int32_t* ptr, int32_t* ent, int B, int G, int K, void* stream) {
  if (bad_ptr(idx) || bad_ptr(ptr) || bad_ptr(ent)) return 1;
  Plan p;
  if (const int rc = plan(B, G, K, 4, p)) return rc;
  hipLaunchKernelGGL(lnp_neighbours_kernel, dim3(B), dim3(NB_NT), 0, (hipStream_t)stream, idx, ptr, ent, G, K);
  return u3d_util::launched();
}

int u3d_lnp_fwd(const float* x, long long x_batch_stride, const int32_t* idx, const float* alpha, const float* beta, float* out,
                float* lse, float* stats, void* scratch, int B, int G, int K, int C, float eps, void* stream) {
  if (bad_ptr(x) || bad_ptr(idx) || bad_ptr(alpha) || bad_ptr(beta) || bad_ptr(out) || bad_ptr(lse) || bad_ptr(stats) || bad_ptr(scratch)) return 1;
  Plan p;
  if (const int rc = plan(B, G, K, C, p)) return rc;
  if (x_batch_stride < (long long)G * C || (x_batch_stride & 3) || !(eps >= 0.f) || !(eps < INFINITY)) return 1;
  double* part = static_cast<double*>(scratch);
  hipLaunchKernelGGL(lnp_stats_kernel, dim3(p.stat_wg), dim3(ROW_NT), 0, (hipStream_t)stream, x, x_batch_stride, idx, part, G, K, C,
                     p.rows, p.stat_wg);
  if (const int rc = u3d_util::launched()) return rc;
  hipLaunchKernelGGL(lnp_fwd_kernel, dim3(p.row_blocks), dim3(ROW_NT), 0, (hipStream_t)stream, x, x_batch_stride, idx, alpha, beta, out,
                     lse, stats, part, G, K, C, p.rows, p.stat_wg, (double)p.rows * K * C, eps);
  return u3d_util::launched();
}

int u3d_lnp_bwd(const float* x, long long x_batch_stride, const int32_t* idx, const int32_t* ptr, const int32_t* ent,
                const float* alpha, const float* beta, const float* out, const float* lse, const float* stats, const float* dout,
                float* dx, float* dalpha, float* dbeta, void* scratch, int B, int G, int K, int C, void* stream) {
  if (bad_ptr(x) || bad_ptr(idx) || bad_ptr(ptr) || bad_ptr(ent) || bad_ptr(alpha) || bad_ptr(beta) || bad_ptr(out) || bad_ptr(lse) ||
      bad_ptr(stats) || bad_ptr(dout) || bad_ptr(dx) || bad_ptr(dalpha) || bad_ptr(dbeta) || bad_ptr(scratch))
    return 1;
  Plan p;
  if (const int rc = plan(B, G, K, C, p)) return rc;
  if (x_batch_stride < (long long)G * C || (x_batch_stride & 3)) return 1;
  double* tpart = static_cast<double*>(scratch);
  float* ppart = reinterpret_cast<float*>(tpart + 2 * (size_t)p.bwd_wg);
  hipLaunchKernelGGL(lnp_bwd_partial_kernel, dim3(p.bwd_wg), dim3(BWD_NT), 0, (hipStream_t)stream, x, x_batch_stride, idx, alpha, beta,
                     out, lse, stats, dout, tpart, ppart, G, K, C, p.rows, p.bwd_wg);
  if (const int rc = u3d_util::launched()) return rc;
  hipLaunchKernelGGL(lnp_bwd_dx_kernel, dim3(p.row_blocks + p.param_blocks), dim3(ROW_NT), 0, (hipStream_t)stream, x, x_batch_stride,
                     idx, ptr, ent, alpha, beta, out, lse, stats, dout, tpart, ppart, dx, dalpha, dbeta, G, K, C, p.rows, p.bwd_wg,
                     p.row_blocks);
  return u3d_util::launched();
}

}  // extern "C"
