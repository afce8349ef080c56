// The two operators of a Mamba block around its selective scan, for gfx950, forward and backward; see include/unipre3d_mambaops.h.
//
// Causal depthwise conv1d (+ SiLU).  One wave owns one (batch, channel) row and walks it in chunks of 64 R steps (R = 1 .. 4 from L, as
// the scan's passes); inside a chunk lane i owns steps i, 64 + i, ..: every load and store is one coalesced dword per lane, which is all
// a row of length 129 allows (its base is only 4-byte aligned).  The W - 1 earlier taps of a step are the neighbouring lanes' loads,
// moved one lane at a time with wave_shr:1; the lanes at the left edge of a 64-step group take the three steps in front of it, which the
// wave holds already (the group before, in registers; zero in front of the row), through the DPP `old` operand, so the forward reads
// every x exactly once and uses no LDS.  The backward walks the chunks last to first: it recomputes pre from x (left halo: the group
// before, or three global loads at the chunk's left edge), forms dpre, and takes dpre at the W - 1 LATER steps from the lanes above
// (wave_shl:1) and, at the right edge, from the group or chunk processed just before.  dweight / dbias accumulate per lane over the
// row, are summed across the wave in one fixed order, written per (b, d) and summed over b by a second launch.
//
// Residual add + LayerNorm / RMSNorm.  One wave per row, the row in registers (float4 per lane where N and the pointers allow, a dword
// otherwise); sums across the wave by DPP in one fixed order.  LayerNorm's mean is taken of r - r[0] (exact where the row's values are
// close to each other, which is where a plain sum loses the variance) and the variance of the centred values.  The backward gives each
// wave a contiguous run of rows, keeps dweight / dbias in registers over the run -- in double, xhat included: they are sums over all M
// rows and are rounded to fp32 once, by the reduce -- and writes one partial row per wave; a second launch (16 waves per 64 columns,
// each over a contiguous run of partial rows, then across the 16 through LDS) sums the partials in a fixed order.
// No float atomics anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unipre3d_mambaops.h"
#include "u3d_util.h"

namespace {

using namespace u3d_util;

constexpr int NT = 256;                   // threads per workgroup (four waves)
constexpr int NW = NT / 64;
constexpr int MAXW = U3D_CCONV_MAX_WIDTH;
constexpr int NPAR = MAXW + 1;            // conv partials per (b,d): dweight by tap distance 0 .. 3, dbias
constexpr int MAXN = U3D_ADDNORM_MAX_N;
constexpr int ROWS_PER_WAVE = 4;          // norm backward: rows a wave owns before more rows mean more waves ...
constexpr int MAX_BWD_WAVES = 2048;       // ... up to this many (two per SIMD of 256 CUs); beyond it the runs grow
constexpr int RT = 1024;                  // threads of the norm's reduce workgroup (16 waves over 64 columns)

inline int bwd_waves(int M) {
  if (M < 1) return 0;
  const int want = (M + ROWS_PER_WAVE - 1) / ROWS_PER_WAVE;
  return want < MAX_BWD_WAVES ? want : MAX_BWD_WAVES;
}

__device__ __forceinline__ float from_below(float edge, float v) { return dpp_f<0x138, 0xf>(edge, v); }   // wave_shr:1, lane 0 := edge
__device__ __forceinline__ float from_above(float edge, float v) { return dpp_f<0x130, 0xf>(edge, v); }   // wave_shl:1, lane 63 := edge

// ---- causal conv ---------------------------------------------------------------------------------------------------------------------
struct ConvArgs {
  const float *x, *w, *bias, *dout;
  float *out, *dx, *par;
  long long sb, sd;
  size_t rows;
  int D, L, W, silu;
};

// wk[k] multiplies x[l - k]: weight[d, W-1-k], 0 for k >= W
__device__ __forceinline__ void load_taps(const ConvArgs& p, int d, float (&wk)[MAXW]) {
#pragma unroll
  for (int k = 0; k < MAXW; ++k) wk[k] = k < p.W ? p.w[(size_t)d * p.W + (p.W - 1 - k)] : 0.f;
}
// taps in ascending w, as the formula is written
__device__ __forceinline__ float pre_act(const float (&wk)[MAXW], float bias, float x0, float x1, float x2, float x3) {
  return fmaf(wk[0], x0, fmaf(wk[1], x1, fmaf(wk[2], x2, fmaf(wk[3], x3, bias))));
}

template <int R>
__global__ __launch_bounds__(NT) void cconv_fwd_kernel(const ConvArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * NW + wave;
  if (row >= p.rows) return;                              // (wave-uniform; no workgroup barrier in this kernel)
  const int L = p.L, d = (int)(row % p.D);
  const float* x = p.x + (long long)(row / p.D) * p.sb + (long long)d * p.sd;
  float* out = p.out + row * L;
  float wk[MAXW];
  load_taps(p, d, wk);
  const float bias = p.bias ? p.bias[d] : 0.f;
  float h0 = 0.f, h1 = 0.f, h2 = 0.f;                     // x one, two, three steps in front of the next 64-step group
  for (int l0 = 0; l0 < L; l0 += 64 * R) {
    float x0[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {                         // steps at or beyond L load element 0 (always there) and select 0: no branch
      const int l = l0 + 64 * r + lane;
      const float v = x[l < L ? l : 0];
      x0[r] = l < L ? v : 0.f;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int l = l0 + 64 * r + lane;
      const float x1 = from_below(h0, x0[r]), x2 = from_below(h1, x1), x3 = from_below(h2, x2);
      float v = pre_act(wk, bias, x0[r], x1, x2, x3);
      if (p.silu) v *= sigmoid_f(v);
      if (l < L) out[l] = v;
      h0 = lane_f<63>(x0[r]); h1 = lane_f<62>(x0[r]); h2 = lane_f<61>(x0[r]);
    }
  }
}

template <int R>
__global__ __launch_bounds__(NT) void cconv_bwd_kernel(const ConvArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const size_t row = (size_t)blockIdx.x * NW + wave;
  if (row >= p.rows) return;
  const int L = p.L, d = (int)(row % p.D);
  const float* x = p.x + (long long)(row / p.D) * p.sb + (long long)d * p.sd;
  const float* dout = p.dout + row * L;
  float* dx = p.dx + row * L;
  float wk[MAXW], aw[MAXW] = {0.f, 0.f, 0.f, 0.f}, ab = 0.f;
  load_taps(p, d, wk);
  const float bias = p.bias ? p.bias[d] : 0.f;
  float c0 = 0.f, c1 = 0.f, c2 = 0.f;                     // dpre one, two, three steps past the chunk's right edge (0 past the row)
  for (int l0 = (L - 1) / (64 * R) * (64 * R); l0 >= 0; l0 -= 64 * R) {
    float x0[R], dp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int l = l0 + 64 * r + lane;
      const float v = x[l < L ? l : 0], g = dout[l < L ? l : 0];
      x0[r] = l < L ? v : 0.f;
      dp[r] = l < L ? g : 0.f;
    }
    const int hl = l0 - 1 - lane;                         // lanes 0 .. 2: the three steps in front of the chunk
    const bool halo = lane < MAXW - 1 && hl >= 0;
    const float hx = x[halo ? hl : 0], hv = halo ? hx : 0.f;
    float h0 = lane_f<0>(hv), h1 = lane_f<1>(hv), h2 = lane_f<2>(hv);
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const float x1 = from_below(h0, x0[r]), x2 = from_below(h1, x1), x3 = from_below(h2, x2);
      if (p.silu) {
        const float v = pre_act(wk, bias, x0[r], x1, x2, x3), s = sigmoid_f(v);
        dp[r] *= s * (1.f + v * (1.f - s));
      }
      ab += dp[r];
      aw[0] = fmaf(x0[r], dp[r], aw[0]);
      aw[1] = fmaf(x1, dp[r], aw[1]);
      aw[2] = fmaf(x2, dp[r], aw[2]);
      aw[3] = fmaf(x3, dp[r], aw[3]);
      h0 = lane_f<63>(x0[r]); h1 = lane_f<62>(x0[r]); h2 = lane_f<61>(x0[r]);
    }
#pragma unroll
    for (int r = R - 1; r >= 0; --r) {
      const int l = l0 + 64 * r + lane;
      const float d1 = from_above(c0, dp[r]), d2 = from_above(c1, d1), d3 = from_above(c2, d2);
      const float v = fmaf(wk[3], d3, fmaf(wk[2], d2, fmaf(wk[1], d1, wk[0] * dp[r])));
      if (l < L) dx[l] = v;
      c0 = lane_f<0>(dp[r]); c1 = lane_f<1>(dp[r]); c2 = lane_f<2>(dp[r]);
    }
  }
  float sums[NPAR];
#pragma unroll
  for (int k = 0; k < MAXW; ++k) sums[k] = wave_sum(aw[k]);
  sums[MAXW] = wave_sum(ab);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NPAR; ++k) p.par[row * NPAR + k] = sums[k];
  }
}

// dweight (D,W) and dbias (D) from the per-(b,d) partials, b ascending
__global__ __launch_bounds__(NT) void cconv_reduce_kernel(const float* par, float* dweight, float* dbias, int B, int D, int W) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= D * NPAR) return;
  const int d = i / NPAR, k = i % NPAR;
  float* dst = k < W ? dweight + (size_t)d * W + (W - 1 - k) : k == MAXW && dbias ? dbias + d : nullptr;
  if (!dst) return;
  float sum = 0.f;
  for (int b = 0; b < B; ++b) sum += par[((size_t)b * D + d) * NPAR + k];
  *dst = sum;
}

// ---- add + norm ----------------------------------------------------------------------------------------------------------------------
struct NormArgs {
  const float *x, *res, *w, *b, *dy, *dres, *r, *mean_in, *rstd_in;
  float *y, *r_out, *mean, *rstd, *dx;
  double *dwp, *dbp;                                      // per-wave partial rows of dweight / dbias
  int M, N, rms, nwaves;
  float eps;
};

template <int V>
__device__ __forceinline__ void load_v(const float* p, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = *p;
  }
}
template <int V>
__device__ __forceinline__ void store_v(float* p, const float (&v)[V]) {
  if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else *p = v[0];
}

// lane i holds the V elements from (i + 64 j) V, j < NJ; elements at or beyond N are 0 and are never stored
template <int V, int NJ>
__global__ __launch_bounds__(NT) void addnorm_fwd_kernel(const NormArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int row = blockIdx.x * NW + wave, N = p.N;
  if (row >= p.M) return;                                 // (wave-uniform; no workgroup barrier in this kernel)
  const size_t off = (size_t)row * N;
  float v[NJ][V];
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int e = (lane + 64 * j) * V;
#pragma unroll
    for (int i = 0; i < V; ++i) v[j][i] = 0.f;
    if (e < N) {
      load_v<V>(p.x + off + e, v[j]);
      if (p.res) {
        float t[V];
        load_v<V>(p.res + off + e, t);
#pragma unroll
        for (int i = 0; i < V; ++i) v[j][i] += t[i];
      }
      if (p.r_out) store_v<V>(p.r_out + off + e, v[j]);
    }
  }
  float rstd;
  if (p.rms) {
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
#pragma unroll
      for (int i = 0; i < V; ++i) ss = fmaf(v[j][i], v[j][i], ss);
    }
    rstd = 1.f / sqrtf(wave_sum(ss) / (float)N + p.eps);
  } else {
    const float r0 = lane_f<0>(v[0][0]);                  // the row's first element: the sums below are of r - r0
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = (lane + 64 * j) * V;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        v[j][i] = e < N ? v[j][i] - r0 : 0.f;
        s += v[j][i];
      }
    }
    const float m = wave_sum(s) / (float)N;
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = (lane + 64 * j) * V;
#pragma unroll
      for (int i = 0; i < V; ++i) {
        v[j][i] = e < N ? v[j][i] - m : 0.f;
        ss = fmaf(v[j][i], v[j][i], ss);
      }
    }
    rstd = 1.f / sqrtf(wave_sum(ss) / (float)N + p.eps);
    if (lane == 0) p.mean[row] = r0 + m;
  }
  if (lane == 0) p.rstd[row] = rstd;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int e = (lane + 64 * j) * V;
    if (e < N) {
      float w[V], o[V];
      load_v<V>(p.w + e, w);
#pragma unroll
      for (int i = 0; i < V; ++i) o[i] = v[j][i] * rstd * w[i];
      if (p.b) {
        float b[V];
        load_v<V>(p.b + e, b);
#pragma unroll
        for (int i = 0; i < V; ++i) o[i] = fmaf(v[j][i] * rstd, w[i], b[i]);
      }
      store_v<V>(p.y + off + e, o);
    }
  }
}

template <int V, int NJ>
__global__ __launch_bounds__(NT) void addnorm_bwd_kernel(const NormArgs p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.x * NW + wave, N = p.N;
  if (g >= p.nwaves) return;                              // (wave-uniform; no workgroup barrier in this kernel)
  const int base = p.M / p.nwaves, rem = p.M % p.nwaves;
  const int row0 = g * base + min(g, rem), nrow = base + (g < rem ? 1 : 0);
  float w[NJ][V];
  double aw[NJ][V], ab[NJ][V];                            // sums over rows: in double, rounded once by the reduce
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int e = (lane + 64 * j) * V;
#pragma unroll
    for (int i = 0; i < V; ++i) { w[j][i] = 0.f; aw[j][i] = ab[j][i] = 0.0; }
    if (e < N) load_v<V>(p.w + e, w[j]);
  }
  for (int row = row0; row < row0 + nrow; ++row) {
    const size_t off = (size_t)row * N;
    const float mean = p.rms ? 0.f : p.mean_in[row], rstd = p.rstd_in[row];
    float dy[NJ][V], xh[NJ][V], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = (lane + 64 * j) * V;
#pragma unroll
      for (int i = 0; i < V; ++i) dy[j][i] = xh[j][i] = 0.f;
      if (e < N) {
        load_v<V>(p.dy + off + e, dy[j]);
        load_v<V>(p.r + off + e, xh[j]);
#pragma unroll
        for (int i = 0; i < V; ++i) {
          aw[j][i] = fma((double)dy[j][i], ((double)xh[j][i] - (double)mean) * (double)rstd, aw[j][i]);
          ab[j][i] += (double)dy[j][i];
          xh[j][i] = (xh[j][i] - mean) * rstd;
        }
      }
#pragma unroll
      for (int i = 0; i < V; ++i) {
        const float wdy = w[j][i] * dy[j][i];
        s1 = fmaf(xh[j][i], wdy, s1);
        s2 += wdy;
      }
    }
    const float c1 = wave_sum(s1) / (float)N, c2 = p.rms ? 0.f : wave_sum(s2) / (float)N;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      const int e = (lane + 64 * j) * V;
      float o[V];
#pragma unroll
      for (int i = 0; i < V; ++i) {
        o[i] = (w[j][i] * dy[j][i] - xh[j][i] * c1 - c2) * rstd;
      }
      if (e < N) {
        if (p.dres) {
          float t[V];
          load_v<V>(p.dres + off + e, t);
#pragma unroll
          for (int i = 0; i < V; ++i) o[i] += t[i];
        }
        store_v<V>(p.dx + off + e, o);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    const int e = (lane + 64 * j) * V;
    if (e < N) {
#pragma unroll
      for (int i = 0; i < V; ++i) {
        p.dwp[(size_t)g * N + e + i] = aw[j][i];
        if (p.dbp) p.dbp[(size_t)g * N + e + i] = ab[j][i];
      }
    }
  }
}

// dweight / dbias (N) from the per-wave partial rows: wave k of 16 sums a contiguous run of partial rows in ascending order, then the
// 16 sums are added in ascending k
__global__ __launch_bounds__(RT) void addnorm_reduce_kernel(const double* dwp, const double* dbp, float* dw, float* db, int nwaves, int N) {
  __shared__ double s_sum[2][RT / 64][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + lane;
  const int per = (nwaves + RT / 64 - 1) / (RT / 64), i0 = wave * per, i1 = min(i0 + per, nwaves);
  double a = 0.0, b = 0.0;
  if (n < N) {
#pragma unroll 8
    for (int i = i0; i < i1; ++i) a += dwp[(size_t)i * N + n];
    if (dbp) {
#pragma unroll 8
      for (int i = i0; i < i1; ++i) b += dbp[(size_t)i * N + n];
    }
  }
  s_sum[0][wave][lane] = a;
  s_sum[1][wave][lane] = b;
  __syncthreads();
  if (wave == 0 && n < N) {
    a = b = 0.0;
#pragma unroll
    for (int k = 0; k < RT / 64; ++k) { a += s_sum[0][k][lane]; b += s_sum[1][k][lane]; }
    dw[n] = (float)a;
    if (db) db[n] = (float)b;
  }
}

// V = 4 where N and every pointer allow 16-byte accesses; NJ = the 64-lane groups a row needs, rounded up to an instantiated count
template <bool BWD>
int launch_norm(const NormArgs& p, bool vec, int blocks, hipStream_t st) {
#define U3D_NORM_LAUNCH(V, NJ)                                                                                   \
  do {                                                                                                           \
    if (BWD) hipLaunchKernelGGL((addnorm_bwd_kernel<V, NJ>), dim3(blocks), dim3(NT), 0, st, p);                  \
    else hipLaunchKernelGGL((addnorm_fwd_kernel<V, NJ>), dim3(blocks), dim3(NT), 0, st, p);                      \
  } while (0)
  if (vec) {
    const int items = p.N / 4;
    if (items <= 64) U3D_NORM_LAUNCH(4, 1);
    else if (items <= 128) U3D_NORM_LAUNCH(4, 2);
    else U3D_NORM_LAUNCH(4, 4);
  } else {
    if (p.N <= 64) U3D_NORM_LAUNCH(1, 1);
    else if (p.N <= 256) U3D_NORM_LAUNCH(1, 4);
    else U3D_NORM_LAUNCH(1, 16);
  }
#undef U3D_NORM_LAUNCH
  return launched();
}

int check_conv(int B, int D, int L, int W) {
  if (B < 1 || D < 1 || L < 1) return 1;
  if (W < 2 || W > MAXW) return 2;
  if (((size_t)B * D + NW - 1) / NW > 0x7fffffffull) return 2;
  return 0;
}

}  // namespace

extern "C" {

int u3d_mambaops_abi_version(void) { return U3D_MAMBAOPS_ABI_VERSION; }

int u3d_cconv_chunk_len(int L) { return 64 * steps_per_lane(L); }

size_t u3d_cconv_bwd_scratch_bytes(int B, int D) {
  if (B < 1 || D < 1) return 0;
  return align256((size_t)B * D * NPAR * sizeof(float));
}

int u3d_cconv_fwd(const float* x, const float* weight, const float* bias, float* out, int64_t x_batch_stride, int64_t x_chan_stride,
                  int B, int D, int L, int W, int silu, void* stream) {
  if (!x || !weight || !out || x_batch_stride < 0 || x_chan_stride < 0) return 1;
  if (const int rc = check_conv(B, D, L, W)) return rc;
  ConvArgs p = {};
  p.x = x; p.w = weight; p.bias = bias; p.out = out; p.sb = x_batch_stride; p.sd = x_chan_stride;
  p.rows = (size_t)B * D; p.D = D; p.L = L; p.W = W; p.silu = silu != 0;
  const dim3 grid((unsigned)((p.rows + NW - 1) / NW));
  hipStream_t st = (hipStream_t)stream;
  switch (steps_per_lane(L)) {
    case 1: hipLaunchKernelGGL(cconv_fwd_kernel<1>, grid, dim3(NT), 0, st, p); break;
    case 2: hipLaunchKernelGGL(cconv_fwd_kernel<2>, grid, dim3(NT), 0, st, p); break;
    case 3: hipLaunchKernelGGL(cconv_fwd_kernel<3>, grid, dim3(NT), 0, st, p); break;
    default: hipLaunchKernelGGL(cconv_fwd_kernel<4>, grid, dim3(NT), 0, st, p); break;
  }
  return launched();
}

int u3d_cconv_bwd(const float* x, const float* weight, const float* bias, const float* dout, float* dx, float* dweight, float* dbias,
                  void* scratch, size_t scratch_bytes, int64_t x_batch_stride, int64_t x_chan_stride, int B, int D, int L, int W,
                  int silu, void* stream) {
  if (!x || !weight || !dout || !dx || !dweight || !scratch || x_batch_stride < 0 || x_chan_stride < 0) return 1;
  if (const int rc = check_conv(B, D, L, W)) return rc;
  if (scratch_bytes < u3d_cconv_bwd_scratch_bytes(B, D) || ((uintptr_t)scratch & 255)) return 1;
  if ((size_t)D * NPAR > 0x7fffffffull) return 2;
  ConvArgs p = {};
  p.x = x; p.w = weight; p.bias = bias; p.dout = dout; p.dx = dx; p.par = (float*)scratch; p.sb = x_batch_stride; p.sd = x_chan_stride;
  p.rows = (size_t)B * D; p.D = D; p.L = L; p.W = W; p.silu = silu != 0;
  const dim3 grid((unsigned)((p.rows + NW - 1) / NW));
  hipStream_t st = (hipStream_t)stream;
  switch (steps_per_lane(L)) {
    case 1: hipLaunchKernelGGL(cconv_bwd_kernel<1>, grid, dim3(NT), 0, st, p); break;
    case 2: hipLaunchKernelGGL(cconv_bwd_kernel<2>, grid, dim3(NT), 0, st, p); break;
    case 3: hipLaunchKernelGGL(cconv_bwd_kernel<3>, grid, dim3(NT), 0, st, p); break;
    default: hipLaunchKernelGGL(cconv_bwd_kernel<4>, grid, dim3(NT), 0, st, p); break;
  }
  if (const int rc = launched()) return rc;
  hipLaunchKernelGGL(cconv_reduce_kernel, dim3((D * NPAR + NT - 1) / NT), dim3(NT), 0, st, p.par, dweight, bias ? dbias : nullptr, B, D, W);
  return launched();
}

int u3d_addnorm_max_n(void) { return MAXN; }

int u3d_addnorm_bwd_waves(int M) { return bwd_waves(M); }

size_t u3d_addnorm_bwd_scratch_bytes(int M, int N) {
  if (M < 1 || N < 1 || N > MAXN) return 0;
  return 2 * align256((size_t)bwd_waves(M) * N * sizeof(double));
}

int u3d_addnorm_fwd(const float* x, const float* residual, const float* weight, const float* bias, float* y, float* r_out, float* mean,
                    float* rstd, int M, int N, float eps, int is_rms, void* stream) {
  if (!x || !weight || !y || !rstd || (!is_rms && !mean) || M < 1 || N < 1) return 1;
  if (N > MAXN) return 2;
  NormArgs p = {};
  p.x = x; p.res = residual; p.w = weight; p.b = bias; p.y = y; p.r_out = r_out; p.mean = mean; p.rstd = rstd;
  p.M = M; p.N = N; p.rms = is_rms != 0; p.eps = eps;
  const bool vec = N % 4 == 0 && aligned16(x) && aligned16(residual) && aligned16(weight) && aligned16(bias) && aligned16(y) && aligned16(r_out);
  return launch_norm<false>(p, vec, (M + NW - 1) / NW, (hipStream_t)stream);
}

int u3d_addnorm_bwd(const float* dy, const float* dres, const float* r, const float* weight, const float* mean, const float* rstd,
                    float* dx, float* dweight, float* dbias, void* scratch, size_t scratch_bytes, int M, int N, int is_rms, void* stream) {
  if (!dy || !r || !weight || !rstd || (!is_rms && !mean) || !dx || !dweight || !scratch || M < 1 || N < 1) return 1;
  if (N > MAXN) return 2;
  if (scratch_bytes < u3d_addnorm_bwd_scratch_bytes(M, N) || ((uintptr_t)scratch & 255)) return 1;
  const int nwaves = bwd_waves(M);
  const size_t part_bytes = align256((size_t)nwaves * N * sizeof(double));
  NormArgs p = {};
  p.dy = dy; p.dres = dres; p.r = r; p.w = weight; p.mean_in = mean; p.rstd_in = rstd; p.dx = dx;
  p.dwp = (double*)scratch; p.dbp = dbias ? (double*)((char*)scratch + part_bytes) : nullptr;
  p.M = M; p.N = N; p.rms = is_rms != 0; p.nwaves = nwaves;
  const bool vec = N % 4 == 0 && aligned16(dy) && aligned16(dres) && aligned16(r) && aligned16(weight) && aligned16(dx);
  hipStream_t st = (hipStream_t)stream;
  if (const int rc = launch_norm<true>(p, vec, (nwaves + NW - 1) / NW, st)) return rc;
  hipLaunchKernelGGL(addnorm_reduce_kernel, dim3((N + 63) / 64), dim3(RT), 0, st, p.dwp, p.dbp, dweight, dbias, nwaves, N);
  return launched();
}

}  // extern "C"
