// libunipre3d_local_grouper.so: the LocalGrouper of PointMLP and PCM (gathers, group-mean or anchor subtraction, one std per batch element,
// affine, cat with the anchor's feature), fp32, gfx950, wave64.
// include/unipre3d_local_grouper.h states what is computed; DESIGN.md section 8 the cut into kernels and the order of every reduction.
//
// One wave owns one (b, s) row in the forward kernels and in the first backward kernel, and one (b, j) source point in the second.  Its lanes
// run over channels (c = lane, lane + 64, ...), except where the forward writes the row: there they run over the row's K C outputs in storage
// order, so the one write of `out` is contiguous in either layout.  The row's K neighbour indices sit in lanes 0 .. K-1 and are handed round
// with v_readlane (k uniform) or ds_bpermute (k per lane).  Every loop has a wave-uniform trip count; the channel predicate is applied inside.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "u3d_group.h"
#include "u3d_util.h"
#include "unipre3d_local_grouper.h"

namespace {

using u3d_group::lane_value;
using u3d_group::load_neighbours;      // (idx_row, K, a, N, lane): lane k < K has neighbour k of row s, the anchor a where idx is outside [0, N)
using u3d_util::bad_ptr;
using u3d_util::block_tree_sum;

constexpr int ROW_NT = 256, ROW_WAVES = 4;       // stats / forward / dpoints kernels: four rows per workgroup
constexpr int STAT_MAX_WG = 128;                 // per batch element: partials of (sum d, sum d^2), one double2 per workgroup
constexpr int BWD_NT = 512, BWD_WAVES = 8;       // first backward kernel: eight rows per workgroup pass
constexpr int BWD_MAX_WG = 32;                   // per batch element: partials of T_b and of the 2 (D + A) parameter sums
constexpr int LIST_NT = 1024, LIST_WAVES = 16;
constexpr int PR_Q = 16, PR_GROUPS = 16;         // parameter reduce: 16 columns x 16 groups of partial rows per workgroup
constexpr int MAX_CN = U3D_LOCAL_GROUPER_MAX_CHANNELS + 3;
constexpr int SLOTS = (MAX_CN + 63) / 64;                            // channels per lane among the D + A normalised ones
constexpr int DSLOTS = U3D_LOCAL_GROUPER_MAX_CHANNELS / 64;          // ... among the D feature channels
enum { NORM_NONE = 0, NORM_CENTER = 1, NORM_ANCHOR = 2 };

// one batch element's sources: points through its strides, xyz behind it as channels D .. D+2
struct Src {
  const float* pts;
  const float* xyz;
  long long sp, sc;
  int D;
};
__device__ __forceinline__ float src_at(const Src& s, int j, int c) {
  return c < s.D ? s.pts[(long long)j * s.sp + (long long)c * s.sc] : s.xyz[3 * j + (c - s.D)];
}
__device__ __forceinline__ int fps_of(const int32_t* fps_b, int s, int N) {      // anchor s; outside [0, N): point s
  if (fps_b == nullptr) return s;
  const int v = fps_b[s];
  return ((unsigned)v < (unsigned)N) ? v : s;
}

// ---- inverse lists (u3d_group.h) ------------------------------------------------------------------------------------------------
// target of entry e of a table with K entries per anchor: what it names, or the anchor (tab == nullptr: the identity fps)
struct ListTarget {
  const int32_t* tab;
  const int32_t* fps_b;
  int K, N;
  __device__ __forceinline__ int operator()(int e) const {
    const int v = tab != nullptr ? tab[e] : -1;
    return ((unsigned)v < (unsigned)N) ? v : fps_of(fps_b, e / K, N);
  }
};

// both tables of a batch element by one workgroup: the neighbours', then the anchors' with the same cursors and scan words
__global__ __launch_bounds__(LIST_NT) void lg_list_build_kernel(const int32_t* __restrict__ fps, const int32_t* __restrict__ idx,
                                                                int32_t* ptr, int32_t* fptr, int32_t* cur, int32_t* tmpe, int32_t* tmpf,
                                                                int N, int S, int K) {
  __shared__ uint32_t wt[LIST_WAVES];
  const size_t b = blockIdx.x;
  const int32_t* fps_b = fps != nullptr ? fps + b * S : nullptr;
  u3d_group::build_lists<LIST_NT, LIST_WAVES, false>(ListTarget{idx + b * S * K, fps_b, K, N}, S * K, N, ptr + b * (N + 1), cur + b * N,
                                                     tmpe + b * S * K, wt);
  __threadfence();
  __syncthreads();
  u3d_group::build_lists<LIST_NT, LIST_WAVES, false>(ListTarget{fps_b, fps_b, 1, N}, S, N, fptr + b * (N + 1), cur + b * N, tmpf + b * S, wt);
}

__global__ __launch_bounds__(ROW_NT) void lg_list_sort_kernel(const int32_t* __restrict__ ptr, const int32_t* __restrict__ fptr,
                                                              const int32_t* __restrict__ tmpe, const int32_t* __restrict__ tmpf,
                                                              int32_t* __restrict__ ent, int32_t* __restrict__ fent, int N, int S, int K,
                                                              long long rows) {
  const uint32_t lane = u3d_util::lane_id();
  const long long row = (long long)blockIdx.x * ROW_WAVES + (threadIdx.x >> 6);
  if (row >= rows) return;
  const long long b = row / N;
  const int j = (int)(row % N), n = S * K;
  const int32_t* pb = ptr + b * (N + 1);
  const int32_t* fb = fptr + b * (N + 1);
  const int e0 = max(0, min(pb[j], n)), e1 = max(e0, min(pb[j + 1], n));
  u3d_group::rank_list(tmpe + b * n, ent + b * n, e0, e1, lane);
  const int f0 = max(0, min(fb[j], S)), f1 = max(f0, min(fb[j + 1], S));
  u3d_group::rank_list(tmpf + b * S, fent + b * S, f0, f1, lane);
}

// ---- forward --------------------------------------------------------------------------------------------------------------------
struct Dims {
  int N, S, K, D, Cn, C;     // Cn = D + A, C = 2 D + A
};

__global__ __launch_bounds__(ROW_NT) void lg_stats_kernel(const float* __restrict__ xyz, const float* __restrict__ points, long long pb,
                                                          long long pp, long long pc, const int32_t* __restrict__ fps,
                                                          const int32_t* __restrict__ idx, float* __restrict__ mean,
                                                          double* __restrict__ part, Dims dm, int normalize, int nwg) {
  __shared__ double sh[2][ROW_WAVES];
  const uint32_t lane = u3d_util::lane_id();
  const int wave = threadIdx.x >> 6;
  const size_t b = blockIdx.x / nwg;
  const int w = blockIdx.x % nwg;
  const Src sr{points + b * pb, xyz + b * dm.N * 3, pp, pc, dm.D};
  const int32_t* fps_b = fps != nullptr ? fps + b * dm.S : nullptr;
  const float kf = (float)dm.K;
  double s1 = 0.0, s2 = 0.0;
  for (int s = w * ROW_WAVES + wave; s < dm.S; s += nwg * ROW_WAVES) {
    const int a = fps_of(fps_b, s, dm.N);
    const int jn = load_neighbours(idx + (b * dm.S + s) * dm.K, dm.K, a, dm.N, lane);
    float* mrow = mean + (b * dm.S + s) * dm.Cn;
    for (int c0 = 0; c0 < dm.Cn; c0 += 64) {
      const int c = c0 + (int)lane;
      const bool on = c < dm.Cn;
      float m = 0.f;
      if (normalize == NORM_CENTER) {
        float sum = 0.f;
        for (int k = 0; k < dm.K; ++k) {
          const int j = lane_value(jn, k);
          if (on) sum += src_at(sr, j, c);
        }
        m = sum / kf;
      } else if (on) {
        m = src_at(sr, a, c);
      }
      if (on) mrow[c] = m;
      for (int k = 0; k < dm.K; ++k) {
        const int j = lane_value(jn, k);
        if (on) {
          const double d = (double)(src_at(sr, j, c) - m);
          s1 += d;
          s2 += d * d;
        }
      }
    }
  }
  u3d_group::wave_sums_to_lds<ROW_WAVES, 2>(s1, s2, sh, lane, wave);
  __syncthreads();
  u3d_group::block_sums_to_part<ROW_WAVES, 2>(sh, part, 2 * (size_t)blockIdx.x);
}

__global__ __launch_bounds__(ROW_NT) void lg_fwd_kernel(const float* __restrict__ xyz, const float* __restrict__ points, long long pb,
                                                        long long pp, long long pc, const int32_t* __restrict__ fps,
                                                        const int32_t* __restrict__ idx, const float* __restrict__ alpha,
                                                        const float* __restrict__ beta, float* __restrict__ out, float* __restrict__ new_xyz,
                                                        const float* __restrict__ mean, float* __restrict__ stats,
                                                        const double* __restrict__ part, Dims dm, int normalize, int cf, int nstat, int rb,
                                                        float eps) {
  __shared__ double sh[ROW_NT];
  const size_t b = blockIdx.x / rb;
  const int blk = blockIdx.x % rb;
  float r = 1.f;
  if (normalize != NORM_NONE) {
    // every workgroup of a batch element sums the same partials in the same tree: mu, s and r have the same bits everywhere
    const bool has = (int)threadIdx.x < nstat;
    const double* pt = part + 2 * b * nstat;
    const double S1 = block_tree_sum<ROW_NT>(has ? pt[2 * threadIdx.x] : 0.0, sh);
    const double S2 = block_tree_sum<ROW_NT>(has ? pt[2 * threadIdx.x + 1] : 0.0, sh);
    const double n = (double)dm.S * dm.K * dm.Cn;
    r = u3d_group::norm_stats(S1, S2, n, eps, blk, stats + 4 * b);
  }
  const uint32_t lane = u3d_util::lane_id();
  const int s = blk * ROW_WAVES + (int)(threadIdx.x >> 6);
  if (s >= dm.S) return;
  const Src sr{points + b * pb, xyz + b * dm.N * 3, pp, pc, dm.D};
  const int a = fps_of(fps != nullptr ? fps + b * dm.S : nullptr, s, dm.N);
  const int jn = load_neighbours(idx + (b * dm.S + s) * dm.K, dm.K, a, dm.N, lane);
  if (lane < 3) new_xyz[(b * dm.S + s) * 3 + lane] = sr.xyz[3 * a + lane];
  const int total = dm.K * dm.C;
  float* orow = out + (b * dm.S + s) * total;
  const float* mrow = mean + (b * dm.S + s) * dm.Cn;       // (not dereferenced with normalize = none)
  for (int o0 = 0; o0 < total; o0 += 64) {
    const int o = o0 + (int)lane;
    const bool on = o < total;
    const unsigned oo = on ? (unsigned)o : 0u;
    int k, c;
    if (cf) { c = (int)(oo / (unsigned)dm.K); k = (int)(oo - (unsigned)c * dm.K); }
    else { k = (int)(oo / (unsigned)dm.C); c = (int)(oo - (unsigned)k * dm.C); }
    const int j = __shfl(jn, k);
    if (on) {
      float v;
      if (c < dm.Cn) {
        v = src_at(sr, j, c);
        if (normalize != NORM_NONE) v = fmaf(alpha[c], (v - mrow[c]) * r, beta[c]);
      } else {
        v = src_at(sr, a, c - dm.Cn);
      }
      orow[o] = v;
    }
  }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BWD_NT) void lg_bwd_partial_kernel(const float* __restrict__ xyz, const float* __restrict__ points, long long pb,
                                                                long long pp, long long pc, const int32_t* __restrict__ fps,
                                                                const int32_t* __restrict__ idx, const float* __restrict__ alpha,
                                                                const float* __restrict__ mean, const float* __restrict__ stats,
                                                                const float* __restrict__ dout, double* __restrict__ tpart,
                                                                float* __restrict__ ppart, float* __restrict__ gysum, float* __restrict__ dsum,
                                                                float* __restrict__ gasum, Dims dm, int normalize, int dcf, int nwg) {
  __shared__ float shp[2 * MAX_CN];      // [dalpha | dbeta], Cn each
  __shared__ double sht[1][BWD_WAVES];
  const uint32_t lane = u3d_util::lane_id();
  const int wave = threadIdx.x >> 6;
  const size_t b = blockIdx.x / nwg;
  const int w = blockIdx.x % nwg;
  const Src sr{points + b * pb, xyz + b * dm.N * 3, pp, pc, dm.D};
  const int32_t* fps_b = fps != nullptr ? fps + b * dm.S : nullptr;
  const int dk = dcf ? 1 : dm.C, dc = dcf ? dm.K : 1;
  const bool norm = normalize != NORM_NONE;
  const float r = norm ? stats[4 * b + 2] : 1.f;
  float da[SLOTS], db[SLOTS];
#pragma unroll
  for (int i = 0; i < SLOTS; ++i) da[i] = db[i] = 0.f;
  double t = 0.0;
  for (int s = w * BWD_WAVES + wave; s < dm.S; s += nwg * BWD_WAVES) {
    const size_t row = b * dm.S + s;
    const float* drow = dout + row * dm.K * dm.C;
    if (norm) {
      const int a = fps_of(fps_b, s, dm.N);
      const int jn = load_neighbours(idx + row * dm.K, dm.K, a, dm.N, lane);
#pragma unroll
      for (int i = 0; i < SLOTS; ++i) {
        if (64 * i < dm.Cn) {
          const int c = 64 * i + (int)lane;
          const bool on = c < dm.Cn;
          const float m = on ? mean[row * dm.Cn + c] : 0.f, al = on ? alpha[c] : 0.f;
          float gys = 0.f, ds = 0.f;
          for (int k = 0; k < dm.K; ++k) {
            const int j = lane_value(jn, k);
            if (on) {
              const float gy = drow[k * dk + c * dc];
              const float d = src_at(sr, j, c) - m;
              gys += gy;
              ds += d;
              da[i] = fmaf(gy, d * r, da[i]);
              db[i] += gy;
              t += (double)((al * gy) * d);
            }
          }
          if (on) {
            gysum[row * dm.Cn + c] = gys;
            dsum[row * dm.Cn + c] = ds;
          }
        }
      }
    }
    for (int c0 = 0; c0 < dm.D; c0 += 64) {
      const int c = c0 + (int)lane;
      if (c < dm.D) {
        float ga = 0.f;
        for (int k = 0; k < dm.K; ++k) ga += drow[k * dk + (dm.Cn + c) * dc];
        gasum[row * dm.D + c] = ga;
      }
    }
  }
  if (!norm) return;
  u3d_group::wave_sums_to_lds<BWD_WAVES, 1>(t, 0.0, sht, lane, wave);
  // the eight waves' rows, added in wave order
  for (int wv = 0; wv < BWD_WAVES; ++wv) {
    if (wave == wv) {
#pragma unroll
      for (int i = 0; i < SLOTS; ++i) {
        const int c = 64 * i + (int)lane;
        if (c < dm.Cn) {
          if (wv == 0) { shp[c] = da[i]; shp[dm.Cn + c] = db[i]; }
          else { shp[c] += da[i]; shp[dm.Cn + c] += db[i]; }
        }
      }
    }
    __syncthreads();
  }
  for (int i = threadIdx.x; i < 2 * dm.Cn; i += BWD_NT) ppart[(size_t)blockIdx.x * 2 * dm.Cn + i] = shp[i];
  u3d_group::block_sums_to_part<BWD_WAVES, 1>(sht, tpart, 2 * (size_t)blockIdx.x);      // (T_b's part, 0)
}

__global__ __launch_bounds__(ROW_NT) void lg_bwd_dpoints_kernel(const float* __restrict__ points, long long pb, long long pp, long long pc,
                                                                const int32_t* __restrict__ ptr, const int32_t* __restrict__ ent,
                                                                const int32_t* __restrict__ fptr, const int32_t* __restrict__ fent,
                                                                const float* __restrict__ alpha, const float* __restrict__ mean,
                                                                const float* __restrict__ stats, const float* __restrict__ dout,
                                                                const double* __restrict__ tpart, const float* __restrict__ ppart,
                                                                const float* __restrict__ gysum, const float* __restrict__ dsum,
                                                                const float* __restrict__ gasum, float* __restrict__ dpoints, long long gb,
                                                                long long gp, long long gc, float* __restrict__ dalpha,
                                                                float* __restrict__ dbeta, Dims dm, int normalize, int dcf, int nwg, int rb,
                                                                int dx_blocks, int npart) {
  __shared__ double sh[ROW_NT];
  if ((int)blockIdx.x >= dx_blocks) {
    // dalpha / dbeta: column q of the (npart, 2 Cn) partial array, 16 groups of rows in f64, then the groups in order
    const int ql = threadIdx.x % PR_Q, grp = threadIdx.x / PR_Q;
    const int q = ((int)blockIdx.x - dx_blocks) * PR_Q + ql;
    double x = 0.0;
    if (q < 2 * dm.Cn)
      for (int i = grp; i < npart; i += PR_GROUPS) x += (double)ppart[(size_t)i * 2 * dm.Cn + q];
    sh[threadIdx.x] = x;
    __syncthreads();
    if (grp == 0 && q < 2 * dm.Cn) {
      double tot = 0.0;
      for (int g = 0; g < PR_GROUPS; ++g) tot += sh[g * PR_Q + ql];
      if (q < dm.Cn) dalpha[q] = (float)tot;
      else dbeta[q - dm.Cn] = (float)tot;
    }
    return;
  }
  const size_t b = blockIdx.x / rb;
  const int blk = blockIdx.x % rb;
  const bool norm = normalize != NORM_NONE;
  float mu = 0.f, r = 1.f, coef = 0.f;
  if (norm) {
    const double t = block_tree_sum<ROW_NT>((int)threadIdx.x < nwg ? tpart[2 * (b * nwg + threadIdx.x)] : 0.0, sh);
    mu = stats[4 * b];
    r = stats[4 * b + 2];
    coef = (float)(t * (double)stats[4 * b + 3]);
  }
  const uint32_t lane = u3d_util::lane_id();
  const int j = blk * ROW_WAVES + (int)(threadIdx.x >> 6);
  if (j >= dm.N) return;
  const float kf = (float)dm.K, kmu = kf * mu;
  const int dk = dcf ? 1 : dm.C, dc = dcf ? dm.K : 1;
  float acc[DSLOTS], xj[DSLOTS], al[DSLOTS];
#pragma unroll
  for (int i = 0; i < DSLOTS; ++i) {
    const int c = 64 * i + (int)lane;
    const bool on = c < dm.D && norm;
    acc[i] = 0.f;
    xj[i] = on ? points[b * pb + (long long)j * pp + (long long)c * pc] : 0.f;
    al[i] = on ? alpha[c] : 0.f;
  }
  // (s, k) entries that name j: d = points[j] - m[s]
  const int n = dm.S * dm.K;
  const int32_t* pbj = ptr + b * (dm.N + 1);
  const int32_t* eb = ent + b * n;
  const int e0 = max(0, min(pbj[j], n)), e1 = max(e0, min(pbj[j + 1], n));
  for (int e = e0; e < e1; ++e) {
    const unsigned ev = (unsigned)eb[e];
    const unsigned s = ev / (unsigned)dm.K;
    if (s >= (unsigned)dm.S) continue;
    const int k = (int)(ev - s * dm.K);
    const size_t row = b * dm.S + s;
    const float* dk_row = dout + row * dm.K * dm.C + k * dk;
#pragma unroll
    for (int i = 0; i < DSLOTS; ++i) {
      const int c = 64 * i + (int)lane;
      if (c < dm.D) {
        const float gy = dk_row[c * dc];
        if (!norm) {
          acc[i] += gy;
        } else {
          const float d = xj[i] - mean[row * dm.Cn + c];
          float gd = fmaf(al[i] * gy, r, -(coef * (d - mu)));
          if (normalize == NORM_CENTER)
            gd -= fmaf(al[i] * r, gysum[row * dm.Cn + c], -(coef * (dsum[row * dm.Cn + c] - kmu))) / kf;
          acc[i] += gd;
        }
      }
    }
  }
  // anchors that are j: the cat's half, and minus the row's sum_k gd with normalize = anchor
  const int32_t* fbj = fptr + b * (dm.N + 1);
  const int32_t* fe = fent + b * dm.S;
  const int f0 = max(0, min(fbj[j], dm.S)), f1 = max(f0, min(fbj[j + 1], dm.S));
  for (int f = f0; f < f1; ++f) {
    const unsigned s = (unsigned)fe[f];
    if (s >= (unsigned)dm.S) continue;
    const size_t row = b * dm.S + s;
#pragma unroll
    for (int i = 0; i < DSLOTS; ++i) {
      const int c = 64 * i + (int)lane;
      if (c < dm.D) {
        acc[i] += gasum[row * dm.D + c];
        if (normalize == NORM_ANCHOR) acc[i] -= fmaf(al[i] * r, gysum[row * dm.Cn + c], -(coef * (dsum[row * dm.Cn + c] - kmu)));
      }
    }
  }
#pragma unroll
  for (int i = 0; i < DSLOTS; ++i) {
    const int c = 64 * i + (int)lane;
    if (c < dm.D) dpoints[b * gb + (long long)j * gp + (long long)c * gc] = acc[i];
  }
}

// ---- host -----------------------------------------------------------------------------------------------------------------------
struct Plan {
  Dims dm;
  long long rows_s, rows_n;      // B S, B N
  int rb_s, rb_n, stat_wg, bwd_wg, param_blocks;
};

int plan(int B, int N, int S, int K, int D, int use_xyz, int normalize, Plan& p) {
  if (B < 1 || N < 1 || S < 1 || K < 1 || D < 1) return 1;
  if ((use_xyz != 0 && use_xyz != 1) || normalize < NORM_NONE || normalize > NORM_ANCHOR) return 1;
  if (S > N || N > U3D_LOCAL_GROUPER_MAX_POINTS || K < 2 || K > U3D_LOCAL_GROUPER_MAX_K || (D & 3) || D > U3D_LOCAL_GROUPER_MAX_CHANNELS)
    return 2;
  p.rows_s = (long long)B * S;
  p.rows_n = (long long)B * N;
  if (p.rows_s * K >= (1ll << 24) || p.rows_n >= (1ll << 24)) return 2;
  const int A = use_xyz ? 3 : 0;
  p.dm = Dims{N, S, K, D, D + A, 2 * D + A};
  p.rb_s = u3d_util::blocks(S, ROW_WAVES);
  p.rb_n = u3d_util::blocks(N, ROW_WAVES);
  p.stat_wg = p.rb_s < STAT_MAX_WG ? p.rb_s : STAT_MAX_WG;
  const int bw = u3d_util::blocks(S, BWD_WAVES);
  p.bwd_wg = bw < BWD_MAX_WG ? bw : BWD_MAX_WG;
  p.param_blocks = normalize != NORM_NONE ? u3d_util::blocks(2 * p.dm.Cn, PR_Q) : 0;
  return 0;
}

size_t fwd_scratch(const Plan& p, int B, int normalize) { return normalize != NORM_NONE ? (size_t)B * p.stat_wg * 2 * sizeof(double) : 0; }
size_t bwd_scratch(const Plan& p, int B, int normalize) {
  size_t bytes = (size_t)p.rows_s * p.dm.D * sizeof(float);
  if (normalize != NORM_NONE)
    bytes += (size_t)B * p.bwd_wg * (2 * sizeof(double) + (size_t)2 * p.dm.Cn * sizeof(float)) + 2 * (size_t)p.rows_s * p.dm.Cn * sizeof(float);
  return bytes;
}
size_t list_scratch(const Plan& p) { return ((size_t)p.rows_n + (size_t)p.rows_s * p.dm.K + (size_t)p.rows_s) * sizeof(int32_t); }

bool bad_strides(long long sb, long long sp, long long sc, int N, int D) {
  return !((sp == D && sc == 1) || (sp == 1 && sc == N)) || sb < (long long)N * D;
}

}  // namespace

extern "C" {

int u3d_local_grouper_abi_version(void) { return U3D_LOCAL_GROUPER_ABI_VERSION; }

size_t u3d_local_grouper_scratch_bytes(int B, int N, int S, int K, int D, int use_xyz, int normalize, int pass) {
  Plan p;
  if (plan(B, N, S, K, D, use_xyz, normalize, p)) return 0;
  return pass == 0 ? fwd_scratch(p, B, normalize) : pass == 1 ? bwd_scratch(p, B, normalize) : pass == 2 ? list_scratch(p) : 0;
}

int u3d_local_grouper_lists(const int32_t* fps, const int32_t* idx, int32_t* ptr, int32_t* ent, int32_t* fptr, int32_t* fent, void* scratch,
                            int B, int N, int S, int K, void* stream) {
  if ((fps != nullptr && !u3d_util::aligned16(fps)) || bad_ptr(idx) || bad_ptr(ptr) || bad_ptr(ent) || bad_ptr(fptr) || bad_ptr(fent) ||
      bad_ptr(scratch))
    return 1;
  Plan p;
  if (const int rc = plan(B, N, S, K, 4, 0, NORM_NONE, p)) return rc;
  if (fps == nullptr && S != N) return 1;
  int32_t* cur = static_cast<int32_t*>(scratch);
  int32_t* tmpe = cur + p.rows_n;
  int32_t* tmpf = tmpe + p.rows_s * K;
  hipLaunchKernelGGL(lg_list_build_kernel, dim3(B), dim3(LIST_NT), 0, (hipStream_t)stream, fps, idx, ptr, fptr, cur, tmpe, tmpf, N, S, K);
  if (const int rc = u3d_util::launched()) return rc;
  hipLaunchKernelGGL(lg_list_sort_kernel, dim3(u3d_util::blocks(p.rows_n, ROW_WAVES)), dim3(ROW_NT), 0, (hipStream_t)stream, ptr, fptr, tmpe,
                     tmpf, ent, fent, N, S, K, p.rows_n);
  return u3d_util::launched();
}

int u3d_local_grouper_fwd(const float* xyz, const float* points, long long p_batch, long long p_point, long long p_chan, const int32_t* fps,
                          const int32_t* idx, const float* alpha, const float* beta, float* out, float* new_xyz, float* mean, float* stats,
                          void* scratch, int B, int N, int S, int K, int D, int use_xyz, int normalize, int channels_first, float eps,
                          void* stream) {
  if (bad_ptr(xyz) || bad_ptr(points) || (fps != nullptr && !u3d_util::aligned16(fps)) || bad_ptr(idx) || bad_ptr(out) || bad_ptr(new_xyz)) return 1;
  Plan p;
  if (const int rc = plan(B, N, S, K, D, use_xyz, normalize, p)) return rc;
  if (normalize != NORM_NONE && (bad_ptr(alpha) || bad_ptr(beta) || bad_ptr(mean) || bad_ptr(stats) || bad_ptr(scratch))) return 1;
  if (bad_strides(p_batch, p_point, p_chan, N, D) || (channels_first != 0 && channels_first != 1) || (fps == nullptr && S != N) ||
      !(eps >= 0.f) || !(eps < INFINITY))
    return 1;
  double* part = static_cast<double*>(scratch);
  if (normalize != NORM_NONE) {
    hipLaunchKernelGGL(lg_stats_kernel, dim3(B * p.stat_wg), dim3(ROW_NT), 0, (hipStream_t)stream, xyz, points, p_batch, p_point, p_chan, fps,
                       idx, mean, part, p.dm, normalize, p.stat_wg);
    if (const int rc = u3d_util::launched()) return rc;
  }
  hipLaunchKernelGGL(lg_fwd_kernel, dim3(B * p.rb_s), dim3(ROW_NT), 0, (hipStream_t)stream, xyz, points, p_batch, p_point, p_chan, fps, idx,
                     alpha, beta, out, new_xyz, mean, stats, part, p.dm, normalize, channels_first, p.stat_wg, p.rb_s, eps);
  return u3d_util::launched();
}

int u3d_local_grouper_bwd(const float* xyz, const float* points, long long p_batch, long long p_point, long long p_chan, const int32_t* fps,
                          const int32_t* idx, const int32_t* ptr, const int32_t* ent, const int32_t* fptr, const int32_t* fent,
                          const float* alpha, const float* mean, const float* stats, const float* dout, float* dpoints, long long g_batch,
                          long long g_point, long long g_chan, float* dalpha, float* dbeta, void* scratch, int B, int N, int S, int K, int D,
                          int use_xyz, int normalize, int dout_channels_first, void* stream) {
  if (bad_ptr(xyz) || bad_ptr(points) || (fps != nullptr && !u3d_util::aligned16(fps)) || bad_ptr(idx) || bad_ptr(ptr) || bad_ptr(ent) ||
      bad_ptr(fptr) || bad_ptr(fent) || bad_ptr(dout) || bad_ptr(dpoints) || bad_ptr(scratch))
    return 1;
  Plan p;
  if (const int rc = plan(B, N, S, K, D, use_xyz, normalize, p)) return rc;
  if (normalize != NORM_NONE && (bad_ptr(alpha) || bad_ptr(mean) || bad_ptr(stats) || bad_ptr(dalpha) || bad_ptr(dbeta))) return 1;
  if (bad_strides(p_batch, p_point, p_chan, N, D) || bad_strides(g_batch, g_point, g_chan, N, D) ||
      (dout_channels_first != 0 && dout_channels_first != 1) || (fps == nullptr && S != N))
    return 1;
  // [tpart | ppart | gysum | dsum] (only with a normalisation), then gasum
  const int npart = B * p.bwd_wg;
  char* base = static_cast<char*>(scratch);
  double* tpart = nullptr;
  float *ppart = nullptr, *gysum = nullptr, *dsum = nullptr;
  if (normalize != NORM_NONE) {
    tpart = reinterpret_cast<double*>(base);
    ppart = reinterpret_cast<float*>(tpart + 2 * (size_t)npart);
    gysum = ppart + (size_t)npart * 2 * p.dm.Cn;
    dsum = gysum + (size_t)p.rows_s * p.dm.Cn;
    base = reinterpret_cast<char*>(dsum + (size_t)p.rows_s * p.dm.Cn);
  }
  float* gasum = reinterpret_cast<float*>(base);
  hipLaunchKernelGGL(lg_bwd_partial_kernel, dim3(npart), dim3(BWD_NT), 0, (hipStream_t)stream, xyz, points, p_batch, p_point, p_chan, fps, idx,
                     alpha, mean, stats, dout, tpart, ppart, gysum, dsum, gasum, p.dm, normalize, dout_channels_first, p.bwd_wg);
  if (const int rc = u3d_util::launched()) return rc;
  const int dx_blocks = B * p.rb_n;
  hipLaunchKernelGGL(lg_bwd_dpoints_kernel, dim3(dx_blocks + p.param_blocks), dim3(ROW_NT), 0, (hipStream_t)stream, points, p_batch, p_point,
                     p_chan, ptr, ent, fptr, fent, alpha, mean, stats, dout, tpart, ppart, gysum, dsum, gasum, dpoints, g_batch, g_point,
                     g_chan, dalpha, dbeta, p.dm, normalize, dout_channels_first, p.bwd_wg, p.rb_n, dx_blocks, npart);
  return u3d_util::launched();
}

}  // extern "C"
