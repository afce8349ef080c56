// libunipre3d_tokenizer.so: the group tokenizer (mini-PointNet `Encoder`) of the transformer and Mamba3D backbones, forward and backward
// in fp32 (include/unipre3d_tokenizer.h).  BN1's statistics come from nine moments of the coordinates, the cat is replaced by a per-group
// bias, and the backward is three phases separated by BatchNorm's two global sums.  The shared MFMA GEMM and split weight-gradient
// kernel (u3d_mfma_tile.h) serve every plain product: what differs between the products is how an operand element is made (a row of f2, relu(A x + d)
// from three coordinates, relu(s2 y3 + t2), dy3 from dh3m and y3) and what the epilogue adds, both template arguments.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "unipre3d_tokenizer.h"
#include "u3d_mfma_tile.h"
#include "u3d_util.h"

namespace {

using namespace u3d_util;
using namespace u3d_mfma_tile;                // NT, the block tile, gemm(), wgrad_kernel and its split rule

constexpr int C1 = 128, C2 = 256, C3 = 512;   // the reference's widths
constexpr int F1_A = 0, F1_D = 384, F1_AH = 512, F1_DH = 896, F1_MEAN = 1024, F1_INV = 1152;   // fold1
constexpr int F2_S = 0, F2_T = 512, F2_MEAN = 1024, F2_INV = 1536;                              // fold2
constexpr int SLAB = 32, PHASES = 8;          // dh3m: columns per workgroup, row phases (NT = SLAB * PHASES)

// ---- the input through its strides ---------------------------------------------------------------------------------------------
struct XView {
  const float* x;
  long long s0, s1, s2, s3;
  int G, n;
};
__device__ __forceinline__ void load_x(const XView& v, long long r, float& a, float& b, float& c) {
  const long long grp = r / v.n;
  const int i = (int)(r - grp * v.n);
  const long long bb = grp / v.G;
  const int gg = (int)(grp - bb * v.G);
  const float* p = v.x + bb * v.s0 + gg * v.s1 + i * v.s2;
  a = p[0];
  b = p[v.s3];
  c = p[2 * v.s3];
}
// BN1's output before the ReLU, the one expression every kernel uses (so the ReLU mask is the same everywhere)
__device__ __forceinline__ float h1_pre(const float* __restrict__ f1, int k, float a, float b, float c) {
  return fmaf(f1[F1_A + k * 3], a, fmaf(f1[F1_A + k * 3 + 1], b, fmaf(f1[F1_A + k * 3 + 2], c, f1[F1_D + k])));
}
__device__ __forceinline__ float xhat1(const float* __restrict__ f1, int k, float a, float b, float c) {
  return fmaf(f1[F1_AH + k * 3], a, fmaf(f1[F1_AH + k * 3 + 1], b, fmaf(f1[F1_AH + k * 3 + 2], c, f1[F1_DH + k])));
}
__device__ __forceinline__ float h3_pre(const float* __restrict__ f2c, int k, float y) { return fmaf(f2c[F2_S + k], y, f2c[F2_T + k]); }
__device__ __forceinline__ float xhat3(const float* __restrict__ f2c, int k, float y) { return (y - f2c[F2_MEAN + k]) * f2c[F2_INV + k]; }
// BatchNorm's input gradient: coef = p, q, w (cols each) with p = gamma invstd, q = sum1 / N, w = sum2 / N
__device__ __forceinline__ float dy_of(const float* __restrict__ coef, int cols, int k, float dh, float xh) {
  return coef[k] * (dh - coef[cols + k] - xh * coef[2 * cols + k]);
}

// ---- operand makers: prep(row) once per row and stage, get(ctx, k) per element ------------------------------------------------------
struct APlain {
  const float* p;
  int ld;
  struct Ctx { const float* row; };
  __device__ __forceinline__ Ctx prep(long long r) const { return Ctx{p + r * ld}; }
  __device__ __forceinline__ float get(const Ctx& c, int k) const { return c.row[k]; }
};
struct AH1 {   // relu(A x + d)
  XView v;
  const float* f1;
  struct Ctx { float a, b, c; };
  __device__ __forceinline__ Ctx prep(long long r) const { Ctx c; load_x(v, r, c.a, c.b, c.c); return c; }
  __device__ __forceinline__ float get(const Ctx& c, int k) const { return fmaxf(h1_pre(f1, k, c.a, c.b, c.c), 0.f); }
};
struct AH3 {   // relu(s2 y3 + t2)
  const float* y;
  const float* f2c;
  struct Ctx { const float* row; };
  __device__ __forceinline__ Ctx prep(long long r) const { return Ctx{y + r * C3}; }
  __device__ __forceinline__ float get(const Ctx& c, int k) const { return fmaxf(h3_pre(f2c, k, c.row[k]), 0.f); }
};
struct ADy3 {  // dy3 from dh3m and y3
  const float* d;
  const float* y;
  const float* f2c;
  const float* coef;
  struct Ctx { const float* dr; const float* yr; };
  __device__ __forceinline__ Ctx prep(long long r) const { return Ctx{d + r * C3, y + r * C3}; }
  __device__ __forceinline__ float get(const Ctx& c, int k) const { return dy_of(coef, C3, k, c.dr[k], xhat3(f2c, k, c.yr[k])); }
};

// ---- epilogues ---------------------------------------------------------------------------------------------------------------------
struct EBias {
  float* out;
  int ld;
  const float* bias;
  __device__ __forceinline__ void store(long long r, int col, float v) const { out[r * ld + col] = v + (bias ? bias[col] : 0.f); }
};
struct EGroupBias {   // y3 = f2 W3l^T + u[group]
  float* out;
  const float* u;
  int n;
  __device__ __forceinline__ void store(long long r, int col, float v) const { out[r * C3 + col] = v + u[(r / n) * C3 + col]; }
};
struct EArgAdd {      // df2 = dy3 W3l, plus dg at the group's arg2 row
  float* out;
  const int32_t* arg;
  const float* dg;
  int n;
  __device__ __forceinline__ void store(long long r, int col, float v) const {
    const long long g = r / n, o = g * C2 + col;
    out[r * C2 + col] = arg[o] == (int)(r - g * n) ? v + dg[o] : v;
  }
};
struct EMaskH1 {      // dh1m = [h1 > 0] (df2 W2)
  float* out;
  XView xv;
  const float* f1;
  __device__ __forceinline__ void store(long long r, int col, float v) const {
    float a, b, c;
    load_x(xv, r, a, b, c);
    out[r * C1 + col] = h1_pre(f1, col, a, b, c) > 0.f ? v : 0.f;
  }
};

// ---- weight gradients: fixed-order split reductions ------------------------------------------------------------------------------
long long group_rows_per_split(long long M) { const long long s = std::max(1ll, std::min(32ll, (M + 63) / 64)); return (M + s - 1) / s; }
int group_splits(long long M) { const long long gps = group_rows_per_split(M); return (int)((M + gps - 1) / gps); }
long long stat_rows_per_split(long long R) { const long long s = std::max(1ll, std::min(256ll, (R + 511) / 512)); return (R + s - 1) / s; }
int stat_splits(long long R) { const long long rps = stat_rows_per_split(R); return (int)((R + rps - 1) / rps); }

// out[i ldo + off + j] = sum over splits, in order, of part[split][i Ng + j]
__global__ __launch_bounds__(NT) void split_sum_kernel(int Ma, int Ng, int splits, const float* __restrict__ part, float* __restrict__ out,
                                                       int ldo, int off) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x, n = (long long)Ma * Ng;
  if (t >= n) return;
  float s = 0.f;
  for (int q = 0; q < splits; ++q) s += part[(size_t)q * n + t];
  const int i = (int)(t / Ng), j = (int)(t - (long long)i * Ng);
  out[(size_t)i * ldo + off + j] = s;
}

template <class AOp, class GOp>
void wgrad(long long R, int Ma, int Ng, const AOp& aop, const GOp& gop, float* part, float* out, int ldo, int off, hipStream_t st) {
  const long long rps = wgrad_rows_per_split(R);
  const int splits = wgrad_splits(R);
  wgrad_kernel<AOp, GOp><<<dim3(blocks(Ma, BM) * blocks(Ng, BN), splits), NT, 0, st>>>(R, Ma, Ng, aop, gop, rps, part);
  split_sum_kernel<<<blocks((long long)Ma * Ng, NT), NT, 0, st>>>(Ma, Ng, splits, part, out, ldo, off);
}

// dW4[c][k] = sum over groups of dout[g][c] h3[row arg4[g][c] of g][k]: a thread per (c, k), groups of a split in order
__global__ __launch_bounds__(NT) void dw4_kernel(long long M, int n, int C, const float* __restrict__ dout, const int32_t* __restrict__ arg4,
                                                 const float* __restrict__ y3, const float* __restrict__ f2c, long long gps,
                                                 float* __restrict__ part) {
  const int k = blockIdx.x * NT + threadIdx.x, c = blockIdx.y, split = blockIdx.z;
  const long long g_beg = split * gps, g_end = min(M, g_beg + gps);
  float acc = 0.f;
  for (long long g = g_beg; g < g_end; ++g) {
    const int row = min(max(arg4[g * C + c], 0), n - 1);
    acc = fmaf(dout[g * C + c], fmaxf(h3_pre(f2c, k, y3[(g * n + row) * C3 + k]), 0.f), acc);
  }
  part[((size_t)split * C + c) * C3 + k] = acc;
}

// dh3m[row][k] = [h3 > 0] sum over the channels c whose arg4 is that row of dout[g][c] W4[c][k]: a workgroup per group and slab of
// 32 columns; every (row, column) of the slab is owned by one thread, which adds its channels in ascending order
__global__ __launch_bounds__(NT) void dh3m_kernel(int n, int C, const float* __restrict__ dout, const int32_t* __restrict__ arg4,
                                                  const float* __restrict__ y3, const float* __restrict__ f2c, const float* __restrict__ W4,
                                                  float* __restrict__ dh3m) {
  __shared__ float acc[U3D_TOK_MAX_N * SLAB];
  __shared__ int sarg[U3D_TOK_MAX_CHANNELS];
  __shared__ float sd[U3D_TOK_MAX_CHANNELS];
  const long long g = blockIdx.x;
  const int tid = threadIdx.x, kc = tid & (SLAB - 1), ph = tid / SLAB, k = blockIdx.y * SLAB + kc;
  for (int c = tid; c < C; c += NT) {
    sarg[c] = arg4[g * C + c];
    sd[c] = dout[g * C + c];
  }
  for (int i = tid; i < n * SLAB; i += NT) acc[i] = 0.f;
  __syncthreads();
  for (int c = 0; c < C; ++c) {
    const int row = sarg[c];
    if ((unsigned)row < (unsigned)n && (row & (PHASES - 1)) == ph) acc[row * SLAB + kc] = fmaf(sd[c], W4[(size_t)c * C3 + k], acc[row * SLAB + kc]);
  }
  __syncthreads();
  for (int row = ph; row < n; row += PHASES) {
    const long long o = (g * n + row) * C3 + k;
    dh3m[o] = h3_pre(f2c, k, y3[o]) > 0.f ? acc[row * SLAB + kc] : 0.f;
  }
}

// ---- group maxima and sums -------------------------------------------------------------------------------------------------------
// the maximum over a group's n rows and the lowest row that attains it
__global__ __launch_bounds__(NT) void groupmax_kernel(long long M, int n, int cols, const float* __restrict__ F, float* __restrict__ val,
                                                      int32_t* __restrict__ arg) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= M * cols) return;
  const long long g = t / cols;
  const int c = (int)(t - g * cols);
  const float* p = F + g * n * cols + c;
  float best = p[0];
  int bi = 0;
  for (int i = 1; i < n; ++i) {
    const float v = p[(size_t)i * cols];
    if (v > best) { best = v; bi = i; }
  }
  val[t] = best;
  arg[t] = bi;
}

// dS[g][j] = sum over the group's rows, in order, of dy3
__global__ __launch_bounds__(NT) void ds_kernel(long long M, int n, ADy3 op, float* __restrict__ dS) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= M * C3) return;
  const long long g = t / C3;
  const int j = (int)(t - g * C3);
  float s = 0.f;
  for (int i = 0; i < n; ++i) s += op.get(op.prep(g * n + i), j);
  dS[t] = s;
}

// ---- column sums in f64 ------------------------------------------------------------------------------------------------------------
struct SPlain {
  const float* p;
  int ld;
  __device__ __forceinline__ void get(long long r, int c, double& a, double& b) const { a = p[r * ld + c]; b = 0.0; }
};
struct SSquare {
  const float* y;
  __device__ __forceinline__ void get(long long r, int c, double& a, double& b) const { a = y[r * C3 + c]; b = a * a; }
};
struct SXhat3 {
  const float* d;
  const float* y;
  const float* f2c;
  __device__ __forceinline__ void get(long long r, int c, double& a, double& b) const {
    a = d[r * C3 + c];
    b = a * (double)xhat3(f2c, c, y[r * C3 + c]);
  }
};
struct SXhat1 {
  const float* d;
  XView xv;
  const float* f1;
  __device__ __forceinline__ void get(long long r, int c, double& a, double& b) const {
    float x0, x1, x2;
    load_x(xv, r, x0, x1, x2);
    a = d[r * C1 + c];
    b = a * (double)xhat1(f1, c, x0, x1, x2);
  }
};

// part[split][2][cols]: 64 columns x 4 row phases per workgroup, the phases added in order
template <class Op>
__global__ __launch_bounds__(NT) void colstats_kernel(long long R, int cols, Op op, long long rps, double* __restrict__ part) {
  __shared__ double red[2][4][64];
  const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
  const long long r_beg = blockIdx.y * rps, r_end = min(R, r_beg + rps);
  double s1 = 0.0, s2 = 0.0;
  if (c < cols)
    for (long long r = r_beg + ph; r < r_end; r += 4) {
      double a, b;
      op.get(r, c, a, b);
      s1 += a;
      s2 += b;
    }
  red[0][ph][cl] = s1;
  red[1][ph][cl] = s2;
  __syncthreads();
  if (ph == 0 && c < cols) {
    double t1 = red[0][0][cl], t2 = red[1][0][cl];
    for (int w = 1; w < 4; ++w) { t1 += red[0][w][cl]; t2 += red[1][w][cl]; }
    part[((size_t)blockIdx.y * 2) * cols + c] = t1;
    part[((size_t)blockIdx.y * 2 + 1) * cols + c] = t2;
  }
}
// sums[0] = count, sums[1 + t] = the splits' part[.][t] in order (t < 2 cols)
__global__ __launch_bounds__(NT) void stats_final_kernel(int cols2, int splits, const double* __restrict__ part, double count,
                                                         double* __restrict__ sums) {
  const int t = blockIdx.x * NT + threadIdx.x;
  if (t == 0) sums[0] = count;
  if (t >= cols2) return;
  double s = 0.0;
  for (int q = 0; q < splits; ++q) s += part[(size_t)q * cols2 + t];
  sums[1 + t] = s;
}
// out[c] = (float) of the first sum alone
__global__ __launch_bounds__(NT) void colsum_final_kernel(int cols, int splits, const double* __restrict__ part, float* __restrict__ out) {
  const int c = blockIdx.x * NT + threadIdx.x;
  if (c >= cols) return;
  double s = 0.0;
  for (int q = 0; q < splits; ++q) s += part[(size_t)q * 2 * cols + c];
  out[c] = (float)s;
}

size_t stat_part_bytes(long long R, int cols) { return (size_t)stat_splits(R) * 2 * cols * sizeof(double); }

template <class Op>
void colstats(long long R, int cols, const Op& op, double* part, hipStream_t st) {
  colstats_kernel<Op><<<dim3(blocks(cols, 64), stat_splits(R)), NT, 0, st>>>(R, cols, op, stat_rows_per_split(R), part);
}
void stats_final(long long R, int cols, const double* part, double* sums, hipStream_t st) {
  stats_final_kernel<<<blocks(2 * cols, NT), NT, 0, st>>>(2 * cols, stat_splits(R), part, (double)R, sums);
}
void colsum_final(long long R, int cols, const double* part, float* out, hipStream_t st) {
  colsum_final_kernel<<<blocks(cols, NT), NT, 0, st>>>(cols, stat_splits(R), part, out);
}

// ---- the moments of the coordinates --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void moments_kernel(long long R, XView xv, long long rps, double* __restrict__ part) {
  __shared__ double sh[NT];
  const long long r_beg = blockIdx.x * rps, r_end = min(R, r_beg + rps);
  double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (long long r = r_beg + threadIdx.x; r < r_end; r += NT) {
    float fa, fb, fc;
    load_x(xv, r, fa, fb, fc);
    const double a = fa, b = fb, c = fc;
    s[0] += a; s[1] += b; s[2] += c;
    s[3] += a * a; s[4] += a * b; s[5] += a * c; s[6] += b * b; s[7] += b * c; s[8] += c * c;
  }
  for (int q = 0; q < 9; ++q) {
    const double t = block_tree_sum<NT>(s[q], sh);
    if (threadIdx.x == 0) part[(size_t)blockIdx.x * 10 + q] = t;
  }
  if (threadIdx.x == 0) part[(size_t)blockIdx.x * 10 + 9] = (double)(r_end - r_beg);   // (records of 10 doubles: the split's row count)
}
__global__ void moments_final_kernel(int splits, const double* __restrict__ part, double count, double* __restrict__ sums) {
  const int q = threadIdx.x;
  if (q == 0) sums[0] = count;
  if (q >= 9) return;
  double s = 0.0;
  for (int i = 0; i < splits; ++i) s += part[(size_t)i * 10 + q];
  sums[1 + q] = s;
}

// ---- folding BatchNorm ------------------------------------------------------------------------------------------------------------
// the running statistics as BatchNorm1d updates them (unbiased variance; momentum < 0: cumulative average over num_batches_tracked)
__device__ __forceinline__ void running_update(float* rm, float* rv, int k, double mean, double var, double N, double factor) {
  if (rm) rm[k] = (float)((1.0 - factor) * (double)rm[k] + factor * mean);
  if (rv) rv[k] = (float)((1.0 - factor) * (double)rv[k] + factor * var * (N / (N - 1.0)));
}
__device__ __forceinline__ double update_factor(long long* nbt, float momentum) {   // every thread of the (single) workgroup
  const long long old = nbt ? nbt[0] : 0;
  __syncthreads();
  if (nbt && threadIdx.x == 0) nbt[0] = old + 1;
  return momentum < 0.f ? 1.0 / (double)(old + 1) : (double)momentum;
}

__global__ __launch_bounds__(C1) void fold1_kernel(const double* __restrict__ sums, const float* __restrict__ W1, const float* __restrict__ b1,
                                                   const float* __restrict__ g1, const float* __restrict__ be1, float* rm, float* rv,
                                                   long long* nbt, float eps, float momentum, float* __restrict__ f1) {
  const int k = threadIdx.x;
  const double w0 = W1[k * 3], w1 = W1[k * 3 + 1], w2 = W1[k * 3 + 2];
  double mean, inv, dh;
  if (sums) {
    const double factor = update_factor(nbt, momentum);
    const double N = sums[0], m0 = sums[1] / N, m1 = sums[2] / N, m2 = sums[3] / N;
    const double sxx = sums[4] / N - m0 * m0, sxy = sums[5] / N - m0 * m1, sxz = sums[6] / N - m0 * m2;
    const double syy = sums[7] / N - m1 * m1, syz = sums[8] / N - m1 * m2, szz = sums[9] / N - m2 * m2;
    const double wm = w0 * m0 + w1 * m1 + w2 * m2;
    double var = w0 * w0 * sxx + w1 * w1 * syy + w2 * w2 * szz + 2.0 * (w0 * w1 * sxy + w0 * w2 * sxz + w1 * w2 * syz);
    var = var > 0.0 ? var : 0.0;
    mean = wm + (double)b1[k];
    inv = 1.0 / sqrt(var + (double)eps);
    dh = -inv * wm;                       // the bias cancels against the batch mean
    running_update(rm, rv, k, mean, var, N, factor);
  } else {
    mean = rm[k];
    inv = 1.0 / sqrt((double)rv[k] + (double)eps);
    dh = inv * ((double)b1[k] - mean);
  }
  const double gam = g1[k];
  f1[F1_AH + k * 3] = (float)(inv * w0);
  f1[F1_AH + k * 3 + 1] = (float)(inv * w1);
  f1[F1_AH + k * 3 + 2] = (float)(inv * w2);
  f1[F1_DH + k] = (float)dh;
  f1[F1_A + k * 3] = (float)(gam * inv * w0);
  f1[F1_A + k * 3 + 1] = (float)(gam * inv * w1);
  f1[F1_A + k * 3 + 2] = (float)(gam * inv * w2);
  f1[F1_D + k] = (float)(gam * dh + (double)be1[k]);
  f1[F1_MEAN + k] = (float)mean;
  f1[F1_INV + k] = (float)inv;
}

__global__ __launch_bounds__(C3) void fold2_kernel(const double* __restrict__ sums, const float* __restrict__ g2, const float* __restrict__ be2,
                                                   float* rm, float* rv, long long* nbt, float eps, float momentum, float* __restrict__ f2c) {
  const int k = threadIdx.x;
  double mean, inv;
  if (sums) {
    const double factor = update_factor(nbt, momentum);
    const double N = sums[0];
    mean = sums[1 + k] / N;
    double var = sums[1 + C3 + k] / N - mean * mean;
    var = var > 0.0 ? var : 0.0;
    inv = 1.0 / sqrt(var + (double)eps);
    running_update(rm, rv, k, mean, var, N, factor);
  } else {
    mean = rm[k];
    inv = 1.0 / sqrt((double)rv[k] + (double)eps);
  }
  const double s = (double)g2[k] * inv;
  f2c[F2_S + k] = (float)s;
  f2c[F2_T + k] = (float)((double)be2[k] - mean * s);
  f2c[F2_MEAN + k] = (float)mean;
  f2c[F2_INV + k] = (float)inv;
}

// dgamma, dbeta from this process's sums; p, q, w of dy from the reduced ones.  dbias = sum of dy over this process's rows, in closed
// form in f64: p (S1 - N q - w sum(xhat)), all sums local except those inside q and w.  In one process it is the exact zero it is
// mathematically (a bias that feeds only a BatchNorm), where the sum of the fp32 dy would be rounding noise; xsum = this process's
// sum of xhat over its rows, without the invstd factor (null in eval mode, where w = 0).
__device__ __forceinline__ double bwd_coef(int cols, int c, const double* __restrict__ local, const double* __restrict__ red, int training,
                                           float gamma, float inv, double xsum, float* __restrict__ coef, float* __restrict__ dgamma,
                                           float* __restrict__ dbeta) {
  dbeta[c] = (float)local[1 + c];
  dgamma[c] = (float)local[1 + cols + c];
  const float p = gamma * inv;
  const double q = training ? red[1 + c] / red[0] : 0.0, w = training ? red[1 + cols + c] / red[0] : 0.0;
  coef[c] = p;
  coef[cols + c] = (float)q;
  coef[2 * cols + c] = (float)w;
  return (double)p * (local[1 + c] - local[0] * q - w * (double)inv * xsum);
}
// BN2: fwd_local / fwd_red are the forward's sums2 blocks (count, sum y3, sum y3^2) of this process and reduced
__global__ __launch_bounds__(C3) void bwd_coef2_kernel(const double* __restrict__ local, const double* __restrict__ red,
                                                       const double* __restrict__ fwd_local, const double* __restrict__ fwd_red, int training,
                                                       const float* __restrict__ gamma, const float* __restrict__ f2c, float* __restrict__ coef,
                                                       float* __restrict__ dgamma, float* __restrict__ dbeta, double* __restrict__ db3_64,
                                                       float* __restrict__ db3) {
  const int c = threadIdx.x;
  const double xsum = training ? fwd_local[1 + c] - fwd_local[0] * (fwd_red[1 + c] / fwd_red[0]) : 0.0;
  const double db = bwd_coef(C3, c, local, red, training, gamma[c], f2c[F2_INV + c], xsum, coef, dgamma, dbeta);
  db3_64[c] = db;
  db3[c] = (float)db;
}
// db2 = sum over rows of df2 = db3 (W3g + W3l): every dg lands in its column exactly once
__global__ __launch_bounds__(C2) void db2_kernel(const double* __restrict__ db3_64, const float* __restrict__ W3, float* __restrict__ db2) {
  const int c = threadIdx.x;
  double s = 0.0;
  for (int j = 0; j < C3; ++j) s += db3_64[j] * ((double)W3[(size_t)j * C3 + c] + (double)W3[(size_t)j * C3 + C2 + c]);
  db2[c] = (float)s;
}
// BN1: fwd_local / fwd_red are the forward's sums1 blocks (count, sum x, ...); sum(xhat1) = invstd W1 (sum x - N m)
__global__ __launch_bounds__(C1) void bwd_coef1_kernel(const double* __restrict__ local, const double* __restrict__ red,
                                                       const double* __restrict__ fwd_local, const double* __restrict__ fwd_red, int training,
                                                       const float* __restrict__ gamma, const float* __restrict__ f1, const float* __restrict__ W1,
                                                       float* __restrict__ coef, float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                       float* __restrict__ db1) {
  const int c = threadIdx.x;
  double xsum = 0.0;
  if (training)
    for (int i = 0; i < 3; ++i) xsum += (double)W1[c * 3 + i] * (fwd_local[1 + i] - fwd_local[0] * (fwd_red[1 + i] / fwd_red[0]));
  db1[c] = (float)bwd_coef(C1, c, local, red, training, gamma[c], f1[F1_INV + c], xsum, coef, dgamma, dbeta);
}

// ---- B3: K = 3 products on the VALU -------------------------------------------------------------------------------------------------
// part[split][k][4] = sums over the split's rows, in order, of dy1 x (3) in f64 (the fourth slot is zero: 32-byte records)
__global__ __launch_bounds__(C1) void b3_kernel(long long R, XView xv, const float* __restrict__ dh1m, const float* __restrict__ f1,
                                                const float* __restrict__ coef, long long rps, double* __restrict__ part) {
  const int k = threadIdx.x;
  const long long r_beg = blockIdx.x * rps, r_end = min(R, r_beg + rps);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (long long r = r_beg; r < r_end; ++r) {
    float a, b, c;
    load_x(xv, r, a, b, c);
    const double dy = dy_of(coef, C1, k, dh1m[r * C1 + k], xhat1(f1, k, a, b, c));
    s0 += dy * a; s1 += dy * b; s2 += dy * c;
  }
  double* p = part + ((size_t)blockIdx.x * C1 + k) * 4;
  p[0] = s0; p[1] = s1; p[2] = s2; p[3] = 0.0;
}
__global__ __launch_bounds__(NT) void b3_final_kernel(int splits, const double* __restrict__ part, float* __restrict__ dW1) {
  const int t = blockIdx.x * NT + threadIdx.x;
  if (t >= C1 * 4) return;
  double s = 0.0;
  for (int q = 0; q < splits; ++q) s += part[(size_t)q * C1 * 4 + t];
  const int k = t >> 2, i = t & 3;
  if (i < 3) dW1[k * 3 + i] = (float)s;
}
__global__ __launch_bounds__(NT) void dx_kernel(long long R, XView xv, const float* __restrict__ dh1m, const float* __restrict__ f1,
                                                const float* __restrict__ coef, const float* __restrict__ W1, float* __restrict__ dx) {
  const long long r = (long long)blockIdx.x * NT + threadIdx.x;
  if (r >= R) return;
  float a, b, c;
  load_x(xv, r, a, b, c);
  float d0 = 0.f, d1 = 0.f, d2 = 0.f;
  for (int k = 0; k < C1; ++k) {
    const float dy = dy_of(coef, C1, k, dh1m[r * C1 + k], xhat1(f1, k, a, b, c));
    d0 = fmaf(dy, W1[k * 3], d0);
    d1 = fmaf(dy, W1[k * 3 + 1], d1);
    d2 = fmaf(dy, W1[k * 3 + 2], d2);
  }
  dx[r * 3] = d0;
  dx[r * 3 + 1] = d1;
  dx[r * 3 + 2] = d2;
}

// ---- shapes and scratch -----------------------------------------------------------------------------------------------------------
int check_shape(long long M, int n, int C) {
  if (M < 1 || n < 1 || C < 1) return 1;
  if (n > U3D_TOK_MAX_N || C > U3D_TOK_MAX_CHANNELS || M * n >= (1ll << 31)) return 2;
  return 0;
}
bool bad_x(const float* x, long long s0, long long s1, long long s2, long long s3) {
  return x == nullptr || ((uintptr_t)x & 3u) != 0 || s0 < 0 || s1 < 0 || s2 < 0 || s3 < 0;
}
int moment_splits(long long R) { return stat_splits(R); }

struct Scratch {   // byte offsets from the start, every one a multiple of 16
  size_t a = 0, b = 0, c = 0, d = 0, e = 0, f = 0, g = 0, total = 0;
};
Scratch carve(long long M, int n, int C, int phase, int training) {
  Scratch s;
  const long long R = M * n;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t o = at; at += bytes; return o; };
  switch (phase) {
    case 0: s.a = take((size_t)moment_splits(R) * 10 * sizeof(double)); break;                    // moment partials
    case 1:
      s.a = take((size_t)M * C3 * sizeof(float));                                                // u
      if (training) s.b = take(stat_part_bytes(R, C3));                                          // y3 statistics partials
      break;
    case 2: s.a = take((size_t)R * C * sizeof(float)); break;                                    // f4
    case 3:
      s.a = take((size_t)group_splits(M) * C * C3 * sizeof(float));                              // dW4 partials
      s.b = take(stat_part_bytes(R, C3));                                                        // dh3m statistics partials
      s.c = take(stat_part_bytes(M, C));                                                         // db4 partials
      break;
    case 4:
      s.a = take((size_t)wgrad_splits(R) * C3 * C2 * sizeof(float));                             // dW3l partials
      s.b = take((size_t)wgrad_splits(M) * C3 * C2 * sizeof(float));                             // dW3g partials
      s.c = take((size_t)wgrad_splits(R) * C2 * C1 * sizeof(float));                             // dW2 partials
      s.d = take((size_t)M * C3 * sizeof(float));                                                // dS
      s.e = take((size_t)M * C2 * sizeof(float));                                                // dg
      s.f = take((size_t)3 * C3 * sizeof(float));                                                // p, q, w of dy3
      s.g = take((size_t)C3 * sizeof(double) + stat_part_bytes(R, C1));                          // db3 in f64, dh1m statistics partials
      break;
    case 5:
      s.a = take((size_t)3 * C1 * sizeof(float));                                                // p, q, w of dy1
      s.b = take((size_t)stat_splits(R) * C1 * 4 * sizeof(double));                              // dW1 / db1 partials
      break;
    default: break;
  }
  s.total = at;
  return s;
}
template <class T>
T* at(void* scratch, size_t off) { return (T*)((char*)scratch + off); }

}  // namespace

extern "C" {

int u3d_tok_abi_version(void) { return U3D_TOK_ABI_VERSION; }

int u3d_tok_wgrad_splits(long long rows) { return rows < 1 ? 0 : wgrad_splits(rows); }

size_t u3d_tok_scratch_bytes(long long M, int n, int C, int phase, int training) {
  if (check_shape(M, n, C) || phase < 0 || phase > 5) return 0;
  return carve(M, n, C, phase, training).total;
}

int u3d_tok_moments(const float* x, long long s0, long long s1, long long s2, long long s3, int B, int G, int n, double* sums1,
                    void* scratch, void* stream) {
  if (B < 1 || G < 1) return 1;
  const long long M = (long long)B * G;
  if (int rc = check_shape(M, n, 1)) return rc;
  if (bad_x(x, s0, s1, s2, s3) || bad_ptr(sums1) || bad_ptr(scratch)) return 1;
  hipStream_t st = (hipStream_t)stream;
  const long long R = M * n;
  const XView xv{x, s0, s1, s2, s3, G, n};
  const int splits = moment_splits(R);
  double* part = at<double>(scratch, carve(M, n, 1, 0, 1).a);
  moments_kernel<<<splits, NT, 0, st>>>(R, xv, stat_rows_per_split(R), part);
  moments_final_kernel<<<1, 64, 0, st>>>(splits, part, (double)R, sums1);
  return launched();
}

int u3d_tok_fwd_a(const float* x, long long s0, long long s1, long long s2, long long s3, int B, int G, int n, const float* W1,
                  const float* b1, const float* g1, const float* be1, const float* W2, const float* b2, const float* W3, const float* b3,
                  const double* sums1, float* run_mean1, float* run_var1, long long* nbt1, float eps, float momentum, float* fold1,
                  float* f2, float* g, int32_t* arg2, float* y3, double* sums2, void* scratch, void* stream) {
  if (B < 1 || G < 1) return 1;
  const long long M = (long long)B * G;
  if (int rc = check_shape(M, n, 1)) return rc;
  const bool training = sums1 != nullptr;
  if (bad_x(x, s0, s1, s2, s3) || bad_ptr(W1) || bad_ptr(b1) || bad_ptr(g1) || bad_ptr(be1) || bad_ptr(W2) || bad_ptr(b2) || bad_ptr(W3) ||
      bad_ptr(b3) || bad_ptr(fold1) || bad_ptr(f2) || bad_ptr(g) || bad_ptr(arg2) || bad_ptr(y3) || bad_ptr(scratch))
    return 1;
  if (!aligned16(sums1) || !aligned16(run_mean1) || !aligned16(run_var1) || !aligned16(nbt1) || !aligned16(sums2)) return 1;
  if (training ? sums2 == nullptr : (sums2 != nullptr || !run_mean1 || !run_var1)) return 1;
  if (!(eps >= 0.f) || !(momentum <= 1.f)) return 1;
  hipStream_t st = (hipStream_t)stream;
  const long long R = M * n;
  const XView xv{x, s0, s1, s2, s3, G, n};
  const Scratch sc = carve(M, n, 1, 1, training);
  float* u = at<float>(scratch, sc.a);
  fold1_kernel<<<1, C1, 0, st>>>(sums1, W1, b1, g1, be1, run_mean1, run_var1, nbt1, eps, momentum, fold1);
  gemm<AH1, true, EBias>(R, C1, C2, AH1{xv, fold1}, W2, C1, 0, EBias{f2, C2, b2}, st);
  groupmax_kernel<<<blocks(M * C2, NT), NT, 0, st>>>(M, n, C2, f2, g, arg2);
  gemm<APlain, true, EBias>(M, C2, C3, APlain{g, C2}, W3, C3, 0, EBias{u, C3, b3}, st);
  gemm<APlain, true, EGroupBias>(R, C2, C3, APlain{f2, C2}, W3, C3, C2, EGroupBias{y3, u, n}, st);
  if (training) {
    double* part = at<double>(scratch, sc.b);
    colstats(R, C3, SSquare{y3}, part, st);
    stats_final(R, C3, part, sums2, st);
  }
  return launched();
}

int u3d_tok_fwd_b(const float* y3, long long M, int n, int C, const float* g2, const float* be2, const float* W4, const float* b4,
                  const double* sums2, float* run_mean2, float* run_var2, long long* nbt2, float eps, float momentum, float* fold2,
                  float* out, int32_t* arg4, void* scratch, void* stream) {
  if (int rc = check_shape(M, n, C)) return rc;
  if (bad_ptr(y3) || bad_ptr(g2) || bad_ptr(be2) || bad_ptr(W4) || bad_ptr(b4) || bad_ptr(fold2) || bad_ptr(out) || bad_ptr(arg4) ||
      bad_ptr(scratch))
    return 1;
  if (!aligned16(sums2) || !aligned16(run_mean2) || !aligned16(run_var2) || !aligned16(nbt2)) return 1;
  if (!sums2 && (!run_mean2 || !run_var2)) return 1;
  if (!(eps >= 0.f) || !(momentum <= 1.f)) return 1;
  hipStream_t st = (hipStream_t)stream;
  const long long R = M * n;
  float* f4 = at<float>(scratch, carve(M, n, C, 2, 1).a);
  fold2_kernel<<<1, C3, 0, st>>>(sums2, g2, be2, run_mean2, run_var2, nbt2, eps, momentum, fold2);
  gemm<AH3, true, EBias>(R, C3, C, AH3{y3, fold2}, W4, C3, 0, EBias{f4, C, b4}, st);
  groupmax_kernel<<<blocks(M * C, NT), NT, 0, st>>>(M, n, C, f4, out, arg4);
  return launched();
}

int u3d_tok_bwd_1(const float* dout, const float* y3, const int32_t* arg4, const float* fold2, const float* W4, long long M, int n, int C,
                  float* dW4, float* db4, float* dh3m, double* sums3, void* scratch, void* stream) {
  if (int rc = check_shape(M, n, C)) return rc;
  if (bad_ptr(dout) || bad_ptr(y3) || bad_ptr(arg4) || bad_ptr(fold2) || bad_ptr(W4) || bad_ptr(dW4) || bad_ptr(db4) || bad_ptr(dh3m) ||
      bad_ptr(sums3) || bad_ptr(scratch))
    return 1;
  hipStream_t st = (hipStream_t)stream;
  const long long R = M * n;
  const Scratch sc = carve(M, n, C, 3, 1);
  float* wpart = at<float>(scratch, sc.a);
  double* spart = at<double>(scratch, sc.b);
  double* bpart = at<double>(scratch, sc.c);
  const int gs = group_splits(M);
  dw4_kernel<<<dim3(C3 / NT, C, gs), NT, 0, st>>>(M, n, C, dout, arg4, y3, fold2, group_rows_per_split(M), wpart);
  split_sum_kernel<<<blocks((long long)C * C3, NT), NT, 0, st>>>(C, C3, gs, wpart, dW4, C3, 0);
  colstats(M, C, SPlain{dout, C}, bpart, st);
  colsum_final(M, C, bpart, db4, st);
  dh3m_kernel<<<dim3((unsigned)M, C3 / SLAB), NT, 0, st>>>(n, C, dout, arg4, y3, fold2, W4, dh3m);
  colstats(R, C3, SXhat3{dh3m, y3, fold2}, spart, st);
  stats_final(R, C3, spart, sums3, st);
  return launched();
}

int u3d_tok_bwd_2(const float* x, long long s0, long long s1, long long s2, long long s3, int B, int G, int n, const float* dh3m,
                  const float* y3, const float* f2, const float* g, const int32_t* arg2, const float* fold1, const float* fold2,
                  const float* g2, const double* sums2_local, const double* sums2, const double* sums3_local, const double* sums3,
                  int training, const float* W2, const float* W3, float* dg2, float* dbe2, float* dW3, float* db3, float* dW2, float* db2,
                  float* df2, float* dh1m, double* sums1b, void* scratch, void* stream) {
  if (B < 1 || G < 1) return 1;
  const long long M = (long long)B * G;
  if (int rc = check_shape(M, n, 1)) return rc;
  if (bad_x(x, s0, s1, s2, s3) || bad_ptr(dh3m) || bad_ptr(y3) || bad_ptr(f2) || bad_ptr(g) || bad_ptr(arg2) || bad_ptr(fold1) ||
      bad_ptr(fold2) || bad_ptr(g2) || bad_ptr(sums3_local) || bad_ptr(sums3) || bad_ptr(W2) || bad_ptr(W3) || bad_ptr(dg2) ||
      bad_ptr(dbe2) || bad_ptr(dW3) || bad_ptr(db3) || bad_ptr(dW2) || bad_ptr(db2) || bad_ptr(df2) || bad_ptr(dh1m) || bad_ptr(sums1b) ||
      bad_ptr(scratch))
    return 1;
  if (training ? (bad_ptr(sums2_local) || bad_ptr(sums2)) : (sums2_local != nullptr || sums2 != nullptr)) return 1;
  hipStream_t st = (hipStream_t)stream;
  const long long R = M * n;
  const XView xv{x, s0, s1, s2, s3, G, n};
  const Scratch sc = carve(M, n, 1, 4, 1);
  float* p3l = at<float>(scratch, sc.a);
  float* p3g = at<float>(scratch, sc.b);
  float* p2 = at<float>(scratch, sc.c);
  float* dS = at<float>(scratch, sc.d);
  float* dg = at<float>(scratch, sc.e);
  float* coef = at<float>(scratch, sc.f);
  double* db3_64 = at<double>(scratch, sc.g);
  double* part_s1 = at<double>(scratch, sc.g + (size_t)C3 * sizeof(double));
  bwd_coef2_kernel<<<1, C3, 0, st>>>(sums3_local, sums3, sums2_local, sums2, training, g2, fold2, coef, dg2, dbe2, db3_64, db3);
  db2_kernel<<<1, C2, 0, st>>>(db3_64, W3, db2);
  const ADy3 dy3{dh3m, y3, fold2, coef};
  ds_kernel<<<blocks(M * C3, NT), NT, 0, st>>>(M, n, dy3, dS);
  wgrad<ADy3, APlain>(R, C3, C2, dy3, APlain{f2, C2}, p3l, dW3, C3, C2, st);
  wgrad<APlain, APlain>(M, C3, C2, APlain{dS, C3}, APlain{g, C2}, p3g, dW3, C3, 0, st);
  gemm<APlain, false, EBias>(M, C3, C2, APlain{dS, C3}, W3, C3, 0, EBias{dg, C2, nullptr}, st);
  gemm<ADy3, false, EArgAdd>(R, C3, C2, dy3, W3, C3, C2, EArgAdd{df2, arg2, dg, n}, st);
  wgrad<APlain, AH1>(R, C2, C1, APlain{df2, C2}, AH1{xv, fold1}, p2, dW2, C1, 0, st);
  gemm<APlain, false, EMaskH1>(R, C2, C1, APlain{df2, C2}, W2, C1, 0, EMaskH1{dh1m, xv, fold1}, st);
  colstats(R, C1, SXhat1{dh1m, xv, fold1}, part_s1, st);
  stats_final(R, C1, part_s1, sums1b, st);
  return launched();
}

int u3d_tok_bwd_3(const float* x, long long s0, long long s1, long long s2, long long s3, int B, int G, int n, const float* dh1m,
                  const float* fold1, const float* g1, const double* sums1_local, const double* sums1, const double* sums1b_local,
                  const double* sums1b, int training, const float* W1, float* dg1, float* dbe1, float* dW1, float* db1, float* dx,
                  void* scratch, void* stream) {
  if (B < 1 || G < 1) return 1;
  const long long M = (long long)B * G;
  if (int rc = check_shape(M, n, 1)) return rc;
  if (bad_x(x, s0, s1, s2, s3) || bad_ptr(dh1m) || bad_ptr(fold1) || bad_ptr(g1) || bad_ptr(sums1b_local) || bad_ptr(sums1b) ||
      bad_ptr(W1) || bad_ptr(dg1) || bad_ptr(dbe1) || bad_ptr(dW1) || bad_ptr(db1) || !aligned16(dx) || bad_ptr(scratch))
    return 1;
  if (training ? (bad_ptr(sums1_local) || bad_ptr(sums1)) : (sums1_local != nullptr || sums1 != nullptr)) return 1;
  hipStream_t st = (hipStream_t)stream;
  const long long R = M * n;
  const XView xv{x, s0, s1, s2, s3, G, n};
  const Scratch sc = carve(M, n, 1, 5, 1);
  float* coef = at<float>(scratch, sc.a);
  double* part = at<double>(scratch, sc.b);
  const int splits = stat_splits(R);
  bwd_coef1_kernel<<<1, C1, 0, st>>>(sums1b_local, sums1b, sums1_local, sums1, training, g1, fold1, W1, coef, dg1, dbe1, db1);
  b3_kernel<<<splits, C1, 0, st>>>(R, xv, dh1m, fold1, coef, stat_rows_per_split(R), part);
  b3_final_kernel<<<blocks(C1 * 4, NT), NT, 0, st>>>(splits, part, dW1);
  if (dx) dx_kernel<<<blocks(R, NT), NT, 0, st>>>(R, xv, dh1m, fold1, coef, W1, dx);
  return launched();
}

}  // extern "C"
