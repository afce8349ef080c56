// libunipre3d_image_fusion.so: GroupNorm + 1x1 convolution of the object-level image branch, evaluated only at the pixel columns the
// z-buffer fusion selects (include/unipre3d_image_fusion.h).  One bandwidth pass over the decoder map for GroupNorm's statistics; the
// forward is the shared f32-MFMA product (u3d_mfma_tile.h) with an operand prologue that normalises the gathered rows; the backward is
// the shared split weight-gradient product S = dout^T xhat (with s = column sums of dout on the side) and two small finishing kernels.
// f64 sums in a fixed order, no atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "unipre3d_image_fusion.h"
#include "u3d_mfma_tile.h"
#include "u3d_util.h"

namespace {

using namespace u3d_util;
using namespace u3d_mfma_tile;                // NT, the block tile, gemm(), wgrad_kernel and its split rule

constexpr int CHUNK = 8192;                   // floats of a group one workgroup of the statistics pass sums (a multiple of 4)
constexpr int MAX_CHANNELS = 8192;

// ---- statistics -------------------------------------------------------------------------------------------------------------------
int stats_chunks(long long L) { return (int)((L + CHUNK - 1) / CHUNK); }

// part[block][2] = sum and sum of squares of the block's chunk: a scalar head up to the next 16-byte boundary, float4 loads, a scalar
// tail; every thread adds its elements in ascending order, the threads are added in a fixed tree
__global__ __launch_bounds__(NT) void stats_partial_kernel(const float* __restrict__ x, long long L, int chunks, double* __restrict__ part) {
  __shared__ double sh[NT];
  const int tid = threadIdx.x;
  const long long seg = blockIdx.x / chunks;
  const int chunk = blockIdx.x - (int)(seg * chunks);
  const long long e0 = seg * L + (long long)chunk * CHUNK;                       // float index into the (16-byte aligned) map
  const long long left = L - (long long)chunk * CHUNK;
  const int n = left < CHUNK ? (int)left : CHUNK;
  const float* p = x + e0;
  const int lead = (int)((4 - (e0 & 3)) & 3), head = lead < n ? lead : n;
  const int nv = (n - head) >> 2, tail0 = head + nv * 4;
  double s1 = 0.0, s2 = 0.0;
  if (tid < head) {
    const double v = p[tid];
    s1 += v;
    s2 += v * v;
  }
  const float4* pv = reinterpret_cast<const float4*>(p + head);
#pragma unroll 4
  for (int i = tid; i < nv; i += NT) {
    const float4 q = pv[i];
    const double a = q.x, b = q.y, c = q.z, d = q.w;
    s1 += a; s2 += a * a;
    s1 += b; s2 += b * b;
    s1 += c; s2 += c * c;
    s1 += d; s2 += d * d;
  }
  if (tid < n - tail0) {
    const double v = p[tail0 + tid];
    s1 += v;
    s2 += v * v;
  }
  const double t1 = block_tree_sum<NT>(s1, sh);
  const double t2 = block_tree_sum<NT>(s2, sh);
  if (tid == 0) {
    part[(size_t)blockIdx.x * 2] = t1;
    part[(size_t)blockIdx.x * 2 + 1] = t2;
  }
}

// stats[seg] = (mean, rstd): the group's chunks in order
__global__ __launch_bounds__(NT) void stats_final_kernel(int segs, int chunks, double L, double eps, const double* __restrict__ part,
                                                         float* __restrict__ stats) {
  const int seg = blockIdx.x * NT + threadIdx.x;
  if (seg >= segs) return;
  double s1 = 0.0, s2 = 0.0;
  for (int q = 0; q < chunks; ++q) {
    s1 += part[((size_t)seg * chunks + q) * 2];
    s2 += part[((size_t)seg * chunks + q) * 2 + 1];
  }
  const double mean = s1 / L;
  double var = s2 / L - mean * mean;
  var = var > 0.0 ? var : 0.0;
  stats[(size_t)seg * 2] = (float)mean;
  stats[(size_t)seg * 2 + 1] = (float)(1.0 / sqrt(var + eps));
}

// ---- operands -----------------------------------------------------------------------------------------------------------------------
struct RowView {   // the gathered rows with what normalises them
  const float* rows;
  const int32_t* sel;
  const float* stats;
  int N, Cin, G;
  uint32_t magic;    // ceil(2^32 / channels per group), 0 for one channel per group: k / cpg = (k magic) >> 32, exact for k, cpg <= 8192
  struct Ctx { const float* row; const float* st; bool win; };
  __device__ __forceinline__ Ctx prep(long long r) const { return Ctx{rows + r * Cin, stats + (r / N) * G * 2, sel[r] >= 0}; }
  __device__ __forceinline__ float xhat(const Ctx& c, int k) const {
    const int g = magic ? (int)__umulhi((uint32_t)k, magic) : k;
    return c.win ? (c.row[k] - c.st[2 * g]) * c.st[2 * g + 1] : 0.f;
  }
};
struct ANorm {     // xhat gamma + beta of a winner row, zeros of any other
  RowView v;
  const float* gamma;
  const float* beta;
  typedef RowView::Ctx Ctx;
  __device__ __forceinline__ Ctx prep(long long r) const { return v.prep(r); }
  __device__ __forceinline__ float get(const Ctx& c, int k) const { return c.win ? fmaf(v.xhat(c, k), gamma[k], beta[k]) : 0.f; }
};
struct AXhat {
  RowView v;
  typedef RowView::Ctx Ctx;
  __device__ __forceinline__ Ctx prep(long long r) const { return v.prep(r); }
  __device__ __forceinline__ float get(const Ctx& c, int k) const { return v.xhat(c, k); }
};
struct ADout {     // the cotangent of a winner row, zeros of any other (whatever it holds there)
  const float* d;
  const int32_t* sel;
  int Cout;
  struct Ctx { const float* row; bool win; };
  __device__ __forceinline__ Ctx prep(long long r) const { return Ctx{d + r * Cout, sel[r] >= 0}; }
  __device__ __forceinline__ float get(const Ctx& c, int k) const { return c.win ? c.row[k] : 0.f; }
};

uint32_t group_magic(int cpg) { return cpg == 1 ? 0u : (uint32_t)((1ull << 32) / (uint32_t)cpg + 1); }

// ---- what the shared products (u3d_mfma_tile.h) store ------------------------------------------------------------------------------
struct EWinner {   // forward: out = [winner] (y W^T + bias)
  const int32_t* sel;
  const float* bias;
  float* out;
  int Nc;
  __device__ __forceinline__ void store(long long r, int col, float v) const { out[r * Nc + col] = sel[r] >= 0 ? v + bias[col] : 0.f; }
};
struct ColSum {    // backward: the workgroups of the first column tile also add spart[split][o] = sum of dout(r, o), row after row
  float* spart;
  struct Acc { float sum = 0.f; };
  __device__ __forceinline__ void stage(Acc& a, const ATile& As, int co0, int tid) const {
    if (co0 == 0 && tid < BM)
      for (int q = 0; q < BK; ++q) a.sum += As[tid][q];
  }
  __device__ __forceinline__ void finish(const Acc& a, int split, int ci0, int co0, int Ma, int tid) const {
    if (co0 == 0 && tid < BM && ci0 + tid < Ma) spart[(size_t)split * Ma + ci0 + tid] = a.sum;
  }
};

// ---- backward ---------------------------------------------------------------------------------------------------------------------
// S and s from the splits in order; dW = gamma S + beta s, dbias = s
__global__ __launch_bounds__(NT) void finish_weight_kernel(int Cout, int Cin, int splits, const float* __restrict__ part,
                                                           const float* __restrict__ spart, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* __restrict__ S, float* __restrict__ s,
                                                           float* __restrict__ dW, float* __restrict__ dbias) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x, n = (long long)Cout * Cin;
  if (t >= n) return;
  const int o = (int)(t / Cin), c = (int)(t - (long long)o * Cin);
  float Ss = 0.f, ss = 0.f;
  for (int q = 0; q < splits; ++q) {
    Ss += part[(size_t)q * n + t];
    ss += spart[(size_t)q * Cout + o];
  }
  S[t] = Ss;
  dW[t] = fmaf(gamma[c], Ss, beta[c] * ss);
  if (c == 0) {
    s[o] = ss;
    dbias[o] = ss;
  }
}

// dgamma[c] = sum_o W[o][c] S[o][c], dbeta[c] = sum_o W[o][c] s[o] in f64: 64 channels x 4 phases of o per workgroup, phases in order
__global__ __launch_bounds__(NT) void finish_affine_kernel(int Cout, int Cin, const float* __restrict__ W, const float* __restrict__ S,
                                                           const float* __restrict__ s, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta) {
  __shared__ double red[2][4][64];
  const int cl = threadIdx.x & 63, ph = threadIdx.x >> 6, c = blockIdx.x * 64 + cl;
  double a = 0.0, b = 0.0;
  if (c < Cin)
    for (int o = ph; o < Cout; o += 4) {
      const double w = W[(size_t)o * Cin + c];
      a += w * (double)S[(size_t)o * Cin + c];
      b += w * (double)s[o];
    }
  red[0][ph][cl] = a;
  red[1][ph][cl] = b;
  __syncthreads();
  if (ph == 0 && c < Cin) {
    double t1 = red[0][0][cl], t2 = red[1][0][cl];
    for (int w = 1; w < 4; ++w) { t1 += red[0][w][cl]; t2 += red[1][w][cl]; }
    dgamma[c] = (float)t1;
    dbeta[c] = (float)t2;
  }
}

// ---- shapes and scratch -----------------------------------------------------------------------------------------------------------
int check_map(int B, int Cin, int G, int H, int W) {
  if (B < 1 || Cin < 1 || G < 1 || H < 1 || W < 1 || Cin % G != 0) return 1;
  if (Cin > MAX_CHANNELS) return 2;
  const long long L = (long long)(Cin / G) * H * W;
  if (L >= (1ll << 31) || (long long)B * G * stats_chunks(L) >= (1ll << 31)) return 2;
  return 0;
}
int check_rows(int B, int N, int Cin, int G, int Cout) {
  if (B < 1 || N < 1 || Cin < 1 || G < 1 || Cout < 1 || Cin % G != 0) return 1;
  if (Cin > MAX_CHANNELS || Cout > MAX_CHANNELS || (long long)B * N >= (1ll << 31)) return 2;
  return 0;
}
struct BwdScratch {   // byte offsets, every one a multiple of 16
  size_t part, spart, S, s, total;
};
BwdScratch carve(long long R, int Cin, int Cout) {
  const size_t splits = (size_t)wgrad_splits(R);
  auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
  BwdScratch b;
  b.part = 0;
  b.spart = b.part + up(splits * Cout * Cin * sizeof(float));
  b.S = b.spart + up(splits * Cout * sizeof(float));
  b.s = b.S + up((size_t)Cout * Cin * sizeof(float));
  b.total = b.s + up((size_t)Cout * sizeof(float));
  return b;
}

}  // namespace

extern "C" {

int u3d_imgfus_abi_version(void) { return U3D_IMGFUS_ABI_VERSION; }

int u3d_imgfus_stats_chunks(int Cin, int G, int H, int W) {
  return check_map(1, Cin, G, H, W) ? 0 : stats_chunks((long long)(Cin / G) * H * W);
}

int u3d_imgfus_row_splits(long long rows) { return rows < 1 ? 0 : wgrad_splits(rows); }

size_t u3d_imgfus_stats_scratch_bytes(int B, int Cin, int G, int H, int W) {
  if (check_map(B, Cin, G, H, W)) return 0;
  return (size_t)B * G * stats_chunks((long long)(Cin / G) * H * W) * 2 * sizeof(double);
}

size_t u3d_imgfus_backward_scratch_bytes(int B, int N, int Cin, int Cout) {
  if (check_rows(B, N, Cin, 1, Cout)) return 0;
  return carve((long long)B * N, Cin, Cout).total;
}

int u3d_imgfus_stats(const float* map, int B, int Cin, int G, int H, int W, float eps, float* stats, void* scratch, void* stream) {
  if (int rc = check_map(B, Cin, G, H, W)) return rc;
  if (bad_ptr(map) || bad_ptr(stats) || bad_ptr(scratch) || !(eps >= 0.f)) return 1;
  hipStream_t st = (hipStream_t)stream;
  const long long L = (long long)(Cin / G) * H * W;
  const int chunks = stats_chunks(L), segs = B * G;
  double* part = (double*)scratch;
  stats_partial_kernel<<<(unsigned)((long long)segs * chunks), NT, 0, st>>>(map, L, chunks, part);
  stats_final_kernel<<<blocks(segs, NT), NT, 0, st>>>(segs, chunks, (double)L, (double)eps, part, stats);
  return launched();
}

int u3d_imgfus_rows_forward(const float* rows, const int32_t* sel, const float* stats, const float* gamma, const float* beta,
                            const float* weight, const float* bias, int B, int N, int Cin, int G, int Cout, float* out, void* stream) {
  if (int rc = check_rows(B, N, Cin, G, Cout)) return rc;
  if (bad_ptr(rows) || bad_ptr(sel) || bad_ptr(stats) || bad_ptr(gamma) || bad_ptr(beta) || bad_ptr(weight) || bad_ptr(bias) || bad_ptr(out))
    return 1;
  hipStream_t st = (hipStream_t)stream;
  const long long R = (long long)B * N;
  const ANorm aop{RowView{rows, sel, stats, N, Cin, G, group_magic(Cin / G)}, gamma, beta};
  gemm<ANorm, true, EWinner>(R, Cin, Cout, aop, weight, Cin, 0, EWinner{sel, bias, out, Cout}, st);
  return launched();
}

int u3d_imgfus_rows_backward(const float* dout, const float* rows, const int32_t* sel, const float* stats, const float* gamma,
                             const float* beta, const float* weight, int B, int N, int Cin, int G, int Cout, float* dweight,
                             float* dbias, float* dgamma, float* dbeta, void* scratch, void* stream) {
  if (int rc = check_rows(B, N, Cin, G, Cout)) return rc;
  if (bad_ptr(dout) || bad_ptr(rows) || bad_ptr(sel) || bad_ptr(stats) || bad_ptr(gamma) || bad_ptr(beta) || bad_ptr(weight) ||
      bad_ptr(dweight) || bad_ptr(dbias) || bad_ptr(dgamma) || bad_ptr(dbeta) || bad_ptr(scratch))
    return 1;
  hipStream_t st = (hipStream_t)stream;
  const long long R = (long long)B * N;
  const BwdScratch sc = carve(R, Cin, Cout);
  float* part = (float*)((char*)scratch + sc.part);
  float* spart = (float*)((char*)scratch + sc.spart);
  float* S = (float*)((char*)scratch + sc.S);
  float* s = (float*)((char*)scratch + sc.s);
  const int splits = wgrad_splits(R);
  const RowView rv{rows, sel, stats, N, Cin, G, group_magic(Cin / G)};
  wgrad_kernel<ADout, AXhat, ColSum><<<dim3(blocks(Cout, BM) * blocks(Cin, BN), splits), NT, 0, st>>>(
      R, Cout, Cin, ADout{dout, sel, Cout}, AXhat{rv}, wgrad_rows_per_split(R), part, ColSum{spart});
  finish_weight_kernel<<<blocks((long long)Cout * Cin, NT), NT, 0, st>>>(Cout, Cin, splits, part, spart, gamma, beta, S, s, dweight, dbias);
  finish_affine_kernel<<<blocks(Cin, 64), NT, 0, st>>>(Cout, Cin, weight, S, s, dgamma, dbeta);
  return launched();
}

}  // extern "C"
