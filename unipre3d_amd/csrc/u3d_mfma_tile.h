// The 64 x 64 x 32 tile product on v_mfma_f32_16x16x4_f32 that the libraries with a linear layer share (internal, like u3d_group.h:
// header-only, no shared object, no public boundary).  Included by u3d_tokenizer.hip, u3d_image_fusion.hip and u3d_sparseconv.hip.
//
// Tile pieces, used by all six MFMA kernels.  A workgroup of NT threads owns a BM x BN block of the output and walks the reduction in
// LDS stages of BK: ATile As[i][k], BTile Bs[k][j], padded against bank conflicts.  Each wave owns a 32 x 32 quarter (wave_of) as
// 2 x 2 MFMA blocks; stage_product is the fragment map and the issue order (kk ascending, i outer, j inner), so it fixes the order of
// every fp32 fma chain and with it the bits of every output; acc_row / acc_col are the map from accumulator element back to (row,
// column).  The loops around them stay in each kernel, and so does the staging that fills As / Bs: sparseconv's kernels
// (gemm_mfma_kernel, wgrad_mfma_kernel) keep their tap loop, their source lists and their skips of empty taps and empty row steps.
// Two pieces stop short, both for the machine code they gave (EXPERIMENTS.md).  The epilogue's i, v, j loops stay in the kernels,
// around acc_row / acc_col: as one function over two callables they changed the register counts of eight of the fourteen
// instantiations.  And sparseconv's two kernels keep a copy of stage_product's block (the reason is given there): a change of the
// fragment map is made here and in those two places.
//
// The whole plain product, used by the tokenizer and the image fusion.  gemm_kernel / gemm() is Y = op(A) W^T or op(A) W; wgrad_kernel
// is the split weight gradient part[split] = A^T G, with wgrad_rows_per_split / wgrad_splits its one split rule.  What differs
// between the products is a template argument: how an operand element is made (prep(row) once per row and stage, get(ctx, k) per
// element), what the epilogue stores (store(row, col, v)), and what a weight gradient adds on the side (NoSide: nothing).  The
// libraries keep their operand makers, epilogues and side policies, and whatever sums the splits.
//
// NOT shared, and to stay apart: sparseconv's VALU kernels, its split_sum / split_sum_wave and colsum kernels and its own split rule
// (it depends on K and the tile count); u3d_mha.hip and u3d_attention.hip, whose fragments live in registers across the whole
// product and which have no LDS block tile.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "u3d_util.h"

namespace u3d_mfma_tile {

constexpr int NT = 256;                       // threads per workgroup (four waves)
constexpr int BM = 64, BN = 64, BK = 32;      // block tile: 64 rows x 64 columns, 32 of the reduction per LDS stage
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float ATile[BM][BK + 1];
typedef float BTile[BK][BN + 4];

// ---- tile pieces -------------------------------------------------------------------------------------------------------------------
struct Wave {   // a thread's lane and the corner of its wave's 32 x 32 quarter
  int lane, wr, wc;
};
__device__ __forceinline__ Wave wave_of(int tid) {
  const int wave = tid >> 6;
  return Wave{tid & 63, (wave >> 1) * 32, (wave & 1) * 32};
}
__device__ __forceinline__ void zero(f32x4 (&acc)[2][2]) {
  for (int i = 0; i < 2; ++i)
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
}
// acc += As Bs over one stage (between the caller's two barriers)
__device__ __forceinline__ void stage_product(const ATile& As, const BTile& Bs, const Wave& w, f32x4 (&acc)[2][2]) {
#pragma unroll
  for (int kk = 0; kk < BK; kk += 4) {
    float a[2], b[2];
    for (int i = 0; i < 2; ++i) a[i] = As[w.wr + i * 16 + (w.lane & 15)][kk + (w.lane >> 4)];
    for (int j = 0; j < 2; ++j) b[j] = Bs[kk + (w.lane >> 4)][w.wc + j * 16 + (w.lane & 15)];
    for (int i = 0; i < 2; ++i)
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
  }
}
// where the thread's element acc[i][j][v] lies: row and column in the tile, added to the caller's `base` (the tile's origin, in the
// caller's own index type: the sum is then formed term by term as the kernels always formed it).  An epilogue walks i, v, j in
// that order and tests the row once, before its two columns.
template <class Index>
__device__ __forceinline__ Index acc_row(const Wave& w, Index base, int i, int v) { return base + w.wr + i * 16 + (w.lane >> 4) * 4 + v; }
__device__ __forceinline__ int acc_col(const Wave& w, int base, int j) { return base + w.wc + j * 16 + (w.lane & 15); }

// ---- Y = op(A) B --------------------------------------------------------------------------------------------------------------------
// BT: B[k][n] = W[n ldw + woff + k] (Y = A W^T), else B[k][n] = W[k ldw + woff + n] (Y = A W)
template <class AOp, bool BT, class Epi>
__global__ __launch_bounds__(NT) void gemm_kernel(long long R, int K, int N, AOp aop, const float* __restrict__ W, int ldw, int woff,
                                                  Epi epi) {
  __shared__ ATile As;
  __shared__ BTile Bs;
  const int tid = threadIdx.x;
  const long long r0 = (long long)blockIdx.x * BM;
  const int n0 = blockIdx.y * BN;
  const Wave w = wave_of(tid);
  f32x4 acc[2][2];
  zero(acc);
  const int ar = tid >> 2, ac = (tid & 3) * 8;     // A stage: 4 threads per row, 8 consecutive k each
  const bool alive = r0 + ar < R;
  const typename AOp::Ctx ctx = aop.prep(alive ? r0 + ar : 0);
  for (int c0 = 0; c0 < K; c0 += BK) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = c0 + ac + j;
      As[ar][ac + j] = (alive && c < K) ? aop.get(ctx, c) : 0.f;
    }
    if (BT) {                                      // 4 threads per column, 8 consecutive k each
      const int bn = tid >> 2, bk0 = (tid & 3) * 8, nn = n0 + bn;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + bk0 + j;
        Bs[bk0 + j][bn] = (nn < N && c < K) ? W[(size_t)nn * ldw + woff + c] : 0.f;
      }
    } else {                                       // 8 threads per k, 8 consecutive columns each
      const int bk = tid >> 3, bc = (tid & 7) * 8, c = c0 + bk;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int nn = n0 + bc + j;
        Bs[bk][bc + j] = (c < K && nn < N) ? W[(size_t)c * ldw + woff + nn] : 0.f;
      }
    }
    __syncthreads();
    stage_product(As, Bs, w, acc);
    __syncthreads();
  }
  for (int i = 0; i < 2; ++i)
    for (int v = 0; v < 4; ++v) {
      const long long r = acc_row(w, r0, i, v);
      if (r >= R) continue;
      for (int j = 0; j < 2; ++j) {
        const int col = acc_col(w, n0, j);
        if (col < N) epi.store(r, col, acc[i][j][v]);
      }
    }
}

template <class AOp, bool BT, class Epi>
void gemm(long long R, int K, int N, const AOp& aop, const float* W, int ldw, int woff, const Epi& epi, hipStream_t st) {
  gemm_kernel<AOp, BT, Epi><<<dim3(u3d_util::blocks(R, BM), u3d_util::blocks(N, BN)), NT, 0, st>>>(R, K, N, aop, W, ldw, woff, epi);
}

// ---- weight gradients: fixed-order split reductions ------------------------------------------------------------------------------
inline long long wgrad_rows_per_split(long long rows) {
  const long long s = std::max(1ll, std::min(64ll, (rows + 255) / 256));
  return ((rows + s - 1) / s + BK - 1) / BK * BK;
}
inline int wgrad_splits(long long rows) { const long long rps = wgrad_rows_per_split(rows); return (int)((rows + rps - 1) / rps); }

// what a weight gradient adds on the side: a value per thread (Acc) that stage() may feed from As after the stage barrier and
// finish() may store after the partial is written; here nothing, and both compile to nothing
struct NoSide {
  struct Acc {};
  __device__ __forceinline__ void stage(Acc&, const ATile&, int /*co0*/, int /*tid*/) const {}
  __device__ __forceinline__ void finish(const Acc&, int /*split*/, int /*ci0*/, int /*co0*/, int /*Ma*/, int /*tid*/) const {}
};

// part[split] (Ma x Ng) = sum over the split's rows r of a(r, i) g(r, j), rows in ascending 32-row steps
template <class AOp, class GOp, class Side = NoSide>
__global__ __launch_bounds__(NT) void wgrad_kernel(long long R, int Ma, int Ng, AOp aop, GOp gop, long long rps, float* __restrict__ part,
                                                   Side side = Side()) {
  __shared__ ATile As;    // As[i][row]
  __shared__ BTile Gs;    // Gs[row][j]
  const int tci = u3d_util::blocks(Ma, BM);
  const int ci0 = (blockIdx.x % tci) * BM, co0 = (blockIdx.x / tci) * BN;
  const int split = blockIdx.y;
  const long long r_beg = split * rps, r_end = min(R, r_beg + rps);
  const int tid = threadIdx.x;
  const Wave w = wave_of(tid);
  f32x4 acc[2][2];
  zero(acc);
  typename Side::Acc sacc;
  const int lr = tid >> 3, lc = (tid & 7) * 8;    // 8 threads per row, 8 consecutive channels each
  for (long long r0 = r_beg; r0 < r_end; r0 += BK) {
    const long long r = r0 + lr;
    const bool live = r < r_end;
    const typename AOp::Ctx ca = aop.prep(live ? r : 0);
    const typename GOp::Ctx cg = gop.prep(live ? r : 0);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = ci0 + lc + j;
      As[lc + j][lr] = (live && c < Ma) ? aop.get(ca, c) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = co0 + lc + j;
      Gs[lr][lc + j] = (live && c < Ng) ? gop.get(cg, c) : 0.f;
    }
    __syncthreads();
    side.stage(sacc, As, co0, tid);
    stage_product(As, Gs, w, acc);
    __syncthreads();
  }
  float* p = part + (size_t)split * Ma * Ng;
  for (int i = 0; i < 2; ++i)
    for (int v = 0; v < 4; ++v) {
      const int ci = acc_row(w, ci0, i, v);
      if (ci >= Ma) continue;
      for (int j = 0; j < 2; ++j) {
        const int co = acc_col(w, co0, j);
        if (co < Ng) p[(size_t)ci * Ng + co] = acc[i][j][v];
      }
    }
  side.finish(sacc, split, ci0, co0, Ma, tid);
}

}  // namespace u3d_mfma_tile
