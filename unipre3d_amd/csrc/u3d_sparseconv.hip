// Sparse 3D convolution for the scene backbones: kernel maps built on the device by a stable radix sort of site keys, implicit GEMM
// on the f32 MFMA (gather form, every output row written once), fixed-order split reductions for the weight and bias gradients;
// see include/unipre3d_sparseconv.h.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "unipre3d_sparseconv.h"
#include "u3d_keysort.h"
#include "u3d_mfma_tile.h"

namespace {

using namespace u3d_util;

// the MFMA tile pieces: constants, LDS tile types, the wave's quarter and the accumulator-to-position map are shared; the loops around
// them are this library's own, and so is the fragment-load-and-MFMA block of its two kernels, a copy of tile::stage_product to be
// kept in step with it: called as the function, the block compiled to other code here (wgrad_mfma_kernel 45 -> 32 VGPRs and 16 -> 32
// AGPRs, gemm_mfma_kernel 42 -> 47 VGPRs) and the weight gradient measured 4 - 9 % slower at 32 - 128 channels (EXPERIMENTS.md)
namespace tile = u3d_mfma_tile;
constexpr int NT = 256;              // threads per workgroup (four waves)
constexpr int NW = NT / 64;
constexpr int ITEMS = 16;            // rounds of NT elements per tile of the sort and scan passes
constexpr int TILE = NT * ITEMS;
constexpr int SCAN_NT = 1024;        // the one-workgroup exclusive scan
// the class boundaries are public (unipre3d_sparseconv.h): the tests place their shapes on both sides of each
using tile::BM; using tile::BN; using tile::BK;   // GEMM block tile: 64 rows x 64 columns, 32 of the reduction per LDS stage
static_assert(BM == U3D_SPCONV_TILE && BN == U3D_SPCONV_TILE && BK == U3D_SPCONV_KSTEP && NT == tile::NT, "the public class boundaries are the shared tile");
constexpr int SMALL_C = U3D_SPCONV_SMALL_C;   // a channel count at or below this takes the VALU kernels (the stem's Cin = 3 / 6)
constexpr int WAVE_SUM_SPLITS = U3D_SPCONV_WAVE_SUM_SPLITS;

inline int bit_len(unsigned long long v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }

struct Scratch {   // carved out of the caller's buffer; every array sized for n rows
  unsigned long long* keys[2];
  uint32_t* vals[2];
  uint32_t* pos;      // identity positions for the tap-major pass of the strided map
  uint32_t* rank;     // output row of each sorted position (strided map)
  uint32_t* hist;     // 256 digit counts per tile + 256 totals (also the per-tile head counts)
};

size_t carve(void* base, int n_rows, Scratch* s) {
  const size_t n = (size_t)(n_rows > 0 ? n_rows : 1);
  const size_t nb = (size_t)blocks((long long)n, TILE);
  Carver c{(char*)base};
  Scratch t;
  t.keys[0] = c.take<unsigned long long>(n * 8);
  t.keys[1] = c.take<unsigned long long>(n * 8);
  t.vals[0] = c.take<uint32_t>(n * 4);
  t.vals[1] = c.take<uint32_t>(n * 4);
  t.pos = c.take<uint32_t>(n * 4);
  t.rank = c.take<uint32_t>(n * 4);
  t.hist = c.take<uint32_t>((nb + 1) * 256 * 4);
  if (s) *s = t;
  return c.off;
}

// first position of key k in the ascending keys[0, n)
__device__ __forceinline__ int lower_bound(const unsigned long long* __restrict__ keys, int n, unsigned long long k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// ---- stable LSD radix sort of (64-bit key, 32-bit value), 8 bits per pass ----------------------------------------------------
// digit: byte `pass` of the key, or (tap_k > 0) the tap key % tap_k of a composite key (255 for the sentinel >= limit)
struct Digit {
  int pass, tap_k; unsigned long long limit;
  __device__ uint32_t operator()(unsigned long long k) const {
    if (tap_k > 0) return k >= limit ? 255u : (uint32_t)(k % (unsigned long long)tap_k);
    return (uint32_t)(k >> (8 * pass)) & 255u;
  }
};

__global__ __launch_bounds__(NT) void radix_hist_kernel(Digit dg, int n, int nb, const unsigned long long* __restrict__ kin,
                                                        uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t base = blockIdx.x * (uint32_t)TILE;
  for (int r = 0; r < ITEMS; ++r) {
    const uint32_t i = base + r * NT + threadIdx.x;
    if (i < (uint32_t)n) atomicAdd(&h[dg(kin[i])], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];   // digit-major: a scan of each digit's row gives (digit, tile) bases
}

// stable scatter of one tile: rounds of NT elements ranked by the ballot multi-split (element order = round, wave, lane)
__global__ __launch_bounds__(NT) void radix_scatter_kernel(Digit dg, int n, int nb, const uint32_t* __restrict__ hist,
                                                           const unsigned long long* __restrict__ kin, const uint32_t* __restrict__ vin,
                                                           unsigned long long* __restrict__ kout, uint32_t* __restrict__ vout) {
  __shared__ RadixLds<NW> lds;
  const uint32_t base = blockIdx.x * (uint32_t)TILE;
  radix_bases<NW>(lds, hist, hist + (size_t)nb * 256, nb);
  for (int r = 0; r < ITEMS; ++r) {
    radix_round_begin<NW>(lds);
    const uint32_t i = base + r * NT + threadIdx.x;
    const bool valid = i < (uint32_t)n;
    unsigned long long k = 0; uint32_t v = 0, digit = 0;
    if (valid) { k = kin[i]; v = vin[i]; digit = dg(k); }
    const uint32_t dst = radix_round_dst<NW>(lds, valid, digit);
    if (valid) {
      kout[dst] = k;
      vout[dst] = v;
    }
    __syncthreads();
  }
}

// sorts (keys[0], vals[0]) over `passes` bytes (or one tap pass); returns the buffer that holds the result
int radix_sort(const Scratch& s, int n, int first_buf, int passes, int tap_k, unsigned long long limit, hipStream_t st) {
  const int nb = blocks(n, TILE);
  int a = first_buf;
  for (int p = 0; p < passes; ++p) {
    const Digit dg{p, tap_k, limit};
    radix_hist_kernel<<<nb, NT, 0, st>>>(dg, n, nb, s.keys[a], s.hist);
    digit_scan_kernel<NT><<<256, NT, 0, st>>>(nb, s.hist);
    radix_scatter_kernel<<<nb, NT, 0, st>>>(dg, n, nb, s.hist, s.keys[a], tap_k > 0 ? s.pos : s.vals[a], s.keys[a ^ 1], s.vals[a ^ 1]);
    a ^= 1;
  }
  return a;
}

// ---- keys ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void site_key_kernel(int n, const int32_t* __restrict__ idx, int D0, int D1, int D2,
                                                      unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const int4 c = reinterpret_cast<const int4*>(idx)[i];
  keys[i] = (((unsigned long long)c.x * D0 + c.y) * D1 + c.z) * D2 + c.w;
  vals[i] = (uint32_t)i;
}

// composite key of a strided conv (kernel == stride = s): output site * K + tap; rows outside the output grid get `limit`
__global__ __launch_bounds__(NT) void down_key_kernel(int n, const int32_t* __restrict__ idx, int s, int O0, int O1, int O2,
                                                      unsigned long long limit, unsigned long long* __restrict__ keys,
                                                      uint32_t* __restrict__ vals, uint32_t* __restrict__ pos) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const int4 c = reinterpret_cast<const int4*>(idx)[i];
  const int o0 = c.y / s, o1 = c.z / s, o2 = c.w / s;
  const int K = s * s * s;
  const int tap = ((c.y - o0 * s) * s + (c.z - o1 * s)) * s + (c.w - o2 * s);
  const bool in = o0 < O0 && o1 < O1 && o2 < O2;
  keys[i] = in ? ((((unsigned long long)c.x * O0 + o0) * O1 + o1) * O2 + o2) * K + tap : limit;
  vals[i] = (uint32_t)i;
  pos[i] = (uint32_t)i;
}

// ---- SubM map ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void subm_table_kernel(int n, int k, const int32_t* __restrict__ idx, int D0, int D1, int D2,
                                                        const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                        int32_t* __restrict__ table) {
  const int K = k * k * k;
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= (long long)n * K) return;
  const int o = (int)(t / K), tap = (int)(t - (long long)o * K);
  const int h = k / 2;
  const int4 c = reinterpret_cast<const int4*>(idx)[o];
  const int a0 = c.y + tap / (k * k) - h, a1 = c.z + (tap / k) % k - h, a2 = c.w + tap % k - h;
  int32_t r = -1;
  if (a0 >= 0 && a0 < D0 && a1 >= 0 && a1 < D1 && a2 >= 0 && a2 < D2) {
    const unsigned long long nk = (((unsigned long long)c.x * D0 + a0) * D1 + a1) * D2 + a2;
    const int p = lower_bound(keys, n, nk);
    if (p < n && keys[p] == nk) r = (int32_t)vals[p];   // the stable sort puts a site's lowest row first
  }
  table[t] = r;
}

// first (lowest row at the same site) and next (following row at the same site) from the sorted order
__global__ __launch_bounds__(NT) void chain_kernel(int n, unsigned long long limit, const unsigned long long* __restrict__ keys,
                                                   const uint32_t* __restrict__ vals, int32_t* __restrict__ first, int32_t* __restrict__ next) {
  const int j = blockIdx.x * NT + threadIdx.x;
  if (j >= n) return;
  const unsigned long long k = keys[j];
  const uint32_t r = vals[j];
  if (k >= limit) { first[r] = (int32_t)r; next[r] = -1; return; }   // a row dropped by a strided map stands alone
  first[r] = (int32_t)vals[lower_bound(keys, j, k) + 0];
  next[r] = (j + 1 < n && keys[j + 1] == k) ? (int32_t)vals[j + 1] : -1;
}

// ---- strided map: output heads, ranks, table, output indices, tap-major list ---------------------------------------------------
__device__ __forceinline__ bool out_head(const unsigned long long* keys, int j, int K, unsigned long long limit) {
  return keys[j] < limit && (j == 0 || keys[j] / K != keys[j - 1] / K);
}

struct OutHeadOp {   // rank = output row of each sorted position
  const unsigned long long* keys; int K; unsigned long long limit; uint32_t* rank;
  __device__ bool flag(uint32_t i) const { return out_head(keys, (int)i, K, limit); }
  __device__ void emit(uint32_t i, uint32_t r, bool f) const { rank[i] = f ? r : r - 1u; }   // r = heads before i
};

__global__ __launch_bounds__(NT) void down_emit_kernel(int n, int K, unsigned long long limit, int O0, int O1, int O2,
                                                       const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                       const uint32_t* __restrict__ rank, int32_t* __restrict__ out_idx,
                                                       int32_t* __restrict__ table) {
  const int j = blockIdx.x * NT + threadIdx.x;
  if (j >= n) return;
  const unsigned long long k = keys[j];
  if (k >= limit) return;
  const uint32_t o = rank[j];
  if (j == 0 || keys[j - 1] != k) table[(size_t)o * K + (int)(k % K)] = (int32_t)vals[j];
  if (out_head(keys, j, K, limit)) {
    unsigned long long q = k / K;
    const int c2 = (int)(q % O2); q /= O2;
    const int c1 = (int)(q % O1); q /= O1;
    const int c0 = (int)(q % O0); q /= O0;
    reinterpret_cast<int4*>(out_idx)[o] = make_int4((int)q, c0, c1, c2);
  }
}

// list entry e of the (tap, output, row) order: its row and output * K + tap (-1: dropped)
__global__ __launch_bounds__(NT) void list_kernel(int n, int K, unsigned long long limit, const unsigned long long* __restrict__ tkeys,
                                                  const uint32_t* __restrict__ tpos, const uint32_t* __restrict__ vals,
                                                  const uint32_t* __restrict__ rank, int32_t* __restrict__ list_row,
                                                  int32_t* __restrict__ list_src) {
  const int e = blockIdx.x * NT + threadIdx.x;
  if (e >= n) return;
  const uint32_t j = tpos[e];
  const unsigned long long k = tkeys[e];
  list_row[e] = (int32_t)vals[j];
  list_src[e] = k >= limit ? -1 : (int32_t)(rank[j] * (uint32_t)K + (uint32_t)(k % K));
}

// ---- implicit GEMM -----------------------------------------------------------------------------------------------------------
// source row of entry e at tap k: the table's entry (table mode) or the list's output when its tap is k (list mode)
__device__ __forceinline__ int src_of(const int32_t* __restrict__ tab, bool list, int K, int e, int k) {
  if (!list) return tab[(size_t)e * K + k];
  const int v = tab[e];
  return (v >= 0 && v % K == k) ? v / K : -1;
}

// Y[out(e)] = bias + sum_k A[src(e,k)] . W[k] on v_mfma_f32_16x16x4_f32 (exact f32 fma chains).  64 x 64 block tile, each wave
// a 32 x 32 quarter as 2 x 2 MFMA blocks; a tap with no source in the block's 64 rows is skipped.
__global__ __launch_bounds__(NT) void gemm_mfma_kernel(int R, int K, int Cin, int Cout, const int32_t* __restrict__ tab,
                                                       const int32_t* __restrict__ list_row, const float* __restrict__ A,
                                                       const float* __restrict__ W, const float* __restrict__ bias,
                                                       const int32_t* __restrict__ mask, float* __restrict__ Y) {
  __shared__ tile::ATile As;
  __shared__ tile::BTile Bs;
  __shared__ int srcs[BM];
  const bool list = list_row != nullptr;
  const int tid = threadIdx.x;
  const int e0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const tile::Wave w = tile::wave_of(tid);
  tile::f32x4 acc[2][2];
  tile::zero(acc);
  const int ar = tid >> 2, ac = (tid & 3) * 8;     // A stage: 4 threads per row, 8 consecutive channels each
  const int bk = tid >> 3, bc = (tid & 7) * 8;     // B stage: 8 threads per reduction row, 8 consecutive columns each
  for (int k = 0; k < K; ++k) {
    int s = -1;
    if (tid < BM && e0 + tid < R) s = src_of(tab, list, K, e0 + tid, k);
    if (tid < BM) srcs[tid] = s;
    if (!__syncthreads_or(s >= 0)) continue;
    const int sa = srcs[ar];
    const float* arow = A + (size_t)(sa >= 0 ? sa : 0) * Cin;
    const float* wk = W + (size_t)k * Cin * Cout;
    for (int c0 = 0; c0 < Cin; c0 += BK) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + ac + j;
        As[ar][ac + j] = (sa >= 0 && c < Cin) ? arow[c] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int c = c0 + bk, nn = n0 + bc + j;
        Bs[bk][bc + j] = (c < Cin && nn < Cout) ? wk[(size_t)c * Cout + nn] : 0.f;
      }
      __syncthreads();
#pragma unroll
      for (int kk = 0; kk < BK; kk += 4) {         // tile::stage_product's block (the note at `namespace tile`)
        float a[2], b[2];
        for (int i = 0; i < 2; ++i) a[i] = As[w.wr + i * 16 + (w.lane & 15)][kk + (w.lane >> 4)];
        for (int j = 0; j < 2; ++j) b[j] = Bs[kk + (w.lane >> 4)][w.wc + j * 16 + (w.lane & 15)];
        for (int i = 0; i < 2; ++i)
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
      }
      __syncthreads();
    }
  }
  for (int i = 0; i < 2; ++i)
    for (int v = 0; v < 4; ++v) {
      const int e = tile::acc_row(w, e0, i, v);
      if (e >= R) continue;
      const int o = list ? list_row[e] : e;
      const bool zero = mask && mask[o] != o;
      for (int j = 0; j < 2; ++j) {
        const int col = tile::acc_col(w, n0, j);
        if (col < Cout) Y[(size_t)o * Cout + col] = zero ? 0.f : acc[i][j][v] + (bias ? bias[col] : 0.f);
      }
    }
}

// the same product on the VALU for small channel counts: one thread per output element, taps and channels in order
__global__ __launch_bounds__(NT) void gemm_valu_kernel(int R, int K, int Cin, int Cout, const int32_t* __restrict__ tab,
                                                       const int32_t* __restrict__ list_row, const float* __restrict__ A,
                                                       const float* __restrict__ W, const float* __restrict__ bias,
                                                       const int32_t* __restrict__ mask, float* __restrict__ Y) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= (long long)R * Cout) return;
  const int e = (int)(t / Cout), col = (int)(t - (long long)e * Cout);
  const bool list = list_row != nullptr;
  const int o = list ? list_row[e] : e;
  float acc = 0.f;
  for (int k = 0; k < K; ++k) {
    const int s = src_of(tab, list, K, e, k);
    if (s < 0) continue;
    const float* a = A + (size_t)s * Cin;
    const float* w = W + (size_t)k * Cin * Cout + col;
    for (int c = 0; c < Cin; ++c) acc = fmaf(a[c], w[(size_t)c * Cout], acc);
  }
  Y[(size_t)o * Cout + col] = (mask && mask[o] != o) ? 0.f : acc + (bias ? bias[col] : 0.f);
}

__global__ __launch_bounds__(NT) void dupsum_kernel(int n, int C, const int32_t* __restrict__ first, const int32_t* __restrict__ next,
                                                    const float* __restrict__ in, float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= (long long)n * C) return;
  const int r = (int)(t / C), c = (int)(t - (long long)r * C);
  float s = 0.f;
  if (first[r] == r) {
    s = in[t];
    for (int j = next[r]; j >= 0; j = next[j]) s += in[(size_t)j * C + c];   // rows at the site in ascending order
  }
  out[t] = s;
}

// ---- weight and bias gradients: fixed-order split reductions --------------------------------------------------------------------
int wgrad_splits(int R, int K, int Cin, int Cout) {
  if (Cin <= SMALL_C || Cout <= SMALL_C) return std::max(1, std::min(256, blocks(R, 512)));   // VALU: short serial row loops
  const int want = std::max(1, 2048 / std::max(1, blocks(Cin, BM) * blocks(Cout, BN) * K));
  return std::max(1, std::min(want, blocks(R, 256)));
}
int wgrad_rows_per_split(int R, int splits) { return blocks(blocks(R, splits), BK) * BK; }

// part[split][k] (Cin x Cout) = sum over the split's rows o of A[ia]^T G[ig]; a 32-row step with no source at tap k is skipped
__global__ __launch_bounds__(NT) void wgrad_mfma_kernel(int R, int K, int Cin, int Cout, const int32_t* __restrict__ tab, int gather_g,
                                                        const float* __restrict__ A, const float* __restrict__ G, int rps,
                                                        float* __restrict__ part) {
  __shared__ tile::ATile As;    // As[ci][row]
  __shared__ tile::BTile Gs;    // Gs[row][co]
  __shared__ int srcs[BK];
  const int tci = blocks(Cin, BM);
  const int ci0 = (blockIdx.x % tci) * BM, co0 = (blockIdx.x / tci) * BN;
  const int k = blockIdx.y, split = blockIdx.z;
  const int r_beg = split * rps, r_end = min(R, r_beg + rps);
  const int tid = threadIdx.x;
  const tile::Wave w = tile::wave_of(tid);
  tile::f32x4 acc[2][2];
  tile::zero(acc);
  const int lr = tid >> 3, lc = (tid & 7) * 8;    // 8 threads per row, 8 consecutive channels each
  for (int r0 = r_beg; r0 < r_end; r0 += BK) {
    int s = -1;
    if (tid < BK && r0 + tid < r_end) s = tab[(size_t)(r0 + tid) * K + k];
    if (tid < BK) srcs[tid] = s;
    if (!__syncthreads_or(s >= 0)) continue;
    const int sr = srcs[lr];
    const bool live = sr >= 0;
    const int ia = gather_g ? r0 + lr : sr, ig = gather_g ? sr : r0 + lr;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = ci0 + lc + j;
      As[lc + j][lr] = (live && c < Cin) ? A[(size_t)ia * Cin + c] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int c = co0 + lc + j;
      Gs[lr][lc + j] = (live && c < Cout) ? G[(size_t)ig * Cout + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < BK; kk += 4) {           // tile::stage_product's block (the note at `namespace tile`)
      float a[2], b[2];
      for (int i = 0; i < 2; ++i) a[i] = As[w.wr + i * 16 + (w.lane & 15)][kk + (w.lane >> 4)];
      for (int j = 0; j < 2; ++j) b[j] = Gs[kk + (w.lane >> 4)][w.wc + j * 16 + (w.lane & 15)];
      for (int i = 0; i < 2; ++i)
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  float* p = part + ((size_t)split * K + k) * Cin * Cout;
  for (int i = 0; i < 2; ++i)
    for (int v = 0; v < 4; ++v) {
      const int ci = tile::acc_row(w, ci0, i, v);
      if (ci >= Cin) continue;
      for (int j = 0; j < 2; ++j) {
        const int co = tile::acc_col(w, co0, j);
        if (co < Cout) p[(size_t)ci * Cout + co] = acc[i][j][v];
      }
    }
}

// small channel counts: one thread per (k, large channel) of a split, the <= SMALL_C small channels in registers, rows in order
template <bool CIN_SMALL>
__global__ __launch_bounds__(NT) void wgrad_valu_kernel(int R, int K, int Cin, int Cout, const int32_t* __restrict__ tab, int gather_g,
                                                        const float* __restrict__ A, const float* __restrict__ G, int rps,
                                                        float* __restrict__ part) {
  const int big = CIN_SMALL ? Cout : Cin, small = CIN_SMALL ? Cin : Cout;
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= (long long)K * big) return;
  const int k = (int)(t / big), c = (int)(t - (long long)k * big);
  const int split = blockIdx.y, r_beg = split * rps, r_end = min(R, r_beg + rps);
  float acc[SMALL_C];
#pragma unroll
  for (int j = 0; j < SMALL_C; ++j) acc[j] = 0.f;
  for (int o = r_beg; o < r_end; ++o) {
    const int s = tab[(size_t)o * K + k];
    if (s < 0) continue;
    const float* a = A + (size_t)(gather_g ? o : s) * Cin;
    const float* g = G + (size_t)(gather_g ? s : o) * Cout;
    const float x = CIN_SMALL ? g[c] : a[c];
#pragma unroll
    for (int j = 0; j < SMALL_C; ++j)
      if (j < small) acc[j] = fmaf(CIN_SMALL ? a[j] : x, CIN_SMALL ? x : g[j], acc[j]);
  }
  float* p = part + ((size_t)split * K + k) * Cin * Cout;
#pragma unroll
  for (int j = 0; j < SMALL_C; ++j)
    if (j < small) p[CIN_SMALL ? (size_t)j * Cout + c : (size_t)c * Cout + j] = acc[j];
}

// out[t] = sum over splits of part[split][t]: a thread per output in split order, or (many splits) a wave per output, lanes over
// splits in order and a fixed butterfly across the lanes
__global__ __launch_bounds__(NT) void split_sum_kernel(long long n, int splits, const float* __restrict__ part, float* __restrict__ out) {
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t >= n) return;
  float s = 0.f;
  for (int q = 0; q < splits; ++q) s += part[(size_t)q * n + t];
  out[t] = s;
}

__global__ __launch_bounds__(NT) void split_sum_wave_kernel(long long n, int splits, const float* __restrict__ part, float* __restrict__ out) {
  const long long w = ((long long)blockIdx.x * NT + threadIdx.x) >> 6;
  if (w >= n) return;
  const int lane = (int)lane_id();
  float s = 0.f;
  for (int q = lane; q < splits; q += 64) s += part[(size_t)q * n + w];
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
  if (lane == 0) out[w] = s;
}

void split_sum(long long n, int splits, const float* part, float* out, hipStream_t st) {
  if (splits >= WAVE_SUM_SPLITS) split_sum_wave_kernel<<<blocks(n * 64, NT), NT, 0, st>>>(n, splits, part, out);
  else split_sum_kernel<<<blocks(n, NT), NT, 0, st>>>(n, splits, part, out);
}

int colsum_splits(int R) { return std::max(1, std::min(256, blocks(R, 2048))); }

// part[split][c] = sum over the split's rows: 64 columns x 4 row phases per workgroup, phases combined in order
__global__ __launch_bounds__(NT) void colsum_kernel(int R, int C, const float* __restrict__ G, int rps, float* __restrict__ part) {
  __shared__ float red[NW][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), ph = threadIdx.x >> 6;
  const int r_beg = blockIdx.y * rps, r_end = min(R, r_beg + rps);
  float s = 0.f;
  if (c < C)
    for (int r = r_beg + ph; r < r_end; r += NW) s += G[(size_t)r * C + c];
  red[ph][threadIdx.x & 63] = s;
  __syncthreads();
  if (ph == 0 && c < C) {
    float t = red[0][threadIdx.x];
    for (int w = 1; w < NW; ++w) t += red[w][threadIdx.x];
    part[(size_t)blockIdx.y * C + c] = t;
  }
}

int check_shape(int n_batch, int D0, int D1, int D2) {
  if (n_batch < 1 || D0 < 1 || D1 < 1 || D2 < 1) return 1;
  const double sites = (double)n_batch * D0 * D1 * D2;
  return sites * 216.0 < 9.0e18 ? 0 : 2;   // keys (times the largest tap count) fit in 63 bits
}

}  // namespace

extern "C" {

int u3d_spconv_abi_version(void) { return U3D_SPCONV_ABI_VERSION; }

size_t u3d_spconv_scratch_bytes(int n) { return n < 0 ? 0 : carve(nullptr, n, nullptr); }

int u3d_spconv_subm_map(int N, const int32_t* indices, int n_batch, int D0, int D1, int D2, int k, int32_t* table, int32_t* first,
                        int32_t* next, void* scratch, void* stream) {
  if (N < 0 || k < 1 || !(k & 1) || k > 7) return 1;
  if (int rc = check_shape(n_batch, D0, D1, D2)) return rc;
  if (N == 0) return 0;
  if (!indices || !table || !first || !next || !scratch) return 1;
  const int K = k * k * k;
  if ((long long)N * K >= (1ll << 31)) return 2;
  hipStream_t st = (hipStream_t)stream;
  Scratch s;
  carve(scratch, N, &s);
  const unsigned long long limit = (unsigned long long)n_batch * D0 * D1 * D2;
  site_key_kernel<<<blocks(N, NT), NT, 0, st>>>(N, indices, D0, D1, D2, s.keys[0], s.vals[0]);
  const int fb = radix_sort(s, N, 0, (bit_len(limit - 1) + 7) / 8, 0, 0, st);
  subm_table_kernel<<<blocks((long long)N * K, NT), NT, 0, st>>>(N, k, indices, D0, D1, D2, s.keys[fb], s.vals[fb], table);
  chain_kernel<<<blocks(N, NT), NT, 0, st>>>(N, limit, s.keys[fb], s.vals[fb], first, next);
  return launched();
}

static void down_geometry(int n_batch, int D0, int D1, int D2, int s, int* O, unsigned long long* limit) {
  O[0] = (D0 - s) / s + 1; O[1] = (D1 - s) / s + 1; O[2] = (D2 - s) / s + 1;
  *limit = (unsigned long long)n_batch * O[0] * O[1] * O[2] * (unsigned long long)(s * s * s);
}

int u3d_spconv_down_map(int N, const int32_t* indices, int n_batch, int D0, int D1, int D2, int s, int32_t* meta, void* scratch,
                        void* stream) {
  if (N < 0 || s < 1 || s > 6 || !meta) return 1;
  if (int rc = check_shape(n_batch, D0, D1, D2)) return rc;
  if (D0 < s || D1 < s || D2 < s) return 2;
  hipStream_t st = (hipStream_t)stream;
  (void)hipMemsetAsync(meta, 0, 4 * sizeof(int32_t), st);
  if (N == 0) return launched();
  if (!indices || !scratch) return 1;
  Scratch sc;
  carve(scratch, N, &sc);
  int O[3];
  unsigned long long limit;
  down_geometry(n_batch, D0, D1, D2, s, O, &limit);
  const int K = s * s * s;
  down_key_kernel<<<blocks(N, NT), NT, 0, st>>>(N, indices, s, O[0], O[1], O[2], limit, sc.keys[0], sc.vals[0], sc.pos);
  const int fb = radix_sort(sc, N, 0, (bit_len(limit) + 7) / 8, 0, 0, st);
  const int nb = blocks(N, TILE);
  const OutHeadOp op{sc.keys[fb], K, limit, sc.rank};
  flag_count_kernel<NT, ITEMS, OutHeadOp><<<nb, NT, 0, st>>>(op, N, nullptr, sc.hist);
  scan_kernel<SCAN_NT><<<1, SCAN_NT, 0, st>>>(nb, sc.hist, meta);
  flag_apply_kernel<NT, ITEMS, OutHeadOp><<<nb, NT, 0, st>>>(op, N, nullptr, sc.hist);
  return launched();
}

int u3d_spconv_down_emit(int N, int M, const int32_t* indices, int n_batch, int D0, int D1, int D2, int s, int32_t* out_indices,
                         int32_t* table, int32_t* first, int32_t* next, int32_t* list_row, int32_t* list_src, void* scratch,
                         void* stream) {
  if (N < 0 || M < 0 || M > N || s < 1 || s > 6) return 1;
  if (int rc = check_shape(n_batch, D0, D1, D2)) return rc;
  if (N == 0) return 0;
  if (!indices || !first || !next || !list_row || !list_src || !scratch || (M > 0 && (!out_indices || !table))) return 1;
  hipStream_t st = (hipStream_t)stream;
  Scratch sc;
  carve(scratch, N, &sc);
  int O[3];
  unsigned long long limit;
  down_geometry(n_batch, D0, D1, D2, s, O, &limit);
  const int K = s * s * s;
  const int fb = ((bit_len(limit) + 7) / 8) & 1;   // where u3d_spconv_down_map's sort left (keys, rows)
  if (M > 0) {
    (void)hipMemsetAsync(table, 0xff, (size_t)M * K * sizeof(int32_t), st);
    down_emit_kernel<<<blocks(N, NT), NT, 0, st>>>(N, K, limit, O[0], O[1], O[2], sc.keys[fb], sc.vals[fb], sc.rank, out_indices, table);
  }
  chain_kernel<<<blocks(N, NT), NT, 0, st>>>(N, limit, sc.keys[fb], sc.vals[fb], first, next);
  // one stable pass on the tap reorders the sorted positions (tap, output, row); the rows stay in vals[fb]
  radix_sort(sc, N, fb, 1, K, limit, st);
  list_kernel<<<blocks(N, NT), NT, 0, st>>>(N, K, limit, sc.keys[fb ^ 1], sc.vals[fb ^ 1], sc.vals[fb], sc.rank, list_row, list_src);
  return launched();
}

int u3d_spconv_gemm(int R, int K, int Cin, int Cout, const int32_t* table, const int32_t* list_row, const float* A, const float* W,
                    const float* bias, const int32_t* mask, float* Y, void* stream) {
  if (R < 0 || K < 1 || Cin < 0 || Cout < 0) return 1;
  if ((long long)R * Cout == 0) return 0;
  if (!table || !Y || (Cin > 0 && (!A || !W))) return 1;
  if ((long long)R * K >= (1ll << 31) || (long long)R * Cout >= (1ll << 40)) return 2;
  hipStream_t st = (hipStream_t)stream;
  if (Cin <= SMALL_C || Cout <= SMALL_C)
    gemm_valu_kernel<<<blocks((long long)R * Cout, NT), NT, 0, st>>>(R, K, Cin, Cout, table, list_row, A, W, bias, mask, Y);
  else
    gemm_mfma_kernel<<<dim3(blocks(R, BM), blocks(Cout, BN)), NT, 0, st>>>(R, K, Cin, Cout, table, list_row, A, W, bias, mask, Y);
  return launched();
}

int u3d_spconv_dupsum(int N, int C, const int32_t* first, const int32_t* next, const float* in, float* out, void* stream) {
  if (N < 0 || C < 0) return 1;
  if ((long long)N * C == 0) return 0;
  if (!first || !next || !in || !out) return 1;
  dupsum_kernel<<<blocks((long long)N * C, NT), NT, 0, (hipStream_t)stream>>>(N, C, first, next, in, out);
  return launched();
}

size_t u3d_spconv_wgrad_partial_floats(int R, int K, int Cin, int Cout) {
  if (R < 0 || K < 1 || Cin < 0 || Cout < 0) return 0;
  return (size_t)wgrad_splits(R, K, Cin, Cout) * K * Cin * Cout;
}

int u3d_spconv_wgrad(int R, int K, int Cin, int Cout, const int32_t* table, int gather_g, const float* A, const float* G, float* partial,
                     float* dW, void* stream) {
  if (R < 0 || K < 1 || Cin < 0 || Cout < 0) return 1;
  const long long nw = (long long)K * Cin * Cout;
  if (nw == 0) return 0;
  if (!dW) return 1;
  hipStream_t st = (hipStream_t)stream;
  if (R == 0) {
    (void)hipMemsetAsync(dW, 0, (size_t)nw * sizeof(float), st);
    return launched();
  }
  if (!table || !A || !G || !partial) return 1;
  if ((long long)R * K >= (1ll << 31)) return 2;
  const int splits = wgrad_splits(R, K, Cin, Cout), rps = wgrad_rows_per_split(R, splits);
  if (Cin <= SMALL_C)
    wgrad_valu_kernel<true><<<dim3(blocks((long long)K * Cout, NT), splits), NT, 0, st>>>(R, K, Cin, Cout, table, gather_g, A, G, rps,
                                                                                         partial);
  else if (Cout <= SMALL_C)
    wgrad_valu_kernel<false><<<dim3(blocks((long long)K * Cin, NT), splits), NT, 0, st>>>(R, K, Cin, Cout, table, gather_g, A, G, rps,
                                                                                          partial);
  else
    wgrad_mfma_kernel<<<dim3(blocks(Cin, BM) * blocks(Cout, BN), K, splits), NT, 0, st>>>(R, K, Cin, Cout, table, gather_g, A, G, rps,
                                                                                          partial);
  split_sum(nw, splits, partial, dW, st);
  return launched();
}

size_t u3d_spconv_colsum_partial_floats(int R, int C) { return R < 0 || C < 0 ? 0 : (size_t)colsum_splits(R) * C; }

int u3d_spconv_colsum(int R, int C, const float* G, float* partial, float* db, void* stream) {
  if (R < 0 || C < 0) return 1;
  if (C == 0) return 0;
  if (!db) return 1;
  hipStream_t st = (hipStream_t)stream;
  if (R == 0) {
    (void)hipMemsetAsync(db, 0, (size_t)C * sizeof(float), st);
    return launched();
  }
  if (!G || !partial) return 1;
  const int splits = colsum_splits(R), rps = blocks(R, splits);
  colsum_kernel<<<dim3(blocks(C, 64), splits), NT, 0, st>>>(R, C, G, rps, partial);
  split_sum(C, splits, partial, db, st);
  return launched();
}

}  // extern "C"
