// PTv3's index plumbing on the device: space-filling-curve codes (one thread per point, registers only), a stable LSD radix sort of
// (64-bit code, 32-bit index) with the row of codes on the second grid dimension, the patch padding of SerializedAttention in one
// launch, and the pooling clusters of SerializedPooling in a count stage and an emit stage; see include/unipre3d_serialization.h.
// Integers only: no float math, no float atomics, every result element is written once with an ordinary store.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unipre3d_serialization.h"
#include "u3d_keysort.h"

namespace {

using namespace u3d_util;

typedef unsigned long long u64;

constexpr int NT = 256;              // threads per workgroup (four waves)
constexpr int NW = NT / 64;
constexpr int ITEMS = 16;            // rounds of NT elements per tile of the sort and scan passes
constexpr int TILE = NT * ITEMS;
constexpr int SCAN_NT = 1024;        // the one-workgroup exclusive scan

struct Scratch {   // carved out of the caller's buffer for K rows of n elements
  u64* keys[2];
  uint32_t* vals[2];
  uint32_t* rank;     // cluster of each sorted position (pooling, row 0 only)
  uint32_t* hist;     // per row: 256 digit counts per tile, then 256 totals (row 0 also holds the per-tile head counts)
};

size_t carve(void* base, int K, int n_rows, Scratch* s) {
  const size_t n = (size_t)(n_rows > 0 ? n_rows : 1), k = (size_t)(K > 0 ? K : 1);
  const size_t nb = (size_t)blocks((long long)n, TILE);
  Carver c{(char*)base};
  Scratch t;
  t.keys[0] = c.take<u64>(k * n * 8);
  t.keys[1] = c.take<u64>(k * n * 8);
  t.vals[0] = c.take<uint32_t>(k * n * 4);
  t.vals[1] = c.take<uint32_t>(k * n * 4);
  t.rank = c.take<uint32_t>(n * 4);
  t.hist = c.take<uint32_t>(k * (nb + 1) * 256 * 4);
  if (s) *s = t;
  return c.off;
}

// ---- codes -----------------------------------------------------------------------------------------------------------------------
// bit i of v (i < 21) to bit 3 i
__host__ __device__ inline u64 spread3(u64 v) {
  v &= 0x1fffffull;
  v = (v | (v << 32)) & 0x1f00000000ffffull;
  v = (v | (v << 16)) & 0x1f0000ff0000ffull;
  v = (v | (v << 8)) & 0x100f00f00f00f00full;
  v = (v | (v << 4)) & 0x10c30c30c30c30c3ull;
  v = (v | (v << 2)) & 0x1249249249249249ull;
  return v;
}

__host__ __device__ inline u64 z_code(uint32_t a, uint32_t b, uint32_t c) {
  return (spread3(a) << 2) | (spread3(b) << 1) | spread3(c);
}

// Skilling's axes-to-transpose walk from the top bit down on three registers, then the interleave (axis 0 in the high bit of a
// triple) and the Gray-to-binary fold of the whole 3 * depth bit word
__host__ __device__ inline u64 hilbert_code(uint32_t x0, uint32_t x1, uint32_t x2, int depth) {
  for (uint32_t q = 1u << (depth - 1); q > 1; q >>= 1) {
    const uint32_t p = q - 1;
    if (x0 & q) x0 ^= p;                                  // axis 0: invert (the exchange with itself is empty)
    if (x1 & q) x0 ^= p; else { const uint32_t t = (x0 ^ x1) & p; x0 ^= t; x1 ^= t; }
    if (x2 & q) x0 ^= p; else { const uint32_t t = (x0 ^ x2) & p; x0 ^= t; x2 ^= t; }
  }
  u64 g = z_code(x0, x1, x2);
  g ^= g >> 1; g ^= g >> 2; g ^= g >> 4; g ^= g >> 8; g ^= g >> 16; g ^= g >> 32;
  return g;
}

__host__ __device__ inline u64 curve_code(int order, uint32_t c0, uint32_t c1, uint32_t c2, int depth) {
  if (order & 1) { const uint32_t t = c0; c0 = c1; c1 = t; }
  return (order & 2) ? hilbert_code(c0, c1, c2, depth) : z_code(c0, c1, c2);
}

template <typename CT>
__global__ __launch_bounds__(NT) void encode_kernel(int n, const CT* __restrict__ coord, const void* __restrict__ batch, int batch64,
                                                    int depth, int K, int orders, long long* __restrict__ code) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  const uint32_t m = (1u << depth) - 1u;
  const uint32_t c0 = (uint32_t)coord[(size_t)i * 3 + 0] & m, c1 = (uint32_t)coord[(size_t)i * 3 + 1] & m,
                 c2 = (uint32_t)coord[(size_t)i * 3 + 2] & m;
  u64 hi = 0;
  if (batch) hi = (u64)(batch64 ? ((const long long*)batch)[i] : (long long)((const int32_t*)batch)[i]) << (3 * depth);
  for (int k = 0; k < K; ++k) code[(size_t)k * n + i] = (long long)(hi | curve_code((orders >> (2 * k)) & 3, c0, c1, c2, depth));
}

// ---- stable LSD radix sort of (64-bit key, 32-bit index), 8 bits per pass, row = blockIdx.y ------------------------------------
// flip: 0, or 0x80 in the top pass of a SIGNED sort (the sign bit inverted puts the negative keys first)
__device__ __forceinline__ uint32_t digit_of(u64 k, int shift, int pre, uint32_t flip = 0) {
  return ((uint32_t)((k >> pre) >> shift) & 255u) ^ flip;
}

// hist: per row 256 x nb counts, digit-major (a scan of each digit's line gives the (digit, tile) bases), then 256 totals
__global__ __launch_bounds__(NT) void radix_hist_kernel(int shift, int pre, uint32_t flip, int n, int nb, size_t kstride,
                                                        const u64* __restrict__ kin, uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  kin += kstride * blockIdx.y;
  hist += (size_t)blockIdx.y * (nb + 1) * 256;
  const uint32_t base = blockIdx.x * (uint32_t)TILE;
  for (int r = 0; r < ITEMS; ++r) {
    const uint32_t i = base + r * NT + threadIdx.x;
    if (i < (uint32_t)n) atomicAdd(&h[digit_of(kin[i], shift, pre, flip)], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

// stable scatter of one tile: rounds of NT elements ranked by the ballot multi-split (element order = round, wave, lane).
// FIRST: the index of an element is its position (no vin).  FINAL: writes order (the index, widened) and inverse, not (kout, vout).
template <bool FIRST, bool FINAL>
__global__ __launch_bounds__(NT) void radix_scatter_kernel(int shift, int pre, uint32_t flip, int n, int nb, const uint32_t* __restrict__ hist,
                                                           size_t kstride, const u64* __restrict__ kin, const uint32_t* __restrict__ vin,
                                                           u64* __restrict__ kout, uint32_t* __restrict__ vout,
                                                           long long* __restrict__ order, long long* __restrict__ inverse) {
  __shared__ RadixLds<NW> lds;
  const size_t row = (size_t)blockIdx.y * n;
  kin += kstride * blockIdx.y;
  hist += (size_t)blockIdx.y * (nb + 1) * 256;
  const uint32_t base = blockIdx.x * (uint32_t)TILE;
  radix_bases<NW>(lds, hist, hist + (size_t)nb * 256, nb);
  for (int r = 0; r < ITEMS; ++r) {
    radix_round_begin<NW>(lds);
    const uint32_t i = base + r * NT + threadIdx.x;
    const bool valid = i < (uint32_t)n;
    u64 k = 0; uint32_t v = 0, digit = 0;
    if (valid) { k = kin[i]; v = FIRST ? i : vin[row + i]; digit = digit_of(k, shift, pre, flip); }
    const uint32_t dst = radix_round_dst<NW>(lds, valid, digit);
    if (valid) {
      if (FINAL) {
        order[row + dst] = (long long)v;
        inverse[row + v] = (long long)dst;
      } else {
        kout[row + dst] = k;
        vout[row + dst] = v;
      }
    }
    __syncthreads();
  }
}

// Sorts K rows of n keys (src, row stride n) on the low key_bits bits of key >> pre.  final: the last pass writes order / inverse;
// otherwise the result is (keys[b], vals[b]) with b the returned buffer.  Keys move unshifted.  is_signed: the keys are int64 and all
// 64 bits are sorted, the top pass with the sign bit inverted.
int radix_sort(const Scratch& s, int K, int n, int key_bits, int pre, const u64* src, bool final, long long* order, long long* inverse,
               hipStream_t st, bool is_signed = false) {
  const int nb = blocks(n, TILE), passes = (key_bits + 7) / 8;
  const dim3 gt(nb, K), gs(256, K);
  const size_t ks = (size_t)n;
  for (int p = 0; p < passes; ++p) {
    const u64* kin = p == 0 ? src : s.keys[(p - 1) & 1];
    const uint32_t* vin = p == 0 ? nullptr : s.vals[(p - 1) & 1];
    u64* kout = s.keys[p & 1];
    uint32_t* vout = s.vals[p & 1];
    const bool last = final && p == passes - 1;
    const uint32_t flip = (is_signed && p == 7) ? 0x80u : 0u;
    radix_hist_kernel<<<gt, NT, 0, st>>>(8 * p, pre, flip, n, nb, ks, kin, s.hist);
    digit_scan_kernel<NT><<<gs, NT, 0, st>>>(nb, s.hist);
    if (p == 0 && last)
      radix_scatter_kernel<true, true><<<gt, NT, 0, st>>>(8 * p, pre, flip, n, nb, s.hist, ks, kin, vin, kout, vout, order, inverse);
    else if (p == 0)
      radix_scatter_kernel<true, false><<<gt, NT, 0, st>>>(8 * p, pre, flip, n, nb, s.hist, ks, kin, vin, kout, vout, order, inverse);
    else if (last)
      radix_scatter_kernel<false, true><<<gt, NT, 0, st>>>(8 * p, pre, flip, n, nb, s.hist, ks, kin, vin, kout, vout, order, inverse);
    else
      radix_scatter_kernel<false, false><<<gt, NT, 0, st>>>(8 * p, pre, flip, n, nb, s.hist, ks, kin, vin, kout, vout, order, inverse);
  }
  return (passes - 1) & 1;
}

// ---- patch padding -----------------------------------------------------------------------------------------------------------------
// the item i with a[i] <= t < a[i + 1] in the ascending a[0 .. B] (a[0] = 0, t < a[B])
__device__ __forceinline__ int item_of(const long long* __restrict__ a, int B, long long t) {
  int lo = 0, hi = B;   // invariant: a[lo] <= t < a[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (a[mid] <= t) lo = mid; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(NT) void patch_padding_kernel(int B, int patch, long long T, long long T_pad, long long S,
                                                           const long long* __restrict__ meta, long long* __restrict__ pad,
                                                           long long* __restrict__ unpad, int32_t* __restrict__ cu) {
  const long long* off = meta;
  const long long* offp = meta + (B + 1);
  const long long* offs = meta + 2 * (size_t)(B + 1);
  const long long t = (long long)blockIdx.x * NT + threadIdx.x;
  if (t < T_pad) {
    const int i = item_of(offp, B, t);
    const long long n = off[i + 1] - off[i], np = offp[i + 1] - offp[i], j = t - offp[i];
    pad[t] = off[i] + ((np != n && j >= n) ? j - patch : j);   // a padded item's tail slots j >= n re-read the patch before
  }
  if (t < T) {
    const int i = item_of(off, B, t);
    unpad[t] = t + offp[i] - off[i];
  }
  if (t < S) {
    const int i = item_of(offs, B, t);
    cu[t] = (int32_t)(offp[i] + (t - offs[i]) * patch);
  } else if (t == S) {
    cu[t] = (int32_t)T_pad;
  }
}

// ---- pooling clusters --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool is_head(const u64* keys, int j, int shift) {
  return j == 0 || (keys[j] >> shift) != (keys[j - 1] >> shift);
}

struct ClusterOp {   // heads of the sorted keys >> shift; rank = cluster of each sorted position
  const u64* keys; int shift; uint32_t* rank;
  __device__ bool flag(uint32_t i) const { return is_head(keys, (int)i, shift); }
  __device__ void emit(uint32_t i, uint32_t r, bool f) const { rank[i] = f ? r : r - 1u; }   // r = heads before i
};

__global__ __launch_bounds__(NT) void pool_emit_kernel(int K, int n, int M, int shift, const long long* __restrict__ code,
                                                       const u64* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                       const uint32_t* __restrict__ rank, long long* __restrict__ cluster,
                                                       long long* __restrict__ indices, long long* __restrict__ idx_ptr,
                                                       long long* __restrict__ head_indices, long long* __restrict__ pcode) {
  const int j = blockIdx.x * NT + threadIdx.x;
  if (j >= n) return;
  const uint32_t r = rank[j], v = vals[j];
  cluster[v] = (long long)r;
  indices[j] = (long long)v;
  if (j == 0) idx_ptr[M] = (long long)n;
  if (r < (uint32_t)M && is_head(keys, j, shift)) {
    idx_ptr[r] = (long long)j;
    head_indices[r] = (long long)v;
    for (int k = 0; k < K; ++k) pcode[(size_t)k * M + r] = code[(size_t)k * n + v] >> shift;
  }
}

bool bad_shape(int K, int N) { return K < 1 || K > 4 || N < 1; }

// ---- PCM's order serialization ---------------------------------------------------------------------------------------------------
// meta: words 0..2 the global maxima of the grid per axis, 3 the depth, 4 the flag, 5..7 zero, then three maxima per item.
constexpr int META_HEAD = U3D_SER_PCM_META_HEAD;
constexpr int SMALL_SORT = U3D_SER_SMALL_SORT;   // most keys the one-workgroup sort takes

struct I3 { long long v[3]; };

// min (IS_MIN) or max over the NT threads of three values, in every thread
template <bool IS_MIN>
__device__ __forceinline__ I3 block_reduce3(I3 x, long long (*sh)[3]) {
  for (int a = 0; a < 3; ++a)
    for (int o = 32; o > 0; o >>= 1) {
      const long long y = __shfl_xor(x.v[a], o);
      x.v[a] = IS_MIN ? (y < x.v[a] ? y : x.v[a]) : (y > x.v[a] ? y : x.v[a]);
    }
  if (lane_id() == 0) for (int a = 0; a < 3; ++a) sh[threadIdx.x >> 6][a] = x.v[a];
  __syncthreads();
  for (int a = 0; a < 3; ++a) {
    long long r = sh[0][a];
    for (int w = 1; w < NW; ++w) r = IS_MIN ? (sh[w][a] < r ? sh[w][a] : r) : (sh[w][a] > r ? sh[w][a] : r);
    x.v[a] = r;
  }
  __syncthreads();
  return x;
}

// floor(p / grid_size) as the reference's int64; the division is IEEE (no fast reciprocal).  A quotient that is not finite or does not
// fit raises `bad` and counts as cell 0.
__device__ __forceinline__ long long cell_of(float p, float grid_size, bool& bad) {
  const float q = floorf(p / grid_size);
  if (!(fabsf(q) < 4.0e18f)) { bad = true; return 0; }
  return (long long)q;
}

// one workgroup per item: the item's minimum cell, then grid = cell - minimum and the item's maxima of it (meta's tail).  A relative
// cell above 65535 is stored clamped to 2^30 and reaches the flag through the maxima; word 0 of an item's maxima carries `bad` in bit 31.
__global__ __launch_bounds__(NT) void pcm_grid_kernel(int N, float grid_size, const float* __restrict__ pos, int32_t* __restrict__ grid,
                                                      int32_t* __restrict__ meta) {
  __shared__ long long sh[NW][3];
  const size_t row0 = (size_t)blockIdx.x * N;
  bool bad = false;
  I3 lo{{INT64_MAX, INT64_MAX, INT64_MAX}};
  for (int i = threadIdx.x; i < N; i += NT)
    for (int a = 0; a < 3; ++a) {
      const long long c = cell_of(pos[(row0 + i) * 3 + a], grid_size, bad);
      lo.v[a] = c < lo.v[a] ? c : lo.v[a];
    }
  lo = block_reduce3<true>(lo, sh);
  I3 hi{{0, 0, 0}};
  for (int i = threadIdx.x; i < N; i += NT)
    for (int a = 0; a < 3; ++a) {
      long long c = cell_of(pos[(row0 + i) * 3 + a], grid_size, bad) - lo.v[a];
      if (c < 0) c = 0;                       // only after `bad`
      if (c > (1ll << 30)) c = 1ll << 30;
      grid[(row0 + i) * 3 + a] = (int32_t)c;
      hi.v[a] = c > hi.v[a] ? c : hi.v[a];
    }
  hi.v[0] |= bad ? (1ll << 31) : 0;           // above every clamped cell: survives the maximum
  hi = block_reduce3<false>(hi, sh);
  if (threadIdx.x < 3) meta[META_HEAD + 3 * blockIdx.x + threadIdx.x] = (int32_t)(uint32_t)hi.v[threadIdx.x];
}

// one workgroup: the global maxima over the B items, the depth (bit_length of the largest) and the flag
__global__ __launch_bounds__(NT) void pcm_meta_kernel(int B, int32_t* __restrict__ meta) {
  __shared__ long long sh[NW][3];
  I3 hi{{0, 0, 0}};
  for (int b = threadIdx.x; b < B; b += NT)
    for (int a = 0; a < 3; ++a) {
      const long long c = (long long)(uint32_t)meta[META_HEAD + 3 * b + a];
      hi.v[a] = c > hi.v[a] ? c : hi.v[a];
    }
  hi = block_reduce3<false>(hi, sh);
  if (threadIdx.x == 0) {
    const bool bad = (hi.v[0] >> 31) & 1;
    hi.v[0] &= 0x7fffffffll;
    long long m = hi.v[0] > hi.v[1] ? hi.v[0] : hi.v[1];
    m = m > hi.v[2] ? m : hi.v[2];
    for (int a = 0; a < 3; ++a) meta[a] = (int32_t)hi.v[a];
    meta[3] = m == 0 ? 0 : 64 - __clzll(m);
    meta[4] = (bad || m > 65535) ? 1 : 0;
    meta[5] = meta[6] = meta[7] = 0;
  }
}

// PCM order ids: 0 z, 1 z-trans, 2 hilbert, 3 hilbert-trans (the library's curves at the meta block's depth, batch << 3 depth above), 4..9 the
// axis orders xyz xzy yxz yzx zxy zyx in closed form: with c1 the first-named axis' cell and m1, m2, m3 the global maxima in the order's
// sequence, s(m) = +1 for even m else -1 and e(m) = m + (m & 1):  code = b m1 m2 m3 + e(m3) m1 m2 + s(m3) (e(m2) m1 + s(m2) c1).
__constant__ const int8_t AXES[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2}, {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

__global__ __launch_bounds__(NT) void pcm_encode_kernel(int N, long long rows, int order, const int32_t* __restrict__ grid,
                                                        const int32_t* __restrict__ meta, long long* __restrict__ code) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  if (i >= rows) return;
  const long long b = i / N;
  if (order < 4) {
    int depth = meta[3];
    depth = depth > 16 ? 16 : depth;                      // flagged by the grid pass; the coordinates are masked
    const uint32_t m = (1u << depth) - 1u;
    const uint32_t c0 = (uint32_t)grid[i * 3 + 0] & m, c1 = (uint32_t)grid[i * 3 + 1] & m, c2 = (uint32_t)grid[i * 3 + 2] & m;
    const u64 curve = depth == 0 ? 0ull : curve_code(order, c0, c1, c2, depth);   // depth 0: one cell, the code is the batch id
    code[i] = (long long)(((u64)b << (3 * depth)) | curve);
  } else {
    const int8_t* ax = AXES[order - 4];
    // in u64, where sums and products wrap as the reference's int64 tensors do (two's complement: -1 is ~0)
    const u64 c1 = (u64)(long long)grid[i * 3 + ax[0]], m1 = (u64)(long long)meta[ax[0]], m2 = (u64)(long long)meta[ax[1]],
              m3 = (u64)(long long)meta[ax[2]];
    const u64 s2 = (m2 & 1) ? ~0ull : 1ull, s3 = (m3 & 1) ? ~0ull : 1ull, e2 = m2 + (m2 & 1), e3 = m3 + (m3 & 1);
    code[i] = (long long)((u64)b * m1 * m2 * m3 + e3 * m1 * m2 + s3 * (e2 * m1 + s2 * c1));
  }
}

// The whole signed sort of n <= SMALL_SORT keys in ONE workgroup: eight LSD passes over (key, index) in the scratch's two buffers, a
// pass whose digit is the same in every key skipped (the decision is the workgroup's own: no host read, no pass count to bound).
// k0/k1/v0/v1 are read and written in turn, hence not __restrict__; __syncthreads orders the workgroup's global stores and loads.
__global__ __launch_bounds__(NT) void small_sort_kernel(int n, const u64* __restrict__ code, u64* k0, u64* k1, uint32_t* v0, uint32_t* v1,
                                                        long long* __restrict__ order, long long* __restrict__ inverse) {
  __shared__ RadixLds<NW> lds;
  __shared__ uint32_t h[256];
  const int tid = threadIdx.x;
  const u64* kin = code;
  const uint32_t* vin = nullptr;
  int nxt = 0;
  for (int p = 0; p < 8; ++p) {
    const int shift = 8 * p;
    const uint32_t flip = p == 7 ? 0x80u : 0u;
    h[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += NT) atomicAdd(&h[digit_of(kin[i], shift, 0, flip)], 1u);
    __syncthreads();
    if (__syncthreads_or(h[tid] == (uint32_t)n)) continue;          // uniform: every thread sees the same answer
    uint32_t all;
    lds.digit_base[tid] = block_excl_scan<NW>(h[tid], lds.wt, all);
    u64* kout = nxt ? k1 : k0;
    uint32_t* vout = nxt ? v1 : v0;
    u64 kn = 0; uint32_t vn = 0;
    if (tid < n) { kn = kin[tid]; vn = vin ? vin[tid] : (uint32_t)tid; }
    for (int base = 0; base < n; base += NT) {
      radix_round_begin<NW>(lds);
      const int i = base + tid;
      const bool valid = i < n;
      const u64 k = kn; const uint32_t v = vn;
      if (i + NT < n) { kn = kin[i + NT]; vn = vin ? vin[i + NT] : (uint32_t)(i + NT); }   // the next round's, in flight over the barriers
      const uint32_t dst = radix_round_dst<NW>(lds, valid, valid ? digit_of(k, shift, 0, flip) : 0u);
      if (valid) { kout[dst] = k; vout[dst] = v; }
      __syncthreads();
    }
    kin = kout; vin = vout; nxt ^= 1;
  }
  for (int i = tid; i < n; i += NT) {
    const uint32_t v = vin ? vin[i] : (uint32_t)i;
    order[i] = (long long)v;
    inverse[v] = (long long)i;
  }
}

// rows of up to 8 tensors moved by one index: dst_t[i] = src_t[index[i]].  V floats per load (4 where every row of the tensor is 16-byte
// aligned); an index outside [0, rows) gives a row of zeros.
struct GatherArgs {
  const float* src[U3D_SER_GATHER_MAX];
  float* dst[U3D_SER_GATHER_MAX];
  int32_t channels[U3D_SER_GATHER_MAX];
  int32_t vec[U3D_SER_GATHER_MAX];
};

template <typename VT>
__device__ __forceinline__ void gather_tensor(long long rows, uint32_t per, const long long* __restrict__ index, const VT* __restrict__ src,
                                              VT* __restrict__ dst) {
  const unsigned long long total = (unsigned long long)rows * per, step = (unsigned long long)gridDim.x * NT;
  for (unsigned long long e = (unsigned long long)blockIdx.x * NT + threadIdx.x; e < total; e += step) {
    unsigned long long row; uint32_t col;
    if (total < (1ull << 32)) { row = (uint32_t)e / per; col = (uint32_t)e - (uint32_t)row * per; }
    else { row = e / per; col = (uint32_t)(e - row * per); }
    const long long j = index[row];
    VT x{};
    if ((unsigned long long)j < (unsigned long long)rows) x = src[(unsigned long long)j * per + col];
    dst[e] = x;
  }
}

__global__ __launch_bounds__(NT) void gather_rows_kernel(long long rows, const long long* __restrict__ index, GatherArgs a) {
  const int t = blockIdx.y;
  if (a.vec[t]) gather_tensor<float4>(rows, (uint32_t)a.channels[t] / 4u, index, (const float4*)a.src[t], (float4*)a.dst[t]);
  else gather_tensor<float>(rows, (uint32_t)a.channels[t], index, a.src[t], a.dst[t]);
}

bool bad_pcm(int B, int N) { return B < 1 || N < 1 || (long long)B * N > U3D_SER_MAX_ROWS; }

}  // namespace

extern "C" {

int u3d_ser_abi_version(void) { return U3D_SER_ABI_VERSION; }

size_t u3d_ser_scratch_bytes(int K, int N) { return bad_shape(K, N) || N > U3D_SER_MAX_ROWS ? 0 : carve(nullptr, K, N, nullptr); }

int u3d_ser_encode(int N, const void* grid_coord, int coord64, const void* batch, int batch64, int depth, int K, int orders,
                   int64_t* code, void* stream) {
  if (bad_shape(K, N) || depth < 1 || depth > 16 || orders < 0 || orders > 255 || !grid_coord || !code) return 1;
  if (N > U3D_SER_MAX_ROWS) return 2;
  hipStream_t st = (hipStream_t)stream;
  if (coord64)
    encode_kernel<long long><<<blocks(N, NT), NT, 0, st>>>(N, (const long long*)grid_coord, batch, batch64, depth, K, orders, (long long*)code);
  else
    encode_kernel<int32_t><<<blocks(N, NT), NT, 0, st>>>(N, (const int32_t*)grid_coord, batch, batch64, depth, K, orders, (long long*)code);
  return launched();
}

int u3d_ser_sort(int K, int N, int key_bits, const int64_t* code, int64_t* order, int64_t* inverse, void* scratch, void* stream) {
  if (bad_shape(K, N) || key_bits < 1 || key_bits > 64 || !code || !order || !inverse || !scratch) return 1;
  if (N > U3D_SER_MAX_ROWS) return 2;
  Scratch s;
  carve(scratch, K, N, &s);
  radix_sort(s, K, N, key_bits, 0, (const u64*)code, true, (long long*)order, (long long*)inverse, (hipStream_t)stream);
  return launched();
}

int u3d_ser_serialize(int N, const void* grid_coord, int coord64, const void* batch, int batch64, int depth, int K, int orders,
                      int key_bits, int64_t* code, int64_t* order, int64_t* inverse, void* scratch, void* stream) {
  if (int rc = u3d_ser_encode(N, grid_coord, coord64, batch, batch64, depth, K, orders, code, stream)) return rc;
  return u3d_ser_sort(K, N, key_bits, code, order, inverse, scratch, stream);
}

int u3d_ser_patch_padding(int B, int patch, long long T, long long T_pad, long long S, const int64_t* meta, int64_t* pad, int64_t* unpad,
                          int32_t* cu_seqlens, void* stream) {
  if (B < 1 || patch < 1 || T < B || T_pad < T || S < B || !meta || !pad || !unpad || !cu_seqlens) return 1;
  if (T_pad >= (1ll << 31)) return 2;   // cu_seqlens is int32
  const long long n = T_pad > S + 1 ? T_pad : S + 1;
  patch_padding_kernel<<<blocks(n, NT), NT, 0, (hipStream_t)stream>>>(B, patch, T, T_pad, S, (const long long*)meta, (long long*)pad,
                                                                      (long long*)unpad, cu_seqlens);
  return launched();
}

int u3d_ser_pool_count(int K, int N, int shift, int key_bits, const int64_t* code, int32_t* meta, void* scratch, void* stream) {
  if (bad_shape(K, N) || shift < 0 || shift > 48 || key_bits < 1 || key_bits + shift > 64 || !code || !meta || !scratch) return 1;
  if (N > U3D_SER_MAX_ROWS) return 2;
  hipStream_t st = (hipStream_t)stream;
  Scratch s;
  carve(scratch, K, N, &s);
  const int fb = radix_sort(s, 1, N, key_bits, shift, (const u64*)code, false, nullptr, nullptr, st);
  const int nb = blocks(N, TILE);
  const ClusterOp op{s.keys[fb], shift, s.rank};
  flag_count_kernel<NT, ITEMS, ClusterOp><<<nb, NT, 0, st>>>(op, N, nullptr, s.hist);
  scan_kernel<SCAN_NT><<<1, SCAN_NT, 0, st>>>(nb, s.hist, meta);
  flag_apply_kernel<NT, ITEMS, ClusterOp><<<nb, NT, 0, st>>>(op, N, nullptr, s.hist);
  return launched();
}

int u3d_ser_pool_emit(int K, int N, int M, int shift, int key_bits, const int64_t* code, int64_t* cluster, int64_t* indices,
                      int64_t* idx_ptr, int64_t* head_indices, int64_t* pcode, int64_t* porder, int64_t* pinverse, void* scratch,
                      void* stream) {
  if (bad_shape(K, N) || M < 1 || M > N || shift < 0 || shift > 48 || key_bits < 1 || key_bits + shift > 64) return 1;
  if (!code || !cluster || !indices || !idx_ptr || !head_indices || !pcode || !porder || !pinverse || !scratch) return 1;
  if (N > U3D_SER_MAX_ROWS) return 2;
  hipStream_t st = (hipStream_t)stream;
  Scratch s;
  carve(scratch, K, N, &s);
  const int fb = ((key_bits + 7) / 8 - 1) & 1;   // where u3d_ser_pool_count's sort left (keys, rows)
  pool_emit_kernel<<<blocks(N, NT), NT, 0, st>>>(K, N, M, shift, (const long long*)code, s.keys[fb], s.vals[fb], s.rank, (long long*)cluster,
                                                 (long long*)indices, (long long*)idx_ptr, (long long*)head_indices, (long long*)pcode);
  // the pooled stage's own sort: the emit above is done with the scratch (same stream), so it is carved again for (K, M)
  Scratch p;
  carve(scratch, K, M, &p);
  radix_sort(p, K, M, key_bits, 0, (const u64*)pcode, true, (long long*)porder, (long long*)pinverse, st);
  return launched();
}

int u3d_ser_pcm_grid(int B, int N, const float* pos, float grid_size, int32_t* grid, int32_t* meta, void* stream) {
  if (bad_pcm(B, N) || !pos || !grid || !meta || !(grid_size > 0.f) || !(grid_size < 3.0e38f)) return 1;
  hipStream_t st = (hipStream_t)stream;
  pcm_grid_kernel<<<B, NT, 0, st>>>(N, grid_size, pos, grid, meta);
  pcm_meta_kernel<<<1, NT, 0, st>>>(B, meta);
  return launched();
}

int u3d_ser_pcm_encode(int B, int N, int order, const int32_t* grid, const int32_t* meta, int64_t* code, void* stream) {
  if (bad_pcm(B, N) || order < 0 || order >= U3D_SER_PCM_ORDERS || !grid || !meta || !code) return 1;
  const long long rows = (long long)B * N;
  pcm_encode_kernel<<<blocks(rows, NT), NT, 0, (hipStream_t)stream>>>(N, rows, order, grid, meta, (long long*)code);
  return launched();
}

int u3d_ser_sort_signed(int N, const int64_t* code, int64_t* order, int64_t* inverse, void* scratch, void* stream) {
  if (N < 1 || !code || !order || !inverse || !scratch) return 1;
  if (N > U3D_SER_MAX_ROWS) return 2;
  hipStream_t st = (hipStream_t)stream;
  Scratch s;
  carve(scratch, 1, N, &s);
  if (N <= SMALL_SORT)
    small_sort_kernel<<<1, NT, 0, st>>>(N, (const u64*)code, s.keys[0], s.keys[1], s.vals[0], s.vals[1], (long long*)order, (long long*)inverse);
  else
    radix_sort(s, 1, N, 64, 0, (const u64*)code, true, (long long*)order, (long long*)inverse, st, true);
  return launched();
}

int u3d_ser_pcm_order(int B, int N, const float* pos, float grid_size, int order, int32_t* grid, int32_t* meta, int64_t* code,
                      int64_t* order_out, int64_t* inverse, void* scratch, void* stream) {
  if (order < 0 || order >= U3D_SER_PCM_ORDERS) return 1;
  if (int rc = u3d_ser_pcm_grid(B, N, pos, grid_size, grid, meta, stream)) return rc;
  if (int rc = u3d_ser_pcm_encode(B, N, order, grid, meta, code, stream)) return rc;
  return u3d_ser_sort_signed(B * N, code, order_out, inverse, scratch, stream);
}

int u3d_ser_gather_rows(long long rows, int T, const int64_t* index, const void* const* src, void* const* dst, const int32_t* channels,
                        void* stream) {
  if (rows < 1 || T < 1 || T > U3D_SER_GATHER_MAX || !index || !src || !dst || !channels) return 1;
  if (rows > U3D_SER_MAX_ROWS) return 2;
  GatherArgs a{};
  long long most = 0;
  for (int t = 0; t < T; ++t) {
    if (!src[t] || !dst[t] || src[t] == dst[t] || channels[t] < 1 || channels[t] > U3D_SER_GATHER_MAX_CHANNELS) return 1;
    a.src[t] = (const float*)src[t];
    a.dst[t] = (float*)dst[t];
    a.channels[t] = channels[t];
    a.vec[t] = channels[t] % 4 == 0 && aligned16(src[t]) && aligned16(dst[t]);
    const long long work = rows * (channels[t] / (a.vec[t] ? 4 : 1));
    most = work > most ? work : most;
  }
  const long long nb = (most + NT - 1) / NT;      // the kernel strides over what 4096 workgroups do not cover
  gather_rows_kernel<<<dim3((unsigned)(nb < 4096 ? nb : 4096), T), NT, 0, (hipStream_t)stream>>>(rows, (const long long*)index, a);
  return launched();
}

}  // extern "C"
