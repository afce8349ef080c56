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
__device__ __forceinline__ uint32_t digit_of(u64 k, int shift, int pre) { return (uint32_t)((k >> pre) >> shift) & 255u; }

// hist: per row 256 x nb counts, digit-major (a scan of each digit's line gives the (digit, tile) bases), then 256 totals
__global__ __launch_bounds__(NT) void radix_hist_kernel(int shift, int pre, int n, int nb, size_t kstride, const u64* __restrict__ kin,
                                                        uint32_t* __restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  kin += kstride * blockIdx.y;
  hist += (size_t)blockIdx.y * (nb + 1) * 256;
  const uint32_t base = blockIdx.x * (uint32_t)TILE;
  for (int r = 0; r < ITEMS; ++r) {
    const uint32_t i = base + r * NT + threadIdx.x;
    if (i < (uint32_t)n) atomicAdd(&h[digit_of(kin[i], shift, pre)], 1u);
  }
  __syncthreads();
  hist[(size_t)threadIdx.x * nb + blockIdx.x] = h[threadIdx.x];
}

// stable scatter of one tile: rounds of NT elements ranked by the ballot multi-split (element order = round, wave, lane).
// FIRST: the index of an element is its position (no vin).  FINAL: writes order (the index, widened) and inverse, not (kout, vout).
template <bool FIRST, bool FINAL>
__global__ __launch_bounds__(NT) void radix_scatter_kernel(int shift, int pre, int n, int nb, const uint32_t* __restrict__ hist,
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
    if (valid) { k = kin[i]; v = FIRST ? i : vin[row + i]; digit = digit_of(k, shift, pre); }
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
// otherwise the result is (keys[b], vals[b]) with b the returned buffer.  Keys move unshifted.
int radix_sort(const Scratch& s, int K, int n, int key_bits, int pre, const u64* src, bool final, long long* order, long long* inverse,
               hipStream_t st) {
  const int nb = blocks(n, TILE), passes = (key_bits + 7) / 8;
  const dim3 gt(nb, K), gs(256, K);
  const size_t ks = (size_t)n;
  for (int p = 0; p < passes; ++p) {
    const u64* kin = p == 0 ? src : s.keys[(p - 1) & 1];
    const uint32_t* vin = p == 0 ? nullptr : s.vals[(p - 1) & 1];
    u64* kout = s.keys[p & 1];
    uint32_t* vout = s.vals[p & 1];
    const bool last = final && p == passes - 1;
    radix_hist_kernel<<<gt, NT, 0, st>>>(8 * p, pre, n, nb, ks, kin, s.hist);
    digit_scan_kernel<NT><<<gs, NT, 0, st>>>(nb, s.hist);
    if (p == 0 && last)
      radix_scatter_kernel<true, true><<<gt, NT, 0, st>>>(8 * p, pre, n, nb, s.hist, ks, kin, vin, kout, vout, order, inverse);
    else if (p == 0)
      radix_scatter_kernel<true, false><<<gt, NT, 0, st>>>(8 * p, pre, n, nb, s.hist, ks, kin, vin, kout, vout, order, inverse);
    else if (last)
      radix_scatter_kernel<false, true><<<gt, NT, 0, st>>>(8 * p, pre, n, nb, s.hist, ks, kin, vin, kout, vout, order, inverse);
    else
      radix_scatter_kernel<false, false><<<gt, NT, 0, st>>>(8 * p, pre, n, nb, s.hist, ks, kin, vin, kout, vout, order, inverse);
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

}  // extern "C"
