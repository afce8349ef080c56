// What the libraries that sort (64-bit key, 32-bit row) pairs in HBM share (internal, like u3d_util.h): the scratch carver, the two
// scans, the scatter core of a stable 8-bit LSD radix pass and order-preserving flag ranking.  Not a sort: where n comes from, what
// the digit is, what a pass loads and what the last pass writes differ per library, so each keeps its own radix_hist_kernel,
// radix_scatter_kernel and driver, and its own NT / ITEMS / SCAN_NT, passed here as template arguments.  A tile is NT * ITEMS
// elements (blocks(n, TILE) of them); a pass's histogram is 256 x nb counts, digit-major, then the 256 digit totals.
#pragma once
#include "u3d_util.h"

namespace u3d_util {

struct Carver {   // hands out 256-byte aligned pieces of a caller's buffer; with base == nullptr it only adds up the size
  char* base;
  size_t off = 0;
  template <class T> T* take(size_t bytes) { T* q = base ? (T*)(base + off) : nullptr; off += align256(bytes); return q; }
};

#ifdef __HIPCC__
// Exclusive scan of each digit's line of tile counts (one workgroup per digit, coalesced), the digit's total after the counts; the
// scatter adds the exclusive prefix of the 256 totals.  Grid (256 digits, rows); a row's histogram is (nb + 1) * 256 words.
// (One workgroup scanning all 256 x tiles entries took ~0.1 ms per pass at 2.4 M points.)
template <int NT>
__global__ __launch_bounds__(NT) void digit_scan_kernel(int nb, uint32_t* __restrict__ hist) {
  __shared__ uint32_t wt[NT / 64];
  hist += (size_t)blockIdx.y * (nb + 1) * 256;
  uint32_t* line = hist + (size_t)blockIdx.x * nb;
  uint32_t carry = 0;
  for (int b0 = 0; b0 < nb; b0 += NT) {
    const int b = b0 + threadIdx.x;
    const uint32_t x = b < nb ? line[b] : 0u;
    uint32_t all;
    const uint32_t e = block_excl_scan<NT / 64>(x, wt, all);
    if (b < nb) line[b] = carry + e;
    carry += all;
  }
  if (threadIdx.x == 0) hist[(size_t)nb * 256 + blockIdx.x] = carry;
}

// exclusive scan of L counts in place by ONE workgroup; the total goes to *total when total != NULL
template <int SCAN_NT>
__global__ __launch_bounds__(SCAN_NT) void scan_kernel(int L, uint32_t* __restrict__ v, int32_t* __restrict__ total) {
  const int t = threadIdx.x;
  const int ch = (L + SCAN_NT - 1) / SCAN_NT;
  const int b = min(L, t * ch), e = min(L, b + ch);
  uint32_t s = 0;
  for (int i = b; i < e; ++i) s += v[i];
  // inclusive scan of the per-thread sums: inside each wave by shuffles, then over the wave totals
  __shared__ uint32_t wt[SCAN_NT / 64];
  const uint32_t lane = lane_id();
  uint32_t inc = s;
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t u = (uint32_t)__shfl_up((int)inc, o);
    if ((int)lane >= o) inc += u;
  }
  if (lane == 63) wt[t >> 6] = inc;
  __syncthreads();
  uint32_t run = inc - s;
  for (int w = 0; w < (t >> 6); ++w) run += wt[w];
  for (int i = b; i < e; ++i) { const uint32_t x = v[i]; v[i] = run; run += x; }
  if (t == SCAN_NT - 1 && total) *total = (int32_t)run;
}

// ---- scatter core: one tile of a pass moves in rounds of 64 NW elements (element order = round, wave, lane) ----------------------
template <int NW>
struct RadixLds {
  static_assert(NW == 4, "one thread per digit: the workgroup is 256 threads");
  uint32_t wave_cnt[NW][256];   // a round's per-wave digit counts, then each wave's first destination of the digit
  uint32_t digit_base[256];     // where the round's first element of each digit goes
  uint32_t wt[NW];
};

// the tile's bases from the scanned histogram (hist, its digit totals tot, nb tiles); called once, by all 64 NW threads
template <int NW>
__device__ __forceinline__ void radix_bases(RadixLds<NW>& s, const uint32_t* __restrict__ hist, const uint32_t* __restrict__ tot, int nb) {
  const int tid = threadIdx.x;
  uint32_t all;
  s.digit_base[tid] = block_excl_scan<NW>(tot[tid], s.wt, all) + hist[(size_t)tid * nb + blockIdx.x];
}

// One round, every step called by all 64 NW threads: radix_round_begin, the kernel's own load and digit, radix_round_dst, the
// kernel's own store, __syncthreads(): four barriers with the three inside, and the load after the first one, as each library's
// copy had it; timed against the copies in EXPERIMENTS.md.
template <int NW>
__device__ __forceinline__ void radix_round_begin(RadixLds<NW>& s) {
  for (int w = 0; w < NW; ++w) s.wave_cnt[w][threadIdx.x] = 0;
  __syncthreads();
}
// The destination of this thread's element (!valid: digit 0's, not to be stored to).  Elements are ranked inside their wave by the ballot multi-split; one
// prefix over the waves turns the per-wave counts into destinations and moves digit_base past the round.  Stable.
template <int NW>
__device__ __forceinline__ uint32_t radix_round_dst(RadixLds<NW>& s, bool valid, uint32_t digit) {
  const int tid = threadIdx.x, wave = tid >> 6;
  const uint32_t lane = lane_id();
  unsigned long long same = __ballot(valid);
#pragma unroll
  for (int b = 0; b < 8; ++b) {
    const bool bit = (digit >> b) & 1u;
    const unsigned long long m = __ballot(bit);
    same &= bit ? m : ~m;
  }
  const uint32_t rank = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
  if (valid && rank == 0) s.wave_cnt[wave][digit] = (uint32_t)__popcll(same);
  __syncthreads();
  {
    uint32_t run = s.digit_base[tid];
#pragma unroll
    for (int w = 0; w < NW; ++w) { const uint32_t c = s.wave_cnt[w][tid]; s.wave_cnt[w][tid] = run; run += c; }
    s.digit_base[tid] = run;
  }
  __syncthreads();
  return s.wave_cnt[wave][digit] + rank;   // < n: the bases are an exclusive scan of counts that sum to n
}

// ---- order-preserving flag ranking: per-tile counts -> scan_kernel -> ranked emission ---------------------------------------------
// Op: flag(i) marks element i; emit(i, r, f) gets r = flags before i and f = flag(i).  n = n_fixed, or *n_dev when n_fixed < 0.
template <int NT, int ITEMS, class Op>
__global__ __launch_bounds__(NT) void flag_count_kernel(Op op, int n_fixed, const int32_t* __restrict__ n_dev, uint32_t* __restrict__ cnt) {
  const uint32_t n = n_fixed >= 0 ? (uint32_t)n_fixed : (uint32_t)*n_dev;
  const uint32_t base = blockIdx.x * (uint32_t)(NT * ITEMS);
  uint32_t c = 0;
  for (int r = 0; r < ITEMS; ++r) {
    const uint32_t i = base + r * NT + threadIdx.x;
    if (i < n && op.flag(i)) ++c;
  }
  for (int o = 32; o > 0; o >>= 1) c += (uint32_t)__shfl_xor((int)c, o);
  __shared__ uint32_t part[NT / 64];
  if (lane_id() == 0) part[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
    for (int w = 0; w < NT / 64; ++w) t += part[w];
    cnt[blockIdx.x] = t;
  }
}

template <int NT, int ITEMS, class Op>
__global__ __launch_bounds__(NT) void flag_apply_kernel(Op op, int n_fixed, const int32_t* __restrict__ n_dev, const uint32_t* __restrict__ excl) {
  const uint32_t n = n_fixed >= 0 ? (uint32_t)n_fixed : (uint32_t)*n_dev;
  const uint32_t base = blockIdx.x * (uint32_t)(NT * ITEMS);
  if (base >= n) return;
  __shared__ uint32_t wc[NT / 64];
  const int wave = threadIdx.x >> 6;
  const uint32_t lane = lane_id();
  uint32_t run = excl[blockIdx.x];
  for (int r = 0; r < ITEMS; ++r) {
    const uint32_t i = base + r * NT + threadIdx.x;
    const bool valid = i < n;
    const bool f = valid && op.flag(i);
    const unsigned long long m = __ballot(f);
    if (lane == 0) wc[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = run, all = 0;
    for (int w = 0; w < NT / 64; ++w) { if (w < wave) before += wc[w]; all += wc[w]; }
    if (valid) op.emit(i, before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)), f);
    run += all;
    __syncthreads();
  }
}
#endif

}  // namespace u3d_util
