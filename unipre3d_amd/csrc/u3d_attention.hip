// libunipre3d_attention.so: varlen packed-QKV attention (forward + backward) on v_mfma_f32_16x16x16_f16 and segment_csr, for gfx950.
// Contract: include/unipre3d_attention.h.
//
// Fragment maps of v_mfma_f32_16x16x16_f16 (lane l, r = l & 15, g = l >> 4): A holds A[row r][k = 4g + j], B holds B[k = 4g + j][col r]
// (j = 0..3, four halves = 8 bytes), C/D holds D[row 4g + i][col r] (i = 0..3).  With head dim 16 one MFMA is one 16 x 16 tile, and a
// C/D tile rounded to fp16 is directly the B operand of a product that sums over its ROW index.  Every product here is oriented so
// that this holds and no tile ever moves between lanes:
//   forward   S^T[key][q] = K.Q^T         (A = K rows, B = Q rows)      -> P^T is the B operand of  O^T[d][q] = V^T[d][key].P^T[key][q]
//   backward  S^T, dP^T = V.dO^T          -> dS^T is the B operand of    dQ^T[d][q] = K^T[d][key].dS^T[key][q]   (wave owns a query block)
//             S[q][key] = Q.K^T, dP = dO.V^T (operands swapped)         -> P, dS are the B operands of
//                                            dV^T[d][key] = dO^T[d][q].P[q][key], dK^T[d][key] = Q^T[d][q].dS[q][key]   (wave owns a key tile)
// The A operands that are transposes (V^T, K^T, Q^T, dO^T) are read from LDS images [d][row] written once per (sequence, head); the
// softmax row statistics sit on the lane (column r) or in the four registers and need two cross-lane steps per 64 keys.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "unipre3d_attention.h"

namespace {

typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

constexpr int TAIL_BLOCKS = 64;     // extra workgroups that zero the rows at or beyond cu_seqlens[S]
constexpr int TPAD = 4;             // halves of padding per row of a transposed LDS image (keeps 8-byte alignment, spreads banks)
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

__device__ __forceinline__ f4 mfma16(h4 a, h4 b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x16f16(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float xor_lane(float v, int m) { return __shfl_xor(v, m, 64); }
__device__ __forceinline__ h4 to_h4(f4 v) { return h4{(_Float16)v[0], (_Float16)v[1], (_Float16)v[2], (_Float16)v[3]}; }
__device__ __forceinline__ h4 ld_h4(const _Float16* p) { return *reinterpret_cast<const h4*>(p); }
__device__ __forceinline__ void st_h4(_Float16* p, h4 v) { *reinterpret_cast<h4*>(p) = v; }

// rows [0, nrows) of one head's 16-half column block into LDS: row-major (32 B per row) and / or transposed [d][row]; rows >= len as 0
template <bool ROW, bool TR>
__device__ __forceinline__ void stage(const _Float16* __restrict__ src, size_t stride, int len, int nrows, _Float16* row, _Float16* tr,
                                      int trs, int tid, int nthr) {
  for (int r = tid; r < nrows; r += nthr) {
    union { uint4 u[2]; _Float16 h[16]; } v;
    v.u[0] = make_uint4(0, 0, 0, 0);
    v.u[1] = v.u[0];
    if (r < len) {
      const uint4* p = reinterpret_cast<const uint4*>(src + (size_t)r * stride);
      v.u[0] = p[0];
      v.u[1] = p[1];
    }
    if (ROW) {
      uint4* d = reinterpret_cast<uint4*>(row + r * 16);
      d[0] = v.u[0];
      d[1] = v.u[1];
    }
    if (TR) {
#pragma unroll
      for (int d = 0; d < 16; ++d) tr[d * trs + r] = v.h[d];
    }
  }
}

struct Seq { int beg, len, raw; };
// rows of sequence s, clamped so that nothing outside [0, T) is ever touched; len = the rows that attend (at most max_seqlen)
__device__ __forceinline__ Seq sequence(const int32_t* cu, int s, int T, int max_seqlen) {
  int beg = cu[s], end = cu[s + 1];
  if (end > T) end = T;
  Seq q;
  q.beg = beg;
  q.raw = (beg < 0 || end < beg) ? 0 : end - beg;
  if (beg < 0) q.beg = 0;
  q.len = q.raw < max_seqlen ? q.raw : max_seqlen;
  return q;
}
__device__ __forceinline__ int tail_begin(const int32_t* cu, int S, int T) {
  int b = cu[S];
  return b < 0 ? 0 : (b > T ? T : b);
}

// ---------------------------------------------------------------------------------------------------------------- forward
// WPH waves share one (sequence, head); a workgroup holds HPB heads of one sequence.  LDS per head: K rows (cap x 16), V^T (16 x (cap + TPAD)).
template <int WPH, int HPB>
__global__ __launch_bounds__(64 * WPH * HPB) void attn_fwd_kernel(const _Float16* __restrict__ qkv, const int32_t* __restrict__ cu,
                                                                  _Float16* __restrict__ out, float* __restrict__ lse, int T, int S, int H,
                                                                  int cap, int max_seqlen, float scale, int hb) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int nwork = S * hb;
  if ((int)blockIdx.x >= nwork) {   // tail rows: zeros
    const int tb = blockIdx.x - nwork, nthr = TAIL_BLOCKS * blockDim.x, tid = tb * blockDim.x + threadIdx.x;
    const int beg = tail_begin(cu, S, T);
    const size_t n16 = (size_t)(T - beg) * H * 2;   // uint4 = 8 halves; a row of one head is two
    uint4* o = reinterpret_cast<uint4*>(out + (size_t)beg * H * 16);
    for (size_t i = tid; i < n16; i += nthr) o[i] = make_uint4(0, 0, 0, 0);
    const size_t nl = (size_t)(T - beg) * H;
    for (size_t i = tid; i < nl; i += nthr) lse[(i / (T - beg)) * T + beg + i % (T - beg)] = 0.f;
    return;
  }
  const int s = blockIdx.x / hb, h0 = (blockIdx.x % hb) * HPB;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, slot = wave / WPH, sub = wave % WPH, h = h0 + slot;
  const int r = lane & 15, g = lane >> 4;
  const bool hv = h < H;
  const Seq sq = sequence(cu, s, T, max_seqlen);
  const int len = sq.len, nt = (len + 15) >> 4, trs = cap + TPAD;
  const size_t rs = (size_t)3 * H * 16;
  _Float16* Krow = reinterpret_cast<_Float16*>(smem) + (size_t)slot * (cap * 16 + 16 * trs);
  _Float16* Vt = Krow + cap * 16;
  const _Float16* qbase = qkv + (size_t)sq.beg * rs + h * 16;
  if (hv) {
    const int tid = sub * 64 + lane;
    stage<true, false>(qbase + H * 16, rs, len, nt * 16, Krow, nullptr, 0, tid, WPH * 64);
    stage<false, true>(qbase + 2 * H * 16, rs, len, nt * 16, nullptr, Vt, trs, tid, WPH * 64);
    for (int q = len + tid; q < sq.raw; q += WPH * 64) {   // rows beyond max_seqlen (a caller error): zeros
      uint4* o = reinterpret_cast<uint4*>(out + ((size_t)(sq.beg + q) * H + h) * 16);
      o[0] = make_uint4(0, 0, 0, 0);
      o[1] = make_uint4(0, 0, 0, 0);
      lse[(size_t)h * T + sq.beg + q] = 0.f;
    }
  }
  __syncthreads();
  if (!hv) return;
  const float c = scale * LOG2E;
  for (int qb = sub; qb < nt; qb += WPH) {
    const int q = qb * 16 + r;
    h4 bq = {0, 0, 0, 0};
    if (q < len) bq = ld_h4(qbase + (size_t)q * rs + 4 * g);
    float m = -INFINITY, l = 0.f;
    f4 o = {0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < nt; k0 += 4) {   // 64 keys per softmax step
      f4 sc[4];
      float tmax = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        sc[t] = f4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        if (k0 + t < nt) {
          const int kb = (k0 + t) * 16;
          f4 x = mfma16(ld_h4(Krow + (kb + r) * 16 + 4 * g), bq, f4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            sc[t][i] = (kb + 4 * g + i < len) ? x[i] * c : -INFINITY;   // in units of log2: any sign of softmax_scale
            tmax = fmaxf(tmax, sc[t][i]);
          }
        }
      }
      tmax = fmaxf(tmax, xor_lane(tmax, 16));
      tmax = fmaxf(tmax, xor_lane(tmax, 32));
      const float mn = fmaxf(m, tmax);   // finite: key k0 * 16 < len exists in every step
      const float alpha = __builtin_amdgcn_exp2f(m - mn);
      m = mn;
      l *= alpha;
      o *= alpha;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (k0 + t < nt) {
          f4 p;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            p[i] = __builtin_amdgcn_exp2f(sc[t][i] - mn);
            l += p[i];
          }
          o = mfma16(ld_h4(Vt + r * trs + (k0 + t) * 16 + 4 * g), to_h4(p), o);
        }
      }
    }
    l += xor_lane(l, 16);
    l += xor_lane(l, 32);
    if (q < len) {
      const float inv = 1.f / l;
      st_h4(out + ((size_t)(sq.beg + q) * H + h) * 16 + 4 * g, to_h4(o * inv));
      if (g == 0) lse[(size_t)h * T + sq.beg + q] = (m + __log2f(l)) * LN2;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- backward
// LDS per head: lse * log2(e) and delta (cap floats each), two row-major images R0 / R1 (cap x 16) and two transposed T0 / T1
// (16 x (cap + TPAD)).  Phase A (dQ): R0 = K, R1 = V, T0 = K^T.  Phase B (dK, dV): R0 = Q, R1 = dO, T0 = Q^T, T1 = dO^T.
template <int WPH, int HPB>
__global__ __launch_bounds__(64 * WPH * HPB) void attn_bwd_kernel(const _Float16* __restrict__ qkv, const int32_t* __restrict__ cu,
                                                                  const _Float16* __restrict__ out, const _Float16* __restrict__ dout,
                                                                  const float* __restrict__ lse, _Float16* __restrict__ dqkv, int T, int S,
                                                                  int H, int cap, int max_seqlen, float scale, int hb) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int nwork = S * hb;
  if ((int)blockIdx.x >= nwork) {
    const int tb = blockIdx.x - nwork, nthr = TAIL_BLOCKS * blockDim.x, tid = tb * blockDim.x + threadIdx.x;
    const int beg = tail_begin(cu, S, T);
    const size_t n16 = (size_t)(T - beg) * H * 6;
    uint4* o = reinterpret_cast<uint4*>(dqkv + (size_t)beg * 3 * H * 16);
    for (size_t i = tid; i < n16; i += nthr) o[i] = make_uint4(0, 0, 0, 0);
    return;
  }
  const int s = blockIdx.x / hb, h0 = (blockIdx.x % hb) * HPB;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, slot = wave / WPH, sub = wave % WPH, h = h0 + slot;
  const int r = lane & 15, g = lane >> 4, tid = sub * 64 + lane;
  const bool hv = h < H;
  const Seq sq = sequence(cu, s, T, max_seqlen);
  const int len = sq.len, nt = (len + 15) >> 4, trs = cap + TPAD;
  const size_t rs = (size_t)3 * H * 16, os = (size_t)H * 16;
  const size_t slot_bytes = (size_t)cap * 8 + 2 * ((size_t)cap * 32 + (size_t)trs * 32);
  float* lseS = reinterpret_cast<float*>(smem + slot * slot_bytes);
  float* delS = lseS + cap;
  _Float16* R0 = reinterpret_cast<_Float16*>(delS + cap);
  _Float16* R1 = R0 + cap * 16;
  _Float16* T0 = R1 + cap * 16;
  _Float16* T1 = T0 + 16 * trs;
  const _Float16* qbase = qkv + (size_t)sq.beg * rs + h * 16;
  const _Float16* dobase = dout + (size_t)sq.beg * os + h * 16;
  const _Float16* obase = out + (size_t)sq.beg * os + h * 16;
  _Float16* dbase = dqkv + (size_t)sq.beg * rs + h * 16;
  const float c = scale * LOG2E;
  if (hv) {
    for (int q = tid; q < nt * 16; q += WPH * 64) {
      float lq = 0.f, dl = 0.f;
      if (q < len) {
        union { uint4 u[2]; _Float16 h[16]; } a, b;
        const uint4* pa = reinterpret_cast<const uint4*>(dobase + (size_t)q * os);
        const uint4* pb = reinterpret_cast<const uint4*>(obase + (size_t)q * os);
        a.u[0] = pa[0]; a.u[1] = pa[1]; b.u[0] = pb[0]; b.u[1] = pb[1];
#pragma unroll
        for (int d = 0; d < 16; ++d) dl = fmaf((float)a.h[d], (float)b.h[d], dl);
        lq = lse[(size_t)h * T + sq.beg + q] * LOG2E;
      }
      lseS[q] = lq;
      delS[q] = dl;
    }
    stage<true, true>(qbase + H * 16, rs, len, nt * 16, R0, T0, trs, tid, WPH * 64);
    stage<true, false>(qbase + 2 * H * 16, rs, len, nt * 16, R1, nullptr, 0, tid, WPH * 64);
    for (int q = len + tid; q < sq.raw; q += WPH * 64) {   // rows beyond max_seqlen: zero gradient
#pragma unroll
      for (int w = 0; w < 3; ++w) {
        uint4* o = reinterpret_cast<uint4*>(dbase + (size_t)q * rs + w * H * 16);
        o[0] = make_uint4(0, 0, 0, 0);
        o[1] = make_uint4(0, 0, 0, 0);
      }
    }
  }
  __syncthreads();
  if (hv) {   // phase A: this wave's query blocks against every key tile
    for (int qb = sub; qb < nt; qb += WPH) {
      const int q = qb * 16 + r;
      h4 bq = {0, 0, 0, 0}, bdo = {0, 0, 0, 0};
      if (q < len) {
        bq = ld_h4(qbase + (size_t)q * rs + 4 * g);
        bdo = ld_h4(dobase + (size_t)q * os + 4 * g);
      }
      const float lq = lseS[q], dl = delS[q];
      f4 dq = {0.f, 0.f, 0.f, 0.f};
      for (int kt = 0; kt < nt; ++kt) {
        const int kb = kt * 16;
        const f4 st = mfma16(ld_h4(R0 + (kb + r) * 16 + 4 * g), bq, f4{0.f, 0.f, 0.f, 0.f});
        const f4 dp = mfma16(ld_h4(R1 + (kb + r) * 16 + 4 * g), bdo, f4{0.f, 0.f, 0.f, 0.f});
        f4 ds;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float p = (kb + 4 * g + i < len && q < len) ? __builtin_amdgcn_exp2f(st[i] * c - lq) : 0.f;
          ds[i] = p * (dp[i] - dl);
        }
        dq = mfma16(ld_h4(T0 + r * trs + kb + 4 * g), to_h4(ds), dq);
      }
      if (q < len) st_h4(dbase + (size_t)q * rs + 4 * g, to_h4(dq * scale));
    }
  }
  __syncthreads();
  if (hv) {
    stage<true, true>(qbase, rs, len, nt * 16, R0, T0, trs, tid, WPH * 64);
    stage<true, true>(dobase, os, len, nt * 16, R1, T1, trs, tid, WPH * 64);
  }
  __syncthreads();
  if (!hv) return;
  for (int kt = sub; kt < nt; kt += WPH) {   // phase B: this wave's key tiles against every query block, in ascending order
    const int key = kt * 16 + r;
    h4 bk = {0, 0, 0, 0}, bv = {0, 0, 0, 0};
    if (key < len) {
      bk = ld_h4(qbase + (size_t)key * rs + H * 16 + 4 * g);
      bv = ld_h4(qbase + (size_t)key * rs + 2 * H * 16 + 4 * g);
    }
    f4 dk = {0.f, 0.f, 0.f, 0.f}, dv = {0.f, 0.f, 0.f, 0.f};
    for (int qb = 0; qb < nt; ++qb) {
      const int q0 = qb * 16;
      const f4 sn = mfma16(ld_h4(R0 + (q0 + r) * 16 + 4 * g), bk, f4{0.f, 0.f, 0.f, 0.f});
      const f4 dp = mfma16(ld_h4(R1 + (q0 + r) * 16 + 4 * g), bv, f4{0.f, 0.f, 0.f, 0.f});
      const f4 lq = *reinterpret_cast<const f4*>(lseS + q0 + 4 * g);
      const f4 dl = *reinterpret_cast<const f4*>(delS + q0 + 4 * g);
      f4 p, ds;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        p[i] = (q0 + 4 * g + i < len && key < len) ? __builtin_amdgcn_exp2f(sn[i] * c - lq[i]) : 0.f;
        ds[i] = p[i] * (dp[i] - dl[i]);
      }
      dv = mfma16(ld_h4(T1 + r * trs + q0 + 4 * g), to_h4(p), dv);
      dk = mfma16(ld_h4(T0 + r * trs + q0 + 4 * g), to_h4(ds), dk);
    }
    if (key < len) {
      st_h4(dbase + (size_t)key * rs + H * 16 + 4 * g, to_h4(dk * scale));
      st_h4(dbase + (size_t)key * rs + 2 * H * 16 + 4 * g, to_h4(dv));
    }
  }
}

size_t fwd_lds(int cap, int hpb) { return (size_t)hpb * ((size_t)cap * 32 + (size_t)(cap + TPAD) * 32); }
size_t bwd_lds(int cap, int hpb) { return (size_t)hpb * ((size_t)cap * 8 + 2 * ((size_t)cap * 32 + (size_t)(cap + TPAD) * 32)); }

template <int WPH, int HPB>
int launch_fwd(const _Float16* qkv, const int32_t* cu, _Float16* out, float* lse, int T, int S, int H, int cap, int max_seqlen,
               float scale, hipStream_t st) {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(attn_fwd_kernel<WPH, HPB>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)fwd_lds(HPB == 1 ? U3D_ATTN_MAX_SEQLEN : 64, HPB));
  if (attr != hipSuccess) return 3;
  const int hb = (H + HPB - 1) / HPB;
  attn_fwd_kernel<WPH, HPB><<<dim3((unsigned)((size_t)S * hb + TAIL_BLOCKS)), 64 * WPH * HPB, fwd_lds(cap, HPB), st>>>(
      qkv, cu, out, lse, T, S, H, cap, max_seqlen, scale, hb);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}
template <int WPH, int HPB>
int launch_bwd(const _Float16* qkv, const int32_t* cu, const _Float16* out, const _Float16* dout, const float* lse, _Float16* dqkv, int T,
               int S, int H, int cap, int max_seqlen, float scale, hipStream_t st) {
  static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(attn_bwd_kernel<WPH, HPB>),
                                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)bwd_lds(HPB == 1 ? U3D_ATTN_MAX_SEQLEN : 64, HPB));
  if (attr != hipSuccess) return 3;
  const int hb = (H + HPB - 1) / HPB;
  attn_bwd_kernel<WPH, HPB><<<dim3((unsigned)((size_t)S * hb + TAIL_BLOCKS)), 64 * WPH * HPB, bwd_lds(cap, HPB), st>>>(
      qkv, cu, out, dout, lse, dqkv, T, S, H, cap, max_seqlen, scale, hb);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

int check_attn(const void* a, const void* b, const void* c, const void* d, int T, int S, int H, int D, int max_seqlen) {
  if (!a || !b || !c || !d || T < 0 || S < 0 || H < 1) return 1;
  if ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(c)) & 15) return 1;
  if (D != 16 || max_seqlen < 1 || max_seqlen > U3D_ATTN_MAX_SEQLEN) return 2;
  if ((size_t)S * ((H + 3) / 4) + TAIL_BLOCKS >= (size_t)1 << 31 || (size_t)T * 3 * H * 16 >= (size_t)1 << 40) return 2;
  return 0;
}

// ---------------------------------------------------------------------------------------------------------------- segment_csr
__device__ __forceinline__ bool takes(float v, float best, bool is_max) {
  if (best != best) return false;   // a NaN stays (the lowest NaN row is the argument)
  if (v != v) return true;
  return is_max ? v > best : v < best;
}
__global__ __launch_bounds__(256) void segment_csr_fwd_kernel(const float* __restrict__ src, const int64_t* __restrict__ indptr,
                                                              float* __restrict__ out, int64_t* __restrict__ arg, int N, int M, int C,
                                                              int reduce) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)M * C) return;
  const int m = (int)(e / C), ch = (int)(e % C);
  int64_t a = indptr[m], b = indptr[m + 1];
  if (a < 0) a = 0;
  if (b > N) b = N;
  float acc = 0.f;
  int64_t best = -1;
  if (reduce <= 1) {
    for (int64_t n = a; n < b; ++n) acc += src[n * C + ch];
    if (reduce == 1 && b > a) acc /= (float)(b - a);
  } else if (b > a) {
    acc = src[a * C + ch];
    best = a;
    for (int64_t n = a + 1; n < b; ++n) {
      const float v = src[n * C + ch];
      if (takes(v, acc, reduce == 2)) {
        acc = v;
        best = n;
      }
    }
  }
  out[e] = acc;
  if (arg) arg[e] = best;
}
// one thread per (segment, channel) writes the gradient of all its rows; segment M stands for the rows no segment covers
__global__ __launch_bounds__(256) void segment_csr_bwd_kernel(const float* __restrict__ dout, const int64_t* __restrict__ indptr,
                                                              const int64_t* __restrict__ arg, float* __restrict__ dsrc, int N, int M,
                                                              int C, int reduce) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (size_t)(M + 1) * C) return;
  const int m = (int)(e / C), ch = (int)(e % C);
  if (m == M) {
    int64_t lo = indptr[0], hi = indptr[M];
    if (lo < 0) lo = 0;
    if (hi > N) hi = N;
    if (hi < lo) hi = lo;
    for (int64_t n = 0; n < lo && n < N; ++n) dsrc[n * C + ch] = 0.f;
    for (int64_t n = hi; n < N; ++n) dsrc[n * C + ch] = 0.f;
    return;
  }
  int64_t a = indptr[m], b = indptr[m + 1];
  if (a < 0) a = 0;
  if (b > N) b = N;
  if (b <= a) return;
  float gv = dout[e];
  if (reduce == 1) gv /= (float)(b - a);
  const int64_t best = reduce >= 2 ? arg[e] : -1;
  for (int64_t n = a; n < b; ++n) dsrc[n * C + ch] = (reduce <= 1 || n == best) ? gv : 0.f;
}

}  // namespace

extern "C" {

int u3d_attn_abi_version(void) { return U3D_ATTN_ABI_VERSION; }

int u3d_attn_varlen_fwd(const void* qkv, const int32_t* cu_seqlens, void* out, float* lse, int T, int S, int H, int D, int max_seqlen,
                        float softmax_scale, void* stream) {
  if (int rc = check_attn(qkv, cu_seqlens, out, lse, T, S, H, D, max_seqlen)) return rc;
  const _Float16* x = static_cast<const _Float16*>(qkv);
  _Float16* o = static_cast<_Float16*>(out);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int cap = (max_seqlen + 15) & ~15;
  if (cap <= 64) return launch_fwd<1, 4>(x, cu_seqlens, o, lse, T, S, H, 64, max_seqlen, softmax_scale, st);
  if (cap <= 256) return launch_fwd<4, 1>(x, cu_seqlens, o, lse, T, S, H, cap, max_seqlen, softmax_scale, st);
  if (cap <= 512) return launch_fwd<8, 1>(x, cu_seqlens, o, lse, T, S, H, cap, max_seqlen, softmax_scale, st);
  return launch_fwd<16, 1>(x, cu_seqlens, o, lse, T, S, H, cap, max_seqlen, softmax_scale, st);
}

int u3d_attn_varlen_bwd(const void* qkv, const int32_t* cu_seqlens, const void* out, const void* dout, const float* lse, void* dqkv,
                        int T, int S, int H, int D, int max_seqlen, float softmax_scale, void* stream) {
  if (int rc = check_attn(qkv, cu_seqlens, dqkv, lse, T, S, H, D, max_seqlen)) return rc;
  if (!out || !dout || ((reinterpret_cast<uintptr_t>(out) | reinterpret_cast<uintptr_t>(dout)) & 15)) return 1;
  const _Float16* x = static_cast<const _Float16*>(qkv);
  const _Float16* o = static_cast<const _Float16*>(out);
  const _Float16* go = static_cast<const _Float16*>(dout);
  _Float16* gx = static_cast<_Float16*>(dqkv);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int cap = (max_seqlen + 15) & ~15;
  if (cap <= 64) return launch_bwd<1, 4>(x, cu_seqlens, o, go, lse, gx, T, S, H, 64, max_seqlen, softmax_scale, st);
  if (cap <= 256) return launch_bwd<4, 1>(x, cu_seqlens, o, go, lse, gx, T, S, H, cap, max_seqlen, softmax_scale, st);
  if (cap <= 512) return launch_bwd<8, 1>(x, cu_seqlens, o, go, lse, gx, T, S, H, cap, max_seqlen, softmax_scale, st);
  return launch_bwd<16, 1>(x, cu_seqlens, o, go, lse, gx, T, S, H, cap, max_seqlen, softmax_scale, st);
}

int u3d_segment_csr_fwd(const float* src, const int64_t* indptr, float* out, int64_t* arg, int N, int M, int C, int reduce,
                        void* stream) {
  if (!indptr || N < 0 || M < 0 || C < 1 || reduce < 0 || reduce > 3 || (reduce >= 2 && !arg && M > 0)) return 1;
  if (M == 0) return 0;
  if (!out || (!src && N > 0)) return 1;
  const size_t n = (size_t)M * C;
  if ((n + 255) / 256 >= (size_t)1 << 31) return 2;
  segment_csr_fwd_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, static_cast<hipStream_t>(stream)>>>(src, indptr, out, arg, N, M, C,
                                                                                                          reduce);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

int u3d_segment_csr_bwd(const float* dout, const int64_t* indptr, const int64_t* arg, float* dsrc, int N, int M, int C, int reduce,
                        void* stream) {
  if (!indptr || N < 0 || M < 0 || C < 1 || reduce < 0 || reduce > 3 || (reduce >= 2 && !arg && M > 0)) return 1;
  if (N == 0) return 0;
  if (!dsrc || (!dout && M > 0)) return 1;
  const size_t n = (size_t)(M + 1) * C;
  if ((n + 255) / 256 >= (size_t)1 << 31) return 2;
  segment_csr_bwd_kernel<<<dim3((unsigned)((n + 255) / 256)), 256, 0, static_cast<hipStream_t>(stream)>>>(dout, indptr, arg, dsrc, N, M, C,
                                                                                                          reduce);
  return hipGetLastError() == hipSuccess ? 0 : 3;
}

}  // extern "C"
