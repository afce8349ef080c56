// libunipre3d_mha.so: dense fp32 multi-head attention over the packed qkv of nn.Linear, forward and backward (include/unipre3d_mha.h).
//
// Fragment maps of v_mfma_f32_16x16x4_f32 (lane l, r = l & 15, g = l >> 4): A holds A[row r][k = g], B holds B[k = g][col r], C / D hold
// C[row 4g + i][col r] in register i.  The result is a k-ordered f32 fma chain.
//
// One workgroup is four waves and one block of 64 rows of one (batch, head); a wave owns 16 of them, held as 16 operand registers
// (lane (r, g) holds row r's channels 16t + 4g + j, t, j = 0 .. 3: one 16-byte load per t).  The other side streams through LDS in
// blocks of 64 rows (row pitch 68 floats; the next block is fetched into registers while this one is computed on), read as 16-byte
// pieces in the same channel order, so both operands of a step agree on k.
//
//   forward   S^T = K Q^T: C has the query on r and the key on 4g + i -- which is the A operand of P V over the keys 4g + i of
//             step i, with V's B operand read from row 4g + i: no transpose of P.  Row max / sum: 16 registers and the lane groups g.
//   dQ grid   the same orientation: S^T and dP^T = V dO^T, dS^T is the A operand of dS K.
//   dK/dV grid  S = Q K^T and dP = dO V^T with the key on r and the query on 4g + i: P^T and dS^T are the A operands of P^T dO and
//             dS^T Q over the queries 4g + i.  It loops over query blocks in ascending order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include "unipre3d_mha.h"
#include "u3d_util.h"

namespace {

using f4 = __attribute__((ext_vector_type(4))) float;
constexpr int HD = U3D_MHA_HEAD_DIM;   // channels per head
constexpr int BLK = 64;                // rows per workgroup and per LDS block
constexpr int LDW = HD + 4;            // LDS row pitch in floats: 16-byte rows, and a column read of 4 rows x 16 lanes hits 64 banks
constexpr int NT = 256;
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ f4 mfma(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
__device__ __forceinline__ float group_max(float v) {   // over the four lanes that share r
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float group_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// Staging rows r0 .. r0 + 63 of a matrix of 64-float rows `pitch` floats apart: a thread's share is four 16-byte pieces (rows
// tid / 16 + 16 i, channels 4 (tid % 16) ..), fetched into registers and put into LDS one block later, so that the next block's loads
// are in flight while the current block is computed on.  Rows at or beyond N are zeros.
struct Piece { f4 v[4]; };
__device__ __forceinline__ void fetch(Piece& p, const float* __restrict__ src, size_t pitch, int r0, int N, int tid) {
  const int c = (tid & 15) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (tid >> 4) + 16 * i;
    p.v[i] = f4{0.f, 0.f, 0.f, 0.f};
    if (r0 + row < N) p.v[i] = *reinterpret_cast<const f4*>(src + (size_t)(r0 + row) * pitch + c);
  }
}
__device__ __forceinline__ void put(float* __restrict__ dst, const Piece& p, int tid) {
  const int c = (tid & 15) * 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) *reinterpret_cast<f4*>(dst + ((tid >> 4) + 16 * i) * LDW + c) = p.v[i];
}

// the wave's operand registers: x[4t + j] = src[row][16t + 4g + j]; zeros when the row is beyond N
__device__ __forceinline__ void load_operand(float (&x)[16], const float* __restrict__ src, size_t pitch, int row, int N, int g) {
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < N) v = *reinterpret_cast<const f4*>(src + (size_t)row * pitch + 16 * t + 4 * g);
#pragma unroll
    for (int j = 0; j < 4; ++j) x[4 * t + j] = v[j];
  }
}

struct Where {
  int b, h, blk;
  size_t pitch;          // floats between two tokens of qkv
  const float *q, *k, *v;
};
__device__ __forceinline__ Where where(const float* qkv, int N, int H, int nblk) {
  Where w;
  const int bh = blockIdx.x / nblk;
  w.blk = blockIdx.x % nblk;
  w.h = bh % H;
  w.b = bh / H;
  w.pitch = (size_t)3 * H * HD;
  w.q = qkv + (size_t)w.b * N * w.pitch + (size_t)w.h * HD;
  w.k = w.q + (size_t)H * HD;
  w.v = w.k + (size_t)H * HD;
  return w;
}

// ---- forward -----------------------------------------------------------------------------------------------------------------
// scores of the wave's 16 queries against one staged block of keys; FULL: all 64 keys exist
template <bool FULL>
__device__ __forceinline__ void scores(f4 (&s)[4], const float* __restrict__ Ks, const float (&q)[16], int kb, int N, int r, int g) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int tile = 0; tile < 4; ++tile)
      if (FULL || kb + 16 * tile < N) {
        const f4 kk = *reinterpret_cast<const f4*>(Ks + (16 * tile + r) * LDW + 16 * t + 4 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[tile] = mfma(kk[j], q[4 * t + j], s[tile]);
      }
  if (!FULL)
#pragma unroll
    for (int tile = 0; tile < 4; ++tile)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (kb + 16 * tile + 4 * g + i >= N) s[tile][i] = -INFINITY;
}

__global__ __launch_bounds__(NT) void mha_fwd_kernel(const float* __restrict__ qkv, float* __restrict__ out, float* __restrict__ lse,
                                                     int N, int H, int nblk, float scale, float c) {
  __shared__ __attribute__((aligned(16))) float Ks[BLK * LDW];
  __shared__ __attribute__((aligned(16))) float Vs[BLK * LDW];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const Where w = where(qkv, N, H, nblk);
  const int q0 = w.blk * BLK + wave * 16;
  const bool live = q0 < N;   // a wave without a query still stages
  float q[16];
  load_operand(q, w.q, w.pitch, q0 + r, N, g);
  f4 o[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) o[db] = f4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;   // running max of query r; this lane's part of its running sum

  Piece pk, pv;
  fetch(pk, w.k, w.pitch, 0, N, tid);
  fetch(pv, w.v, w.pitch, 0, N, tid);
  for (int kb = 0; kb < N; kb += BLK) {
    __syncthreads();
    put(Ks, pk, tid);
    put(Vs, pv, tid);
    __syncthreads();
    if (kb + BLK < N) {
      fetch(pk, w.k, w.pitch, kb + BLK, N, tid);
      fetch(pv, w.v, w.pitch, kb + BLK, N, tid);
    }
    if (!live) continue;
    f4 s[4];
#pragma unroll
    for (int tile = 0; tile < 4; ++tile) s[tile] = f4{0.f, 0.f, 0.f, 0.f};
    if (kb + BLK <= N) scores<true>(s, Ks, q, kb, N, r, g);
    else scores<false>(s, Ks, q, kb, N, r, g);
    float mx = -INFINITY;
#pragma unroll
    for (int tile = 0; tile < 4; ++tile)
#pragma unroll
      for (int i = 0; i < 4; ++i) mx = fmaxf(mx, s[tile][i]);
    const float mn = fmaxf(m, group_max(mx));   // finite: key kb exists
    const float alpha = exp2f((m - mn) * c), mc = mn * c;
    m = mn;
    float sum = 0.f;
#pragma unroll
    for (int tile = 0; tile < 4; ++tile)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[tile][i] = exp2f(fmaf(s[tile][i], c, -mc));   // a key beyond N: exp2(-inf) = 0
        sum += s[tile][i];
      }
    l = fmaf(l, alpha, sum);
    // the block's P V in accumulators of its own: the chain over keys stays 64 long whatever N is, and o is a sum of block sums
    f4 ob[4];
#pragma unroll
    for (int db = 0; db < 4; ++db) ob[db] = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int tile = 0; tile < 4; ++tile)
      if (kb + 16 * tile < N)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float* vrow = Vs + (16 * tile + 4 * g + j) * LDW + r;
#pragma unroll
          for (int db = 0; db < 4; ++db) ob[db] = mfma(s[tile][j], vrow[16 * db], ob[db]);
        }
    // o's rows are the queries 4g + i: their factors are in the lanes 4g + i
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float a = __shfl(alpha, 4 * g + i);
#pragma unroll
      for (int db = 0; db < 4; ++db) o[db][i] = fmaf(o[db][i], a, ob[db][i]);
    }
  }
  if (!live) return;
  l = group_sum(l);
  const float inv = 1.f / l;
  if (g == 0 && q0 + r < N) lse[((size_t)w.b * H + w.h) * N + q0 + r] = fmaf(m, scale, logf(l));
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float a = __shfl(inv, 4 * g + i);
    const int n = q0 + 4 * g + i;
    if (n < N) {
      float* dst = out + (((size_t)w.b * N + n) * H + w.h) * HD + r;
#pragma unroll
      for (int db = 0; db < 4; ++db) dst[16 * db] = o[db][i] * a;
    }
  }
}

// ---- backward: dQ ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void mha_bwd_dq_kernel(const float* __restrict__ qkv, const float* __restrict__ out,
                                                        const float* __restrict__ dout, const float* __restrict__ lse,
                                                        float* __restrict__ dqkv, int N, int H, int nblk, float scale, float c) {
  __shared__ __attribute__((aligned(16))) float Ks[BLK * LDW];
  __shared__ __attribute__((aligned(16))) float Vs[BLK * LDW];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const Where w = where(qkv, N, H, nblk);
  const int q0 = w.blk * BLK + wave * 16;
  const bool live = q0 < N;
  const size_t opitch = (size_t)H * HD;
  const size_t obase = (size_t)w.b * N * opitch + (size_t)w.h * HD;
  float q[16], dO[16], delta = 0.f;
  load_operand(q, w.q, w.pitch, q0 + r, N, g);
  load_operand(dO, dout + obase, opitch, q0 + r, N, g);
  {
    float o[16];
    load_operand(o, out + obase, opitch, q0 + r, N, g);
#pragma unroll
    for (int x = 0; x < 16; ++x) delta = fmaf(dO[x], o[x], delta);
    delta = group_sum(delta);
  }
  // a query beyond N: q = dO = 0 and lse = +inf, so its P is exp2(-inf) = 0
  const float L = q0 + r < N ? lse[((size_t)w.b * H + w.h) * N + q0 + r] * LOG2E : INFINITY;
  f4 dq[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) dq[db] = f4{0.f, 0.f, 0.f, 0.f};

  Piece pk, pv;
  fetch(pk, w.k, w.pitch, 0, N, tid);
  fetch(pv, w.v, w.pitch, 0, N, tid);
  for (int kb = 0; kb < N; kb += BLK) {
    __syncthreads();
    put(Ks, pk, tid);
    put(Vs, pv, tid);
    __syncthreads();
    if (kb + BLK < N) {
      fetch(pk, w.k, w.pitch, kb + BLK, N, tid);
      fetch(pv, w.v, w.pitch, kb + BLK, N, tid);
    }
    if (!live) continue;
#pragma unroll
    for (int tile = 0; tile < 4; ++tile) {
      if (kb + 16 * tile >= N) break;
      f4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f4 kk = *reinterpret_cast<const f4*>(Ks + (16 * tile + r) * LDW + 16 * t + 4 * g);
        const f4 vv = *reinterpret_cast<const f4*>(Vs + (16 * tile + r) * LDW + 16 * t + 4 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s = mfma(kk[j], q[4 * t + j], s);
          dp = mfma(vv[j], dO[4 * t + j], dp);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float p = kb + 16 * tile + 4 * g + i < N ? exp2f(fmaf(s[i], c, -L)) : 0.f;
        s[i] = p * (dp[i] - delta);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* krow = Ks + (16 * tile + 4 * g + j) * LDW + r;
#pragma unroll
        for (int db = 0; db < 4; ++db) dq[db] = mfma(s[j], krow[16 * db], dq[db]);
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = q0 + 4 * g + i;
    if (n < N) {
      float* dst = dqkv + (size_t)w.b * N * w.pitch + (size_t)n * w.pitch + (size_t)w.h * HD + r;
#pragma unroll
      for (int db = 0; db < 4; ++db) dst[16 * db] = dq[db][i] * scale;
    }
  }
}

// ---- backward: dK and dV -----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void mha_bwd_dkv_kernel(const float* __restrict__ qkv, const float* __restrict__ out,
                                                         const float* __restrict__ dout, const float* __restrict__ lse,
                                                         float* __restrict__ dqkv, int N, int H, int nblk, float scale, float c) {
  __shared__ __attribute__((aligned(16))) float Qs[BLK * LDW];
  __shared__ __attribute__((aligned(16))) float Gs[BLK * LDW];    // dout
  __shared__ __attribute__((aligned(16))) float Ls[BLK];          // lse * log2(e); +inf for a query beyond N
  __shared__ __attribute__((aligned(16))) float Ds[BLK];          // delta
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 15, g = lane >> 4;
  const Where w = where(qkv, N, H, nblk);
  const int k0 = w.blk * BLK + wave * 16;
  const bool live = k0 < N;
  const bool key_ok = k0 + r < N;
  const size_t opitch = (size_t)H * HD;
  const size_t obase = (size_t)w.b * N * opitch + (size_t)w.h * HD;
  float k[16], v[16];
  load_operand(k, w.k, w.pitch, k0 + r, N, g);
  load_operand(v, w.v, w.pitch, k0 + r, N, g);
  f4 dk[4], dv[4];
#pragma unroll
  for (int db = 0; db < 4; ++db) dk[db] = dv[db] = f4{0.f, 0.f, 0.f, 0.f};

  const float* lrow = lse + ((size_t)w.b * H + w.h) * N;
  Piece pq, pg, po;
  fetch(pq, w.q, w.pitch, 0, N, tid);
  fetch(pg, dout + obase, opitch, 0, N, tid);
  fetch(po, out + obase, opitch, 0, N, tid);
  float pl = tid < BLK && tid < N ? lrow[tid] : INFINITY;   // lse of query tid of the block; +inf for a query beyond N
  for (int qb = 0; qb < N; qb += BLK) {
    __syncthreads();
    put(Qs, pq, tid);
    put(Gs, pg, tid);
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // delta of dout's rows: 16 lanes hold one row
      float d = pg.v[i][0] * po.v[i][0];
      d = fmaf(pg.v[i][1], po.v[i][1], d);
      d = fmaf(pg.v[i][2], po.v[i][2], d);
      d = fmaf(pg.v[i][3], po.v[i][3], d);
      d += __shfl_xor(d, 1);
      d += __shfl_xor(d, 2);
      d += __shfl_xor(d, 4);
      d += __shfl_xor(d, 8);
      if ((tid & 15) == 0) Ds[(tid >> 4) + 16 * i] = d;
    }
    if (tid < BLK) Ls[tid] = pl * LOG2E;
    __syncthreads();
    if (qb + BLK < N) {
      fetch(pq, w.q, w.pitch, qb + BLK, N, tid);
      fetch(pg, dout + obase, opitch, qb + BLK, N, tid);
      fetch(po, out + obase, opitch, qb + BLK, N, tid);
      pl = tid < BLK && qb + BLK + tid < N ? lrow[qb + BLK + tid] : INFINITY;
    }
    if (!live) continue;
#pragma unroll
    for (int tile = 0; tile < 4; ++tile) {
      if (qb + 16 * tile >= N) break;
      f4 s = {0.f, 0.f, 0.f, 0.f}, dp = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const f4 qq = *reinterpret_cast<const f4*>(Qs + (16 * tile + r) * LDW + 16 * t + 4 * g);
        const f4 gg = *reinterpret_cast<const f4*>(Gs + (16 * tile + r) * LDW + 16 * t + 4 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          s = mfma(qq[j], k[4 * t + j], s);
          dp = mfma(gg[j], v[4 * t + j], dp);
        }
      }
      const f4 L4 = *reinterpret_cast<const f4*>(Ls + 16 * tile + 4 * g);
      const f4 D4 = *reinterpret_cast<const f4*>(Ds + 16 * tile + 4 * g);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        s[i] = key_ok ? exp2f(fmaf(s[i], c, -L4[i])) : 0.f;
        dp[i] = s[i] * (dp[i] - D4[i]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float* grow = Gs + (16 * tile + 4 * g + j) * LDW + r;
        const float* qrow = Qs + (16 * tile + 4 * g + j) * LDW + r;
#pragma unroll
        for (int db = 0; db < 4; ++db) {
          dv[db] = mfma(s[j], grow[16 * db], dv[db]);
          dk[db] = mfma(dp[j], qrow[16 * db], dk[db]);
        }
      }
    }
  }
  if (!live) return;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int n = k0 + 4 * g + i;
    if (n < N) {
      float* dst = dqkv + (size_t)w.b * N * w.pitch + (size_t)n * w.pitch + (size_t)(H + w.h) * HD + r;
#pragma unroll
      for (int db = 0; db < 4; ++db) {
        dst[16 * db] = dk[db][i] * scale;
        dst[(size_t)H * HD + 16 * db] = dv[db][i];
      }
    }
  }
}

int validate(int B, int N, int H, int D, float scale, int& nblk, unsigned& grid) {
  if (B < 1 || N < 1 || H < 1 || !(scale > 0.f) || !(scale < INFINITY)) return 1;
  if (D != HD || N > U3D_MHA_MAX_SEQLEN) return 2;
  nblk = (N + BLK - 1) / BLK;
  const size_t blocks = (size_t)B * H * nblk;
  if (blocks >= (size_t)1 << 31) return 2;
  grid = (unsigned)blocks;
  return 0;
}

}  // namespace

extern "C" {

int u3d_mha_abi_version(void) { return U3D_MHA_ABI_VERSION; }

int u3d_mha_fwd(const float* qkv, float* out, float* lse, int B, int N, int H, int D, float softmax_scale, void* stream) {
  if (!qkv || !out || !lse) return 1;
  if (!u3d_util::aligned16(qkv) || !u3d_util::aligned16(out) || !u3d_util::aligned16(lse)) return 1;
  int nblk = 0;
  unsigned grid = 0;
  if (const int rc = validate(B, N, H, D, softmax_scale, nblk, grid)) return rc;
  hipLaunchKernelGGL(mha_fwd_kernel, dim3(grid), dim3(NT), 0, (hipStream_t)stream, qkv, out, lse, N, H, nblk, softmax_scale,
                     softmax_scale * LOG2E);
  return u3d_util::launched();
}

int u3d_mha_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv, int B, int N, int H, int D,
                float softmax_scale, void* stream) {
  if (!qkv || !out || !dout || !lse || !dqkv) return 1;
  if (!u3d_util::aligned16(qkv) || !u3d_util::aligned16(out) || !u3d_util::aligned16(dout) || !u3d_util::aligned16(lse) ||
      !u3d_util::aligned16(dqkv))
    return 1;
  int nblk = 0;
  unsigned grid = 0;
  if (const int rc = validate(B, N, H, D, softmax_scale, nblk, grid)) return rc;
  hipLaunchKernelGGL(mha_bwd_dkv_kernel, dim3(grid), dim3(NT), 0, (hipStream_t)stream, qkv, out, dout, lse, dqkv, N, H, nblk,
                     softmax_scale, softmax_scale * LOG2E);
  if (const int rc = u3d_util::launched()) return rc;
  hipLaunchKernelGGL(mha_bwd_dq_kernel, dim3(grid), dim3(NT), 0, (hipStream_t)stream, qkv, out, dout, lse, dqkv, N, H, nblk,
                     softmax_scale, softmax_scale * LOG2E);
  return u3d_util::launched();
}

}  // extern "C"
