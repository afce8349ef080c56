// Mamba's selective scan (the S6 recurrence) for gfx950, forward and backward; see include/unipre3d_selective_scan.h.
//
// The recurrence x_l = a_l x_{l-1} + b_l (a_l = exp(dt_l A), b_l = dt_l B_l u_l) is a scan of the pairs (a, b) under
// (a1,b1) o (a2,b2) = (a1 a2, a2 b1 + b2).  One wave owns one (batch, channel) row; L is the parallel axis: lane i owns R consecutive
// steps of a pass of 64 R steps, composes them into one pair, the 64 pairs are scanned with DPP moves (row_shr 1/2/4/8 inside the
// 16-lane rows, then the two row broadcasts), the exclusive result applied to the state carried in from the previous pass gives the
// state in front of the lane's run, and the run is replayed.  Steps at or beyond L are the identity (1, 0), so the last lane's
// inclusive pair always carries the whole pass.  The 16 states of a channel are 16 independent scans over the same loads.
//
// The backward recomputes the states of a pass from the state the forward saved at the end of the pass before, and runs the passes
// last to first: h_l = a_l (C_l dy_l + h_{l+1}) is the same kind of scan in reversed time (the pairs are mirrored across the wave, scanned
// with the same DPP sequence, and mirrored back).  A workgroup of four waves walks a slab of 64 channels of one group: dB / dC
// accumulate in registers across a wave's 16 channels, are summed across the four waves through LDS in a fixed order, and are written
// once per slab.  dA / dD / ddelta_bias are wave sums per (b, d), accumulated over the passes in LDS, written as per-(b,d) partials and
// reduced over b by a second launch.  No float atomics anywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unipre3d_selective_scan.h"
#include "u3d_util.h"

namespace {

using namespace u3d_util;

constexpr int NT = 256;                   // threads per workgroup (four waves)
constexpr int NW = NT / 64;
constexpr int NS = U3D_SSCAN_DSTATE;      // states per channel
constexpr int SLAB = U3D_SSCAN_SLAB;      // channels one backward workgroup walks
constexpr int CPW = SLAB / NW;            // ... per wave
constexpr int NPAR = NS + 2;              // per-(b,d) partials: dA[16], dD, ddelta_bias

// (a, b) of this lane := (a, b) of the DPP source lane, THEN this lane's own; lanes without a source compose with the identity
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ void compose_from(float& a, float& b) {
  const float ao = dpp_f<CTRL, ROW_MASK>(1.f, a), bo = dpp_f<CTRL, ROW_MASK>(0.f, b);
  b = fmaf(a, bo, b);
  a *= ao;
}
__device__ __forceinline__ void wave_scan(float& a, float& b) {   // inclusive scan of the pairs in lane order
  compose_from<0x111, 0xf>(a, b);   // row_shr:1
  compose_from<0x112, 0xf>(a, b);   // row_shr:2
  compose_from<0x114, 0xf>(a, b);   // row_shr:4
  compose_from<0x118, 0xf>(a, b);   // row_shr:8
  compose_from<0x142, 0xa>(a, b);   // row_bcast:15 into rows 1 and 3
  compose_from<0x143, 0xc>(a, b);   // row_bcast:31 into rows 2 and 3
}
__device__ __forceinline__ float softplus_f(float x) { return x > 20.f ? x : log1pf(expf(x)); }

struct Args {
  const float *u, *delta, *A, *Bm, *Cm, *Dv, *z, *delta_bias, *dout, *xsave_in;
  float *out, *last_state, *xsave, *du, *ddelta, *dz, *partB, *partC, *par;
  int D, G, L, npass, spg, nslab, softplus;
};

template <int R>
__global__ __launch_bounds__(NT) void sscan_fwd_kernel(const Args p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int d = blockIdx.x * NW + wave, b = blockIdx.y;
  if (d >= p.D) return;                                   // (no workgroup barrier in this kernel)
  const int L = p.L, g = d / (p.D / p.G);
  const size_t bd = (size_t)b * p.D + d, row = bd * L, bc = ((size_t)b * p.G + g) * NS * L;
  float An[NS], carry[NS];
#pragma unroll
  for (int n = 0; n < NS; ++n) { An[n] = p.A[(size_t)d * NS + n]; carry[n] = 0.f; }
  const float bias = p.delta_bias ? p.delta_bias[d] : 0.f, Dd = p.Dv ? p.Dv[d] : 0.f;
  for (int ps = 0; ps < p.npass; ++ps) {
    const int l0 = (ps * 64 + lane) * R;
    float uu[R], dt[R], y[R];
    int li[R];                                            // steps at or beyond L load element 0 (always there) and select 0: no branch
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const bool ok = l0 + r < L;
      li[r] = ok ? l0 + r : 0;
      const float uv = p.u[row + li[r]], dv = p.delta[row + li[r]];
      uu[r] = ok ? uv : 0.f;
      float t = dv + bias;
      if (p.softplus) t = softplus_f(t);
      dt[r] = ok ? t : 0.f;
      y[r] = 0.f;
    }
#pragma unroll
    for (int n = 0; n < NS; ++n) {
      float ar[R], br[R], cr[R], a = 1.f, bb = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const bool ok = l0 + r < L;
        const float Bl = p.Bm[bc + (size_t)n * L + li[r]], Cl = p.Cm[bc + (size_t)n * L + li[r]];
        const float Bv = ok ? Bl : 0.f;
        cr[r] = ok ? Cl : 0.f;
        ar[r] = expf(dt[r] * An[n]);
        br[r] = dt[r] * Bv * uu[r];
        bb = fmaf(ar[r], bb, br[r]);
        a *= ar[r];
      }
      wave_scan(a, bb);
      float x = fmaf(dpp_f<0x138, 0xf>(1.f, a), carry[n], dpp_f<0x138, 0xf>(0.f, bb));   // wave_shr:1 = the exclusive pair
#pragma unroll
      for (int r = 0; r < R; ++r) {
        x = fmaf(ar[r], x, br[r]);
        y[r] = fmaf(cr[r], x, y[r]);
      }
      carry[n] = fmaf(lane_f<63>(a), carry[n], lane_f<63>(bb));
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
      if (l0 + r < L) {
        float v = fmaf(Dd, uu[r], y[r]);
        if (p.z) { const float zz = p.z[row + l0 + r]; v *= zz * sigmoid_f(zz); }
        p.out[row + l0 + r] = v;
      }
    }
    if (p.xsave && lane == 0) {
#pragma unroll
      for (int n = 0; n < NS; ++n) p.xsave[(bd * p.npass + ps) * NS + n] = carry[n];
    }
  }
  if (p.last_state && lane == 0) {
#pragma unroll
    for (int n = 0; n < NS; ++n) p.last_state[bd * NS + n] = carry[n];
  }
}

template <int R>
__global__ __launch_bounds__(NT) void sscan_bwd_kernel(const Args p) {
  __shared__ float s_red[NW][8 * R][64];     // half of dB or dC of every wave, for the fixed-order sum across the waves
  __shared__ float s_h[NW][CPW][NS];         // h = a_l dx_l flowing out of a pass into the one before it, per channel and state
  __shared__ float s_par[NW][CPW][NPAR];     // dA[16], dD, ddelta_bias of a (b, d), accumulated over the passes
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int L = p.L, D = p.D, G = p.G, Dg = D / G;
  const int g = blockIdx.x / p.spg, s = blockIdx.x % p.spg, b = blockIdx.y;
  const int ch0 = g * Dg + s * SLAB, nch = min(SLAB, Dg - s * SLAB);
  for (int i = lane; i < CPW * NS; i += 64) (&s_h[wave][0][0])[i] = 0.f;
  for (int i = lane; i < CPW * NPAR; i += 64) (&s_par[wave][0][0])[i] = 0.f;
  __syncthreads();
  const size_t bc = ((size_t)b * G + g) * NS * L;
  const size_t slab_row = ((size_t)b * p.nslab + blockIdx.x) * NS;
  for (int ps = p.npass - 1; ps >= 0; --ps) {
    const int l0 = (ps * 64 + lane) * R;
    float accB[NS][R], accC[NS][R];
    int li[R];                                            // steps at or beyond L load element 0 (always there) and select 0: no branch
#pragma unroll
    for (int r = 0; r < R; ++r) li[r] = l0 + r < L ? l0 + r : 0;
#pragma unroll
    for (int n = 0; n < NS; ++n) {
#pragma unroll
      for (int r = 0; r < R; ++r) accB[n][r] = accC[n][r] = 0.f;
    }
    for (int ci = wave, k = 0; ci < nch; ci += NW, ++k) {
      const int d = ch0 + ci;
      const size_t bd = (size_t)b * D + d, row = bd * L;
      const float bias = p.delta_bias ? p.delta_bias[d] : 0.f, Dd = p.Dv ? p.Dv[d] : 0.f;
      float uu[R], dt[R], sp[R], dy[R], dov[R], zz[R], sig[R], y[R], ddt[R], du[R];
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const bool ok = l0 + r < L;
        const float uv = p.u[row + li[r]], dv = p.delta[row + li[r]], gv = p.dout[row + li[r]];
        uu[r] = ok ? uv : 0.f;
        float t = dv + bias;
        float dsp = 1.f;                                  // d softplus / d raw: sigmoid, 1 above 20
        if (p.softplus) { dsp = t > 20.f ? 1.f : sigmoid_f(t); t = softplus_f(t); }
        dt[r] = ok ? t : 0.f;
        sp[r] = ok ? dsp : 0.f;
        dov[r] = ok ? gv : 0.f;
        zz[r] = 0.f; sig[r] = 0.f;
        dy[r] = dov[r];
        if (p.z) {
          const float zv = p.z[row + li[r]];
          zz[r] = ok ? zv : 0.f;
          sig[r] = sigmoid_f(zz[r]);
          dy[r] = dov[r] * zz[r] * sig[r];
        }
        y[r] = ddt[r] = du[r] = 0.f;
      }
#pragma unroll
      for (int n = 0; n < NS; ++n) {
        const float An = p.A[(size_t)d * NS + n];
        const float xin = ps > 0 ? p.xsave_in[(bd * p.npass + ps - 1) * NS + n] : 0.f;
        const float hin = s_h[wave][k][n];
        float ar[R], br[R], cr[R], Bv[R], xp[R], a = 1.f, bb = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const bool ok = l0 + r < L;
          const float Bl = p.Bm[bc + (size_t)n * L + li[r]], Cl = p.Cm[bc + (size_t)n * L + li[r]];
          Bv[r] = ok ? Bl : 0.f;
          cr[r] = ok ? Cl : 0.f;
          ar[r] = expf(dt[r] * An);
          br[r] = dt[r] * Bv[r] * uu[r];
          bb = fmaf(ar[r], bb, br[r]);
          a *= ar[r];
        }
        wave_scan(a, bb);
        float x = fmaf(dpp_f<0x138, 0xf>(1.f, a), xin, dpp_f<0x138, 0xf>(0.f, bb));
#pragma unroll
        for (int r = 0; r < R; ++r) {
          xp[r] = x;
          x = fmaf(ar[r], x, br[r]);
          y[r] = fmaf(cr[r], x, y[r]);
          accC[n][r] = fmaf(dy[r], x, accC[n][r]);
        }
        // reversed time: h_out = a_r (C_r dy_r + h_in), the run composed last step first, the wave mirrored so that later runs come first
        float ra = 1.f, rb = 0.f;
#pragma unroll
        for (int r = R - 1; r >= 0; --r) {
          rb = fmaf(ar[r], rb, ar[r] * cr[r] * dy[r]);
          ra *= ar[r];
        }
        ra = __shfl(ra, 63 - lane);
        rb = __shfl(rb, 63 - lane);
        wave_scan(ra, rb);
        float h = fmaf(dpp_f<0x138, 0xf>(1.f, ra), hin, dpp_f<0x138, 0xf>(0.f, rb));
        const float hout = fmaf(lane_f<63>(ra), hin, lane_f<63>(rb));
        h = __shfl(h, 63 - lane);
        float dAp = 0.f;
#pragma unroll
        for (int r = R - 1; r >= 0; --r) {
          const float gx = fmaf(cr[r], dy[r], h);          // d loss / d x_l
          const float ax = ar[r] * xp[r];
          ddt[r] = fmaf(gx, fmaf(An, ax, Bv[r] * uu[r]), ddt[r]);
          du[r] = fmaf(gx * dt[r], Bv[r], du[r]);
          dAp = fmaf(gx * dt[r], ax, dAp);
          accB[n][r] = fmaf(gx * dt[r], uu[r], accB[n][r]);
          h = ar[r] * gx;
        }
        const float dAs = wave_sum(dAp);
        if (lane == 0) {
          s_h[wave][k][n] = hout;
          s_par[wave][k][n] += dAs;
        }
      }
      float dDp = 0.f, dbp = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        if (l0 + r < L) {
          p.du[row + l0 + r] = fmaf(Dd, dy[r], du[r]);
          const float dd = ddt[r] * sp[r];
          p.ddelta[row + l0 + r] = dd;
          dbp += dd;
          dDp = fmaf(dy[r], uu[r], dDp);
          if (p.z && p.dz) p.dz[row + l0 + r] = dov[r] * fmaf(Dd, uu[r], y[r]) * sig[r] * (1.f + zz[r] * (1.f - sig[r]));
        }
      }
      const float s1 = wave_sum(dDp), s2 = wave_sum(dbp);
      if (lane == 0) {
        s_par[wave][k][NS] += s1;
        s_par[wave][k][NS + 1] += s2;
      }
    }
    // dB then dC of this pass, eight states at a time: every wave posts its sums, wave w adds states 2w and 2w+1 of the half over
    // the waves in the order 0, 1, 2, 3
#pragma unroll
    for (int st = 0; st < 4; ++st) {
      __syncthreads();
#pragma unroll
      for (int j = 0; j < 8; ++j) {
#pragma unroll
        for (int r = 0; r < R; ++r) s_red[wave][j * R + r][lane] = st < 2 ? accB[(st & 1) * 8 + j][r] : accC[(st & 1) * 8 + j][r];
      }
      __syncthreads();
      float* dst = st < 2 ? p.partB : p.partC;
#pragma unroll
      for (int j2 = 0; j2 < 2; ++j2) {
        const int j = wave * 2 + j2, n = (st & 1) * 8 + j;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float v = ((s_red[0][j * R + r][lane] + s_red[1][j * R + r][lane]) + s_red[2][j * R + r][lane]) + s_red[3][j * R + r][lane];
          if (l0 + r < L) dst[(slab_row + n) * L + l0 + r] = v;
        }
      }
    }
  }
  __syncthreads();
  for (int i = lane; i < CPW * NPAR; i += 64) {
    const int k = i / NPAR, j = i % NPAR, ci = wave + k * NW;
    if (ci < nch) p.par[((size_t)b * D + ch0 + ci) * NPAR + j] = s_par[wave][k][j];
  }
}

// dB / dC (B,G,N,L) from the per-slab partials (B,nslab,N,L), slabs of a group in ascending order
__global__ __launch_bounds__(NT) void sscan_reduce_bc_kernel(const float* partB, const float* partC, float* dB, float* dC, int G, int spg,
                                                             size_t NL, size_t total) {
  const size_t i = (size_t)blockIdx.x * NT + threadIdx.x;
  if (i >= total) return;
  const size_t bg = i / NL, e = i % NL;
  const size_t b = bg / G, g = bg % G;
  const size_t base = (b * G * spg + g * spg) * NL + e;
  float sb = 0.f, sc = 0.f;
  for (int s = 0; s < spg; ++s) { sb += partB[base + (size_t)s * NL]; sc += partC[base + (size_t)s * NL]; }
  dB[i] = sb;
  dC[i] = sc;
}

// dA (D,N), dD (D), ddelta_bias (D) from the per-(b,d) partials, b ascending
__global__ __launch_bounds__(NT) void sscan_reduce_par_kernel(const float* par, float* dA, float* dD, float* dbias, int B, int D) {
  const int i = blockIdx.x * NT + threadIdx.x;
  if (i >= D * NPAR) return;
  const int d = i / NPAR, j = i % NPAR;
  float* dst = j < NS ? dA + (size_t)d * NS + j : j == NS ? (dD ? dD + d : nullptr) : (dbias ? dbias + d : nullptr);
  if (!dst) return;
  float sum = 0.f;
  for (int b = 0; b < B; ++b) sum += par[((size_t)b * D + d) * NPAR + j];
  *dst = sum;
}

int check_shape(int B, int D, int G, int N, int L) {
  if (B < 1 || D < 1 || G < 1 || L < 1 || N < 1) return 1;
  if (N != NS || D % G != 0 || B > 65535) return 2;
  return 0;
}
inline int slabs_per_group(int D, int G) { return (D / G + SLAB - 1) / SLAB; }

}  // namespace

extern "C" {

int u3d_sscan_abi_version(void) { return U3D_SSCAN_ABI_VERSION; }

int u3d_sscan_pass_len(int L) { return 64 * steps_per_lane(L); }

size_t u3d_sscan_bwd_scratch_bytes(int B, int D, int G, int L) {
  if (B < 1 || D < 1 || G < 1 || L < 1 || D % G != 0) return 0;
  size_t bytes = align256((size_t)B * D * NPAR * sizeof(float));
  const int spg = slabs_per_group(D, G);
  if (spg > 1) bytes += 2 * align256((size_t)B * G * spg * NS * L * sizeof(float));
  return bytes;
}

int u3d_sscan_fwd(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm, const float* Dv, const float* z,
                  const float* delta_bias, float* out, float* last_state, float* xsave, int B, int D, int G, int N, int L,
                  int delta_softplus, void* stream) {
  if (!u || !delta || !A || !Bm || !Cm || !out) return 1;
  if (const int rc = check_shape(B, D, G, N, L)) return rc;
  const int R = steps_per_lane(L);
  Args p = {};
  p.u = u; p.delta = delta; p.A = A; p.Bm = Bm; p.Cm = Cm; p.Dv = Dv; p.z = z; p.delta_bias = delta_bias;
  p.out = out; p.last_state = last_state; p.xsave = xsave;
  p.D = D; p.G = G; p.L = L; p.npass = (L + 64 * R - 1) / (64 * R); p.softplus = delta_softplus != 0;
  const dim3 grid((D + NW - 1) / NW, B);
  hipStream_t st = (hipStream_t)stream;
  switch (R) {
    case 1: hipLaunchKernelGGL(sscan_fwd_kernel<1>, grid, dim3(NT), 0, st, p); break;
    case 2: hipLaunchKernelGGL(sscan_fwd_kernel<2>, grid, dim3(NT), 0, st, p); break;
    case 3: hipLaunchKernelGGL(sscan_fwd_kernel<3>, grid, dim3(NT), 0, st, p); break;
    default: hipLaunchKernelGGL(sscan_fwd_kernel<4>, grid, dim3(NT), 0, st, p); break;
  }
  return launched();
}

int u3d_sscan_bwd(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm, const float* Dv, const float* z,
                  const float* delta_bias, const float* dout, const float* xsave, float* du, float* ddelta, float* dA, float* dB,
                  float* dC, float* dD, float* dz, float* ddelta_bias, void* scratch, size_t scratch_bytes, int B, int D, int G, int N,
                  int L, int delta_softplus, void* stream) {
  if (!u || !delta || !A || !Bm || !Cm || !dout || !du || !ddelta || !dA || !dB || !dC || !scratch) return 1;
  if (const int rc = check_shape(B, D, G, N, L)) return rc;
  const int R = steps_per_lane(L), npass = (L + 64 * R - 1) / (64 * R);
  if (npass > 1 && !xsave) return 1;
  if (scratch_bytes < u3d_sscan_bwd_scratch_bytes(B, D, G, L) || ((uintptr_t)scratch & 255)) return 1;
  const int spg = slabs_per_group(D, G);
  if (((size_t)B * G * NS * L + NT - 1) / NT > 0x7fffffffull) return 2;
  const size_t par_bytes = align256((size_t)B * D * NPAR * sizeof(float));
  const size_t part_bytes = align256((size_t)B * G * spg * NS * L * sizeof(float));
  Args p = {};
  p.u = u; p.delta = delta; p.A = A; p.Bm = Bm; p.Cm = Cm; p.Dv = Dv; p.z = z; p.delta_bias = delta_bias; p.dout = dout;
  p.xsave_in = xsave; p.du = du; p.ddelta = ddelta; p.dz = z ? dz : nullptr;
  p.par = (float*)scratch;
  // one slab per group: the slab's sums ARE the group's, (B,nslab,N,L) with nslab == G is dB's own layout
  p.partB = spg > 1 ? (float*)((char*)scratch + par_bytes) : dB;
  p.partC = spg > 1 ? (float*)((char*)scratch + par_bytes + part_bytes) : dC;
  p.D = D; p.G = G; p.L = L; p.npass = npass; p.spg = spg; p.nslab = G * spg; p.softplus = delta_softplus != 0;
  const dim3 grid(G * spg, B);
  hipStream_t st = (hipStream_t)stream;
  switch (R) {
    case 1: hipLaunchKernelGGL(sscan_bwd_kernel<1>, grid, dim3(NT), 0, st, p); break;
    case 2: hipLaunchKernelGGL(sscan_bwd_kernel<2>, grid, dim3(NT), 0, st, p); break;
    case 3: hipLaunchKernelGGL(sscan_bwd_kernel<3>, grid, dim3(NT), 0, st, p); break;
    default: hipLaunchKernelGGL(sscan_bwd_kernel<4>, grid, dim3(NT), 0, st, p); break;
  }
  if (const int rc = launched()) return rc;
  if (spg > 1) {
    const size_t NL = (size_t)NS * L, total = (size_t)B * G * NL;
    hipLaunchKernelGGL(sscan_reduce_bc_kernel, dim3((unsigned)((total + NT - 1) / NT)), dim3(NT), 0, st, p.partB, p.partC, dB, dC, G, spg,
                       NL, total);
    if (const int rc = launched()) return rc;
  }
  hipLaunchKernelGGL(sscan_reduce_par_kernel, dim3((D * NPAR + NT - 1) / NT), dim3(NT), 0, st, p.par, dA, Dv ? dD : nullptr,
                     delta_bias ? ddelta_bias : nullptr, B, D);
  return launched();
}

}  // extern "C"
