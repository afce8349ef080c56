/*
 * unipre3d_selective_scan.h -- C-ABI of Mamba's selective scan (the S6 recurrence), forward and backward, for the mamba3d and pcm
 * backbones.  gfx950, fp32 throughout, real A, input-dependent B and C, state size N == 16.  Everything runs on the caller's stream;
 * no allocation, no host sync, no host read of device data, no float atomics: two calls on the same inputs give the same bits.
 *
 *   dt[b,d,l]  = delta[b,d,l] (+ delta_bias[d]); softplus when delta_softplus (identity above 20, torch's rule)
 *   x[b,d,n,l] = exp(dt * A[d,n]) * x[b,d,n,l-1] + dt * B[b,g(d),n,l] * u[b,d,l],   x[.,.,.,-1] = 0
 *   y[b,d,l]   = sum_n C[b,g(d),n,l] * x[b,d,n,l] (+ D[d] * u[b,d,l])
 *   out        = y (* silu(z[b,d,l]) when z is given)
 *
 * Layouts (all contiguous): u, delta, z, out, dout (B,D,L); A (D,N); B, C (B,G,N,L) with G dividing D and g(d) = d / (D/G);
 * D, delta_bias (D); last_state (B,D,N).  Dv, z and delta_bias may be NULL (absent).
 *
 * One wave owns one (b, d) row and walks L in passes of u3d_sscan_pass_len(L) steps (64 lanes x 1 .. 4 steps per lane, chosen from L);
 * the state is carried from pass to pass.  npass = ceil(L / pass_len).
 *
 *   u3d_sscan_fwd   writes out; last_state (may be NULL) = x[., ., ., L-1]; xsave (may be NULL; (B,D,npass,N)) = the state at the END
 *                   of every pass, which the backward starts its recomputation from.
 *   u3d_sscan_bwd   from dout and the forward's inputs and xsave: du, ddelta (B,D,L), dA (D,N), dB, dC (B,G,N,L) always; dD, dz,
 *                   ddelta_bias only when the matching input AND the output pointer are given (a NULL output is never written).
 *                   scratch: u3d_sscan_bwd_scratch_bytes(B, D, G, L) bytes of device memory, 256-byte aligned, contents irrelevant.
 *                   dB / dC are summed over the channels of a group in a fixed order (registers per wave, LDS across the four waves
 *                   of a workgroup, and a partials buffer plus a reduce launch when a group spans more than one 64-channel slab);
 *                   dA / dD / ddelta_bias are per-(b,d) partials reduced over b in ascending order by a second launch.
 *
 * Returns 0 ok, 1 invalid argument, 2 unsupported shape (N != 16, G not dividing D, B > 65535), 3 launch failure.
 */
#ifndef UNIPRE3D_SELECTIVE_SCAN_H
#define UNIPRE3D_SELECTIVE_SCAN_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define U3D_SSCAN_ABI_VERSION 1
#define U3D_SSCAN_DSTATE 16
#define U3D_SSCAN_SLAB 64
int u3d_sscan_abi_version(void);
int u3d_sscan_pass_len(int L);
size_t u3d_sscan_bwd_scratch_bytes(int B, int D, int G, int L);
int u3d_sscan_fwd(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm, const float* Dv, const float* z,
                  const float* delta_bias, float* out, float* last_state, float* xsave, int B, int D, int G, int N, int L,
                  int delta_softplus, void* stream);
int u3d_sscan_bwd(const float* u, const float* delta, const float* A, const float* Bm, const float* Cm, const float* Dv, const float* z,
                  const float* delta_bias, const float* dout, const float* xsave, float* du, float* ddelta, float* dA, float* dB,
                  float* dC, float* dD, float* dz, float* ddelta_bias, void* scratch, size_t scratch_bytes, int B, int D, int G, int N,
                  int L, int delta_softplus, void* stream);
#ifdef __cplusplus
}
#endif
#endif
