/*
 * unipre3d_sparseconv.h -- C-ABI of the spconv-compatible sparse 3D convolution (SubMConv3d, SparseConv3d with kernel == stride,
 * SparseInverseConv3d) used by fuseTo3d and the scene backbones.  fp32, gfx950, everything on the caller's stream.
 *
 * Sites: DEVICE indices (N,4) int32 rows (batch, d0, d1, d2), 0 <= d < (D0, D1, D2) (host ints), batch < n_batch.  A site's key is its linear index
 * ((b * D0 + d0) * D1 + d1) * D2 + d2, so ascending keys are ascending (batch, d0, d1, d2).  Keys are sorted on the device with a
 * stable 8-bit LSD radix sort of (key, row), so every site's rows come out in ascending row order.
 *
 * Maps (integers, deterministic):
 *   u3d_spconv_subm_map   table (N,K) int32: for row o and tap k = (k0*k + k1)*k + k2, the LOWEST row at site(o) + (k0,k1,k2) - k/2,
 *                         or -1.  first (N): the lowest row at the row's own site.  next (N): the next row at the same site, or -1.
 *   u3d_spconv_down_map   SparseConv3d with kernel == stride = s, padding 0: output site of a row is d / s; rows whose output lies
 *                         outside out_shape = (D - s) / s + 1 are dropped.  Writes meta[0] = M output sites (the caller reads it to
 *                         size the outputs); u3d_spconv_down_emit then writes out_indices (M,4) ascending, table (M,K) (the lowest row
 *                         of each (output, tap)), first / next over rows at the same input site, and the tap-major list of all N rows:
 *                         list_row[e], list_src[e] = output * K + tap (-1 for a dropped row), ordered by (tap, output, row).
 * GEMM (Y rows written once, no float atomics):
 *   u3d_spconv_gemm       table mode (list_row == NULL): Y[o] = bias + sum_k A[table[o,k]] . W[k], rows o < R, table (R,K);
 *                         list mode: Y[list_row[e]] = bias + A[list_src[e] / K] . W[list_src[e] % K].  W is (K, Cin, Cout) row-major.
 *                         mask != NULL: rows with mask[o] != o are written as 0 (the input gradient of SubM's repeated rows).
 *   u3d_spconv_dupsum     out[r] = sum of in over r's chain (r, next[r], ...) where first[r] == r, else 0.
 *   u3d_spconv_wgrad      dW[k] = sum_o A[ia] (x) G[ig], ia = table[o,k], ig = o (gather_g == 0) or ia = o, ig = table[o,k] (gather_g == 1);
 *                         fixed-order split reduction through `partial` (u3d_spconv_wgrad_partial_floats floats).
 *   u3d_spconv_colsum     db[c] = sum_o G[o,c], fixed order through `partial` (u3d_spconv_colsum_partial_floats floats).
 * Which kernel a shape launches (the U3D_SPCONV_* macros below; a channel count of U3D_SPCONV_SMALL_C or less is "small"):
 *   gemm    Cin or Cout small: one VALU thread per output element; else the MFMA kernel, U3D_SPCONV_TILE rows x U3D_SPCONV_TILE
 *           columns per block, the channels in stages of U3D_SPCONV_KSTEP; a tap with no source in a block's rows is skipped.
 *   wgrad   Cin small: VALU, a thread per (tap, Cout channel); else Cout small: VALU, a thread per (tap, Cin channel); else MFMA,
 *           U3D_SPCONV_TILE x U3D_SPCONV_TILE of (Cin, Cout) per block, rows in steps of U3D_SPCONV_KSTEP (a step with no source at
 *           the tap is skipped).  Rows are divided over u3d_spconv_wgrad_partial_floats / (K * Cin * Cout) splits of equal length,
 *           a multiple of U3D_SPCONV_KSTEP, so trailing splits may own no row; a split's partial is then 0.
 *   colsum  u3d_spconv_colsum_partial_floats / C splits of rows.
 *   Partials are added per output by one thread in split order, or, from U3D_SPCONV_WAVE_SUM_SPLITS splits on, by one wave.
 * scratch: u3d_spconv_scratch_bytes(N) bytes, shared by a map call and its emit.
 * Returns 0 ok, 1 invalid argument, 2 unsupported shape, 3 launch failure.
 */
#ifndef UNIPRE3D_SPARSECONV_H
#define UNIPRE3D_SPARSECONV_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define U3D_SPCONV_ABI_VERSION 1
#define U3D_SPCONV_SMALL_C 8           /* a channel count at or below this takes the VALU kernels */
#define U3D_SPCONV_TILE 64             /* rows and columns of an MFMA block tile */
#define U3D_SPCONV_KSTEP 32            /* reduction elements per LDS stage; rows per wgrad step */
#define U3D_SPCONV_WAVE_SUM_SPLITS 64  /* from this many splits on, a wave adds an output's partials */
int u3d_spconv_abi_version(void);
size_t u3d_spconv_scratch_bytes(int n);
int u3d_spconv_subm_map(int N, const int32_t* indices, int n_batch, int D0, int D1, int D2, int k, int32_t* table, int32_t* first,
                        int32_t* next, void* scratch, void* stream);
int u3d_spconv_down_map(int N, const int32_t* indices, int n_batch, int D0, int D1, int D2, int s, int32_t* meta, void* scratch,
                        void* stream);
int u3d_spconv_down_emit(int N, int M, const int32_t* indices, int n_batch, int D0, int D1, int D2, int s, int32_t* out_indices,
                         int32_t* table, int32_t* first, int32_t* next, int32_t* list_row, int32_t* list_src, void* scratch,
                         void* stream);
int u3d_spconv_gemm(int R, int K, int Cin, int Cout, const int32_t* table, const int32_t* list_row, const float* A, const float* W,
                    const float* bias, const int32_t* mask, float* Y, void* stream);
int u3d_spconv_dupsum(int N, int C, const int32_t* first, const int32_t* next, const float* in, float* out, void* stream);
size_t u3d_spconv_wgrad_partial_floats(int R, int K, int Cin, int Cout);
int u3d_spconv_wgrad(int R, int K, int Cin, int Cout, const int32_t* table, int gather_g, const float* A, const float* G, float* partial,
                     float* dW, void* stream);
size_t u3d_spconv_colsum_partial_floats(int R, int C);
int u3d_spconv_colsum(int R, int C, const float* G, float* partial, float* db, void* stream);
#ifdef __cplusplus
}
#endif
#endif
