/*
 * unipre3d_serialization.h -- C-ABI of PTv3's index plumbing: space-filling-curve codes, their stable sort, the patch padding of
 * SerializedAttention and the pooling clusters of SerializedPooling.  Integers only, gfx950, everything on the caller's stream.
 *
 * Orders: 0 z, 1 z-trans, 2 hilbert, 3 hilbert-trans, packed two bits each into `orders` (order k in bits 2k, 2k+1), K = 1 .. 4 of
 * them.  A code is batch << 3*depth | curve(c0, c1, c2) with depth 1 .. 16; the -trans orders swap c0 and c1.  z is the bit
 * interleave with c0 in the high bit of each triple; hilbert is Skilling's transform on three registers, the same interleave, and
 * the Gray-to-binary fold of the interleaved word.  Only the low `depth` bits of a coordinate are used.
 *
 *   u3d_ser_encode      code (K,N) int64 from grid_coord (N,3) int32 (coord64 == 0) or int64, batch (N,) int32 / int64 (batch64) or
 *                       NULL.  One thread per point.
 *   u3d_ser_sort        order[k] = the STABLE ascending sort of code[k] (equal codes in ascending index), inverse[k][order[k][i]] = i,
 *                       both (K,N) int64.  8-bit LSD radix sort of (64-bit key, 32-bit index) over ceil(key_bits / 8) passes, all K
 *                       rows in one launch set; keys must be below 2^key_bits, key_bits 1 .. 64.  scratch: u3d_ser_scratch_bytes(K, N).
 *   u3d_ser_serialize   u3d_ser_encode then u3d_ser_sort.
 *   u3d_ser_patch_padding  meta (3, B+1) int64 on the DEVICE: rows offset, padded offset and sequence offset of the items, each with
 *                       a leading 0.  pad (meta[1][B],) int64, unpad (meta[0][B],) int64, cu_seqlens (meta[2][B] + 1,) int32; the
 *                       three totals are also passed as host ints (T, T_pad, S).  One launch; each slot finds its item by a binary
 *                       search over the B + 1 offsets.  An item of n <= patch rows is one sequence of n; a longer one is padded to a
 *                       multiple of patch and the tail slots of its last patch re-read the same positions of the patch before.
 *   u3d_ser_pool_count  stable sort of code[0] >> shift; writes meta[0] = M distinct values (the caller reads it to size the outputs).
 *   u3d_ser_pool_emit   cluster (N,), indices (N,), idx_ptr (M+1,), head_indices (M,), pooled code / order / inverse (K,M), all int64,
 *                       from the scratch u3d_ser_pool_count left.  key_bits is the width of the SHIFTED keys in both calls.
 *
 * PCM's order serialization (openpoints/models/PCM/PCM_utils.py `serialization`), B items of N points, rows = B N <= U3D_SER_MAX_ROWS:
 *   u3d_ser_pcm_grid    grid (B N, 3) int32 = floor(pos / grid_size) minus the item's minimum per axis, pos (B, N, 3) fp32; the division
 *                       is IEEE fp32 division.  meta (U3D_SER_PCM_META_HEAD + 3 B,) int32: words 0..2 the maxima of grid over all items
 *                       per axis, 3 depth = bit_length of the largest, 4 a flag (1 when a cell needs more than 16 bits or a quotient is
 *                       not finite; the results are then unspecified but every store stays in bounds), 5..7 zero, then per item its three
 *                       maxima (the workgroups' hand-off; word 0 of an item may carry bit 31).  Two launches, no atomics.
 *   u3d_ser_pcm_encode  code (B N,) int64 of PCM order `order`: 0 z, 1 z-trans, 2 hilbert, 3 hilbert-trans at meta's depth (depth 0: the
 *                       batch id), 4..9 xyz xzy yxz yzx zxy zyx as the reference's encode_cts computes them: with c1 the cell on the
 *                       first-named axis, m1 m2 m3 meta's maxima in the order's sequence, s(m) = 1 - 2 (m & 1), e(m) = m + (m & 1):
 *                       code = b m1 m2 m3 + e(m3) m1 m2 + s(m3) (e(m2) m1 + s(m2) c1).  Such codes may be negative.
 *   u3d_ser_sort_signed order (N,), inverse (N,) int64: the STABLE ascending sort of ANY int64 codes as signed numbers.  N <=
 *                       U3D_SER_SMALL_SORT: one workgroup runs the eight radix passes and skips those whose digit is the same in every
 *                       key; above: eight passes of the sort above, the top one with the sign bit inverted.  scratch:
 *                       u3d_ser_scratch_bytes(1, N).
 *   u3d_ser_pcm_order   the three above in a row (four launches up to U3D_SER_SMALL_SORT rows).
 *   u3d_ser_gather_rows dst[t][i] = src[t][index[i]] for T <= U3D_SER_GATHER_MAX tensors (rows, channels[t]) fp32, contiguous, 1 <=
 *                       channels[t] <= U3D_SER_GATHER_MAX_CHANNELS, in one launch; src, dst and channels are HOST arrays of T entries,
 *                       index (rows,) int64 on the device.  A row whose index is outside [0, rows) is written as zeros.  With the inverse
 *                       permutation as index it is its own backward.  No atomics.
 * Returns 0 ok, 1 invalid argument, 2 unsupported shape, 3 launch failure.
 */
#ifndef UNIPRE3D_SERIALIZATION_H
#define UNIPRE3D_SERIALIZATION_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define U3D_SER_ABI_VERSION 1
#define U3D_SER_MAX_ROWS (1 << 30)   /* most elements per row of codes */
int u3d_ser_abi_version(void);
size_t u3d_ser_scratch_bytes(int K, int N);
int u3d_ser_encode(int N, const void* grid_coord, int coord64, const void* batch, int batch64, int depth, int K, int orders,
                   int64_t* code, void* stream);
int u3d_ser_sort(int K, int N, int key_bits, const int64_t* code, int64_t* order, int64_t* inverse, void* scratch, void* stream);
int u3d_ser_serialize(int N, const void* grid_coord, int coord64, const void* batch, int batch64, int depth, int K, int orders,
                      int key_bits, int64_t* code, int64_t* order, int64_t* inverse, void* scratch, void* stream);
int u3d_ser_patch_padding(int B, int patch, long long T, long long T_pad, long long S, const int64_t* meta, int64_t* pad, int64_t* unpad,
                          int32_t* cu_seqlens, void* stream);
int u3d_ser_pool_count(int K, int N, int shift, int key_bits, const int64_t* code, int32_t* meta, void* scratch, void* stream);
int u3d_ser_pool_emit(int K, int N, int M, int shift, int key_bits, const int64_t* code, int64_t* cluster, int64_t* indices,
                      int64_t* idx_ptr, int64_t* head_indices, int64_t* pcode, int64_t* porder, int64_t* pinverse, void* scratch,
                      void* stream);
#define U3D_SER_PCM_META_HEAD 8             /* words of meta before the per-item maxima */
#define U3D_SER_PCM_ORDERS 10
#define U3D_SER_SMALL_SORT 8192             /* most keys of the one-workgroup signed sort */
#define U3D_SER_GATHER_MAX 8                /* tensors per gather launch */
#define U3D_SER_GATHER_MAX_CHANNELS 2048
int u3d_ser_pcm_grid(int B, int N, const float* pos, float grid_size, int32_t* grid, int32_t* meta, void* stream);
int u3d_ser_pcm_encode(int B, int N, int order, const int32_t* grid, const int32_t* meta, int64_t* code, void* stream);
int u3d_ser_sort_signed(int N, const int64_t* code, int64_t* order, int64_t* inverse, void* scratch, void* stream);
int u3d_ser_pcm_order(int B, int N, const float* pos, float grid_size, int order, int32_t* grid, int32_t* meta, int64_t* code,
                      int64_t* order_out, int64_t* inverse, void* scratch, void* stream);
int u3d_ser_gather_rows(long long rows, int T, const int64_t* index, const void* const* src, void* const* dst, const int32_t* channels,
                        void* stream);
#ifdef __cplusplus
}
#endif
#endif
