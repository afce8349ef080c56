/*
 * unipre3d_pointfusion.h -- C-ABI of the scene-level 2D->3D PointFusion: the reference's
 * fusion/point_fusion.py:35-190 with pointcept's GridSample(mode="train"|"test", hash_type="fnv") done on the device.
 *
 * The reference copies every valid unprojected pixel to the host and runs numpy there; this library keeps the points on the
 * device and the caller reads ONE small int32 record (`meta`, 4 words) per call to size the outputs:
 *   1. u3d_pointfusion_minmax   per-set min / max corner of a point set (the box of init_3d_data["coord"]).
 *   2. u3d_pointfusion_compact  order-preserving compaction of the (P,4) unprojected pixels: keep w != 0 (NaN counts as valid) and the
 *                               inclusive fp32 box; writes the kept xyz rows, their pixel indices and meta[0] = n.
 *   3. u3d_pointfusion_voxelize the grid coordinate (correctly rounded fp32 division; float -> int64 as numpy on x86: exact where the floor
 *                               fits, INT64_MIN for NaN and everything else) with one of GridSample's two origins,
 *                                 origin 0 (min_coord given):  grid = floor(fp32((xyz - min) / grid_size)), min = the caller's row;
 *                                 origin 1 (min_coord=None):   grid = floor(fp32(xyz / grid_size)) - floor(fp32(min / grid_size)), min = the
 *                                   set's OWN minimum (u3d_pointfusion_minmax): the reference's g - g.min(0), the cells of the absolute grid,
 *                               then the FNV-1a key of the reference's loop (multiply, then xor), a stable LSD radix sort of (set, key, index), segment heads.  Writes
 *                               meta[1] = M voxels, meta[2] = largest voxel count, voxel_offsets (n_sets + 1, voxels of each set).
 *                               n comes from meta[0] when n < 0 (after compact) -- no host read in between.
 *   4. u3d_pointfusion_pick     per voxel one point: start + r % count, r = draws[v] (replayed numpy draws) or a counter-based
 *                               hash of (seed, voxel rank in its set) modulo the set's largest count (mode 0 = train), or
 *                               start + part % count (mode 1 = test).  Writes the set-local point index, xyz, grid coordinate (same
 *                               min_coord and origin as voxelize) and (with src_map) the source pixel.
 *   5. u3d_pointfusion_inverse  per point its set-local voxel rank.
 *   6. u3d_pointfusion_gather_forward / _backward  feat[v][c] = feat_2d[view][c][pixel] straight from NCHW; the backward in gather
 *                               form: every element of the (V,C,H,W) gradient written exactly once (zero where no voxel picked the pixel).
 *                               PRECONDITION of the backward: src names every pixel at most once (true of the picks: a voxel picks one
 *                               point and a point lies in one voxel); with repeats it is not a general gather's gradient.
 * Ragged batches: n_sets point sets stored back to back, set_offsets = n_sets + 1 DEVICE int32 prefix sums (NULL when n_sets == 1);
 * voxels come out grouped by set, each group equal to a single-set call.  min_coord: DEVICE floats, row s at min_coord + s * min_stride.
 * scratch: u3d_pointfusion_scratch_bytes(n_max, n_sets) bytes, shared by compact / voxelize / pick / inverse of one call.
 * Point counts below 2^31.  Returns 0 ok, 1 invalid argument, 2 unsupported shape, 3 launch failure.
 */
#ifndef UNIPRE3D_POINTFUSION_H
#define UNIPRE3D_POINTFUSION_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define U3D_POINTFUSION_ABI_VERSION 2
int u3d_pointfusion_abi_version(void);
size_t u3d_pointfusion_scratch_bytes(int n_max, int n_sets);
int u3d_pointfusion_minmax(int n, int n_sets, const int32_t* set_offsets, const float* coord, float* minmax, void* stream);
int u3d_pointfusion_compact(int P, const float* uc4, const float* box, float* coord_out, int32_t* src_out, int32_t* meta,
                            void* scratch, void* stream);
int u3d_pointfusion_voxelize(int n_max, int n, int n_sets, const int32_t* set_offsets, const float* coord, const float* min_coord,
                             int min_stride, int origin, float grid_size, int32_t* meta, int32_t* voxel_offsets, void* scratch,
                             void* stream);
int u3d_pointfusion_pick(int M, int n_max, int n_sets, const int32_t* set_offsets, const int32_t* voxel_offsets, const float* coord,
                         const float* min_coord, int min_stride, int origin, float grid_size, int mode, int part, const int64_t* draws,
                         uint64_t seed, const int32_t* src_map, int64_t* out_index, float* out_coord, int64_t* out_grid,
                         int32_t* out_src, const void* scratch, void* stream);
int u3d_pointfusion_inverse(int n, int n_max, int n_sets, const int32_t* set_offsets, const int32_t* voxel_offsets, int64_t* inverse,
                            const void* scratch, void* stream);
int u3d_pointfusion_gather_forward(int M, int C, int HW, const float* feat, const int32_t* src, float* out, void* stream);
int u3d_pointfusion_gather_backward(int V, int C, int HW, int M, const float* grad_out, const int32_t* src, int32_t* pixel_map,
                                    float* grad_feat, void* stream);
#ifdef __cplusplus
}
#endif
#endif
