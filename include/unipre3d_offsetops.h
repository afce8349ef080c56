/*
 * unipre3d_offsetops.h -- C-ABI of the MI355X (gfx950) offset-batched ("ragged") point operators: the counterpart of
 * openpoints/cpp/pointops (knnquery, ballquery, grouping, interpolation, subtraction, aggregation; furthestsampling is u3d_offset_furthest_sampling of
 * unipre3d_pointops.h, beside the dense furthest point sampling whose tie keys and contraction modes it shares) and of the
 * `pointops.knn_query` call of pointcept/engines/hooks/evaluator.py.  Semantics restated on the CPU in tests/offsetops_ref.py.
 *
 * Conventions (as unipre3d_knn.h): raw DEVICE pointers and a HIP stream; fp32 data, int32 indices, int32 offsets; contiguous
 * row-major tensors.  Returns 0 on success, 1 invalid argument, 3 launch failure.  Every argument check returns before anything
 * touches a device.  Invalid (1): a negative size, k of u3d_offset_knn / nsample of u3d_offset_ballquery outside
 * 1..U3D_KNN_MAX_K (64, include/unipre3d_knn.h), n of the two searches above 2^31 - 1 - U3D_KNN_TILE, c % w_c != 0 or w_c < 1, a NULL
 * mandatory pointer of a non-empty call, more than 2^31 - 1 workgroups.  An empty call (valid sizes, but nothing to read or nothing
 * to write: b, m, c, n or m * nsample zero) returns 0 without a launch and writes NOTHING, the zero-fill of a (+) output included.
 * Every flat index is 64-bit.
 *
 * Batching.  A batch of b clouds is concatenated: xyz (n,3) with offset (b) the cumulative ENDS of the clouds, queries new_xyz (m,3)
 * with new_offset (b).  Query row j belongs to segment s, the first s with j < new_offset[s]; its support range is
 * [offset[s-1], offset[s]) with 0 for s = 0, clamped to [0, n]; end < start counts as empty.  A row at or beyond new_offset[b-1]
 * belongs to no segment and is treated like one with an empty range.  Whatever the offset arrays hold, no kernel reads outside xyz
 * and every written index is in [0, n) or is the documented fill.
 *
 *   u3d_offset_knn(b, n, m, k, xyz, new_xyz, offset, new_offset, dist2 (m,k) or NULL, idx (m,k), stream)
 *        Per query the k smallest (d2, index) pairs of its own segment in lexicographic order, ascending; indices are global rows
 *        of xyz.  d2 = (dx*dx + dy*dy) + dz*dz, every operation rounded on its own (unipre3d_knn.h); the selection is the one of
 *        u3d_knn (csrc/u3d_knn_core.h).  k may exceed the segment's size: slots without a neighbour get dist2 = 1e10f and the
 *        segment's first row as index (what the reference's initialisation leaves there), or -1 where the segment is empty.
 *   u3d_offset_ballquery(b, n, m, radius, nsample, xyz, new_xyz, offset, new_offset, idx (m,nsample), stream)
 *        The first nsample rows of the segment, in index order, with d2 < radius * radius (same d2, the product in fp32); remaining
 *        slots repeat the first hit; a query without a hit gets 0 in every slot.
 *
 * Index-addressed operators.  `idx` entries outside [0, rows) of the tensor they address never cause an access: the term they name
 * is skipped -- group writes 0, subtract reads the missing in2 row as 0, interpolate and aggregate drop the whole term (and its
 * gradients), the scatter-adds add nothing.
 *
 *   u3d_offset_group_forward(m, nsample, c, n, input (n,c), idx (m,nsample), out (m,nsample,c), stream)         out = input[idx]
 *   u3d_offset_group_backward(m, nsample, c, n, grad_out (m,nsample,c), idx, grad_in (n,c), stream)             scatter-add (+)
 *   u3d_offset_interpolate_forward(n_out, c, k, m_in, input (m_in,c), idx (n_out,k), weight (n_out,k), out (n_out,c), stream)
 *        out[i,ch] = sum_j input[idx[i,j],ch] * weight[i,j]
 *   u3d_offset_interpolate_backward(n_out, c, k, m_in, grad_out (n_out,c), idx, weight, grad_input (m_in,c), stream)   scatter-add (+)
 *   u3d_offset_subtract_forward(n, nsample, c, in1 (n,c), in2 (n,c), idx (n,nsample), out (n,nsample,c), stream)
 *        out[i,s] = in1[i] - in2[idx[i,s]]
 *   u3d_offset_subtract_backward(n, nsample, c, idx, grad_out (n,nsample,c), grad_in1 (n,c), grad_in2 (n,c), stream)
 *        grad_in1[i] = sum_s grad_out[i,s] (one writer per element, summed in registers in order of s);
 *        grad_in2 = scatter-add of -grad_out (+)
 *   u3d_offset_aggregate_forward(n, nsample, c, w_c, input (n,c), position (n,nsample,c), weight (n,nsample,w_c), idx (n,nsample),
 *                                out (n,c), stream)
 *        out[i,ch] = sum_s (input[idx[i,s],ch] + position[i,s,ch]) * weight[i,s,ch % w_c]
 *   u3d_offset_aggregate_backward(n, nsample, c, w_c, input, position, weight, idx, grad_out (n,c), grad_input (n,c),
 *                                 grad_position (n,nsample,c), grad_weight (n,nsample,w_c), stream)
 *        grad_position[i,s,ch] = g[i,ch] * weight[i,s,ch % w_c] (plain store);
 *        grad_weight[i,s,wc] = sum over ch = wc (mod w_c), ascending, of g[i,ch] * (input[idx[i,s],ch] + position[i,s,ch])
 *        (one writer per element); grad_input = scatter-add of g * weight (+)
 *
 * (+) The library zero-fills these outputs on the stream and adds into them with float atomics: their values depend on the order
 * in which the adds arrive, in their last bits, and may differ between two launches on the same inputs.  Every other output is
 * computed by one thread in a fixed order and is reproducible; the gathers (group forward, subtract forward) are bit-exact.
 */
#ifndef UNIPRE3D_OFFSETOPS_H
#define UNIPRE3D_OFFSETOPS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int u3d_offset_knn(int b, int n, int m, int k, const float* xyz, const float* new_xyz, const int32_t* offset, const int32_t* new_offset,
                   float* dist2, int32_t* idx, void* stream);
int u3d_offset_ballquery(int b, int n, int m, float radius, int nsample, const float* xyz, const float* new_xyz, const int32_t* offset,
                         const int32_t* new_offset, int32_t* idx, void* stream);
int u3d_offset_group_forward(int m, int nsample, int c, int n, const float* input, const int32_t* idx, float* out, void* stream);
int u3d_offset_group_backward(int m, int nsample, int c, int n, const float* grad_out, const int32_t* idx, float* grad_in, void* stream);
int u3d_offset_interpolate_forward(int n_out, int c, int k, int m_in, const float* input, const int32_t* idx, const float* weight,
                                   float* out, void* stream);
int u3d_offset_interpolate_backward(int n_out, int c, int k, int m_in, const float* grad_out, const int32_t* idx, const float* weight,
                                    float* grad_input, void* stream);
int u3d_offset_subtract_forward(int n, int nsample, int c, const float* in1, const float* in2, const int32_t* idx, float* out,
                                void* stream);
int u3d_offset_subtract_backward(int n, int nsample, int c, const int32_t* idx, const float* grad_out, float* grad_in1, float* grad_in2,
                                 void* stream);
int u3d_offset_aggregate_forward(int n, int nsample, int c, int w_c, const float* input, const float* position, const float* weight,
                                 const int32_t* idx, float* out, void* stream);
int u3d_offset_aggregate_backward(int n, int nsample, int c, int w_c, const float* input, const float* position, const float* weight,
                                  const int32_t* idx, const float* grad_out, float* grad_input, float* grad_position, float* grad_weight,
                                  void* stream);

#ifdef __cplusplus
}
#endif
#endif
