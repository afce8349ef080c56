/*
 * unipre3d_pointops.h -- C-ABI of the MI355X (gfx950) point sampling / grouping operators.
 *
 * Drop-in for the reference's `pointnet2_batch_cuda` extension (openpoints/cpp/pointnet2_batch/src/pointnet2_api.cpp:10-24),
 * which the transformer / pointmlp backbones and the ShapeNet loader need before anything can feed the render-loss path
 * (openpoints/models/layers/subsample.py:77-107, group.py:76-203; dataset/shapenet.py:368).  Each function takes the
 * reference wrapper's integer arguments in the same order, raw DEVICE pointers instead of at::Tensor, and a HIP stream.
 * fp32 data, int32 indices, contiguous row-major.  Returns 0 on success, 1 invalid argument, 3 launch failure (2: over the grid form's capacity, below).
 *
 *   u3d_furthest_point_sampling  <- furthest_point_sampling_wrapper(b, n, m, points (B,N,3), temp (B,N), idx (B,M))
 *        Start index 0; ties in the arg-max resolve exactly as the reference's block reduction does for its block size
 *        opt_n_threads(n) (cuda_utils.h:10-14), see oracle/pointops_oracle.c.  Up to 8192 points `temp` is unused, kept for
 *        signature parity (may be NULL): minimum distances live in registers.  Above 8192 points it is required (NULL: returns 1)
 *        and every element of it is written: the running minimum distances.
 *   u3d_ball_query               <- ball_query_wrapper(b, n, m, radius, nsample, new_xyz (B,M,3), xyz (B,N,3), idx (B,M,nsample))
 *        First `nsample` support points with d^2 < r^2 in index order, padded with the first hit; rows without any hit
 *        are written as zeros (the reference relies on the caller's zero_()).
 *   u3d_group_points[_grad]      <- group_points[_grad]_wrapper(b, c, n, npoints, nsample, points (B,C,N), idx, out (B,C,npoints,nsample))
 *   u3d_gather_points[_grad]     <- gather_points[_grad]_wrapper(b, c, n, npoints, points (B,C,N), idx (B,npoints), out (B,C,npoints))
 *        The *_grad forms ACCUMULATE into grad_points (B,C,N) with float atomics; zero it first like the reference does.
 *   u3d_three_nn                 <- three_nn_wrapper(b, n, m, unknown (B,N,3), known (B,M,3), dist2 (B,N,3), idx (B,N,3))
 *        (pointnet2_api.cpp:21, interpolate_gpu.cu:16-59) squared distances and indices of the three nearest known points of
 *        every unknown point, ascending; ties keep the lower index (the reference's strict `<` insertions in index order);
 *        with fewer than three known points the unfilled slots hold the reference's initial 1e40 (stored as +inf) and index 0.
 *   u3d_three_interpolate        <- three_interpolate_wrapper(b, c, m, n, points (B,C,M), idx (B,N,3), weight (B,N,3), out (B,C,N))
 *        (:22, interpolate_gpu.cu:84-103) out[b][c][i] = sum_k weight[b][i][k] * points[b][c][idx[b][i][k]].
 *   u3d_three_interpolate_grad   <- three_interpolate_grad_wrapper(b, c, n, m, grad_out (B,C,N), idx, weight, grad_points (B,C,M))
 *        (:23, interpolate_gpu.cu:127-148) ACCUMULATES grad_out * weight into grad_points with float atomics; zero it first
 *        (openpoints/models/layers/upsampling.py:86).
 *   u3d_group_points_grad_rows, u3d_three_interpolate_grad_rows, u3d_group_points_form, u3d_three_interpolate_form
 *        Host-arithmetic queries (below): which kernel a shape launches, for tests that must reach every one of them.
 *
 * Furthest point sampling over a grid of workgroups (csrc/u3d_fps_grid.h; DESIGN.md, "Furthest point sampling over a grid of workgroups"):
 * one cloud is cut into slices of P = u3d_fps_grid_points_per_workgroup() rows, one workgroup per slice, which meet once per selection.
 *   u3d_furthest_point_sampling_grid(b, n, m, points (B,N,3), workspace, idx (B,M), stream)
 *        The same selection as u3d_furthest_point_sampling, bit for bit, in every contraction mode, for clouds of any size.
 *   u3d_offset_furthest_sampling(b, n, m, xyz (n,3), offset (b), new_offset (b), workspace, idx (m), stream)
 *        <- furthestsampling_cuda (openpoints/cpp/pointops/src/sampling/sampling_cuda_kernel.cu; functions/pointops.py:10-29) for a
 *        concatenated batch: segment s = rows [offset[s-1], offset[s]) (0 for s = 0; clamped to [0, n]; end < start is empty) writes
 *        idx[new_offset[s-1] .. new_offset[s]) (clamped to [0, m]) with ABSOLUTE rows.  Its first selection is its first row, running
 *        minima start at 1e10f, d2 = (x2-x1)^2 + (y2-y1)^2 + (z2-z1)^2 in the contraction mode, and equal distances resolve as the
 *        reference's block does for the block size opt_n_threads(n_max) of the LARGEST segment (computed on the device).  A segment
 *        asked for more selections than it has rows simply goes on (all minima 0, the tie order decides).  Departures: a segment asked
 *        for nothing writes nothing; an EMPTY segment asked for selections gets -1; idx beyond new_offset[b-1] is not written.
 * Both take a caller-provided DEVICE workspace of u3d_fps_grid_workspace_bytes(b) bytes, which the library clears on the stream before
 * the launch; its first 32-bit word is a status word: 0 after a sound call, non-zero when a wait inside the kernel gave up (2 s), in
 * which case the unfinished segments' remaining outputs are -1.  The grid is at most 256 workgroups, so the capacity is
 * rows <= (256 - b) * P (rows = b * n for the dense form): beyond it the call returns 2 and launches nothing.  Only one such grid is in
 * flight per device: the library chains the launches with an event (the one state that outlives a call); under stream capture the
 * calls return 1.
 */
#ifndef UNIPRE3D_POINTOPS_H
#define UNIPRE3D_POINTOPS_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/*
 * Floating-point contraction of the reference's three-term sums.  `dx*dx + dy*dy + dz*dz` (sampling_gpu.cu:140, ball_query_gpu.cu:38,
 * interpolate_gpu.cu:40) and `w0*p0 + w1*p1 + w2*p2` (interpolate_gpu.cu:103) are built by nvcc with its default -fmad=true, i.e. as
 * one rounded product and two fused multiply-adds; WHICH product is the rounded one is the compiler's choice, it changes results in
 * the last bit, and furthest point sampling turns a last-bit difference into a different index set (ties between equidistant
 * points).  The reference binary cannot be built here (no nvcc), so the choice is a process-wide mode of this library, each
 * mode bit-exact against oracle/pointops_oracle.c built the same way:
 *   U3D_PO_FMA_LLVM   fma(c, c, fma(a, a, b*b))  -- DEFAULT.  NVVM is LLVM: its DAG combiner folds the multiply of the FIRST operand of an
 *                     fadd into an fma before it looks at the second (visitFADDForFMACombine: "fold (fadd (fmul x, y), z) -> (fma x, y, z)"),
 *                     so ((a*a + b*b) + c*c) becomes fma(c, c, fma(a, a, b*b)) with b*b the lone rounded product.
 *   U3D_PO_FMA_CHAIN  fma(c, c, fma(b, b, a*a))  -- the left-to-right reading rounds 1-3 of this build used (first product rounded).
 *   U3D_PO_NO_FMA     every product rounded, sums left to right: what nvcc emits under -fmad=false.
 * tests/test_pointops_oracle.py reports on which clouds the three differ (random clouds: FPS never; lattices with exact ties: often).
 */
#define U3D_PO_FMA_LLVM 0
#define U3D_PO_FMA_CHAIN 1
#define U3D_PO_NO_FMA 2
int u3d_pointops_set_contraction(int mode); /* 0 ok, 1 unknown mode; applies to the launches that follow */
int u3d_pointops_get_contraction(void);

int u3d_furthest_point_sampling(int b, int n, int m, const float* points, float* temp, int32_t* idx, void* stream);
size_t u3d_fps_grid_workspace_bytes(int b);
int u3d_fps_grid_points_per_workgroup(void); /* P, for callers and tests */
int u3d_furthest_point_sampling_grid(int b, int n, int m, const float* points, void* workspace, int32_t* idx, void* stream);
int u3d_offset_furthest_sampling(int b, int n, int m, const float* xyz, const int32_t* offset, const int32_t* new_offset,
                                 void* workspace, int32_t* idx, void* stream);
int u3d_ball_query(int b, int n, int m, float radius, int nsample, const float* new_xyz, const float* xyz, int32_t* idx,
                   void* stream);
int u3d_group_points(int b, int c, int n, int npoints, int nsample, const float* points, const int32_t* idx, float* out,
                     void* stream);
int u3d_group_points_grad(int b, int c, int n, int npoints, int nsample, const float* grad_out, const int32_t* idx,
                          float* grad_points, void* stream);
int u3d_gather_points(int b, int c, int n, int npoints, const float* points, const int32_t* idx, float* out, void* stream);
int u3d_gather_points_grad(int b, int c, int n, int npoints, const float* grad_out, const int32_t* idx, float* grad_points,
                           void* stream);
int u3d_three_nn(int b, int n, int m, const float* unknown, const float* known, float* dist2, int32_t* idx, void* stream);
int u3d_three_interpolate(int b, int c, int m, int n, const float* points, const int32_t* idx, const float* weight, float* out,
                          void* stream);
int u3d_three_interpolate_grad(int b, int c, int n, int m, const float* grad_out, const int32_t* idx, const float* weight,
                               float* grad_points, void* stream);

/*
 * Which kernel the two scatter-add gradients launch for a shape: the channel rows one workgroup accumulates in LDS (1, 2, 4, 8 or 16),
 * or 0 for the global-atomic kernel (a row of n resp. m floats does not fit).  The launch and the query share one helper;
 * host arithmetic only, no device is touched (tests ask it without a GPU).
 * u3d_gather_points_grad is u3d_group_points_grad with nsample = 1 and selects alike.
 */
int u3d_group_points_grad_rows(int b, int c, int n);
int u3d_three_interpolate_grad_rows(int b, int c, int m);

/*
 * Which FORWARD kernel a call launches, likewise through the helper the launch itself uses; host arithmetic on the shape and on the
 * pointers' values, no device is touched and nothing is dereferenced.
 *   u3d_group_points_form       1: the vector kernel (four outputs per thread: npoints * nsample a multiple of 4, idx and out on 16-byte
 *                               boundaries, at most 65535 chunks of 1024 outputs), 0: the scalar kernel.  u3d_gather_points is
 *                               u3d_group_points with nsample = 1 and selects alike.
 *   u3d_three_interpolate_form  1: the kernel that stages channel rows of the known cloud in LDS (0 < m <= 2048), 0: the global-gather kernel.
 */
int u3d_group_points_form(int npoints, int nsample, const void* idx, const void* out);
int u3d_three_interpolate_form(int c, int m);

#ifdef __cplusplus
}
#endif
#endif
