/*
 * unipre3d_tokenizer.h -- C-ABI of the group tokenizer of the transformer and Mamba3D backbones (the mini-PointNet `Encoder`:
 * Conv1d(3,128) BN ReLU Conv1d(128,256), group max, cat, Conv1d(512,512) BN ReLU Conv1d(512,C), group max), forward and backward, fp32,
 * gfx950.  Everything runs on the caller's stream, reads no device data on the host, uses no float atomics and sums across workgroups
 * in a fixed order: two calls on the same inputs give the same bits and a forward + backward can be captured into a graph.
 *
 * Shapes.  M = B G groups of n points, rows = M n.  x is (B,G,n,3) fp32 read through its four strides (in floats, any non-negative
 * values); everything else is contiguous.  W1 (128,3) b1 g1 be1 (128) | W2 (256,128) b2 (256) | W3 (512,512) = [W3g | W3l] b3 g2 be2
 * (512) | W4 (C,512) b4 (C).  The plain products run on v_mfma_f32_16x16x4_f32 in 64 x 64 tiles.
 *
 * The phases are separated where a global sum (and, across processes, a collective) sits; each `sums` block is f64 with the row count
 * in element 0, so a caller may add other processes' blocks before the next phase.
 *
 *   u3d_tok_moments   sums1[10] = count, sum x (3), sum x x^T (xx xy xz yy yz zz).
 *   u3d_tok_fwd_a     folds BN1 from sums1 (null: eval mode, from the running statistics), updates running_mean / running_var /
 *                     num_batches_tracked (null pointers: no update; momentum < 0: cumulative average) and writes
 *                       fold1[1280]: A (128,3) and d (128) with h1 = relu(A x + d); Ah (128,3) and dh (128) with xhat1 = Ah x + dh;
 *                                    mean1 (128), invstd1 (128)
 *                       f2 (rows,256) = h1 W2^T + b2     g (M,256), arg2 (M,256) int32 = group max of f2 and its lowest row
 *                       y3 (rows,512) = f2 W3l^T + (g W3g^T + b3)[group]
 *                       sums2[1025] = count, column sums of y3, of y3^2 (null in eval mode).
 *   u3d_tok_fwd_b     folds BN2 from sums2 (null: eval) into fold2[2048] = s2, t2, mean2, invstd2 (512 each), updates the running
 *                     statistics as above, out (M,C) = group max of relu(s2 y3 + t2) W4^T + b4, arg4 (M,C) int32.
 *   u3d_tok_bwd_1     dW4 (C,512), db4 (C), dh3m (rows,512) = [h3 > 0] (dF4 W4) with dF4 = dout placed at arg4,
 *                     sums3[1025] = count, column sums of dh3m, of dh3m xhat3.
 *   u3d_tok_bwd_2     dg2 = dgamma2 and dbe2 = dbeta2 from sums3_local; dy3 from sums3 (the reduced block; the same pointer in one
 *                     process; in eval mode the statistics terms drop out); dW3 (512,512), db3, dW2 (256,128), db2,
 *                     df2 (rows,256), dh1m (rows,128), sums1b[257] = count, column sums of dh1m, of dh1m xhat1.
 *   u3d_tok_bwd_3     dg1, dbe1 from sums1b_local; dW1 (128,3), db1 (128) and, where dx is not null, dx (rows,3) contiguous.
 *
 * db1, db2 and db3 are the sums of dy1, df2 and dy3 over this process's rows in closed form, in f64, from the sums alone:
 * dbias = gamma invstd (S1 - N q - w sum(xhat)), with q, w from the reduced backward block and sum(xhat) from the forward's blocks
 * (sums1 / sums2, this process's and the reduced one; null pointers in eval mode), and db2 = db3 (W3g + W3l).  In one process in
 * training mode that is the exact zero it is mathematically: each of the three biases feeds only a BatchNorm.
 *
 * scratch: u3d_tok_scratch_bytes(M, n, C, phase, training) bytes, 16-byte aligned, phase 0 .. 5 in the order above; each call writes
 * exactly that many bytes from its start and carries nothing to the next.  Weight gradients are split over u3d_tok_wgrad_splits(rows)
 * row ranges (a multiple of 32 rows each, the last one ragged) whose partial products are added in order.
 *
 * M >= 1, 1 <= n <= 256, 1 <= C <= 1024, M n < 2^31.  An arg2 / arg4 entry outside [0, n) is never used as an address.  Returns 0 ok,
 * 1 invalid argument (a null or misaligned pointer: 16 bytes, x 4 bytes), 2 unsupported shape, 3 launch failure; the size query
 * returns 0 for a shape the library does not take.
 */
#ifndef UNIPRE3D_TOKENIZER_H
#define UNIPRE3D_TOKENIZER_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define U3D_TOK_ABI_VERSION 1
#define U3D_TOK_MAX_N 256
#define U3D_TOK_MAX_CHANNELS 1024
#define U3D_TOK_FOLD1_FLOATS 1280
#define U3D_TOK_FOLD2_FLOATS 2048
int u3d_tok_abi_version(void);
int u3d_tok_wgrad_splits(long long rows);
size_t u3d_tok_scratch_bytes(long long M, int n, int C, int phase, int training);
int u3d_tok_moments(const float* x, long long s0, long long s1, long long s2, long long s3, int B, int G, int n, double* sums1,
                    void* scratch, void* stream);
int u3d_tok_fwd_a(const float* x, long long s0, long long s1, long long s2, long long s3, int B, int G, int n, const float* W1,
                  const float* b1, const float* g1, const float* be1, const float* W2, const float* b2, const float* W3, const float* b3,
                  const double* sums1, float* run_mean1, float* run_var1, long long* nbt1, float eps, float momentum, float* fold1,
                  float* f2, float* g, int32_t* arg2, float* y3, double* sums2, void* scratch, void* stream);
int u3d_tok_fwd_b(const float* y3, long long M, int n, int C, const float* g2, const float* be2, const float* W4, const float* b4,
                  const double* sums2, float* run_mean2, float* run_var2, long long* nbt2, float eps, float momentum, float* fold2,
                  float* out, int32_t* arg4, void* scratch, void* stream);
int u3d_tok_bwd_1(const float* dout, const float* y3, const int32_t* arg4, const float* fold2, const float* W4, long long M, int n, int C,
                  float* dW4, float* db4, float* dh3m, double* sums3, void* scratch, void* stream);
int u3d_tok_bwd_2(const float* x, long long s0, long long s1, long long s2, long long s3, int B, int G, int n, const float* dh3m,
                  const float* y3, const float* f2, const float* g, const int32_t* arg2, const float* fold1, const float* fold2,
                  const float* g2, const double* sums2_local, const double* sums2, const double* sums3_local, const double* sums3,
                  int training, const float* W2, const float* W3, float* dg2, float* dbe2, float* dW3, float* db3, float* dW2, float* db2,
                  float* df2, float* dh1m, double* sums1b, void* scratch, void* stream);
int u3d_tok_bwd_3(const float* x, long long s0, long long s1, long long s2, long long s3, int B, int G, int n, const float* dh1m,
                  const float* fold1, const float* g1, const double* sums1_local, const double* sums1, const double* sums1b_local,
                  const double* sums1b, int training, const float* W1, float* dg1, float* dbe1, float* dW1, float* db1, float* dx,
                  void* scratch, void* stream);
#ifdef __cplusplus
}
#endif
#endif
