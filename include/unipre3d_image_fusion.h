/*
 * unipre3d_image_fusion.h -- C-ABI of the pixel-sparse evaluation of UniPre3D's object-level image branch.
 *
 * The reference runs image_conv = Sequential(GroupNorm(G, Cin, eps), Conv2d(Cin, Cout, 1)) over the whole decoder map (B, Cin, H, W)
 * (model/gaussian_predictor.py:139, 210-214) and FeatureFusion then reads one pixel column per point that wins its z-test
 * (fusion/feat_fusion.py:86-131): at most B N columns of B H W.  Here the map is read once, for GroupNorm's statistics, and the
 * normalisation and the 1x1 convolution are evaluated on the gathered rows only; no (B, ., H, W) tensor is made or kept.
 *
 *   statistics  mean[b][g], rstd[b][g] = 1 / sqrt(var + eps) over the Cin / G channels x H W pixels of a group (biased variance), from
 *               the contiguous NCHW fp32 map.  A group is Cin / G * H * W contiguous floats; it is cut into chunks of 8192 floats, one
 *               workgroup each (u3d_imgfus_stats_chunks: a function of the shape only), summed in f64 in a fixed order; a second kernel
 *               adds the chunks in order and writes stats[(b G + g) 2 + {0, 1}] = (float) mean, (float) rstd.
 *   rows        rows (B, N, Cin) and sel (B, N) are what u3d_zbuffer_fusion_forward (unipre3d_fusion.h) returns for the RAW map with
 *               C = Cin: the winners' pixel columns, and the pixel index or -1.
 *   forward     out[r][o] = sum_c W[o][c] (xhat[r][c] gamma[c] + beta[c]) + bias[o],  xhat[r][c] = (rows[r][c] - mean) * rstd, for a
 *               row with sel >= 0; +0.0 for every other row.  One launch; out needs no pre-fill.
 *   backward    the map is frozen.  Over winner rows S[o][c] = sum_r dout[r][o] xhat[r][c], s[o] = sum_r dout[r][o], by a split over
 *               rows (u3d_imgfus_row_splits) whose partials are added in order; then
 *               dbias = s,  dW[o][c] = gamma[c] S[o][c] + beta[c] s[o],  dgamma[c] = sum_o W[o][c] S[o][c],  dbeta[c] = sum_o W[o][c] s[o].
 *               Rows with sel < 0 contribute nothing, whatever dout holds there.
 *
 * Every entry point runs on `stream`, reads nothing back to the host, uses no atomics (bit-reproducible) and can be captured into a
 * graph.  Limits: Cin % G == 0, Cin and Cout <= 8192, B N < 2^31, a group shorter than 2^31 floats.  Every pointer must be 16-byte
 * aligned and non-null; scratch comes from the two size functions.  Returns 0 ok, 1 invalid argument, 2 unsupported shape,
 * 3 launch failure; 1 and 2 are returned before anything is launched.
 */
#ifndef UNIPRE3D_IMAGE_FUSION_H
#define UNIPRE3D_IMAGE_FUSION_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define U3D_IMGFUS_ABI_VERSION 1
int u3d_imgfus_abi_version(void);
/* host only: chunks a group is cut into, row splits of the backward, scratch sizes (0 for a shape the library refuses) */
int u3d_imgfus_stats_chunks(int Cin, int G, int H, int W);
int u3d_imgfus_row_splits(long long rows);
size_t u3d_imgfus_stats_scratch_bytes(int B, int Cin, int G, int H, int W);
size_t u3d_imgfus_backward_scratch_bytes(int B, int N, int Cin, int Cout);

int u3d_imgfus_stats(const float* map, int B, int Cin, int G, int H, int W, float eps, float* stats, void* scratch, void* stream);
int u3d_imgfus_rows_forward(const float* rows, const int32_t* sel, const float* stats, const float* gamma, const float* beta,
                            const float* weight, const float* bias, int B, int N, int Cin, int G, int Cout, float* out, void* stream);
int u3d_imgfus_rows_backward(const float* dout, const float* rows, const int32_t* sel, const float* stats, const float* gamma,
                             const float* beta, const float* weight, int B, int N, int Cin, int G, int Cout, float* dweight,
                             float* dbias, float* dgamma, float* dbeta, void* scratch, void* stream);
#ifdef __cplusplus
}
#endif
#endif
