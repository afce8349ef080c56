/*
 * unipre3d_metrics.h -- C-ABI of the MI355X (gfx950) evaluation metrics: per-image SSIM, the squared-error sum PSNR is formed from and
 * the "target is all zero" flag, in one pass over two image stacks, and the gradient of the mean SSIM with respect to the first stack.
 *
 * Stands in for utils/loss_utils.py:47-87 (`ssim`, five grouped 121-tap conv2d calls) and eval.py:28-30 / :122 of the reference.
 * fp32 data, contiguous (N, C, H, W), raw DEVICE pointers and a HIP stream; flat indices are 64-bit.  Returns 0 on success, 1 invalid
 * argument, 3 launch failure.
 *
 * SSIM is the reference's: the 11-tap Gaussian window of sigma 1.5 (the fp32 values `gaussian(11, 1.5)` gives, applied separably: a row
 * pass, then a column pass), zero padding of 5 pixels without renormalisation at the borders, the moments E[x], E[y], E[x^2], E[y^2],
 * E[xy], C1 = 0.01^2, C2 = 0.03^2 and the map ((2 mu1 mu2 + C1)(2 s12 + C2)) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)).
 *
 *   u3d_metrics_tiles(c, h, w)
 *        Host arithmetic only: the number of U3D_METRICS_TILE x U3D_METRICS_TILE tiles (one workgroup each) of ONE image,
 *        c * ceil(h / T) * ceil(w / T); 0 where the launches would refuse the shape (a size below 1, or a count beyond 2^31 - 1).
 *   u3d_metrics_forward(n, c, h, w, img1, img2, partial, ssim, sqsum, all_zero, dmaps, stream)
 *        ssim (n): the mean of the SSIM map of image i; sqsum (n): the sum of (img1 - img2)^2 over image i; all_zero (n) int32: 1 where
 *        every element of img2's image i compares equal to 0 (so -0.0 counts as zero and a NaN does not), else 0.
 *        partial: scratch of n * u3d_metrics_tiles(c, h, w) * 3 floats; every tile writes its three partial sums to its own row and a
 *        second kernel adds the rows of an image in one fixed order: no atomics, the same input gives the same bits.
 *        dmaps: NULL, or (3, n, c, h, w) floats that receive the per-pixel derivatives of the map with respect to mu1 (total: through
 *        both variances as well), to sigma1^2 and to sigma12, which u3d_metrics_ssim_backward reads.
 *        Invalid (1): n < 0, a refused shape, n * tiles beyond 2^31 - 1, a NULL mandatory pointer.  n == 0: 0 without a launch.
 *   u3d_metrics_ssim_backward(n, c, h, w, img1, img2, dmaps, weight, dimg1, stream)
 *        dimg1 (n, c, h, w) = d(sum_i weight[i] * ssim[i]) / d img1
 *                           = s_i * (blur(d_mu1) + 2 img1 blur(d_sigma1^2) + img2 blur(d_sigma12)),  s_i = weight[i] / (c h w),
 *        with the same window and the same zero padding.  weight (n) is read on the device.  Arguments are checked as in the forward.
 */
#ifndef UNIPRE3D_METRICS_H
#define UNIPRE3D_METRICS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define U3D_METRICS_TILE 32   /* edge of the square output tile of one workgroup */
#define U3D_METRICS_HALO 5    /* window_size / 2: the tile is staged with this many pixels on every side */

int u3d_metrics_tiles(int c, int h, int w);
int u3d_metrics_forward(int n, int c, int h, int w, const float* img1, const float* img2, float* partial, float* ssim, float* sqsum,
                        int32_t* all_zero, float* dmaps, void* stream);
int u3d_metrics_ssim_backward(int n, int c, int h, int w, const float* img1, const float* img2, const float* dmaps, const float* weight,
                              float* dimg1, void* stream);

#ifdef __cplusplus
}
#endif
#endif
