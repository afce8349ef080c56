// Evaluation metrics for gfx950 (include/unipre3d_metrics.h): per-image mean SSIM, squared-error sum and the all-zero-target flag in one
// pass over both image stacks, and the gradient of the mean SSIM with respect to the first stack; semantics restated on the CPU in
// tests/metrics_ref.py.
//
// The reference convolves five image-sized products with a 121-tap window, one grouped conv2d each.  Here a workgroup of four waves
// owns one T x T tile of one channel plane: it stages the (T + 10)^2 window of both images in LDS once (zeros outside the image: the
// reference's zero padding), runs the 11-tap row pass into five moment planes in LDS and the 11-tap column pass out of them, and keeps
// the SSIM map in registers.  In both passes a thread owns FOUR adjacent outputs and walks their 14 shared inputs once, so an input
// is read from LDS once per four outputs instead of once per tap.  Pitches are odd (T + 11, T + 1): the row pass runs down a column
// of the tile (lane = row), the column pass along a row (lane = column), and both are conflict-free.
//
// Reduction: every tile writes (sum of the map, sum of squared differences, non-zero target pixels) to its own scratch row; a second
// kernel adds an image's rows in one fixed order.  No atomics anywhere.
//
// Backward: the forward (only when asked) stores the per-pixel derivatives of the map with respect to mu1, sigma1^2 and sigma12; the
// backward kernel blurs those three maps with the same tile machinery and combines them with the two images.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "unipre3d_metrics.h"
#include "u3d_util.h"

namespace {

using namespace u3d_util;

constexpr int T = U3D_METRICS_TILE;
constexpr int R = U3D_METRICS_HALO;
constexpr int E = T + 2 * R;       // edge of the staged window
constexpr int PIN = E + 1;         // its pitch in LDS (odd)
constexpr int PM = T + 1;          // pitch of a row-passed plane (E rows of T columns)
constexpr int NT = 256;
constexpr int SPAN = 4 + 2 * R;    // inputs under four adjacent outputs
static_assert(T % 4 == 0 && NT == (T / 4) * T, "one thread per column and group of four rows in the column pass");

// gaussian(11, 1.5) of utils/loss_utils.py, as fp32 (recorded in tests/golden/g18_metrics.npz)
#define U3D_METRICS_WINDOW                                                                                                             \
  {0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c3ep-3f, 0x1.10656p-2f,                                     \
   0x1.b43c3ep-3f,  0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f}

struct TileAt {
  int y0, x0;
  size_t plane;   // n * C + c
};

__device__ __forceinline__ TileAt tile_at(int tiles_x, int tiles_y) {
  unsigned b = blockIdx.x;
  const unsigned tx = b % (unsigned)tiles_x;
  b /= (unsigned)tiles_x;
  const unsigned ty = b % (unsigned)tiles_y;
  return {(int)ty * T, (int)tx * T, (size_t)(b / (unsigned)tiles_y)};
}

// the E x E windows of M planes around the tile into s (M windows of E * PIN words), zeros outside the image.  Every load of the
// thread is issued before the first LDS write, so one round trip to memory covers the whole window instead of one per pass.
template <int M>
__device__ __forceinline__ void stage(const float* const (&plane)[M], int H, int W, int y0, int x0, float* s) {
  constexpr int NS = (E * E + NT - 1) / NT;
  float v[NS][M];
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int e = threadIdx.x + i * NT;
    const int r = e / E, c = e - r * E;
    const int y = y0 - R + r, x = x0 - R + c;
    const bool in = e < E * E && y >= 0 && y < H && x >= 0 && x < W;
#pragma unroll
    for (int m = 0; m < M; ++m) v[i][m] = in ? plane[m][(size_t)y * W + x] : 0.f;
  }
#pragma unroll
  for (int i = 0; i < NS; ++i) {
    const int e = threadIdx.x + i * NT;
    const int r = e / E, c = e - r * E;
    if (e < E * E) {
#pragma unroll
      for (int m = 0; m < M; ++m) s[m * (E * PIN) + r * PIN + c] = v[i][m];
    }
  }
}

// row pass: M planes of E rows x T columns (pitch PM) from the staged windows; src(offset into a staged window, v[M])
template <int M, class Src>
__device__ __forceinline__ void row_pass(Src src, float* s_m) {
  constexpr float G[11] = U3D_METRICS_WINDOW;
  for (int it = threadIdx.x; it < E * (T / 4); it += NT) {
    const int cg = it / E, r = it - cg * E;            // consecutive lanes: consecutive rows
    float acc[M][4];
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int o = 0; o < 4; ++o) acc[m][o] = 0.f;
#pragma unroll
    for (int j = 0; j < SPAN; ++j) {
      float v[M];
      src(r * PIN + cg * 4 + j, v);
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int k = j - o;
        if (k >= 0 && k < 11) {
#pragma unroll
          for (int m = 0; m < M; ++m) acc[m][o] += G[k] * v[m];
        }
      }
    }
#pragma unroll
    for (int m = 0; m < M; ++m)
#pragma unroll
      for (int o = 0; o < 4; ++o) s_m[m * (E * PM) + r * PM + cg * 4 + o] = acc[m][o];
  }
}

// column pass: this thread's column c and rows r0 .. r0 + 3 of the tile
template <int M>
__device__ __forceinline__ void col_pass(const float* s_m, int r0, int c, float (&acc)[M][4]) {
  constexpr float G[11] = U3D_METRICS_WINDOW;
#pragma unroll
  for (int m = 0; m < M; ++m)
#pragma unroll
    for (int o = 0; o < 4; ++o) acc[m][o] = 0.f;
#pragma unroll
  for (int j = 0; j < SPAN; ++j) {
    float v[M];
#pragma unroll
    for (int m = 0; m < M; ++m) v[m] = s_m[m * (E * PM) + (r0 + j) * PM + c];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int k = j - o;
      if (k >= 0 && k < 11) {
#pragma unroll
        for (int m = 0; m < M; ++m) acc[m][o] += G[k] * v[m];
      }
    }
  }
}

template <bool SAVE>
__global__ __launch_bounds__(NT) void metrics_tile_kernel(int H, int W, int tiles_x, int tiles_y, size_t total, const float* __restrict__ img1,
                                                          const float* __restrict__ img2, float* __restrict__ partial,
                                                          float* __restrict__ dmaps) {
  __shared__ float s_in[2 * E * PIN], s_m[5 * E * PM], s_red[4 * 3];
  const float *s_a = s_in, *s_b = s_in + E * PIN;
  const TileAt t = tile_at(tiles_x, tiles_y);
  const size_t base = t.plane * (size_t)H * (size_t)W;
  const float* const planes[2] = {img1 + base, img2 + base};
  stage<2>(planes, H, W, t.y0, t.x0, s_in);
  __syncthreads();
  row_pass<5>([&](int o, float (&v)[5]) {
    const float a = s_a[o], b = s_b[o];
    v[0] = a, v[1] = b, v[2] = a * a, v[3] = b * b, v[4] = a * b;
  }, s_m);
  __syncthreads();
  const int c = threadIdx.x & (T - 1), r0 = (threadIdx.x / T) * 4;
  float mo[5][4];
  col_pass<5>(s_m, r0, c, mo);
  const float C1 = (float)(0.01 * 0.01), C2 = (float)(0.03 * 0.03);
  float sum_map = 0.f, sum_sq = 0.f, nonzero = 0.f;
  const int x = t.x0 + c;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int y = t.y0 + r0 + o;
    if (y < H && x < W) {
      const float a = s_a[(r0 + o + R) * PIN + c + R], b = s_b[(r0 + o + R) * PIN + c + R];
      const float d = a - b;
      sum_sq += d * d;
      nonzero += (b == 0.f) ? 0.f : 1.f;          // -0.0 == 0; a NaN is not zero
      const float mu1 = mo[0][o], mu2 = mo[1][o];
      const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
      const float s1 = mo[2][o] - mu1_sq, s2 = mo[3][o] - mu2_sq, s12 = mo[4][o] - mu12;
      const float A1 = 2.f * mu12 + C1, A2 = 2.f * s12 + C2, B1 = mu1_sq + mu2_sq + C1, B2 = s1 + s2 + C2;
      const float S = (A1 * A2) / (B1 * B2);
      sum_map += S;
      if (SAVE) {
        const float inv = 1.f / (B1 * B2);
        const float d_s1 = -S / B2, d_s12 = 2.f * A1 * inv;
        const float d_mu1 = 2.f * mu2 * A2 * inv - 2.f * mu1 * S / B1 - 2.f * mu1 * d_s1 - mu2 * d_s12;
        const size_t p = base + (size_t)y * W + x;
        dmaps[p] = d_mu1, dmaps[total + p] = d_s1, dmaps[2 * total + p] = d_s12;
      }
    }
  }
  sum_map = wave_sum(sum_map), sum_sq = wave_sum(sum_sq), nonzero = wave_sum(nonzero);
  if (lane_id() == 0) {
    float* q = s_red + (threadIdx.x >> 6) * 3;
    q[0] = sum_map, q[1] = sum_sq, q[2] = nonzero;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int k = threadIdx.x;
    partial[(size_t)blockIdx.x * 3 + k] = ((s_red[k] + s_red[3 + k]) + s_red[6 + k]) + s_red[9 + k];
  }
}

// one workgroup per image: its tiles' rows in thread-strided order, then the lanes, then the waves
__global__ __launch_bounds__(NT) void metrics_reduce_kernel(int tiles, float count, const float* __restrict__ partial, float* __restrict__ ssim,
                                                            float* __restrict__ sqsum, int32_t* __restrict__ all_zero) {
  __shared__ float s_red[4 * 3];
  const float* p = partial + (size_t)blockIdx.x * tiles * 3;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f;
  for (int t = threadIdx.x; t < tiles; t += NT) s0 += p[(size_t)t * 3], s1 += p[(size_t)t * 3 + 1], s2 += p[(size_t)t * 3 + 2];
  s0 = wave_sum(s0), s1 = wave_sum(s1), s2 = wave_sum(s2);
  if (lane_id() == 0) {
    float* q = s_red + (threadIdx.x >> 6) * 3;
    q[0] = s0, q[1] = s1, q[2] = s2;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    ssim[blockIdx.x] = (((s_red[0] + s_red[3]) + s_red[6]) + s_red[9]) / count;
    sqsum[blockIdx.x] = ((s_red[1] + s_red[4]) + s_red[7]) + s_red[10];
    const float nz = ((s_red[2] + s_red[5]) + s_red[8]) + s_red[11];
    all_zero[blockIdx.x] = (nz == 0.f) ? 1 : 0;    // a count: never NaN, never negative
  }
}

__global__ __launch_bounds__(NT) void ssim_backward_kernel(int C, int H, int W, int tiles_x, int tiles_y, size_t total, const float* __restrict__ img1,
                                                           const float* __restrict__ img2, const float* __restrict__ dmaps,
                                                           const float* __restrict__ weight, float* __restrict__ dimg1) {
  __shared__ float s_d[3 * E * PIN], s_m[3 * E * PM];
  const TileAt t = tile_at(tiles_x, tiles_y);
  const size_t base = t.plane * (size_t)H * (size_t)W;
  const float* const planes[3] = {dmaps + base, dmaps + total + base, dmaps + 2 * total + base};
  stage<3>(planes, H, W, t.y0, t.x0, s_d);
  __syncthreads();
  row_pass<3>([&](int o, float (&v)[3]) { v[0] = s_d[o], v[1] = s_d[E * PIN + o], v[2] = s_d[2 * E * PIN + o]; }, s_m);
  __syncthreads();
  const int c = threadIdx.x & (T - 1), r0 = (threadIdx.x / T) * 4;
  float g[3][4];
  col_pass<3>(s_m, r0, c, g);
  const float scale = weight[t.plane / (size_t)C] / ((float)C * (float)H * (float)W);
  const int x = t.x0 + c;
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const int y = t.y0 + r0 + o;
    if (y < H && x < W) {
      const size_t p = base + (size_t)y * W + x;
      dimg1[p] = scale * (g[0][o] + 2.f * img1[p] * g[1][o] + img2[p] * g[2][o]);
    }
  }
}

// 0: the launches refuse the shape; else the tiles of one image
inline long long image_tiles(int c, int h, int w) {
  if (c < 1 || h < 1 || w < 1) return 0;
  const long long per_plane = (((long long)h + T - 1) / T) * (((long long)w + T - 1) / T);
  if (per_plane > 2147483647ll) return 0;
  const long long t = per_plane * c;
  return t > 2147483647ll ? 0 : t;
}

}  // namespace

extern "C" {

int u3d_metrics_tiles(int c, int h, int w) { return (int)image_tiles(c, h, w); }

int u3d_metrics_forward(int n, int c, int h, int w, const float* img1, const float* img2, float* partial, float* ssim, float* sqsum,
                        int32_t* all_zero, float* dmaps, void* stream) {
  const long long tiles = image_tiles(c, h, w);
  if (n < 0 || tiles == 0 || tiles * n > 2147483647ll) return 1;
  if (n == 0) return 0;
  if (!img1 || !img2 || !partial || !ssim || !sqsum || !all_zero) return 1;
  const int tiles_x = (w + T - 1) / T, tiles_y = (h + T - 1) / T;
  const size_t total = (size_t)n * c * h * w;
  const dim3 grid((unsigned)(tiles * n));
  if (dmaps)
    hipLaunchKernelGGL(metrics_tile_kernel<true>, grid, dim3(NT), 0, (hipStream_t)stream, h, w, tiles_x, tiles_y, total, img1, img2, partial, dmaps);
  else
    hipLaunchKernelGGL(metrics_tile_kernel<false>, grid, dim3(NT), 0, (hipStream_t)stream, h, w, tiles_x, tiles_y, total, img1, img2, partial, dmaps);
  if (launched() != 0) return 3;
  hipLaunchKernelGGL(metrics_reduce_kernel, dim3((unsigned)n), dim3(NT), 0, (hipStream_t)stream, (int)tiles, (float)((double)c * h * w), partial,
                     ssim, sqsum, all_zero);
  return launched();
}

int u3d_metrics_ssim_backward(int n, int c, int h, int w, const float* img1, const float* img2, const float* dmaps, const float* weight,
                              float* dimg1, void* stream) {
  const long long tiles = image_tiles(c, h, w);
  if (n < 0 || tiles == 0 || tiles * n > 2147483647ll) return 1;
  if (n == 0) return 0;
  if (!img1 || !img2 || !dmaps || !weight || !dimg1) return 1;
  const int tiles_x = (w + T - 1) / T, tiles_y = (h + T - 1) / T;
  hipLaunchKernelGGL(ssim_backward_kernel, dim3((unsigned)(tiles * n)), dim3(NT), 0, (hipStream_t)stream, c, h, w, tiles_x, tiles_y,
                     (size_t)n * c * h * w, img1, img2, dmaps, weight, dimg1);
  return launched();
}

}  // extern "C"
