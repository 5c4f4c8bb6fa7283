// The box mean cv2.filter2D computes with a ones / box^2 kernel (anchor box / 2, BORDER_REFLECT_101), shared by activate.hip (N4:
// the mean of the relevancy map) and queryvis.hip (N12: the mean of the normalised map).  Two passes over [n, h, w] maps: row
// sums in double to scratch, then the column window; the sum is rounded ONCE, by box_col_mean.
#pragma once
#include "common.h"

namespace {

// cv2.BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba), the default border of cv2.filter2D
__device__ __forceinline__ int reflect101(int i, int n)
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
    return i;
}

// horizontal pass: rowsum[k, y, x] = sum_{dx = -a .. box-1-a} src[k, y, reflect(x + dx)],  a = box / 2 (cv2's anchor).
// Sums in double, rounded once at the end of the vertical pass: the reflected border makes neighbouring windows hold the
// same multiset of pixels, and lerf_localization takes EVERY position that attains the maximum (:174-176) -- fp32 partial
// sums in window order would break such exact ties.
// grid (ceil(w / 256), h, n), 256 threads, (256 + box) floats of dynamic LDS
__global__ __launch_bounds__(256) void box_rows_kernel(int h, int w, int box, const float *__restrict__ src,
                                                       double *__restrict__ rowsum)
{
    extern __shared__ float seg[];  // 256 + box values of the row
    const int y = blockIdx.y, k = blockIdx.z, x0 = blockIdx.x * 256, a = box / 2;
    const float *row = src + ((size_t)k * h + y) * w;
    for (int i = threadIdx.x; i < 256 + box; i += 256) seg[i] = row[reflect101(x0 + i - a, w)];
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    double s = 0.0;
    for (int i = 0; i < box; ++i) s += (double)seg[threadIdx.x + i];
    rowsum[((size_t)k * h + y) * w + x] = s;
}

// vertical pass of pixel (x, y) of map k: (sum over the column window of the row sums) / box^2, rounded to float once
__device__ __forceinline__ float box_col_mean(int h, int w, int box, const double *__restrict__ rowsum, int k, int y, int x)
{
    const double *col = rowsum + (size_t)k * h * w + x;
    const int a = box / 2;
    double s = 0.0;
    for (int i = 0; i < box; ++i) s += col[(size_t)reflect101(y + i - a, h) * w];
    return (float)(s / (double)(box * box));
}

}  // namespace
