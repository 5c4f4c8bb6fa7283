// N7: the photometric loss of the RGB stage -- 3DGS's (1 - lambda) L1 + lambda (1 - SSIM)
// (utils/loss_utils.py:20, 158-198; arguments/__init__.py:88; utils/image_utils.py:17-19 for PSNR) as one forward and one
// backward kernel.  Written with torch the same loss is five grouped 11 x 11 convolutions and some twenty element-wise passes
// each way; here a workgroup stages a 32 x 16 tile of one plane plus its 5-pixel halo in LDS, filters it separably (rows into
// LDS, columns into registers) and finishes the pixel in registers.  HBM traffic per 1080p x 3 loss: forward 2 images in, 3
// maps out; backward 5 in, 1 out (0.27 GB together): a bandwidth kernel.
//
// Layout: x, y and v_x are addressed through element strides (plane, row, column), so the [H, W, 3] tensor the rasterizer
// writes is read where it lies.
//
// Numerics: inputs, stored maps and results are fp32; the filtered moments, the subtraction E[x^2] - mu^2 (which cancels to
// ~1e-4 of its value in fp32 on low-contrast windows), the map, its derivatives and every sum are formed in double.  The
// window's weight is the exact product of two fp32 taps (the reference rounds that product to fp32: 6e-8 relative per weight).
// A tile costs ~110k double-rate VALU operations per 512 pixels, a third of the time its bytes take.
//
// LDS: lanes of a wave are consecutive COLUMNS of one or two tile rows in every pass (staging, row filter, column filter), so
// a 32-lane group always reads 32 consecutive words (floats) or 32 consecutive doubles: no bank is hit twice whatever the row
// pitch.  The input pitch is still odd (43) so that the staging loop's wrap from one row to the next stays spread.
#include "common.h"
#include "gags_next.h"

namespace {

constexpr int PT_W = 32, PT_H = 16, PT_R = 5, PT_TAPS = 2 * PT_R + 1;
constexpr int PT_IW = PT_W + 2 * PT_R, PT_IH = PT_H + 2 * PT_R;  // 42 x 26 staged pixels
constexpr int PT_PITCH = PT_IW + 1;

struct PhotoTaps {
    float w[PT_TAPS];
};

struct PhotoView {  // a strided [planes, h, w] view
    const float *p;
    int64_t sp, sr, sc;
};

// a (PT_IH x PT_IW) patch of one plane around the tile at (x0, y0), zeros outside the image
__device__ __forceinline__ void stage_patch(float (*dst)[PT_PITCH], const float *__restrict__ src, int64_t sr, int64_t sc, int h,
                                            int w, int x0, int y0)
{
    for (int i = threadIdx.x; i < PT_IH * PT_IW; i += 256) {
        const int r = i / PT_IW, c = i - r * PT_IW;
        const int gy = y0 + r - PT_R, gx = x0 + c - PT_R;
        dst[r][c] = (gy >= 0 && gy < h && gx >= 0 && gx < w) ? src[(int64_t)gy * sr + (int64_t)gx * sc] : 0.f;
    }
}

// block-wide sums of three doubles in a fixed order (lanes by a shuffle tree, then the four waves in order); thread 0 holds them
__device__ __forceinline__ void block_sum3(double &a, double &b, double &c, double (*red)[4])
{
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); c += __shfl_down(c, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; red[2][threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        c = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
    }
}

// grid (tiles_x, tiles_y, planes); thread = column lx of the tile and the row pair (2 lyp, 2 lyp + 1): the two pixels share
// ten of their eleven filtered rows
__global__ __launch_bounds__(256) void photometric_fwd_kernel(int h, int w, PhotoView xv, PhotoView yv, PhotoTaps taps,
                                                              float *__restrict__ dm, int64_t dm_stride,
                                                              float *__restrict__ ssim_map, double *__restrict__ partials)
{
    __shared__ float in[2][PT_IH][PT_PITCH];
    __shared__ double hz[5][PT_IH][PT_W];
    __shared__ double red[3][4];
    const int tid = threadIdx.x, plane = blockIdx.z;
    const int x0 = blockIdx.x * PT_W, y0 = blockIdx.y * PT_H;
    stage_patch(in[0], xv.p + (int64_t)plane * xv.sp, xv.sr, xv.sc, h, w, x0, y0);
    stage_patch(in[1], yv.p + (int64_t)plane * yv.sp, yv.sr, yv.sc, h, w, x0, y0);
    double tw[PT_TAPS];
#pragma unroll
    for (int k = 0; k < PT_TAPS; ++k) tw[k] = (double)taps.w[k];
    __syncthreads();
    // rows: sum_k w_k of x, y, x^2, y^2, xy (the products of two floats are exact in double)
    for (int i = tid; i < PT_IH * PT_W; i += 256) {
        const int r = i / PT_W, c = i - r * PT_W;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
        for (int k = 0; k < PT_TAPS; ++k) {
            const double xd = (double)in[0][r][c + k], yd = (double)in[1][r][c + k];
            const double wx = tw[k] * xd, wy = tw[k] * yd;
            a0 += wx; a1 += wy;
            a2 = fma(wx, xd, a2); a3 = fma(wy, yd, a3); a4 = fma(wx, yd, a4);
        }
        hz[0][r][c] = a0; hz[1][r][c] = a1; hz[2][r][c] = a2; hz[3][r][c] = a3; hz[4][r][c] = a4;
    }
    __syncthreads();
    // columns, for the pixel pair
    const int lx = tid & (PT_W - 1), lyp = tid / PT_W;
    double m[2][5];
#pragma unroll
    for (int q = 0; q < 5; ++q) m[0][q] = m[1][q] = 0.0;
#pragma unroll
    for (int r = 0; r < PT_TAPS + 1; ++r) {
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const double v = hz[q][2 * lyp + r][lx];
            if (r < PT_TAPS) m[0][q] = fma(tw[r], v, m[0][q]);
            if (r > 0) m[1][q] = fma(tw[r - 1], v, m[1][q]);
        }
    }
    const double C1 = (double)0.0001f, C2 = (double)0.0009f;  // 0.01 ** 2, 0.03 ** 2 as floats
    double s_map = 0.0, s_abs = 0.0, s_sq = 0.0;
    const int gx = x0 + lx;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int ly = 2 * lyp + j, gy = y0 + ly;
        if (gx >= w || gy >= h) continue;
        const double mu1 = m[j][0], mu2 = m[j][1];
        const double s1 = m[j][2] - mu1 * mu1, s2 = m[j][3] - mu2 * mu2, s12 = m[j][4] - mu1 * mu2;
        const double A1 = 2.0 * mu1 * mu2 + C1, A2 = 2.0 * s12 + C2;
        const double B1 = mu1 * mu1 + mu2 * mu2 + C1, B2 = s1 + s2 + C2;
        const double i1 = 1.0 / B1, i2 = 1.0 / B2;
        const double val = (A1 * A2) * (i1 * i2);
        const double xd = (double)in[0][ly + PT_R][lx + PT_R], yd = (double)in[1][ly + PT_R][lx + PT_R];
        const double d = xd - yd;  // (exact)
        s_map += val; s_abs += fabs(d); s_sq = fma(d, d, s_sq);
        const int64_t o = ((int64_t)plane * h + gy) * w + gx;
        if (ssim_map) ssim_map[o] = (float)val;
        if (dm) {
            // map as a function of (mu1, sigma1^2, sigma12) with x's other moments fixed, the usual fused-SSIM split; the
            // chain through sigma1^2 = E[x^2] - mu1^2 and sigma12 = E[xy] - mu1 mu2 is folded into the first map
            const double d_s1 = -val * i2, d_s12 = 2.0 * A1 * (i1 * i2);
            const double d_mu1 = 2.0 * mu2 * A2 * (i1 * i2) - 2.0 * mu1 * val * i1 - 2.0 * mu1 * d_s1 - mu2 * d_s12;
            dm[o] = (float)d_mu1; dm[dm_stride + o] = (float)d_s1; dm[2 * dm_stride + o] = (float)d_s12;
        }
    }
    block_sum3(s_map, s_abs, s_sq, red);
    if (tid == 0) {
        double *p = partials + 3 * (((int64_t)plane * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x);
        p[0] = s_map; p[1] = s_abs; p[2] = s_sq;
    }
}

// One workgroup: the partials of every image added in a fixed order (a thread adds a run of consecutive partials, thread 0 adds
// the 256 runs in thread order; images in order), then the results of gags_photometric_fwd's comment.
__global__ __launch_bounds__(256) void photometric_sum_kernel(int n_images, int64_t per_image, double n_elem,
                                                              const double *__restrict__ partials, double bias, double wa, double wb,
                                                              int reduce_all, double *__restrict__ sums, float *__restrict__ out,
                                                              float *__restrict__ k)
{
    __shared__ double run[3][256];
    const int tid = threadIdx.x;
    const int64_t chunk = (per_image + 255) / 256;
    double tot[3] = {0.0, 0.0, 0.0};
    for (int img = 0; img < n_images; ++img) {
        const double *p = partials + 3 * img * per_image;
        double a[3] = {0.0, 0.0, 0.0};
        const int64_t e = (tid + 1) * chunk < per_image ? (tid + 1) * chunk : per_image;
        for (int64_t i = tid * chunk; i < e; ++i) { a[0] += p[3 * i]; a[1] += p[3 * i + 1]; a[2] += p[3 * i + 2]; }
        __syncthreads();
        run[0][tid] = a[0]; run[1][tid] = a[1]; run[2][tid] = a[2];
        __syncthreads();
        if (tid == 0) {
            double s[3] = {0.0, 0.0, 0.0};
            for (int t = 0; t < 256; ++t) { s[0] += run[0][t]; s[1] += run[1][t]; s[2] += run[2][t]; }
#pragma unroll
            for (int q = 0; q < 3; ++q) { sums[3 * img + q] = s[q]; tot[q] += s[q]; }
            if (!reduce_all && out) out[img] = (float)(bias + wa * (s[1] / n_elem) + wb * (s[0] / n_elem));
        }
    }
    if (tid == 0) {
        const double n = reduce_all ? n_elem * (double)n_images : n_elem;
        if (reduce_all && out) out[0] = (float)(bias + wa * (tot[1] / n) + wb * (tot[0] / n));
        if (k) { k[0] = (float)(wa / n); k[1] = (float)(wb / n); }
    }
}

// Same tiling.  The window is symmetric and the padding is zeros, so the adjoint of the filter is the filter: the three maps
// are filtered like the moments were and combined with the pixel's own x and y.
__global__ __launch_bounds__(256) void photometric_bwd_kernel(int h, int w, int planes_per_image, PhotoView xv, PhotoView yv,
                                                              PhotoTaps taps, const float *__restrict__ dm, int64_t dm_stride,
                                                              const float *__restrict__ coef, float *__restrict__ vx, int64_t v_sp,
                                                              int64_t v_sr, int64_t v_sc)
{
    __shared__ float in[3][PT_IH][PT_PITCH];
    __shared__ double hz[3][PT_IH][PT_W];
    const int tid = threadIdx.x, plane = blockIdx.z;
    const int x0 = blockIdx.x * PT_W, y0 = blockIdx.y * PT_H;
#pragma unroll
    for (int q = 0; q < 3; ++q) stage_patch(in[q], dm + q * dm_stride + (int64_t)plane * h * w, w, 1, h, w, x0, y0);
    // the pixel pair's own x and y, requested before the filter so that they arrive under it
    const int lx = tid & (PT_W - 1), lyp = tid / PT_W, gx = x0 + lx;
    float xs[2] = {0.f, 0.f}, ys[2] = {0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int gy = y0 + 2 * lyp + j;
        if (gx < w && gy < h) {
            xs[j] = xv.p[(int64_t)plane * xv.sp + (int64_t)gy * xv.sr + (int64_t)gx * xv.sc];
            ys[j] = yv.p[(int64_t)plane * yv.sp + (int64_t)gy * yv.sr + (int64_t)gx * yv.sc];
        }
    }
    const float *cf = coef + 2 * (plane / planes_per_image);
    const double a = (double)cf[0], b = (double)cf[1];
    double tw[PT_TAPS];
#pragma unroll
    for (int k = 0; k < PT_TAPS; ++k) tw[k] = (double)taps.w[k];
    __syncthreads();
    for (int i = tid; i < PT_IH * PT_W; i += 256) {
        const int r = i / PT_W, c = i - r * PT_W;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
        for (int k = 0; k < PT_TAPS; ++k) {
            a0 = fma(tw[k], (double)in[0][r][c + k], a0);
            a1 = fma(tw[k], (double)in[1][r][c + k], a1);
            a2 = fma(tw[k], (double)in[2][r][c + k], a2);
        }
        hz[0][r][c] = a0; hz[1][r][c] = a1; hz[2][r][c] = a2;
    }
    __syncthreads();
    double f[2][3];
#pragma unroll
    for (int q = 0; q < 3; ++q) f[0][q] = f[1][q] = 0.0;
#pragma unroll
    for (int r = 0; r < PT_TAPS + 1; ++r) {
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            const double v = hz[q][2 * lyp + r][lx];
            if (r < PT_TAPS) f[0][q] = fma(tw[r], v, f[0][q]);
            if (r > 0) f[1][q] = fma(tw[r - 1], v, f[1][q]);
        }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int gy = y0 + 2 * lyp + j;
        if (gx >= w || gy >= h) continue;
        const double xd = (double)xs[j], yd = (double)ys[j];
        const double sgn = xs[j] > ys[j] ? 1.0 : (xs[j] < ys[j] ? -1.0 : 0.0);  // torch.sign: sign(0) = 0
        const double g = a * sgn + b * (f[j][0] + 2.0 * xd * f[j][1] + yd * f[j][2]);
        vx[(int64_t)plane * v_sp + (int64_t)gy * v_sr + (int64_t)gx * v_sc] = (float)g;
    }
}

inline bool photo_shape_ok(int planes, int h, int w)
{
    if (planes <= 0 || h <= 0 || w <= 0 || planes > 65535) return false;
    if ((h + PT_H - 1) / PT_H > 65535) return false;             // grid.y
    return (int64_t)planes * h * w < ((int64_t)1 << 40);         // (offsets are 64-bit; this only keeps 3 planes h w sane)
}

inline bool photo_view_ok(const float *p, int64_t sp, int64_t sr, int64_t sc) { return p && sp >= 0 && sr >= 0 && sc >= 0; }

}  // namespace

extern "C" int64_t gags_photometric_partials(int planes, int h, int w)
{
    if (!photo_shape_ok(planes, h, w)) return 0;
    return (int64_t)planes * ((h + PT_H - 1) / PT_H) * ((w + PT_W - 1) / PT_W);
}

extern "C" int gags_photometric_fwd(int planes, int n_images, int h, int w, const float *x, int64_t x_sp, int64_t x_sr,
                                    int64_t x_sc, const float *y, int64_t y_sp, int64_t y_sr, int64_t y_sc, const float *window,
                                    double bias, double wa, double wb, int reduce_all, float *dm, float *ssim_map, double *partials,
                                    double *sums, float *out, float *k, void *stream)
{
    GAGS_CLEAR_ERR();
    if (!photo_shape_ok(planes, h, w) || n_images <= 0 || planes % n_images != 0) return GAGS_EINVAL;
    if (!photo_view_ok(x, x_sp, x_sr, x_sc) || !photo_view_ok(y, y_sp, y_sr, y_sc) || !window || !partials || !sums)
        return GAGS_EINVAL;
    PhotoTaps taps;
    for (int i = 0; i < PT_TAPS; ++i) taps.w[i] = window[i];
    const dim3 grid((w + PT_W - 1) / PT_W, (h + PT_H - 1) / PT_H, planes);
    hipLaunchKernelGGL(photometric_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, h, w, PhotoView{x, x_sp, x_sr, x_sc},
                       PhotoView{y, y_sp, y_sr, y_sc}, taps, dm, (int64_t)planes * h * w, ssim_map, partials);
    GAGS_CHECK_LAUNCH();
    const int ppi = planes / n_images;
    hipLaunchKernelGGL(photometric_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n_images,
                       (int64_t)ppi * grid.x * grid.y, (double)ppi * (double)h * (double)w, (const double *)partials, bias, wa, wb,
                       reduce_all, sums, out, k);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_photometric_bwd(int planes, int n_images, int h, int w, const float *x, int64_t x_sp, int64_t x_sr,
                                    int64_t x_sc, const float *y, int64_t y_sp, int64_t y_sr, int64_t y_sc, const float *window,
                                    const float *dm, const float *coef, float *v_x, int64_t v_sp, int64_t v_sr, int64_t v_sc,
                                    void *stream)
{
    GAGS_CLEAR_ERR();
    if (!photo_shape_ok(planes, h, w) || n_images <= 0 || planes % n_images != 0) return GAGS_EINVAL;
    if (!photo_view_ok(x, x_sp, x_sr, x_sc) || !photo_view_ok(y, y_sp, y_sr, y_sc) || !window || !dm || !coef) return GAGS_EINVAL;
    if (!v_x || v_sp < 0 || v_sr < 0 || v_sc < 0) return GAGS_EINVAL;
    PhotoTaps taps;
    for (int i = 0; i < PT_TAPS; ++i) taps.w[i] = window[i];
    const dim3 grid((w + PT_W - 1) / PT_W, (h + PT_H - 1) / PT_H, planes);
    hipLaunchKernelGGL(photometric_bwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, h, w, planes / n_images,
                       PhotoView{x, x_sp, x_sr, x_sc}, PhotoView{y, y_sp, y_sr, y_sc}, taps, dm, (int64_t)planes * h * w, coef, v_x,
                       v_sp, v_sr, v_sc);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
