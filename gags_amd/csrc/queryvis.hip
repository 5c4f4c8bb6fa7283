// N12 (include/gags_next.h): the images compute_relvancy.py --image_mode writes per phrase and view (activate_stream :100-144; the
// same images at evaluate_iou_loc.py:108-163, 216-221) and the three maps of --loss_mode (:439-447), without leaving the device.
//
// (a) query images.  The reference runs cv2.filter2D over `output` on the HOST, about fifteen full-image torch passes, three
//     boolean-mask scatters and a LUT gather per phrase.  Here: the box mean of `output` (box_mean.h, the passes activate.hip
//     runs over the relevancy map) and ONE colour kernel -- a thread per pixel, the 256 x 3 LUT staged once per workgroup in LDS,
//     grid (pixel blocks, M) so that one launch serves every phrase of every frame.  Each thread reads heat, output, mask, avg2
//     and its image pixel and writes the three RGB triples (and their uint8 copies when asked).  No atomics, no reduction: the
//     lerf composite's max comes from the stats gags_relevancy_activate already holds.
// (b) loss maps.  Two [C, HW] or [HW, C] maps are reduced over C to three [HW] maps.  A workgroup owns 64 pixels and walks the
//     channels 64 at a time: both tiles are fetched along their own fast axis (256-byte runs either way, every element read
//     once) into LDS as [channel][pixel], four waves each sum a quarter of the tile's channels in double, and the four partial
//     sums meet once at the end.  The order of the sums depends on (pixel, channel) only: both layouts give the same bits.
#include "box_mean.h"
#include "common.h"
#include "gags_next.h"
#include "launch.h"

namespace {

constexpr int LUT_N = 256;

// torch.clip(v, 0, 1): a NaN stays a NaN
__device__ __forceinline__ float clip01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }

// eval/colormaps.py:105-113: nan_to_num, (t * 255).long(); the reference asserts 0..255, here the index is clamped
__device__ __forceinline__ int lut_index(float t)
{
    if (t != t) t = 0.f;
    const float s = fminf(fmaxf(t * 255.0f, 0.f), 255.f);
    return (int)s;
}

// this project's uint8 rule (featurevis._save_image): trunc(clamp(x * 255 + 0.5, 0, 255))
__device__ __forceinline__ unsigned char to_u8(float x)
{
    float v = x * 255.0f;
    v = v + 0.5f;
    v = fminf(fmaxf(v, 0.f), 255.f);  // (a NaN becomes 0)
    return (unsigned char)(int)v;
}

__device__ __forceinline__ void put3(float *__restrict__ rgb, unsigned char *__restrict__ u8, size_t o, float r, float g, float b)
{
    rgb[o] = r; rgb[o + 1] = g; rgb[o + 2] = b;
    if (u8) { u8[o] = to_u8(r); u8[o + 1] = to_u8(g); u8[o + 2] = to_u8(b); }
}

__global__ __launch_bounds__(256) void box_cols_mean_kernel(int h, int w, int box, const double *__restrict__ rowsum,
                                                            float *__restrict__ avg)
{
    const int k = blockIdx.z, y = blockIdx.y, x = blockIdx.x * 256 + threadIdx.x;
    if (x < w) avg[((size_t)k * h + y) * w + x] = box_col_mean(h, w, box, rowsum, k, y, x);
}

// grid (ceil(hw / 256), M); map m uses image m / per_frame
__global__ __launch_bounds__(256) void query_colour_kernel(int64_t hw, int per_frame, const float *__restrict__ heat,
                                                           const float *__restrict__ output, const unsigned char *__restrict__ mask,
                                                           const float *__restrict__ avg2, const float *__restrict__ stats,
                                                           const float *__restrict__ image, const float *__restrict__ lut,
                                                           float *__restrict__ heat_rgb, float *__restrict__ lerf_rgb,
                                                           float *__restrict__ mask_rgb, unsigned char *__restrict__ heat_u8,
                                                           unsigned char *__restrict__ lerf_u8, unsigned char *__restrict__ mask_u8)
{
    __shared__ float L[LUT_N * 3];
    for (int i = threadIdx.x; i < LUT_N * 3; i += 256) L[i] = lut[i];
    __syncthreads();
    const int m = blockIdx.y;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= hw) return;
    const size_t o = (size_t)m * hw + p;
    const float *px = image + ((size_t)(m / per_frame) * hw + p) * 3;
    const float ir = px[0], ig = px[1], ib = px[2];
    const float ht = heat[o], ou = output[o], a2 = avg2[o];
    // heat map: colour(output)
    const float *c0 = L + 3 * lut_index(ou);
    put3(heat_rgb, heat_u8, 3 * o, c0[0], c0[1], c0[2]);
    // lerf composite: colour(clip(p / (max p + 1e-6))) where heat >= 0.5, the dimmed image elsewhere; max p = clip(max heat - 0.5)
    const float pp = clip01(ht - 0.5f);
    const float pmax = clip01(stats[3 * m + 1] - 0.5f);
    const float q = clip01(pp / (pmax + 1e-6f));
    const float *c1 = L + 3 * lut_index(q);
    if (ht < 0.5f)
        put3(lerf_rgb, lerf_u8, 3 * o, ir * 0.3f, ig * 0.3f, ib * 0.3f);
    else
        put3(lerf_rgb, lerf_u8, 3 * o, c1[0], c1[1], c1[2]);
    // mask composite: colour(clip(0.5 output + 0.5 avg2)) inside the mask, 0.4 image + 0.1 outside
    const float b = clip01(0.5f * ou + 0.5f * a2);
    const float *c2 = L + 3 * lut_index(b);
    if (mask[o])
        put3(mask_rgb, mask_u8, 3 * o, c2[0], c2[1], c2[2]);
    else
        put3(mask_rgb, mask_u8, 3 * o, ir * 0.4f + 0.1f, ig * 0.4f + 0.1f, ib * 0.4f + 0.1f);
}

// ---- loss maps ---------------------------------------------------------------------------------------------------------
constexpr int LP = 64;       // pixels per workgroup
constexpr int LC = 64;       // channels per step
constexpr int LPITCH = 65;   // LDS pitch of a channel row (floats): the pixel-major fetch stores a column per wave
constexpr int LQ = LC / 4;   // channels per wave and step

// this thread's 16 elements of the tile (pixels p0.., channels c0..) of a map; past the map: 0
template <int LAYOUT>
__device__ __forceinline__ void tile_fetch(const float *__restrict__ x, int c, int64_t n_pix, int64_t p0, int c0, float (&r)[16])
{
    const int fast = threadIdx.x & 63, slow = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int ch = c0 + (LAYOUT == 1 ? fast : slow + 4 * k);
        const int64_t p = p0 + (LAYOUT == 1 ? slow + 4 * k : fast);
        r[k] = (ch < c && p < n_pix) ? (LAYOUT == 1 ? x[p * c + ch] : x[(int64_t)ch * n_pix + p]) : 0.f;
    }
}

template <int LAYOUT>
__device__ __forceinline__ void tile_store(float *__restrict__ t, const float (&r)[16])
{
    const int fast = threadIdx.x & 63, slow = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int chl = LAYOUT == 1 ? fast : slow + 4 * k, pl = LAYOUT == 1 ? slow + 4 * k : fast;
        t[chl * LPITCH + pl] = r[k];
    }
}

template <int LF, int LG>
__global__ __launch_bounds__(256) void loss_maps_kernel(int c, int64_t n_pix, const float *__restrict__ f,
                                                        const float *__restrict__ gt, const float *__restrict__ mask,
                                                        float *__restrict__ l2, float *__restrict__ mean_abs_f,
                                                        float *__restrict__ mean_abs_gt)
{
    __shared__ __attribute__((aligned(16))) float A[LC * LPITCH];  // gt tile; at the end the partial sums [3 waves][3][LP] double
    __shared__ float B[LC * LPITCH];                               // f tile
    static_assert(sizeof(float) * LC * LPITCH >= sizeof(double) * 9 * LP, "the partial sums fit the tile");
    const int pix = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * LP, p = p0 + pix;
    const float m = p < n_pix ? mask[p] : 0.f;
    double s2 = 0.0, sf = 0.0, sg = 0.0;
    float ra[16], rb[16];
    tile_fetch<LG>(gt, c, n_pix, p0, 0, ra);
    tile_fetch<LF>(f, c, n_pix, p0, 0, rb);
    for (int c0 = 0; c0 < c; c0 += LC) {
        __syncthreads();  // (the previous step's sums have read the tiles)
        tile_store<LG>(A, ra);
        tile_store<LF>(B, rb);
        __syncthreads();
        if (c0 + LC < c) {  // the next step's elements travel while this step is summed
            tile_fetch<LG>(gt, c, n_pix, p0, c0 + LC, ra);
            tile_fetch<LF>(f, c, n_pix, p0, c0 + LC, rb);
        }
#pragma unroll
        for (int i = 0; i < LQ; ++i) {
            if (c0 + LQ * q + i < c) {
                const float a = A[(LQ * q + i) * LPITCH + pix] * m;
                const float b = B[(LQ * q + i) * LPITCH + pix] * m;
                const float d = a - b;
                s2 += (double)(d * d);
                sf += (double)fabsf(b);
                sg += (double)fabsf(a);
            }
        }
    }
    __syncthreads();
    double *part = (double *)A;
    if (q > 0) {
        part[((q - 1) * 3 + 0) * LP + pix] = s2;
        part[((q - 1) * 3 + 1) * LP + pix] = sf;
        part[((q - 1) * 3 + 2) * LP + pix] = sg;
    }
    __syncthreads();
    if (q != 0 || p >= n_pix) return;
    s2 = (s2 + part[0 * LP + pix]) + (part[3 * LP + pix] + part[6 * LP + pix]);
    sf = (sf + part[1 * LP + pix]) + (part[4 * LP + pix] + part[7 * LP + pix]);
    sg = (sg + part[2 * LP + pix]) + (part[5 * LP + pix] + part[8 * LP + pix]);
    l2[p] = sqrtf((float)s2);
    mean_abs_f[p] = (float)(sf / (double)c);
    mean_abs_gt[p] = (float)(sg / (double)c);
}


inline bool query_dims_ok(int n_maps, int n_frames, int h, int w)
{
    return n_maps > 0 && n_frames > 0 && n_maps % n_frames == 0 && h > 0 && w > 0 && n_maps <= 65535 && h <= 65535;
}

}  // namespace

extern "C" int64_t gags_query_images_scratch_bytes(int n_maps, int h, int w)
{
    if (n_maps <= 0 || h <= 0 || w <= 0) return 0;
    return al256((int64_t)n_maps * h * w * 8);
}

extern "C" int gags_query_colour(int n_maps, int n_frames, int h, int w, const float *heat, const float *output,
                                 const unsigned char *mask, const float *avg2, const float *stats, const float *image,
                                 const float *lut, float *heatmap_rgb, float *lerf_rgb, float *mask_rgb, unsigned char *heatmap_u8,
                                 unsigned char *lerf_u8, unsigned char *mask_u8, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_maps == 0 && n_frames >= 0 && h > 0 && w > 0) return GAGS_OK;
    if (!query_dims_ok(n_maps, n_frames, h, w)) return GAGS_EINVAL;
    if (!heat || !output || !mask || !avg2 || !stats || !image || !lut || !heatmap_rgb || !lerf_rgb || !mask_rgb) return GAGS_EINVAL;
    if ((heatmap_u8 != nullptr) != (lerf_u8 != nullptr) || (heatmap_u8 != nullptr) != (mask_u8 != nullptr)) return GAGS_EINVAL;
    const int64_t hw = (int64_t)h * w;
    hipLaunchKernelGGL(query_colour_kernel, dim3((unsigned)((hw + 255) / 256), n_maps), dim3(256), 0, (hipStream_t)stream, hw,
                       n_maps / n_frames, heat, output, mask, avg2, stats, image, lut, heatmap_rgb, lerf_rgb, mask_rgb, heatmap_u8,
                       lerf_u8, mask_u8);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_query_images(int n_maps, int n_frames, int h, int w, const float *heat, const float *output,
                                 const unsigned char *mask, const float *stats, const float *image, const float *lut, int box,
                                 float *avg2, float *heatmap_rgb, float *lerf_rgb, float *mask_rgb, unsigned char *heatmap_u8,
                                 unsigned char *lerf_u8, unsigned char *mask_u8, void *scratch, int64_t scratch_bytes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_maps == 0 && n_frames >= 0 && h > 0 && w > 0 && box >= 1 && box <= 1024) return GAGS_OK;
    if (!query_dims_ok(n_maps, n_frames, h, w) || box < 1 || box > 1024) return GAGS_EINVAL;
    if (!heat || !output || !mask || !stats || !image || !lut || !avg2 || !heatmap_rgb || !lerf_rgb || !mask_rgb || !scratch)
        return GAGS_EINVAL;
    if ((heatmap_u8 != nullptr) != (lerf_u8 != nullptr) || (heatmap_u8 != nullptr) != (mask_u8 != nullptr)) return GAGS_EINVAL;
    if (scratch_bytes < gags_query_images_scratch_bytes(n_maps, h, w)) return GAGS_ESCRATCH;
    const hipStream_t st = (hipStream_t)stream;
    double *rowsum = (double *)scratch;
    const dim3 grid((w + 255) / 256, h, n_maps);
    hipLaunchKernelGGL(box_rows_kernel, grid, dim3(256), (size_t)(256 + box) * 4, st, h, w, box, output, rowsum);
    hipLaunchKernelGGL(box_cols_mean_kernel, grid, dim3(256), 0, st, h, w, box, (const double *)rowsum, avg2);
    GAGS_CHECK_LAUNCH();
    return gags_query_colour(n_maps, n_frames, h, w, heat, output, mask, avg2, stats, image, lut, heatmap_rgb, lerf_rgb, mask_rgb,
                             heatmap_u8, lerf_u8, mask_u8, stream);
}

extern "C" int gags_feature_loss_maps(int c, int64_t n_pix, const float *feature, int feature_layout, const float *gt,
                                      int gt_layout, const float *mask, float *l2, float *mean_abs_feature, float *mean_abs_gt,
                                      void *stream)
{
    GAGS_CLEAR_ERR();
    if (c < 1 || c > 65536 || n_pix < 0 || n_pix > (1ll << 30) || (feature_layout | 1) != 1 || (gt_layout | 1) != 1) return GAGS_EINVAL;
    if (n_pix == 0) return GAGS_OK;
    if (!feature || !gt || !mask || !l2 || !mean_abs_feature || !mean_abs_gt) return GAGS_EINVAL;
    const dim3 grid((unsigned)((n_pix + LP - 1) / LP)), block(256);
    const hipStream_t st = (hipStream_t)stream;
#define GAGS_LOSS_MAPS(LF, LG)                                                                                               \
    hipLaunchKernelGGL((loss_maps_kernel<LF, LG>), grid, block, 0, st, c, n_pix, feature, gt, mask, l2, mean_abs_feature, \
                       mean_abs_gt)
    if (feature_layout == 0 && gt_layout == 0) GAGS_LOSS_MAPS(0, 0);
    else if (feature_layout == 0) GAGS_LOSS_MAPS(0, 1);
    else if (gt_layout == 0) GAGS_LOSS_MAPS(1, 0);
    else GAGS_LOSS_MAPS(1, 1);
#undef GAGS_LOSS_MAPS
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
