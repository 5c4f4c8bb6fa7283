// N14 (include/gags_next.h): the tile cut between N10's kept masks and the CLIP image encoder of the GAS stage
// (preprocess.py:356-371 get_seg_img / pad_img, :476-489 mask2segmap's cv2.resize(..., (224, 224)) and the float conversion)
// from the image and the bit-packed masks, without a per-mask image copy or a host round trip.
//
// (a) tiles: grid (blocks of 256 output pixels, tile); 224 * 224 = 196 * 256, so no block has a tail.  A thread owns one
//     output pixel and its three channels; lanes run along dx, so the three planar fp32 stores of a wave are contiguous runs.
//     The tile's box and mask index are block-uniform (read once per block through the scalar unit); the two tap pairs are
//     computed per thread in float64 / fp32 exactly as the header states them.  Four taps per pixel: four bit tests and four
//     byte triples out of an image that sits in L2; the kernel is bound by its stores (602 KB of fp32 per tile).
//     The 2 x 2 mean at l = 448 needs no branch: there a0 = a1 = 1024 and b (h >> 4) >> 16 is s0 + s1 exactly.
// (b) boxes: a wave per mask, a lane per word (stride 64).  The row comes from the word index; the columns from ctz / clz when
//     the word's 64 pixels lie in one image row, bit by bit otherwise.  The wave's min / max: csrc/reduce.h.
// No atomics, no LDS.  Every index read from device memory (index, boxes) is range-checked before it is used.
#include <climits>
#include "common.h"
#include "gags_next.h"
#include "reduce.h"

namespace {

constexpr int SIDE = 224;
constexpr int TILE_PIXELS = SIDE * SIDE;   // 50 176 = 196 * 256
constexpr int64_t MAX_PIXELS = 1ll << 24;  // exclusive (N10's limit)

// source tap and coefficients of output coordinate d on an axis of l source pixels: taps s0 and s1, a0 + a1 = 2048
__device__ __forceinline__ void taps_of(int d, int l, double scale, int &s0, int &s1, int &a0, int &a1)
{
    const double t = ((double)d + 0.5) * scale;
    float f = (float)(t - 0.5);
    int s = (int)floorf(f);
    f -= (float)s;
    if (s < 0) { s = 0; f = 0.f; }
    if (s >= l - 1) { s = l - 1; f = 0.f; }
    const float g = 1.0f - f;
    a0 = (int)__builtin_rintf(g * 2048.0f);
    a1 = (int)__builtin_rintf(f * 2048.0f);
    s0 = s;
    s1 = s + 1 < l ? s + 1 : l - 1;
}

struct Crop {
    int x, y, w, h, ox, oy, W, rev;
    const unsigned char *image;
    const unsigned long long *bits;
};

// S[v, u, 0..2] of the padded square
__device__ __forceinline__ void square_at(const Crop &c, int v, int u, int &r, int &g, int &b)
{
    r = g = b = 0;
    const int i = v - c.oy, j = u - c.ox;
    if ((unsigned)i >= (unsigned)c.h || (unsigned)j >= (unsigned)c.w) return;
    const int p = (c.y + i) * c.W + c.x + j;  // < H W < 2^24
    if (!((c.bits[p >> 6] >> (p & 63)) & 1ull)) return;
    const unsigned char *px = c.image + (int64_t)p * 3;
    const int c0 = px[0], c1 = px[1], c2 = px[2];
    r = c.rev ? c2 : c0;
    g = c1;
    b = c.rev ? c0 : c2;
}

__device__ __forceinline__ int blend(int s00, int s01, int s10, int s11, int a0, int a1, int b0, int b1)
{
    const int h0 = s00 * a0 + s01 * a1, h1 = s10 * a0 + s11 * a1;
    return (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
}

__global__ __launch_bounds__(256) void tile_kernel(int H, int W, const unsigned char *__restrict__ image, int bgr, int M,
                                                   int64_t nw, const unsigned long long *__restrict__ bits,
                                                   const int *__restrict__ index, const int *__restrict__ boxes,
                                                   unsigned char *__restrict__ tiles_u8, float *__restrict__ tiles_f32)
{
    const int t = blockIdx.y;
    const int d = blockIdx.x * 256 + threadIdx.x;  // < TILE_PIXELS: the grid has no tail
    const int dy = d / SIDE, dx = d - dy * SIDE;
    // block-uniform: the tile's mask and box, clipped as a slice clips it
    const int m = index[t];
    const int x = boxes[4 * t], y = boxes[4 * t + 1], bw = boxes[4 * t + 2], bh = boxes[4 * t + 3];
    const int64_t xe = (int64_t)x + bw, ye = (int64_t)y + bh;
    const int wc = (int)((xe < W ? xe : W) - x), hc = (int)((ye < H ? ye : H) - y);
    const bool ok = (unsigned)m < (unsigned)M && x >= 0 && x < W && y >= 0 && y < H && wc >= 1 && hc >= 1;
    int out[3] = {0, 0, 0};
    if (ok) {
        const int l = wc > hc ? wc : hc;
        Crop c;
        c.x = x; c.y = y; c.w = wc; c.h = hc; c.W = W; c.rev = bgr;
        c.ox = hc > wc ? (l - wc) / 2 : 0;
        c.oy = hc > wc ? 0 : (l - hc) / 2;
        c.image = image;
        c.bits = bits + (int64_t)m * nw;
        const double scale = (double)l / (double)SIDE;
        int u0, u1, a0, a1, v0, v1, b0, b1;
        taps_of(dx, l, scale, u0, u1, a0, a1);
        taps_of(dy, l, scale, v0, v1, b0, b1);
        int s00[3], s01[3], s10[3], s11[3];
        square_at(c, v0, u0, s00[0], s00[1], s00[2]);
        square_at(c, v0, u1, s01[0], s01[1], s01[2]);
        square_at(c, v1, u0, s10[0], s10[1], s10[2]);
        square_at(c, v1, u1, s11[0], s11[1], s11[2]);
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) out[ch] = blend(s00[ch], s01[ch], s10[ch], s11[ch], a0, a1, b0, b1);
    }
    if (tiles_u8) {
        unsigned char *dst = tiles_u8 + ((int64_t)t * TILE_PIXELS + d) * 3;
        dst[0] = (unsigned char)out[0];
        dst[1] = (unsigned char)out[1];
        dst[2] = (unsigned char)out[2];
    }
    if (tiles_f32) {
        float *dst = tiles_f32 + (int64_t)t * 3 * TILE_PIXELS + d;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) dst[(int64_t)ch * TILE_PIXELS] = (float)out[ch] / 255.0f;
    }
}

__global__ __launch_bounds__(256) void boxes_kernel(int M, int W, int hw, int nw, const unsigned long long *__restrict__ bits,
                                                    int *__restrict__ boxes)
{
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;  // wave-uniform
    const unsigned long long *row = bits + (int64_t)m * nw;
    int x0 = INT_MAX, y0 = INT_MAX, x1 = -1, y1 = -1;
    for (int w = lane; w < nw; w += 64) {
        unsigned long long word = row[w];
        const int p0 = w * 64, left = hw - p0;  // left >= 1
        if (left < 64) word &= (1ull << left) - 1;
        if (!word) continue;
        const int r0 = p0 / W, c0 = p0 - r0 * W;
        if (c0 + 63 < W) {  // the word's 64 pixels lie in row r0
            const int lo = c0 + __builtin_ctzll(word), hi = c0 + 63 - __builtin_clzll(word);
            x0 = min(x0, lo); x1 = max(x1, hi);
            y0 = min(y0, r0); y1 = max(y1, r0);
        } else {
            while (word) {
                const int p = p0 + __builtin_ctzll(word);
                word &= word - 1;
                const int r = p / W, c = p - r * W;
                x0 = min(x0, c); x1 = max(x1, c);
                y0 = min(y0, r); y1 = max(y1, r);
            }
        }
    }
    x0 = gags_wave_min(x0); y0 = gags_wave_min(y0);
    x1 = gags_wave_max(x1); y1 = gags_wave_max(y1);
    if (lane == 0) {
        const bool empty = y1 < 0;
        int *dst = boxes + 4 * m;
        dst[0] = empty ? 0 : x0;
        dst[1] = empty ? 0 : y0;
        dst[2] = x1;
        dst[3] = y1;
    }
}

bool bad_image(int H, int W) { return H < 1 || W < 1 || (int64_t)H * W >= MAX_PIXELS; }
bool bad_count(int n) { return n < 0 || n > gags_masks_max_count(); }

}  // namespace

extern "C" int gags_tilecut_side(void) { return SIDE; }

extern "C" int gags_tilecut(int n_tiles, int height, int width, const unsigned char *image, int bgr, int n_masks,
                            const void *bits, const int32_t *index, const int32_t *boxes, unsigned char *tiles_u8,
                            float *tiles_f32, void *stream)
{
    GAGS_CLEAR_ERR();
    if (bad_count(n_tiles) || bad_count(n_masks) || bad_image(height, width) || (bgr != 0 && bgr != 1)) return GAGS_EINVAL;
    if (!tiles_u8 && !tiles_f32) return GAGS_EINVAL;
    if (n_tiles == 0) return GAGS_OK;
    if (n_masks < 1 || !image || !bits || !index || !boxes) return GAGS_EINVAL;
    const int64_t nw = ((int64_t)height * width + 63) / 64;
    hipLaunchKernelGGL(tile_kernel, dim3(TILE_PIXELS / 256, n_tiles), dim3(256), 0, (hipStream_t)stream, height, width, image,
                       bgr, n_masks, nw, (const unsigned long long *)bits, index, boxes, tiles_u8, tiles_f32);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_tilecut_boxes(int n_masks, int height, int width, const void *bits, int32_t *boxes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (bad_count(n_masks) || bad_image(height, width)) return GAGS_EINVAL;
    if (n_masks == 0) return GAGS_OK;
    if (!bits || !boxes) return GAGS_EINVAL;
    const int hw = height * width;
    hipLaunchKernelGGL(boxes_kernel, dim3((n_masks + 3) / 4), dim3(256), 0, (hipStream_t)stream, n_masks, width, hw,
                       (hw + 63) / 64, (const unsigned long long *)bits, boxes);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
