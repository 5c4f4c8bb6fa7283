// The output heads of the decoders and their backward (gags_decoder_head, gags_decoder_head_bwd, gags_softmax_head_bwd_y):
// pixel-major fp32 logits x[P, ld] (C real columns) -> y, and the cotangent g of y -> pixel-major 16-bit dz[P, ld] (columns
// >= C zero).
//   mode 0: y = F.normalize(dim=0) = x / max(||x||_2, 1e-12)   (CNN_decoder, models/networks.py:192)
//           dz = (g - y <y, g>) / max(||x||, eps)
//   mode 1: y = softmax over the channels                      (CNN_scale_decoder, :242)
//           dz = y * (g - <y, g>)
// Four kernel pairs by shape (head_plan): pixel-major output, a handful of channels, register-resident rows, general.
// Operation order is part of the contract (-ffp-contract=off).  The forward kernels and the general / small backward DIVIDE
// by a row's statistics (head_value, head_dz); the register-resident and pixel-major backward kernels multiply by
// reciprocals taken once per pixel.  That difference is deliberate: the two forms are not to be unified.
#include "decoder_common.h"

namespace {

constexpr int HP = 32;      // pixels per workgroup of the register-resident kernels
constexpr int HJ = 16;      // float4 per thread (ld <= 512)
constexpr int HS_MAXC = 4;  // most channels of the small-row kernels

// y from a logit and its row's statistics (the forward form: divisions)
__device__ __forceinline__ float head_value(float v, float s0, float s1, int mode) { return mode == 0 ? v / s0 : expf(v - s0) / s1; }

// dz from y (as head_value gives it), the cotangent g, dot = <y, g> and s0
__device__ __forceinline__ float head_dz(float y, float g, float dot, float s0, int mode) { return mode == 0 ? (g - y * dot) / s0 : y * (g - dot); }

// The statistics of row p in the two general kernels: thread = pixel x quarter q of the channels, four neighbouring lanes
// per pixel; every lane of the four gets the result.
__device__ __forceinline__ void head_strided_stats(const float *x, int64_t p, int C, int ld, int q, int mode, float &s0, float &s1)
{
    float s = 0.f, m = -3.0e38f;
    for (int c = q; c < C; c += 4) {
        const float v = x[p * ld + c];
        s = fmaf(v, v, s);
        m = fmaxf(m, v);
    }
    s += __shfl_xor(s, 1); s += __shfl_xor(s, 2);
    m = fmaxf(m, __shfl_xor(m, 1)); m = fmaxf(m, __shfl_xor(m, 2));
    float z = 0.f;
    if (mode == 1) {
        for (int c = q; c < C; c += 4) z += expf(x[p * ld + c] - m);
        z += __shfl_xor(z, 1); z += __shfl_xor(z, 2);
    }
    s0 = mode == 0 ? fmaxf(sqrtf(s), 1e-12f) : m;
    s1 = z;
}

// The register-resident kernels (ld <= 512, ld % 32 == 0: every decoder of the reference): thread = pixel (tid >> 3) x
// channels c0 + 32 j + 0..3 with c0 = (tid & 7) * 4, so the logits are read ONCE;

// ... the statistics are reduced over the eight lanes of a pixel
__device__ __forceinline__ void head_stats(const float4 (&v)[HJ], int J, int C, int c0, int mode, float &s0, float &s1)
{
    float s = 0.f, m = -3.0e38f;
#pragma unroll
    for (int j = 0; j < HJ; ++j)
        if (j < J) {
            const float e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c0 + 32 * j + k < C) { s = fmaf(e[k], e[k], s); m = fmaxf(m, e[k]); }
        }
    s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
    m = fmaxf(m, __shfl_xor(m, 1)); m = fmaxf(m, __shfl_xor(m, 2)); m = fmaxf(m, __shfl_xor(m, 4));
    if (mode == 0) { s0 = fmaxf(sqrtf(s), 1e-12f); s1 = 0.f; return; }
    float z = 0.f;
#pragma unroll
    for (int j = 0; j < HJ; ++j)
        if (j < J) {
            const float e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c0 + 32 * j + k < C) z += expf(e[k] - m);
        }
    z += __shfl_xor(z, 1); z += __shfl_xor(z, 2); z += __shfl_xor(z, 4);
    s0 = m; s1 = z;
}

// The general head: CHANNEL-major out[C, P] (the reference's [C, H, W]).  One workgroup = 64 pixels; the transpose goes
// through LDS so that both sides are coalesced.
__global__ __launch_bounds__(256) void head_kernel(int64_t P, int C, int ld, int mode, const float *__restrict__ x,
                                                   float *__restrict__ out)
{
    __shared__ float tile[64][65];
    __shared__ float stat[64][2];
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int tid = threadIdx.x;
    // pass 1: per-pixel statistic (thread = pixel x quarter of the channels)
    {
        const int px = tid >> 2, q = tid & 3;
        float s0, s1;
        head_strided_stats(x, min(p0 + px, P - 1), C, ld, q, mode, s0, s1);
        if (q == 0) { stat[px][0] = s0; stat[px][1] = s1; }
    }
    __syncthreads();
    for (int cb = 0; cb < C; cb += 64) {
        // load [64 px][64 ch] pixel-major (channels fastest), store channel-major (pixels fastest)
        for (int e = tid; e < 64 * 64; e += 256) {
            const int px = e >> 6, c = e & 63;
            const int64_t p = min(p0 + px, P - 1);
            float v = 0.f;
            if (cb + c < C) v = head_value(x[p * ld + cb + c], stat[px][0], stat[px][1], mode);
            tile[px][c] = v;
        }
        __syncthreads();
        for (int e = tid; e < 64 * 64; e += 256) {
            const int c = e >> 6, px = e & 63;
            if (cb + c < C && p0 + px < P) out[(size_t)(cb + c) * P + p0 + px] = tile[px][c];
        }
        __syncthreads();
    }
}

// The register-resident head: one workgroup = 32 pixels; the transpose goes through a [channel][pixel ^ (channel & 31)]
// LDS tile (64 KB, conflict-free on the row side) and leaves as 128-byte rows.
__global__ __launch_bounds__(256) void head_fast_kernel(int64_t P, int C, int ld, int mode, const float *__restrict__ x,
                                                        float *__restrict__ out)
{
    __shared__ float tile[512 * HP];
    const int64_t p0 = (int64_t)blockIdx.x * HP;
    const int tid = threadIdx.x, px = tid >> 3, c0 = (tid & 7) * 4, J = ld >> 5;
    const int64_t p = min(p0 + px, P - 1);
    float4 v[HJ];
#pragma unroll
    for (int j = 0; j < HJ; ++j)
        v[j] = j < J ? *reinterpret_cast<const float4 *>(x + p * ld + c0 + 32 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
    float s0, s1;
    head_stats(v, J, C, c0, mode, s0, s1);
#pragma unroll
    for (int j = 0; j < HJ; ++j)
        if (j < J) {
            const float e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c0 + 32 * j + k;
                if (c < C) tile[c * HP + (px ^ (c & 31))] = head_value(e[k], s0, s1, mode);
            }
        }
    __syncthreads();
    const int lp = tid & 31;
    if (p0 + lp < P)
        for (int c = tid >> 5; c < C; c += 8) out[(size_t)c * P + p0 + lp] = tile[c * HP + (lp ^ (c & 31))];
}

// backward of the general head: channel-major cotangent G[C, P] and the saved logits
__global__ __launch_bounds__(256) void head_bwd_kernel(int64_t P, int C, int ld, int mode, const float *__restrict__ x,
                                                       const float *__restrict__ G, unsigned short *__restrict__ dz)
{
    __shared__ float tile[64][65];
    __shared__ float stat[64][3];
    __shared__ float dotp[4][64];  // <y, g> of a pixel's four channel groups: summed in group order below (no atomics)
    const int64_t p0 = (int64_t)blockIdx.x * 64;
    const int tid = threadIdx.x;
    // pass 1a: norm / (max, Z) per pixel from the logits
    {
        const int px = tid >> 2, q = tid & 3;
        float s0, s1;
        head_strided_stats(x, min(p0 + px, P - 1), C, ld, q, mode, s0, s1);
        if (q == 0) { stat[px][0] = s0; stat[px][1] = s1; }
    }
    __syncthreads();
    // pass 1b: <y, g> per pixel (G is channel-major: transpose block-wise through LDS)
    float part = 0.f;  // thread = pixel tid & 63, channels (tid >> 6) + 4 j of each block
    for (int cb = 0; cb < C; cb += 64) {
        for (int e = tid; e < 64 * 64; e += 256) {
            const int c = e >> 6, px = e & 63;
            tile[px][c] = (cb + c < C && p0 + px < P) ? G[(size_t)(cb + c) * P + p0 + px] : 0.f;
        }
        __syncthreads();
        {
            const int px = tid & 63;
            const int64_t p = min(p0 + px, P - 1);
            for (int c = tid >> 6; c < 64 && cb + c < C; c += 4) {  // (head_value and, in pass 2, head_dz written out: called here
                const float v = x[p * ld + cb + c];                 // they cost this kernel 1.2 % at c = 37, ld = 40)
                const float y = mode == 0 ? v / stat[px][0] : expf(v - stat[px][0]) / stat[px][1];
                part = fmaf(y, tile[px][c], part);
            }
        }
        __syncthreads();
    }
    // (an LDS atomic add per thread here left the order of a pixel's four partial sums to the hardware: the gradient of a head
    // wider than 512 channels, and every gradient behind it, changed in the last bit from run to run)
    dotp[tid >> 6][tid & 63] = part;
    __syncthreads();
    if (tid < 64) stat[tid][2] = ((dotp[0][tid] + dotp[1][tid]) + dotp[2][tid]) + dotp[3][tid];
    __syncthreads();
    // pass 2: dz, pixel-major
    for (int cb = 0; cb < ld; cb += 64) {
        for (int e = tid; e < 64 * 64; e += 256) {
            const int c = e >> 6, px = e & 63;
            tile[px][c] = (cb + c < C && p0 + px < P) ? G[(size_t)(cb + c) * P + p0 + px] : 0.f;
        }
        __syncthreads();
        for (int e = tid; e < 64 * 64; e += 256) {
            const int px = e >> 6, c = e & 63;
            if (p0 + px >= P || cb + c >= ld) continue;
            float d = 0.f;
            if (cb + c < C) {
                const float v = x[(p0 + px) * ld + cb + c], g = tile[px][c], dot = stat[px][2];
                if (mode == 0) {
                    const float nrm = stat[px][0];
                    d = (g - (v / nrm) * dot) / nrm;
                } else {
                    const float y = expf(v - stat[px][0]) / stat[px][1];
                    d = y * (g - dot);
                }
            }
            dz[(p0 + px) * ld + cb + c] = h16_from(d);
        }
        __syncthreads();
    }
}

// backward of the register-resident head: the same 32-pixel tiling as head_fast_kernel; the cotangent tile sits in LDS,
// the logits in registers, so G and x are each read once.
__global__ __launch_bounds__(256) void head_bwd_fast_kernel(int64_t P, int C, int ld, int mode, const float *__restrict__ x,
                                                            const float *__restrict__ G, unsigned short *__restrict__ dz)
{
    __shared__ float tile[512 * HP];
    const int64_t p0 = (int64_t)blockIdx.x * HP;
    const int tid = threadIdx.x, px = tid >> 3, c0 = (tid & 7) * 4, J = ld >> 5;
    const int64_t p = min(p0 + px, P - 1);
    float4 v[HJ];
#pragma unroll
    for (int j = 0; j < HJ; ++j)
        v[j] = j < J ? *reinterpret_cast<const float4 *>(x + p * ld + c0 + 32 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
    {
        // the cotangent rows in two batches of 32 loads in flight (a rolled loop would wait for every single row)
        const int lp = tid & 31, cw = tid >> 5;
        const int64_t pg = min(p0 + lp, P - 1);
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            float g[32];
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int c = cw + 8 * (32 * b + i);
                g[i] = c < C ? G[(size_t)c * P + pg] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int c = cw + 8 * (32 * b + i);
                if (c < C) tile[c * HP + (lp ^ (c & 31))] = g[i];
            }
        }
    }
    float s0, s1;
    head_stats(v, J, C, c0, mode, s0, s1);
    __syncthreads();
    // reciprocals once per pixel: the per-element work is one or two FMAs (the result is rounded to bf16 anyway)
    const float inv0 = 1.f / s0, inv1 = mode == 1 ? 1.f / s1 : 0.f;
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < HJ; ++j)
        if (j < J) {
            const float e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c0 + 32 * j + k;
                if (c < C) {
                    const float y = mode == 0 ? e[k] : expf(e[k] - s0) * inv1;   // mode 0: the 1 / norm is applied to the sum
                    dot = fmaf(y, tile[c * HP + (px ^ (c & 31))], dot);
                }
            }
        }
    dot += __shfl_xor(dot, 1); dot += __shfl_xor(dot, 2); dot += __shfl_xor(dot, 4);
    if (mode == 0) dot *= inv0;          // <y, g>
    const float k1 = dot * inv0 * inv0;  // mode 0: dz = g / n - x <y, g> / n^2
    if (p0 + px >= P) return;
#pragma unroll
    for (int j = 0; j < HJ; ++j)
        if (j < J) {
            const float e[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
            unsigned short o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int c = c0 + 32 * j + k;
                float d = 0.f;
                if (c < C) {
                    const float g = tile[c * HP + (px ^ (c & 31))];
                    if (mode == 0) d = fmaf(g, inv0, -e[k] * k1);
                    else d = (expf(e[k] - s0) * inv1) * (g - dot);
                }
                o[k] = h16_from(d);
            }
            uint2 w;
            w.x = (unsigned)o[0] | ((unsigned)o[1] << 16);
            w.y = (unsigned)o[2] | ((unsigned)o[3] << 16);
            *reinterpret_cast<uint2 *>(dz + p * ld + c0 + 32 * j) = w;
        }
}

// Pixel-major heads (layout 1): y[P][C] right next to the logits' own layout -- no transpose at all.  The [C,H,W]
// tensor the caller sees is then a permuted view of [H,W,C] memory, like the rasterizer's own output, and what the
// reference does with it next (compute_relvancy.py:266, evaluate_iou_loc.py:283: .permute(1,2,0)) is free.
__global__ __launch_bounds__(256) void head_pm_kernel(int64_t P, int C, int ld, int mode, const float *__restrict__ x,
                                                      float *__restrict__ out)
{
    const int tid = threadIdx.x, c0 = (tid & 7) * 4, J = ld >> 5;
    const int64_t pr = (int64_t)blockIdx.x * HP + (tid >> 3), p = min(pr, P - 1);
    float4 v[HJ];
#pragma unroll
    for (int j = 0; j < HJ; ++j)
        v[j] = j < J ? *reinterpret_cast<const float4 *>(x + p * ld + c0 + 32 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
    float s0, s1;
    head_stats(v, J, C, c0, mode, s0, s1);
    if (pr >= P) return;
#pragma unroll
    for (int j = 0; j < HJ; ++j)
        if (j < J && c0 + 32 * j < C) {  // C % 4 == 0: the whole float4 is inside
            const float4 e = v[j];       // (the mode is passed as a literal: with `mode` the select moves into every element, 11 % more code)
            *reinterpret_cast<float4 *>(out + p * C + c0 + 32 * j) =
                mode == 0 ? make_float4(head_value(e.x, s0, s1, 0), head_value(e.y, s0, s1, 0), head_value(e.z, s0, s1, 0), head_value(e.w, s0, s1, 0))
                          : make_float4(head_value(e.x, s0, s1, 1), head_value(e.y, s0, s1, 1), head_value(e.z, s0, s1, 1), head_value(e.w, s0, s1, 1));
        }
}

__global__ __launch_bounds__(256) void head_bwd_pm_kernel(int64_t P, int C, int ld, int mode, const float *__restrict__ x,
                                                          const float *__restrict__ G, unsigned short *__restrict__ dz)
{
    const int tid = threadIdx.x, c0 = (tid & 7) * 4, J = ld >> 5;
    const int64_t pr = (int64_t)blockIdx.x * HP + (tid >> 3), p = min(pr, P - 1);
    float4 v[HJ], g[HJ];
#pragma unroll
    for (int j = 0; j < HJ; ++j) {
        v[j] = j < J ? *reinterpret_cast<const float4 *>(x + p * ld + c0 + 32 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
        g[j] = (j < J && c0 + 32 * j < C) ? *reinterpret_cast<const float4 *>(G + p * C + c0 + 32 * j) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    float s0, s1;
    head_stats(v, J, C, c0, mode, s0, s1);
    const float inv0 = 1.f / s0, inv1 = mode == 1 ? 1.f / s1 : 0.f;
    float dot = 0.f;
#pragma unroll
    for (int j = 0; j < HJ; ++j)
        if (j < J && c0 + 32 * j < C) {
            const float e[4] = {v[j].x, v[j].y, v[j].z, v[j].w}, gg[4] = {g[j].x, g[j].y, g[j].z, g[j].w};
#pragma unroll
            for (int k = 0; k < 4; ++k) dot = fmaf(mode == 0 ? e[k] : expf(e[k] - s0) * inv1, gg[k], dot);
        }
    dot += __shfl_xor(dot, 1); dot += __shfl_xor(dot, 2); dot += __shfl_xor(dot, 4);
    if (mode == 0) dot *= inv0;
    const float k1 = dot * inv0 * inv0;
    if (pr >= P) return;
#pragma unroll
    for (int j = 0; j < HJ; ++j)
        if (j < J) {
            const float e[4] = {v[j].x, v[j].y, v[j].z, v[j].w}, gg[4] = {g[j].x, g[j].y, g[j].z, g[j].w};
            float d[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                d[k] = 0.f;
                if (c0 + 32 * j + k < C) d[k] = mode == 0 ? fmaf(gg[k], inv0, -e[k] * k1) : (expf(e[k] - s0) * inv1) * (gg[k] - dot);
            }
            *reinterpret_cast<uint2 *>(dz + p * ld + c0 + 32 * j) = make_uint2(h16_pack(d[0], d[1]), h16_pack(d[2], d[3]));
        }
}

// Heads with a handful of channels (CNN_scale_decoder: softmax over 3): one thread per pixel, the whole row in
// registers; channel-major output / cotangent planes are coalesced along the pixels.  (The tiled kernels above issue 64
// mostly predicated-off loads per thread for such a head: 0.64 ms instead of 0.1.)
__global__ __launch_bounds__(256) void head_small_kernel(int64_t P, int C, int ld, int mode, const float *__restrict__ x,
                                                         float *__restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float4 xv = *reinterpret_cast<const float4 *>(x + p * ld);
    const float e[4] = {xv.x, xv.y, xv.z, xv.w};
    float s = 0.f, m = -3.0e38f;
#pragma unroll
    for (int c = 0; c < HS_MAXC; ++c)
        if (c < C) { s = fmaf(e[c], e[c], s); m = fmaxf(m, e[c]); }
    float z = 0.f;
    if (mode == 1) {
#pragma unroll
        for (int c = 0; c < HS_MAXC; ++c)
            if (c < C) z += expf(e[c] - m);
    }
    const float nrm = fmaxf(sqrtf(s), 1e-12f);
#pragma unroll
    for (int c = 0; c < HS_MAXC; ++c)
        if (c < C) out[(size_t)c * P + p] = head_value(e[c], mode == 0 ? nrm : m, z, mode);
}

__global__ __launch_bounds__(256) void head_bwd_small_kernel(int64_t P, int C, int ld, int mode, const float *__restrict__ x,
                                                             const float *__restrict__ G, unsigned short *__restrict__ dz)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const float4 xv = *reinterpret_cast<const float4 *>(x + p * ld);
    const float e[4] = {xv.x, xv.y, xv.z, xv.w};
    float g[4] = {0.f, 0.f, 0.f, 0.f};
    float s = 0.f, m = -3.0e38f;
#pragma unroll
    for (int c = 0; c < HS_MAXC; ++c)  // (the cotangent loads ride in the statistic's loop: in a loop of their own they cost a register)
        if (c < C) { g[c] = G[(size_t)c * P + p]; s = fmaf(e[c], e[c], s); m = fmaxf(m, e[c]); }
    float z = 0.f, y[4] = {0.f, 0.f, 0.f, 0.f};
    const float nrm = fmaxf(sqrtf(s), 1e-12f);
#pragma unroll
    for (int c = 0; c < HS_MAXC; ++c)
        if (c < C) {
            if (mode == 1) { y[c] = expf(e[c] - m); z += y[c]; } else y[c] = e[c] / nrm;
        }
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < HS_MAXC; ++c)
        if (c < C) { if (mode == 1) y[c] /= z; dot = fmaf(y[c], g[c], dot); }
    float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < HS_MAXC; ++c)
        if (c < C) d[c] = head_dz(y[c], g[c], dot, nrm, mode);
    // the whole padded row: columns >= C are zero
    uint4 *dst = reinterpret_cast<uint4 *>(dz + p * ld);
    dst[0] = make_uint4(h16_pack(d[0], d[1]), h16_pack(d[2], d[3]), 0u, 0u);
    for (int q = 1; q < ld / 8; ++q) dst[q] = make_uint4(0u, 0u, 0u, 0u);
}

// backward of the softmax head from its OUTPUT y [C, P] (what the fused scale-decoder forward leaves: no logits are kept):
// dz = y (g - <y, g>), the same operations in the same order as head_bwd_small_kernel from its y onwards
__global__ __launch_bounds__(256) void softmax_bwd_small_y_kernel(int64_t P, int C, int ld, const float *__restrict__ Y,
                                                                  const float *__restrict__ G, unsigned short *__restrict__ dz)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    float g[4] = {0.f, 0.f, 0.f, 0.f}, y[4] = {0.f, 0.f, 0.f, 0.f}, dot = 0.f;
#pragma unroll
    for (int c = 0; c < HS_MAXC; ++c)
        if (c < C) { g[c] = G[(size_t)c * P + p]; y[c] = Y[(size_t)c * P + p]; }
#pragma unroll
    for (int c = 0; c < HS_MAXC; ++c)
        if (c < C) dot = fmaf(y[c], g[c], dot);
    float d[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < HS_MAXC; ++c)
        if (c < C) d[c] = head_dz(y[c], g[c], dot, 0.f, 1);
    uint4 *dst = reinterpret_cast<uint4 *>(dz + p * ld);
    dst[0] = make_uint4(h16_pack(d[0], d[1]), h16_pack(d[2], d[3]), 0u, 0u);
    for (int q = 1; q < ld / 8; ++q) dst[q] = make_uint4(0u, 0u, 0u, 0u);
}

// Which kernel pair serves a shape, and its grid: the ONE place that knows (both entry points switch on the result).
// HEAD_INVALID: (n_pix, c, ld, mode, layout) is not a head this library has.
enum HeadKernel { HEAD_INVALID, HEAD_PM, HEAD_SMALL, HEAD_REG, HEAD_GENERAL };
inline HeadKernel head_plan(int64_t n_pix, int c, int ld, int mode, int layout, unsigned &grid)
{
    if (n_pix < 0 || c <= 0 || ld < c || (mode != 0 && mode != 1)) return HEAD_INVALID;
    const bool reg = ld <= 512 && ld % 32 == 0;
    if (layout != 0 && !(layout == 1 && c % 4 == 0 && reg)) return HEAD_INVALID;
    const HeadKernel k = layout == 1 ? HEAD_PM : (c <= HS_MAXC && ld % 8 == 0 && ld >= 8) ? HEAD_SMALL : reg ? HEAD_REG : HEAD_GENERAL;
    const int px = k == HEAD_SMALL ? 256 : k == HEAD_GENERAL ? 64 : HP;  // pixels per workgroup
    grid = (unsigned)((n_pix + px - 1) / px);
    return k;
}

}  // namespace

extern "C" int GAGS_DEC(gags_decoder_head)(int64_t n_pix, int c, int ld, int mode, const float *x, float *out, int layout, void *stream)
{
    GAGS_CLEAR_ERR();
    unsigned grid = 0;
    const HeadKernel k = head_plan(n_pix, c, ld, mode, layout, grid);
    if (k == HEAD_INVALID || (n_pix > 0 && (!x || !out))) return GAGS_EINVAL;
    if (n_pix == 0) return GAGS_OK;
    void (*kernel)(int64_t, int, int, int, const float *, float *) = nullptr;
    switch (k) {
    case HEAD_PM: kernel = head_pm_kernel; break;
    case HEAD_SMALL: kernel = head_small_kernel; break;
    case HEAD_REG: kernel = head_fast_kernel; break;
    default: kernel = head_kernel; break;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, n_pix, c, ld, mode, x, out);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int GAGS_DEC(gags_decoder_head_bwd)(int64_t n_pix, int c, int ld, int mode, const float *x, const float *g, void *dz_bf16,
                                     int layout, void *stream)
{
    GAGS_CLEAR_ERR();
    unsigned grid = 0;
    const HeadKernel k = head_plan(n_pix, c, ld, mode, layout, grid);
    if (k == HEAD_INVALID || (n_pix > 0 && (!x || !g || !dz_bf16))) return GAGS_EINVAL;
    if (n_pix == 0) return GAGS_OK;
    void (*kernel)(int64_t, int, int, int, const float *, const float *, unsigned short *) = nullptr;
    switch (k) {
    case HEAD_PM: kernel = head_bwd_pm_kernel; break;
    case HEAD_SMALL: kernel = head_bwd_small_kernel; break;
    case HEAD_REG: kernel = head_bwd_fast_kernel; break;
    default: kernel = head_bwd_kernel; break;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, n_pix, c, ld, mode, x, g, (unsigned short *)dz_bf16);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int GAGS_DEC(gags_softmax_head_bwd_y)(int64_t n_pix, int c, int ld, const float *y, const float *g, void *dz_bf16, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_pix < 0 || c <= 0 || c > HS_MAXC || ld < 8 || ld % 8 != 0 || (n_pix > 0 && (!y || !g || !dz_bf16))) return GAGS_EINVAL;
    if (n_pix == 0) return GAGS_OK;
    hipLaunchKernelGGL(softmax_bwd_small_y_kernel, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_pix, c, ld,
                       y, g, (unsigned short *)dz_bf16);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
