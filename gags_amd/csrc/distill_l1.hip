// N2: ground-truth feature assembly and the masked L1 map of the distillation loss, channel-major and
// pixel-major.  HBM-bound gather work over [C, H, W] maps: coalesced along pixels, the segment embeddings left to L2;
// nothing is reshaped into a GEMM.  Numerics follow the reference's torch ops (fp32).
#include "common.h"
#include "gags_next.h"
#include "reduce.h"
#include "sam_taps.h"

namespace {

// read_sam_clip_feature and the fused distillation L1 (scene/dataset_readers.py:54-121, train.py:165-166).
//
// A workgroup owns 64 consecutive pixels of the [H, W] map and walks the channels in blocks of 64.  Phase A (thread =
// pixel x 16-channel quarter): the level features F_l[c] = bilinear blend of the embedding rows of the pixel's (up to
// four) source pixels, rows read 64 contiguous bytes per thread; they go to LDS.  Phase B (thread = channel x pixel,
// pixels fastest): everything that touches the channel-major maps, coalesced along pixels.
constexpr int TP = 64;       // pixels per workgroup
constexpr int CB = 64;       // channels per block
constexpr int LDP = CB + 1;  // LDS row pitch (floats): conflict-free in both phases

// F_l[ch] for 16 channels starting at c0 of one pixel, as torch computes it:
// h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11); the products by the lambdas are folded into wgt[] here.
// REF_ORDER: the taps enter the fused chain in the order 10, 11, 01, 00 instead of 00, 01, 10, 11 -- the order of torch's CPU
// upsample kernel for the channels-last tensor read_sam_clip_feature hands it, whose bits the max-mode fixture holds (of the 24
// orders only this one reproduces them; tests/featurevis_ref.py).  The default order is what modes 0-3 have always computed.
template <bool REF_ORDER = false>
__device__ __forceinline__ void level_feature16(const Taps &t, int l, const float *__restrict__ img_embed, int c, int c0,
                                                float (&f)[16])
{
#pragma unroll
    for (int j = 0; j < 16; ++j) f[j] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const int k = REF_ORDER ? (kk < 2 ? 2 + kk : 3 - kk) : kk;
        if (t.wgt[k] == 0.f) continue;  // identity resize: a single tap
        const float4 *row = reinterpret_cast<const float4 *>(img_embed + (size_t)t.id[l][k] * c + c0);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = row[q];
            f[4 * q] = fmaf(t.wgt[k], v.x, f[4 * q]); f[4 * q + 1] = fmaf(t.wgt[k], v.y, f[4 * q + 1]);
            f[4 * q + 2] = fmaf(t.wgt[k], v.z, f[4 * q + 2]); f[4 * q + 3] = fmaf(t.wgt[k], v.w, f[4 * q + 3]);
        }
    }
}

// MODE 0: feature_map + mask; 1: v_scale from v_feature; 2: fused L1 map forward; 3: fused L1 map backward;
// 4: max mode (dataset_readers.py:81-88, what render.py asks for): the arg-max level's feature where THAT level is valid
template <int MODE>
__global__ __launch_bounds__(256) void sam_feature_kernel(int c, int H, int W, int h, int w, int n_emb,
                                                          const float *__restrict__ pred /* 2,3: pred; 1: v_feature */,
                                                          const float *__restrict__ img_embed,
                                                          const float *__restrict__ seg_map,
                                                          const float *__restrict__ scale_map,
                                                          const float *__restrict__ v_map, float *__restrict__ out0,
                                                          float *__restrict__ out1)
{
    __shared__ float F[3][TP][LDP];
    __shared__ float red[4][TP][4];
    const int HW = H * W;
    const int p0 = blockIdx.x * TP;
    // phase-A identity: pixel pa, channel quarter qa
    const int pa = threadIdx.x >> 2, qa = threadIdx.x & 3;
    const int pA = min(p0 + pa, HW - 1);
    const Taps tp = make_taps(pA, H, W, h, w, n_emb, seg_map);
    // phase-B identity: pixel pb (fastest), channel residue rb
    const int pb = threadIdx.x & 63, rb = threadIdx.x >> 6;
    const int pB = p0 + pb;
    const bool inB = pB < HW;
    const int pBc = min(pB, HW - 1);
    float sc[3] = {0.f, 0.f, 0.f};
    if (MODE != 1) {
#pragma unroll
        for (int l = 0; l < 3; ++l) sc[l] = scale_map[(size_t)l * HW + pBc];
    }
    // the mask of pixel pb: computed by the phase-A threads of that pixel; hand it over through LDS
    if (qa == 0) red[0][pa][0] = tp.mask;
    __syncthreads();
    const float maskB = red[0][pb][0];
    __syncthreads();
    float lv[3] = {0.f, 0.f, 0.f};  // MODE 4: the levels' own validities, then sc[] = one_hot(argmax scale_map)
    if (MODE == 4) {
        if (qa == 0) { red[0][pa][1] = tp.lvl[0]; red[0][pa][2] = tp.lvl[1]; red[0][pa][3] = tp.lvl[2]; }
        __syncthreads();
#pragma unroll
        for (int l = 0; l < 3; ++l) lv[l] = red[0][pb][1 + l];
        int k = sc[1] > sc[0] ? 1 : 0;  // torch.argmax: the first of equal maxima
        if (sc[2] > sc[k]) k = 2;
#pragma unroll
        for (int l = 0; l < 3; ++l) sc[l] = l == k ? 1.f : 0.f;
    }
    const float vB = (MODE == 3) ? v_map[pBc] * (1.0f / (float)c) : 0.f;
    float acc0 = 0.f, acc1 = 0.f, acc2 = 0.f;  // MODE 2: |diff| sum in acc0; MODE 1 / 3: v_scale partials

    for (int cb = 0; cb < c; cb += CB) {
        // this block's 16 values of the channel-major operand are requested FIRST, all at once, and arrive while the
        // embedding rows are gathered (inside the loop below they would be waited for four at a time)
        float pv[CB / 4];
        if (MODE != 0 && MODE != 4) {
#pragma unroll
            for (int k = 0; k < CB / 4; ++k) pv[k] = pred[(size_t)min(cb + rb + 4 * k, c - 1) * HW + pBc];
            __builtin_amdgcn_sched_barrier(0);  // keep the requests up here (the scheduler would sink them to their uses)
        }
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            float f[16];
            const int c0 = cb + qa * 16;
            if (c0 < c) level_feature16<MODE == 4>(tp, l, img_embed, c, c0, f);
#pragma unroll
            for (int j = 0; j < 16; ++j) F[l][pa][qa * 16 + j] = (c0 < c) ? f[j] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < CB / 4; ++k) {
            const int cl = rb + 4 * k, ch = cb + cl;
            const bool live = ch < c && inB;
            const float f0 = F[0][pb][cl], f1 = F[1][pb][cl], f2 = F[2][pb][cl];
            const size_t o = (size_t)min(ch, c - 1) * HW + pBc;
            if (MODE == 0) {
                // feature_map_s * scale_map[0] + feature_map_m * scale_map[1] + feature_map_l * scale_map[2]
                if (live) out0[o] = (f0 * sc[0] + f1 * sc[1]) + f2 * sc[2];
            } else if (MODE == 4) {
                // feature_map_s * one_hot[0] * mask_s + feature_map_m * one_hot[1] * mask_m + feature_map_l * one_hot[2] * mask_l
                const float v = ((f0 * sc[0]) * lv[0] + (f1 * sc[1]) * lv[1]) + (f2 * sc[2]) * lv[2];
                if (live) out0[o] = v;
                if (live && ch == 0) out1[pB] = v != 0.f ? 1.f : 0.f;  // mask = feature_map[0:1] != 0: channel 0 alone
            } else if (MODE == 1) {
                const float v = live ? pv[k] : 0.f;
                acc0 = fmaf(v, f0, acc0); acc1 = fmaf(v, f1, acc1); acc2 = fmaf(v, f2, acc2);
            } else {
                const float gt = (f0 * sc[0] + f1 * sc[1]) + f2 * sc[2];
                const float diff = ch < c ? pv[k] * maskB - gt * maskB : 0.f;
                if (MODE == 2) {
                    acc0 += fabsf(diff);
                } else {
                    const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
                    const float g = sgn * vB * maskB;  // d |pred*m - gt*m| / d pred, times v / c
                    if (live) out0[o] = g;
                    acc0 = fmaf(-g, f0, acc0); acc1 = fmaf(-g, f1, acc1); acc2 = fmaf(-g, f2, acc2);
                }
            }
        }
        __syncthreads();
    }
    if (MODE == 0) {
        if (rb == 0 && inB) out1[pB] = maskB;
        return;
    }
    if (MODE == 4) return;
    red[rb][pb][0] = acc0; red[rb][pb][1] = acc1; red[rb][pb][2] = acc2;
    __syncthreads();
    if (rb == 0 && inB) {
        if (MODE == 2) {
            out0[pB] = ((red[0][pb][0] + red[1][pb][0]) + (red[2][pb][0] + red[3][pb][0])) / (float)c;
            out1[pB] = maskB;
        } else {
            float *vs = out1;
#pragma unroll
            for (int l = 0; l < 3; ++l)
                vs[(size_t)l * HW + pB] = (red[0][pb][l] + red[1][pb][l]) + (red[2][pb][l] + red[3][pb][l]);
        }
    }
}

// The fused distillation L1 on a PIXEL-major prediction pred[P][c] (what gags_decoder_head writes with layout 1: the
// [C,H,W] tensor the caller sees is a permuted view of it).  Nothing is transposed: thread = (pixel, 4 channels), a
// pixel's 2 KB row is read as consecutive float4 by consecutive lanes, the embedding rows likewise (L2-resident), the
// taps of the tile's 32 pixels are computed once and shared through LDS.  MODE 2: forward, 3: backward.
template <int MODE>
__global__ __launch_bounds__(256) void sam_l1_pm_kernel(int c, int H, int W, int h, int w, int n_emb,
                                                        const float *__restrict__ pred, const float *__restrict__ img_embed,
                                                        const float *__restrict__ seg_map, const float *__restrict__ scale_map,
                                                        const float *__restrict__ v_map, float *__restrict__ out0,
                                                        float *__restrict__ out1)
{
    __shared__ TapsLds tl[TPM];
    __shared__ float red[TPM][4];  // per pixel: |diff| sum (MODE 2) or the three v_scale sums (MODE 3)
    const int HW = H * W;
    const int p0 = blockIdx.x * TPM;
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < TPM) {
        const int pc = min(p0 + tid, HW - 1);
        tl[tid] = make_taps_lds<MODE == 3>(pc, c, H, W, h, w, n_emb, seg_map, scale_map, v_map);
        red[tid][0] = red[tid][1] = red[tid][2] = red[tid][3] = 0.f;
    }
    __syncthreads();
    const int q4 = c >> 2;                 // float4 per pixel
    const int total = min(TPM, HW - p0) * q4;
    for (int i = tid; i - lane < total; i += 256) {  // (whole waves stay in the loop: the sums below are wave-wide)
        const bool live = i < total;
        const int ic = live ? i : total - 1;
        const int px = ic / q4, c4 = ic - px * q4;
        const TapsLds &t = tl[px];
        const size_t o = ((size_t)(p0 + px) * c) + 4 * c4;
        const float4 pv = *reinterpret_cast<const float4 *>(pred + o);
        float f[3][4];
#pragma unroll
        for (int l = 0; l < 3; ++l) {
            f[l][0] = f[l][1] = f[l][2] = f[l][3] = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (t.wgt[k] == 0.f) continue;  // identity resize: a single tap
                const float4 e = *reinterpret_cast<const float4 *>(img_embed + (size_t)t.id[l][k] * c + 4 * c4);
                f[l][0] = fmaf(t.wgt[k], e.x, f[l][0]); f[l][1] = fmaf(t.wgt[k], e.y, f[l][1]);
                f[l][2] = fmaf(t.wgt[k], e.z, f[l][2]); f[l][3] = fmaf(t.wgt[k], e.w, f[l][3]);
            }
        }
        const float pe[4] = {pv.x, pv.y, pv.z, pv.w};
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, gq[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float gt = (f[0][q] * t.sc[0] + f[1][q] * t.sc[1]) + f[2][q] * t.sc[2];
            const float diff = live ? pe[q] * t.mask - gt * t.mask : 0.f;
            if (MODE == 2) {
                a0 += fabsf(diff);
            } else {
                const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
                const float g = sgn * t.v * t.mask;
                gq[q] = g;
                a0 = fmaf(-g, f[0][q], a0); a1 = fmaf(-g, f[1][q], a1); a2 = fmaf(-g, f[2][q], a2);
            }
        }
        if (MODE == 3 && live) *reinterpret_cast<float4 *>(out0 + o) = make_float4(gq[0], gq[1], gq[2], gq[3]);
        // a wave covers 64 consecutive float4 of ONE pixel when c >= 256 (q4 % 64 == 0); otherwise lanes add themselves
        if ((q4 & 63) == 0) {
            a0 = gags_wave_sum(a0);
            if (MODE == 3) { a1 = gags_wave_sum(a1); a2 = gags_wave_sum(a2); }
            if (lane == 0) {
                atomicAdd(&red[px][0], a0);
                if (MODE == 3) { atomicAdd(&red[px][1], a1); atomicAdd(&red[px][2], a2); }
            }
        } else if (live) {
            atomicAdd(&red[px][0], a0);
            if (MODE == 3) { atomicAdd(&red[px][1], a1); atomicAdd(&red[px][2], a2); }
        }
    }
    __syncthreads();
    if (tid < TPM && p0 + tid < HW) {
        if (MODE == 2) {
            out0[p0 + tid] = red[tid][0] / (float)c;
            out1[p0 + tid] = tl[tid].mask;
        } else {
#pragma unroll
            for (int l = 0; l < 3; ++l) out1[(size_t)l * HW + p0 + tid] = red[tid][l];
        }
    }
}

// the L1 map in direction MODE (2: forward, 3: backward) for either layout of pred: 1 = pixel-major [H, W, c], 0 = [c, H, W]
template <int MODE>
int launch_l1_map(int layout, int c, int H, int W, int h, int w, int n_emb, const float *pred, const float *img_embed,
                  const float *seg_map, const float *scale_map, const float *v_map, float *out0, float *out1, hipStream_t st)
{
    const auto kernel = layout == 1 ? sam_l1_pm_kernel<MODE> : sam_feature_kernel<MODE>;
    const int tile = layout == 1 ? TPM : TP;
    hipLaunchKernelGGL(kernel, dim3((H * W + tile - 1) / tile), dim3(256), 0, st, c, H, W, h, w, n_emb, pred, img_embed, seg_map,
                       scale_map, v_map, out0, out1);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

}  // namespace

extern "C" int gags_sam_clip_feature(int c, int H, int W, int h, int w, int n_emb, const float *img_embed,
                                     const float *seg_map, const float *scale_map, float *feature_map, float *mask,
                                     void *stream)
{
    GAGS_CLEAR_ERR();
    if (!sam_args_ok(c, H, W, h, w, n_emb) || !img_embed || !seg_map || !scale_map || !feature_map || !mask) return GAGS_EINVAL;
    hipLaunchKernelGGL(sam_feature_kernel<0>, dim3((H * W + TP - 1) / TP), dim3(256), 0, (hipStream_t)stream, c, H, W, h, w,
                       n_emb, (const float *)nullptr, img_embed, seg_map, scale_map, (const float *)nullptr, feature_map, mask);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_sam_clip_feature_max(int c, int H, int W, int h, int w, int n_emb, const float *img_embed,
                                         const float *seg_map, const float *scale_map, float *feature_map, float *mask,
                                         void *stream)
{
    GAGS_CLEAR_ERR();
    if (!sam_args_ok(c, H, W, h, w, n_emb) || !img_embed || !seg_map || !scale_map || !feature_map || !mask) return GAGS_EINVAL;
    hipLaunchKernelGGL(sam_feature_kernel<4>, dim3((H * W + TP - 1) / TP), dim3(256), 0, (hipStream_t)stream, c, H, W, h, w,
                       n_emb, (const float *)nullptr, img_embed, seg_map, scale_map, (const float *)nullptr, feature_map, mask);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_sam_clip_feature_bwd_scale(int c, int H, int W, int h, int w, int n_emb, const float *img_embed,
                                               const float *seg_map, const float *v_feature, float *v_scale, void *stream)
{
    GAGS_CLEAR_ERR();
    if (!sam_args_ok(c, H, W, h, w, n_emb) || !img_embed || !seg_map || !v_feature || !v_scale) return GAGS_EINVAL;
    hipLaunchKernelGGL(sam_feature_kernel<1>, dim3((H * W + TP - 1) / TP), dim3(256), 0, (hipStream_t)stream, c, H, W, h, w,
                       n_emb, v_feature, img_embed, seg_map, (const float *)nullptr, (const float *)nullptr,
                       (float *)nullptr, v_scale);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_distill_l1_map_fwd(int c, int H, int W, int h, int w, int n_emb, const float *pred, const float *img_embed,
                                       const float *seg_map, const float *scale_map, float *l1_map, float *mask, int layout,
                                       void *stream)
{
    GAGS_CLEAR_ERR();
    if (!sam_args_ok(c, H, W, h, w, n_emb) || !pred || !img_embed || !seg_map || !scale_map || !l1_map || !mask ||
        (layout != 0 && layout != 1))
        return GAGS_EINVAL;
    return launch_l1_map<2>(layout, c, H, W, h, w, n_emb, pred, img_embed, seg_map, scale_map, nullptr, l1_map, mask,
                            (hipStream_t)stream);
}

extern "C" int gags_distill_l1_map_bwd(int c, int H, int W, int h, int w, int n_emb, const float *pred, const float *img_embed,
                                       const float *seg_map, const float *scale_map, const float *v_map, float *v_pred,
                                       float *v_scale, int layout, void *stream)
{
    GAGS_CLEAR_ERR();
    if (!sam_args_ok(c, H, W, h, w, n_emb) || !pred || !img_embed || !seg_map || !scale_map || !v_map || !v_pred || !v_scale ||
        (layout != 0 && layout != 1))
        return GAGS_EINVAL;
    return launch_l1_map<3>(layout, c, H, W, h, w, n_emb, pred, img_embed, seg_map, scale_map, v_map, v_pred, v_scale,
                            (hipStream_t)stream);
}
