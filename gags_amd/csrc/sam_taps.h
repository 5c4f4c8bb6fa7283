// What distill_l1.hip and head_distill.hip share: where a pixel of the [H, W] render falls in the [h, w] segmentation map
// (read_sam_clip_feature, scene/dataset_readers.py:54-121) -- its source pixels' embedding rows, bilinear weights and
// validity -- the per-workgroup table of them in LDS, and the argument check of the entries that take such maps.
#pragma once
#include "common.h"

struct Taps {
    int id[3][4];   // embedding row of (level, tap)
    float wgt[4];   // bilinear weights of the four taps (same for every level)
    float mask;     // 1 if all three levels have a segment at the nearest source pixel
    float lvl[3];   // the same per level (max mode blanks a pixel by its arg-max level's own validity)
};

__device__ __forceinline__ Taps make_taps(int p, int H, int W, int h, int w, int n_emb, const float *__restrict__ seg_map)
{
    Taps t;
    const int y = p / W, x = p - y * W;
    // torch upsample_bilinear2d, align_corners=True: src = dst * (in - 1) / (out - 1)
    const float sy = H > 1 ? (float)(h - 1) / (float)(H - 1) : 0.f, sx = W > 1 ? (float)(w - 1) / (float)(W - 1) : 0.f;
    const float fy = sy * (float)y, fx = sx * (float)x;
    const int y0 = (int)fy, x0 = (int)fx;
    const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
    const float ly = fy - (float)y0, lx = fx - (float)x0;
    t.wgt[0] = (1.f - ly) * (1.f - lx); t.wgt[1] = (1.f - ly) * lx; t.wgt[2] = ly * (1.f - lx); t.wgt[3] = ly * lx;
    const int sp[4] = {y0 * w + x0, y0 * w + x1, y1 * w + x0, y1 * w + x1};
    // nearest resize of the validity mask: src = floor(dst * in / out)
    const int ny = min((int)floorf((float)y * ((float)h / (float)H)), h - 1);
    const int nx = min((int)floorf((float)x * ((float)w / (float)W)), w - 1);
    bool ok = true;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
        const float *lev = seg_map + (size_t)(l + 1) * h * w;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int id = (int)lev[sp[k]];
            t.id[l][k] = id < 0 ? id + n_emb : id;  // img_embed[-1] is the LAST row in the reference (Python indexing)
        }
        const bool ok_l = lev[ny * w + nx] != -1.0f;
        t.lvl[l] = ok_l ? 1.f : 0.f;
        ok = ok && ok_l;
    }
    t.mask = ok ? 1.f : 0.f;
    return t;
}

// The pixel-major kernels compute the taps of a workgroup's TPM pixels once and share them through LDS, together with the
// pixel's three level scales and (WITH_V: the backward kernels) its cotangent over the channel count:
// `if (tid < TPM) tl[tid] = make_taps_lds<...>(min(p0 + tid, H * W - 1), ...)`.
constexpr int TPM = 32;  // pixels per workgroup
struct TapsLds {
    int id[3][4];
    float wgt[4], mask, sc[3], v;
};

template <bool WITH_V>
__device__ __forceinline__ TapsLds make_taps_lds(int pc, int c, int H, int W, int h, int w, int n_emb,
                                                 const float *__restrict__ seg_map, const float *__restrict__ scale_map,
                                                 const float *__restrict__ v_map)
{
    const int HW = H * W;
    const Taps t = make_taps(pc, H, W, h, w, n_emb, seg_map);
    TapsLds q;
#pragma unroll
    for (int l = 0; l < 3; ++l) {
#pragma unroll
        for (int k = 0; k < 4; ++k) q.id[l][k] = t.id[l][k];
        q.sc[l] = scale_map[(size_t)l * HW + pc];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) q.wgt[k] = t.wgt[k];
    q.mask = t.mask;
    q.v = WITH_V ? v_map[pc] * (1.0f / (float)c) : 0.f;
    return q;
}

inline bool sam_args_ok(int c, int H, int W, int h, int w, int n_emb)
{
    return c > 0 && c % 16 == 0 && H > 0 && W > 0 && h > 0 && w > 0 && n_emb > 0;
}
