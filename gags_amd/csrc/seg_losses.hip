// N2: the segment-wise losses of the reference's training loop -- get_trained_seg, the entropy term, the
// per-segment moments and the two losses built on them.  All HBM-bound byte / gather work over [C, H, W] maps: coalesced
// along pixels, small tables (segment statistics) left to L2.  Numerics follow the reference's torch ops (fp32; sums that
// torch does as one big reduction are accumulated in double here).
#include "launch.h"
#include "gags_next.h"
#include "reduce.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------
// get_trained_seg (utils/loss_utils.py:138-154)
// A workgroup = 64 x 4 pixels; the three planes' (64 + 4) x (4 + 4) patches go through LDS once (zero outside the image) and
// every pixel adds its 25 taps in the order of the direct form (rows, then columns; a zero tap adds exactly nothing): the same
// bits as one bounds-checked global load per tap, 94 -> ~20 us at 1080p (round 6).
constexpr int TSW = 64, TSH = 4;
__global__ __launch_bounds__(256) void trained_seg_kernel(int h, int w, const float *__restrict__ seg_map,
                                                          const float *__restrict__ scale_map, float *__restrict__ out)
{
    __shared__ float patch[3][TSH + 4][TSW + 4];
    const int x0 = blockIdx.x * TSW, y0 = blockIdx.y * TSH;
    for (int i = threadIdx.x; i < 3 * (TSH + 4) * (TSW + 4); i += 256) {
        const int ch = i / ((TSH + 4) * (TSW + 4)), r = i - ch * ((TSH + 4) * (TSW + 4));
        const int py = r / (TSW + 4), px = r - py * (TSW + 4);
        const int yy = y0 + py - 2, xx = x0 + px - 2;
        patch[ch][py][px] = (yy >= 0 && yy < h && xx >= 0 && xx < w) ? scale_map[((size_t)ch * h + yy) * w + xx] : 0.f;
    }
    __syncthreads();
    const int lx = threadIdx.x & (TSW - 1), ly = threadIdx.x / TSW;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= w || y >= h) return;
    float best = 0.f;
    int arg = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float s = 0.f;  // conv2d with a 5x5 kernel of 1/25, zero padding 2
#pragma unroll
        for (int dy = 0; dy < 5; ++dy)
#pragma unroll
            for (int dx = 0; dx < 5; ++dx) s = fmaf(patch[ch][ly + dy][lx + dx], 0.04f, s);
        if (ch == 0 || s > best) { best = s; arg = ch; }  // first maximum wins, as torch.argmax
    }
    out[(size_t)y * w + x] = seg_map[((size_t)(1 + arg) * h + y) * w + x];
}

// ---------------------------------------------------------------------------------------------------------------
// scale_regulation_loss (utils/loss_utils.py:59-66)
__global__ __launch_bounds__(256) void entropy_fwd_kernel(int64_t n, const float *__restrict__ s, double *__restrict__ acc)
{
    __shared__ double sm[4];
    double a = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float v = s[i];
        a += (double)(-v * logf(v + 1e-6f));
    }
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(acc, (sm[0] + sm[1]) + (sm[2] + sm[3]));
}

__global__ __launch_bounds__(256) void entropy_bwd_kernel(int64_t n, const float *__restrict__ s, float v, float *__restrict__ vs)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = s[i];
    vs[i] = -(logf(x + 1e-6f) + x / (x + 1e-6f)) * v;
}

// (the cotangent as a device scalar: no host readback in the middle of a backward pass; the factor is formed as the host
// formed it -- the quotient in double, rounded to float once)
__global__ __launch_bounds__(256) void entropy_bwd_dev_kernel(int64_t n, const float *__restrict__ s, const float *__restrict__ v,
                                                              float *__restrict__ vs)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float f = (float)((double)v[0] / (double)n);
    const float x = s[i];
    vs[i] = -(logf(x + 1e-6f) + x / (x + 1e-6f)) * f;
}

// ---------------------------------------------------------------------------------------------------------------
// per-segment moments.  One wave = 64 consecutive pixels.
// FOUR consecutive pixels per lane (one 16-byte load per channel): on real segment maps (large regions) a wave of 256
// pixels still meets one or two ids, so rounds, wave sums and double atomics are a quarter as many per pixel.  (The
// synthetic map of tools/decoder_bench.py draws a random id per 8x8 block -- 32 ids per wave -- and is bound by the
// rounds' wave sums either way: 0.5 ms per call at 1080p, c = 16.)
__global__ __launch_bounds__(256) void segment_stats_kernel(int64_t n_pix, int c, const float *__restrict__ x,
                                                            const float *__restrict__ seg, int n_seg,
                                                            double *__restrict__ s1, double *__restrict__ s2,
                                                            int32_t *__restrict__ cnt, int vec, int copies, int pm)
{   // pm: x is PIXEL-major [n_pix, c] (the rasterizer's own layout: the [C,H,W] map a loss receives is a permuted view of
    // it, and `.contiguous()` on that view is a 132 MB copy per iteration at 1080p, c = 16); else channel-major [c, n_pix]
    // `copies` private sets of accumulators, picked by workgroup: the double atomics execute at the memory side and
    // serialize per ADDRESS (~0.5 us each) -- with a few hundred segments in the image every address takes ~900 of them
    {
        const size_t cp = blockIdx.x % (unsigned)copies;
        s1 += cp * (size_t)n_seg * c; s2 += cp * (size_t)n_seg * c; cnt += cp * (size_t)n_seg;
    }
    const int64_t p0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const int lane = threadIdx.x & 63;
    int id[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        id[q] = -1;
        if (p0 + q < n_pix) {
            const float f = seg[p0 + q];
            id[q] = (f >= 0.f && f < (float)n_seg) ? (int)f : -1;
        }
    }
    // one round per distinct segment id in the wave: the group's values of a channel are summed in fp32 on the VALU (in
    // the lane, then pairwise over the wave; the sums over many waves are the ones that need doubles) and the leader
    // issues ONE double atomic per moment.  Channels in groups of 8 held in registers: read once.
    for (int cb = 0; cb < c; cb += 8) {
        float xv[8][4];
        if (pm && (c & 7) == 0) {  // (uniform) pixel-major rows of whole 8-channel groups: two 16-byte loads per pixel
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float *px = x + (size_t)min(p0 + q, n_pix - 1) * c + cb;
                const float4 t0 = *reinterpret_cast<const float4 *>(px), t1 = *reinterpret_cast<const float4 *>(px + 4);
                xv[0][q] = t0.x; xv[1][q] = t0.y; xv[2][q] = t0.z; xv[3][q] = t0.w;
                xv[4][q] = t1.x; xv[5][q] = t1.y; xv[6][q] = t1.z; xv[7][q] = t1.w;
            }
        } else
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int ch = min(cb + j, c - 1);
            const float *row = x + (size_t)ch * n_pix;
            if (pm) {  // (a lane walks its pixels' rows channel by channel: every 64-byte line is used up over j)
#pragma unroll
                for (int q = 0; q < 4; ++q) xv[j][q] = x[(size_t)min(p0 + q, n_pix - 1) * c + ch];
            } else if (vec) {  // n_pix % 4 == 0 and a 16-byte aligned base: every row is aligned (uniform)
                const float4 t = *reinterpret_cast<const float4 *>(row + min(p0, n_pix - 4));
                xv[j][0] = t.x; xv[j][1] = t.y; xv[j][2] = t.z; xv[j][3] = t.w;
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) xv[j][q] = row[min(p0 + q, n_pix - 1)];
            }
        }
        unsigned pend = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) pend |= (id[q] >= 0 ? 1u : 0u) << q;
        unsigned long long todo = __ballot(pend != 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int fq = __ffs((int)pend) - 1;  // this lane's first pending pixel (-1: none)
            const int first_id = fq == 0 ? id[0] : fq == 1 ? id[1] : fq == 2 ? id[2] : id[3];
            const int cur = __builtin_amdgcn_readlane(first_id, leader);
            const int lq = __builtin_amdgcn_readlane(fq, leader);
            unsigned in = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) in |= ((pend >> q & 1u) && id[q] == cur ? 1u : 0u) << q;
            int n_in = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) n_in += (int)__popcll(__ballot((in >> q & 1u) != 0));
            if (cb == 0 && lane == leader) atomicAdd(&cnt[cur], n_in);
            const double ng = (double)n_in;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                // moments of the group about one of its OWN values (the leader's first pixel): the fp32 sums then carry the
                // spread, not the mean, and the shift goes back in double -- sum x^2 - (sum x)^2 / n used to cancel in fp32
                // rounding once a region's variance fell below ~1e-7 mean^2, which is where this loss drives it
                const float mine = lq == 0 ? xv[j][0] : lq == 1 ? xv[j][1] : lq == 2 ? xv[j][2] : xv[j][3];
                const float sft = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(mine), leader));
                float v = 0.f, vv = 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const float t = (in >> q & 1u) ? xv[j][q] - sft : 0.f;
                    v += t; vv = fmaf(t, t, vv);
                }
                const float a = gags_wave_sum(v), b = gags_wave_sum(vv);
                if (lane == leader && cb + j < c) {
                    const double sd = (double)sft, ad = (double)a;
                    atomicAdd(&s1[(size_t)cur * c + cb + j], ad + ng * sd);
                    atomicAdd(&s2[(size_t)cur * c + cb + j], (double)b + 2.0 * sd * ad + ng * sd * sd);
                }
            }
            pend &= ~in;
            todo = __ballot(pend != 0);
        }
    }
}

// The same moments by RUNS (round 6): every stream of consecutive pixels keeps the sums of its current run of equal ids in
// registers -- about the run's first value, as above -- and adds a finished run to a table of doubles in LDS; the workgroup's
// table leaves as ONE private copy (plain stores; the copies are summed by the caller like the private accumulator sets of
// the kernel above).  No wave sums and no global atomics at all: the work per pixel does not depend on how finely the map is
// cut (the rounds above cost ~200 VALU instructions per distinct id in a wave: 0.48 ms at 1080p, c = 16, on a map of 8 x 8
// blocks), and large regions flush almost nothing.  CL lanes per pixel: 16 = the sixteen channels of a pixel-major row,
// 1 = a single plane.
template <int CL>
__global__ __launch_bounds__(256) void segment_stats_runs_kernel(int64_t n_pix, const float *__restrict__ x,
                                                                 const float *__restrict__ seg, int n_seg, double *__restrict__ s1,
                                                                 double *__restrict__ s2, int32_t *__restrict__ cnt)
{
    extern __shared__ double seg_tab[];  // s1 [n_seg][CL], s2 [n_seg][CL], counts [n_seg]
    constexpr int NS = 256 / CL, RUN = CL == 16 ? 128 : 32;  // streams per workgroup, pixels per stream and block
    const int tid = threadIdx.x, n_tab = n_seg * CL;
    double *t1 = seg_tab, *t2 = seg_tab + n_tab;
    int *tc = reinterpret_cast<int *>(seg_tab + 2 * (size_t)n_tab);
    for (int i = tid; i < 2 * n_tab; i += 256) seg_tab[i] = 0.0;
    for (int i = tid; i < n_seg; i += 256) tc[i] = 0;
    __syncthreads();
    const int j = tid % CL, stream = tid / CL;
    int cur = -1, n = 0;
    float sft = 0.f, v = 0.f, vv = 0.f;
    auto flush = [&]() {
        if (cur >= 0 && n > 0) {
            const double sd = (double)sft, ad = (double)v, ng = (double)n;
            atomicAdd(&t1[cur * CL + j], ad + ng * sd);
            atomicAdd(&t2[cur * CL + j], (double)vv + 2.0 * sd * ad + ng * sd * sd);
            if (j == 0) atomicAdd(&tc[cur], n);
        }
    };
    auto take = [&](float f, float xv) {
        const int id = (f >= 0.f && f < (float)n_seg) ? (int)f : -1;
        if (id != cur) {
            flush();
            cur = id; n = 0; sft = xv; v = 0.f; vv = 0.f;
        }
        const float t = xv - sft;
        v += t; vv = fmaf(t, t, vv); ++n;
    };
    for (int64_t base = (int64_t)blockIdx.x * (NS * RUN); base < n_pix; base += (int64_t)gridDim.x * (NS * RUN)) {
        int64_t p = base + (int64_t)stream * RUN;
        const int64_t pe = min(p + RUN, n_pix);
        for (; p + 4 <= pe; p += 4) {  // four pixels' loads in flight
            float f[4], xv[4];
            if constexpr (CL == 1) {
                if (((reinterpret_cast<uintptr_t>(x + p) | reinterpret_cast<uintptr_t>(seg + p)) & 15) == 0) {
                    const float4 a = *reinterpret_cast<const float4 *>(x + p), b = *reinterpret_cast<const float4 *>(seg + p);
                    xv[0] = a.x; xv[1] = a.y; xv[2] = a.z; xv[3] = a.w; f[0] = b.x; f[1] = b.y; f[2] = b.z; f[3] = b.w;
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q) { xv[q] = x[p + q]; f[q] = seg[p + q]; }
                }
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) { xv[q] = x[(p + q) * CL + j]; f[q] = seg[p + q]; }
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) take(f[q], xv[q]);
        }
        for (; p < pe; ++p) take(seg[p], x[p * CL + j]);
        flush();
        cur = -1; n = 0;
    }
    __syncthreads();
    s1 += (size_t)blockIdx.x * n_tab; s2 += (size_t)blockIdx.x * n_tab; cnt += (size_t)blockIdx.x * n_seg;
    for (int i = tid; i < n_tab; i += 256) { s1[i] = t1[i]; s2[i] = t2[i]; }
    for (int i = tid; i < n_seg; i += 256) cnt[i] = tc[i];
}

// The two segment losses from the moments, in two launches instead of the ~20 element-wise / reduce launches the same
// arithmetic took as torch expressions on [n_seg] tensors (round 6: ~5 us of GPU time each, back to back on the critical path):
// (1) the private copies summed in copy order: sixteen groups of a workgroup take the copies g, g + 16, ... of 64 consecutive
// elements, their sums are added in group order (reproducible);
__global__ __launch_bounds__(1024) void seg_sum_copies_kernel(int k, int n1, int n_seg, unsigned b1, const double *__restrict__ s1c,
                                                              const double *__restrict__ s2c, const int32_t *__restrict__ cntc,
                                                              double *__restrict__ s1, double *__restrict__ s2,
                                                              int32_t *__restrict__ cnt)
{
    __shared__ double sm[2][16][64];
    const int g = threadIdx.x >> 6, l = threadIdx.x & 63;
    if (blockIdx.x >= b1) {  // counts
        const int e = (int)(blockIdx.x - b1) * 64 + l, ec = min(e, n_seg - 1);
        int t = 0;
        for (int cp = g; cp < k; cp += 16) t += cntc[(size_t)cp * n_seg + ec];
        sm[0][g][l] = (double)t;  // (exact: counts are below 2^31)
        __syncthreads();
        if (g == 0 && e < n_seg) {
            double r = 0.0;
#pragma unroll
            for (int i = 0; i < 16; ++i) r += sm[0][i][l];
            cnt[e] = (int32_t)r;
        }
        return;
    }
    const int e = (int)blockIdx.x * 64 + l, ec = min(e, n1 - 1);
    double a = 0.0, b = 0.0;
    for (int cp = g; cp < k; cp += 16) { a += s1c[(size_t)cp * n1 + ec]; b += s2c[(size_t)cp * n1 + ec]; }
    sm[0][g][l] = a; sm[1][g][l] = b;
    __syncthreads();
    if (g == 0 && e < n1) {
        double ra = 0.0, rb = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) { ra += sm[0][i][l]; rb += sm[1][i][l]; }
        s1[e] = ra; s2[e] = rb;
    }
}

__device__ __forceinline__ double block_sum_1024(double v, double *sm16)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm16[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) r += sm16[i];
    return r;
}

// (2) one workgroup: the loss and the per-segment tables its backward gathers from.
//   mode 0, Scale_balance_loss (utils/loss_utils.py:32-57, mix_seg): mean over the PRESENT segments of the segment's mean;
//           coef[i] = 1 / (n_i K) for the backward (K = present segments, at least 1)
//   mode 1, scale_region_regulation_loss (:103-136): sum over segments of >= 2 pixels of n_i mean_c var_c (unbiased) / (H W);
//           mean[i][c] and coef[i] = 2 n_i / ((n_i - 1) c H W) for the backward
__global__ __launch_bounds__(1024) void seg_loss_finalize_kernel(int mode, int n_seg, int c, double hw, const double *__restrict__ s1,
                                                                 const double *__restrict__ s2, const int32_t *__restrict__ cnt,
                                                                 float *__restrict__ loss, float *__restrict__ coef,
                                                                 float *__restrict__ mean)
{
    __shared__ double sm16[16];
    const int tid = threadIdx.x;
    if (mode == 0) {
        double present = 0.0, msum = 0.0;
        for (int i = tid; i < n_seg; i += 1024) {
            const int n = cnt[i];
            if (n > 0) { present += 1.0; msum += s1[i] / (double)n; }
        }
        const double K = fmax(block_sum_1024(present, sm16), 1.0);
        const double total = block_sum_1024(msum, sm16);
        for (int i = tid; i < n_seg; i += 1024) {
            const int n = cnt[i];
            coef[i] = n > 0 ? (float)(1.0 / ((double)n * K)) : 0.f;
        }
        if (tid == 0) loss[0] = (float)(total / K);
        return;
    }
    double acc = 0.0;
    for (int i = tid; i < n_seg; i += 1024) {
        const int n = cnt[i];
        const bool ok = n >= 2;  // segments of 0 or 1 pixels are skipped (loss_utils.py:124-125)
        const double nn = ok ? (double)n : 2.0;
        double vs = 0.0;
        for (int ch = 0; ch < c; ++ch) {
            const double m = s1[(size_t)i * c + ch] / nn;
            // unbiased, as torch.var; the moments arrive accurately summed in double, and a variance is never negative
            vs += fmax((s2[(size_t)i * c + ch] - nn * m * m) / (nn - 1.0), 0.0);
            mean[(size_t)i * c + ch] = (float)m;
        }
        if (ok) acc += nn * (vs / (double)c);
        coef[i] = ok ? (float)(2.0 * nn / ((nn - 1.0) * (double)c * hw)) : 0.f;
    }
    const double total = block_sum_1024(acc, sm16);
    if (tid == 0) loss[0] = (float)(total / hw);
}

// pixel-major [n_pix, c], c % 4 == 0: one lane per float4, consecutive lanes on consecutive 16 bytes of the tensor
__global__ __launch_bounds__(256) void region_var_bwd_pm_kernel(int64_t n_pix, int c, const float *__restrict__ x,
                                                                const float *__restrict__ seg, int n_seg,
                                                                const float *__restrict__ mean, const float *__restrict__ coef,
                                                                float *__restrict__ vx, const float *__restrict__ add)
{
    const int q4 = c >> 2;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_pix * q4) return;
    const int64_t p = t / q4;
    const int ch = (int)(t - p * q4) * 4;
    const float f = seg[p];
    const int id = (f >= 0.f && f < (float)n_seg) ? (int)f : -1;
    const float4 xv = *reinterpret_cast<const float4 *>(x + (size_t)p * c + ch);
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    if (id >= 0) {
        const float k = coef[id];
        const float4 mv = *reinterpret_cast<const float4 *>(mean + (size_t)id * c + ch);
        o = make_float4(k * (xv.x - mv.x), k * (xv.y - mv.y), k * (xv.z - mv.z), k * (xv.w - mv.w));
    }
    if (add) {  // another consumer's gradient of the same map, added here instead of by a separate pass over both tensors
        const float4 g = *reinterpret_cast<const float4 *>(add + (size_t)p * c + ch);
        o = make_float4(o.x + g.x, o.y + g.y, o.z + g.z, o.w + g.w);
    }
    *reinterpret_cast<float4 *>(vx + (size_t)p * c + ch) = o;
}

__global__ __launch_bounds__(256) void region_var_bwd_kernel(int64_t n_pix, int c, const float *__restrict__ x,
                                                             const float *__restrict__ seg, int n_seg,
                                                             const float *__restrict__ mean, const float *__restrict__ coef,
                                                             float *__restrict__ vx, int pm)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pix) return;
    const float f = seg[p];
    const int id = (f >= 0.f && f < (float)n_seg) ? (int)f : -1;
    const float k = id >= 0 ? coef[id] : 0.f;
    for (int ch = 0; ch < c; ++ch) {
        const size_t o = pm ? (size_t)p * c + ch : (size_t)ch * n_pix + p;  // pixel-major [n_pix, c] or channel-major
        vx[o] = id >= 0 ? k * (x[o] - mean[(size_t)id * c + ch]) : 0.f;
    }
}

__global__ __launch_bounds__(256) void gather_seg_coef_kernel(int64_t n_pix, const float *__restrict__ seg, int n_seg,
                                                              const float *__restrict__ coef, float *__restrict__ out)
{
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pix) return;
    const float f = seg[p];
    out[p] = (f >= 0.f && f < (float)n_seg) ? coef[(int)f] : 0.f;
}

inline unsigned nblk(int64_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" int gags_trained_seg(int h, int w, const float *seg_map, const float *scale_map, float *out, void *stream)
{
    GAGS_CLEAR_ERR();
    if (h <= 0 || w <= 0 || !seg_map || !scale_map || !out) return GAGS_EINVAL;
    hipLaunchKernelGGL(trained_seg_kernel, dim3((unsigned)((w + TSW - 1) / TSW), (unsigned)((h + TSH - 1) / TSH)), dim3(256), 0,
                       (hipStream_t)stream, h, w, seg_map, scale_map, out);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_entropy_fwd(int64_t n, const float *s, double *acc, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n < 0 || !acc || (n > 0 && !s)) return GAGS_EINVAL;
    if (n == 0) return GAGS_OK;
    const unsigned grid = (unsigned)(nblk(n) < 2048u ? nblk(n) : 2048u);
    hipLaunchKernelGGL(entropy_fwd_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, n, s, acc);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_entropy_bwd(int64_t n, const float *s, float v_over_n, float *v_s, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n < 0 || (n > 0 && (!s || !v_s))) return GAGS_EINVAL;
    if (n == 0) return GAGS_OK;
    hipLaunchKernelGGL(entropy_bwd_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, n, s, v_over_n, v_s);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_entropy_bwd_dev(int64_t n, const float *s, const float *v, float *v_s, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n < 0 || (n > 0 && (!s || !v || !v_s))) return GAGS_EINVAL;
    if (n == 0) return GAGS_OK;
    hipLaunchKernelGGL(entropy_bwd_dev_kernel, dim3(nblk(n)), dim3(256), 0, (hipStream_t)stream, n, s, v, v_s);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_segment_stats_multi(int64_t n_pix, int c, const float *x, const float *seg, int n_seg, int copies,
                                        double *s1, double *s2, int32_t *cnt, int layout, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_pix < 0 || c <= 0 || n_seg <= 0 || copies <= 0 || !s1 || !s2 || !cnt || (n_pix > 0 && (!x || !seg)) ||
        (layout != 0 && layout != 1))
        return GAGS_EINVAL;
    if (n_pix == 0) return GAGS_OK;
    const int vec = (n_pix % 4 == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) ? 1 : 0;
    hipLaunchKernelGGL(segment_stats_kernel, dim3(nblk((n_pix + 3) / 4)), dim3(256), 0, (hipStream_t)stream, n_pix, c, x, seg, n_seg,
                       s1, s2, cnt, vec, copies, layout);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

namespace {
constexpr int64_t RUNS_LDS_MAX = 150 * 1024;
inline int64_t runs_lds_bytes(int c, int n_seg) { return (int64_t)n_seg * c * 16 + (int64_t)n_seg * 4; }
inline bool runs_shape(int c, int n_seg, int layout)
{
    return ((c == 16 && layout == 1) || c == 1) && n_seg > 0 && runs_lds_bytes(c, n_seg) <= RUNS_LDS_MAX;
}
}  // namespace

extern "C" int gags_segment_stats_runs_copies(int64_t n_pix, int c, int n_seg, int layout)
{
    if (n_pix <= 0 || !runs_shape(c, n_seg, layout)) return 0;
    const int64_t per = c == 16 ? 16 * 128 : 256 * 32;
    const int64_t need = (n_pix + per - 1) / per;
    return (int)(need < 512 ? need : 512);
}

extern "C" int gags_segment_stats_runs(int64_t n_pix, int c, const float *x, const float *seg, int n_seg, int copies, double *s1,
                                       double *s2, int32_t *cnt, int layout, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_pix <= 0 || !runs_shape(c, n_seg, layout) || !x || !seg || !s1 || !s2 || !cnt ||
        copies != gags_segment_stats_runs_copies(n_pix, c, n_seg, layout))
        return GAGS_EINVAL;
    const int64_t lds = runs_lds_bytes(c, n_seg);
    static bool raised[GAGS_MAX_DEVICES];  // (dynamic LDS above 64 KB is an opt-in per kernel and device)
    if (!gags_raise_dynamic_lds(raised, {(const void *)segment_stats_runs_kernel<16>, (const void *)segment_stats_runs_kernel<1>},
                                (int)RUNS_LDS_MAX))
        return GAGS_ELAUNCH;
    if (c == 16)
        hipLaunchKernelGGL(segment_stats_runs_kernel<16>, dim3((unsigned)copies), dim3(256), (size_t)lds, (hipStream_t)stream, n_pix, x,
                           seg, n_seg, s1, s2, cnt);
    else
        hipLaunchKernelGGL(segment_stats_runs_kernel<1>, dim3((unsigned)copies), dim3(256), (size_t)lds, (hipStream_t)stream, n_pix, x,
                           seg, n_seg, s1, s2, cnt);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_segment_loss(int mode, int n_seg, int c, int copies, int64_t n_pix, const double *s1c, const double *s2c,
                                 const int32_t *cntc, double *s1, double *s2, int32_t *cnt, float *loss, float *coef, float *mean,
                                 void *stream)
{
    GAGS_CLEAR_ERR();
    if ((mode != 0 && mode != 1) || n_seg <= 0 || c <= 0 || copies <= 0 || n_pix <= 0 || (mode == 0 && c != 1) || !s1c || !s2c ||
        !cntc || !s1 || !s2 || !cnt || !loss || !coef || (mode == 1 && !mean))
        return GAGS_EINVAL;
    const int64_t n1 = (int64_t)n_seg * c;
    if (n1 > (1 << 24)) return GAGS_EINVAL;
    const unsigned b1 = (unsigned)((n1 + 63) / 64), b2 = (unsigned)((n_seg + 63) / 64);
    hipLaunchKernelGGL(seg_sum_copies_kernel, dim3(b1 + b2), dim3(1024), 0, (hipStream_t)stream, copies, (int)n1, n_seg, b1, s1c, s2c,
                       cntc, s1, s2, cnt);
    hipLaunchKernelGGL(seg_loss_finalize_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, mode, n_seg, c, (double)n_pix, s1, s2,
                       cnt, loss, coef, mean);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_segment_stats(int64_t n_pix, int c, const float *x, const float *seg, int n_seg, double *s1, double *s2,
                                  int32_t *cnt, void *stream)
{
    return gags_segment_stats_multi(n_pix, c, x, seg, n_seg, 1, s1, s2, cnt, 0, stream);
}

extern "C" int gags_region_var_bwd_add(int64_t n_pix, int c, const float *x, const float *seg, int n_seg, const float *mean,
                                       const float *coef, const float *add, float *v_x, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_pix < 0 || c <= 0 || (c & 3) != 0 || n_seg <= 0 || (n_pix > 0 && (!x || !seg || !mean || !coef || !add || !v_x)) ||
        ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(v_x) | reinterpret_cast<uintptr_t>(mean) |
          reinterpret_cast<uintptr_t>(add)) & 15) != 0)
        return GAGS_EINVAL;
    if (n_pix == 0) return GAGS_OK;
    hipLaunchKernelGGL(region_var_bwd_pm_kernel, dim3(nblk(n_pix * (c >> 2))), dim3(256), 0, (hipStream_t)stream, n_pix, c, x, seg, n_seg,
                       mean, coef, v_x, add);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_region_var_bwd_layout(int64_t n_pix, int c, const float *x, const float *seg, int n_seg, const float *mean,
                                          const float *coef, float *v_x, int layout, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_pix < 0 || c <= 0 || n_seg <= 0 || (n_pix > 0 && (!x || !seg || !mean || !coef || !v_x)) || (layout != 0 && layout != 1))
        return GAGS_EINVAL;
    if (n_pix == 0) return GAGS_OK;
    if (layout == 1 && (c & 3) == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(v_x) | reinterpret_cast<uintptr_t>(mean)) & 15) == 0)
        hipLaunchKernelGGL(region_var_bwd_pm_kernel, dim3(nblk(n_pix * (c >> 2))), dim3(256), 0, (hipStream_t)stream, n_pix, c, x, seg,
                           n_seg, mean, coef, v_x, (const float *)nullptr);
    else
        hipLaunchKernelGGL(region_var_bwd_kernel, dim3(nblk(n_pix)), dim3(256), 0, (hipStream_t)stream, n_pix, c, x, seg, n_seg,
                           mean, coef, v_x, layout);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_region_var_bwd(int64_t n_pix, int c, const float *x, const float *seg, int n_seg, const float *mean,
                                   const float *coef, float *v_x, void *stream)
{
    return gags_region_var_bwd_layout(n_pix, c, x, seg, n_seg, mean, coef, v_x, 0, stream);
}

extern "C" int gags_gather_seg_coef(int64_t n_pix, const float *seg, int n_seg, const float *coef, float *out, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_pix < 0 || n_seg <= 0 || (n_pix > 0 && (!seg || !coef || !out))) return GAGS_EINVAL;
    if (n_pix == 0) return GAGS_OK;
    hipLaunchKernelGGL(gather_seg_coef_kernel, dim3(nblk(n_pix)), dim3(256), 0, (hipStream_t)stream, n_pix, seg, n_seg, coef,
                       out);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
