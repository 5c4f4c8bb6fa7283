// N11 (include/gags_next.h): the PCA colouring of render.py's feature_visualize_saving (:33-48) without leaving the device.
// A [C, H, W] map comes channel-major (layout 0: element (c, p) at x[c P + p]) or as the pixel-major memory behind a permuted
// view (layout 1: x[p C + c], what the decoders write); both are read as they are.
//
// (a) moments: sum[C] and gram[C, C] of the L2-normalised rows of every third pixel.  A pre-pass writes the sampled rows' norms;
//     the Gram kernel gives a workgroup one 64 x 64 tile of channel pairs (upper-triangle tiles only) and one chunk of
//     ROW_CHUNK sampled rows, stages 32 normalised rows of both channel tiles in LDS and contracts them on the exact-f32 matrix
//     instruction (v_mfma_f32_32x32x2_f32: a 32 x 32 quadrant per wave, one accumulator -- its issue interval equals its
//     latency).  The float accumulator is a sequential chain, whose rounding error grows with its length (4096 rows of
//     all-positive diagonal terms: 5 x the error of a blocked float32 GEMM, measured): every SUB_ROWS rows it is added to a
//     double copy in registers and cleared.  Diagonal tiles also add up their columns (the row sum) in double.  Every workgroup writes its own partial
//     tile; a second kernel sums the chunks in chunk order in float64 and mirrors the lower triangle.  No float atomics: the
//     result does not depend on the order in which workgroups finish.
// (b) project: t[p, k] = sum_c (x^[c] - mean[c]) components[k, c], one wave per pixel (pixel-major: the row stays in
//     registers) or one thread per pixel (channel-major: coalesced along pixels; the second sweep over the channels is served
//     by the caches).
// (c) select: exact order statistics by two 16-bit histogram passes over order-preserving keys (integer atomics: exact,
//     order-independent); no sort.
// (d) colour: clamp((t - sub) / div, 0, 1), optionally also as trunc(255 vis) bytes.
#include <algorithm>
#include "common.h"
#include "gags_next.h"
#include "launch.h"
#include "reduce.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int MT = 64;           // channels per tile side
constexpr int MK = 32;           // sampled rows staged at a time
constexpr int MPITCH = MT + 32;  // LDS row pitch (floats): the two rows one matrix instruction reads sit 32 banks apart
constexpr int ROW_CHUNK = 4096;  // sampled rows per workgroup (a multiple of SUB_ROWS)
constexpr int SUB_ROWS = 256;    // rows per float accumulation chain (a multiple of MK)
constexpr int MAX_C = 1024, MAX_RANKS = 8, BINS = 1 << 16;
constexpr int64_t MAX_PIXELS = 1ll << 26;  // 64 Mpixel: the chunk count stays a legal grid dimension
constexpr float NORM_EPS = 1e-12f;  // F.normalize's eps

__device__ __forceinline__ float wave_sum_xor(float v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// max(||row||, eps) of a pixel-major row by one wave; v[j] = row[64 j + lane] (0 past C) stays with the caller
__device__ __forceinline__ float row_norm_pm(const float *__restrict__ row, int c, int lane, float (&v)[MAX_C / 64])
{
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < MAX_C / 64; ++j) {
        const int ch = 64 * j + lane;
        v[j] = ch < c ? row[ch] : 0.f;
        ss += v[j] * v[j];
    }
    return fmaxf(sqrtf(wave_sum_xor(ss)), NORM_EPS);
}

// the same of pixel p of a channel-major map by one thread
__device__ __forceinline__ float row_norm_cm(const float *__restrict__ x, int64_t n_pix, int64_t p, int c)
{
    float ss = 0.f;
    for (int ch = 0; ch < c; ++ch) {
        const float v = x[(int64_t)ch * n_pix + p];
        ss += v * v;
    }
    return fmaxf(sqrtf(ss), NORM_EPS);
}

// norms of the sampled rows (pixel 3 s): a wave per row (layout 1) or a thread per row (layout 0)
template <int LAYOUT>
__global__ __launch_bounds__(256) void sample_norm_kernel(int c, int64_t n_pix, int64_t n_samp, const float *__restrict__ x,
                                                          float *__restrict__ nrm)
{
    if (LAYOUT == 1) {
        const int lane = threadIdx.x & 63;
        const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
        if (s >= n_samp) return;
        float v[MAX_C / 64];
        const float n = row_norm_pm(x + 3 * s * c, c, lane, v);
        if (lane == 0) nrm[s] = n;
    } else {
        const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (s < n_samp) nrm[s] = row_norm_cm(x, n_pix, 3 * s, c);
    }
}

// tile pair t (0-based, upper triangle, row-major) of an n x n tile grid -> (ti, tj), ti <= tj
__device__ __forceinline__ void tile_of(int t, int n, int &ti, int &tj)
{
    int i = 0;
    while (t >= n - i) {
        t -= n - i;
        ++i;
    }
    ti = i;
    tj = i + t;
}

template <int LAYOUT>
__global__ __launch_bounds__(256) void moments_kernel(int c, int64_t n_pix, int64_t n_samp, const float *__restrict__ x,
                                                      const float *__restrict__ nrm, float *__restrict__ partial,
                                                      double *__restrict__ psum)
{
    __shared__ float A[MK * MPITCH], B[MK * MPITCH];
    int ti, tj;
    tile_of(blockIdx.x, (c + MT - 1) / MT, ti, tj);
    const bool diag = ti == tj;
    const int a0 = ti * MT, b0 = tj * MT;
    const int64_t s_beg = (int64_t)blockIdx.y * ROW_CHUNK;
    const int64_t s_end = s_beg + ROW_CHUNK < n_samp ? s_beg + ROW_CHUNK : n_samp;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1;
    const float *Bs = diag ? A : B;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    double accd[16] = {};
    double csum = 0.0;
    for (int64_t s0 = s_beg; s0 < s_end; s0 += MK) {
        // stage MK normalised rows x MT channels of both tiles; past the chunk or past C: zero
#pragma unroll
        for (int e = tid; e < MK * MT; e += 256) {
            // consecutive threads run along the memory's fast axis: channels (layout 1) or sampled pixels (layout 0)
            const int r = LAYOUT == 1 ? e >> 6 : e & (MK - 1);
            const int cc = LAYOUT == 1 ? e & (MT - 1) : e >> 5;
            const int64_t s = s0 + r;
            const bool ok = s < s_end;
            const float n = ok ? nrm[s] : 1.f;
            const int64_t p = 3 * s;
            float va = 0.f, vb = 0.f;
            if (ok && a0 + cc < c) va = (LAYOUT == 1 ? x[p * c + a0 + cc] : x[(int64_t)(a0 + cc) * n_pix + p]) / n;
            if (!diag && ok && b0 + cc < c) vb = (LAYOUT == 1 ? x[p * c + b0 + cc] : x[(int64_t)(b0 + cc) * n_pix + p]) / n;
            A[r * MPITCH + cc] = va;
            if (!diag) B[r * MPITCH + cc] = vb;
        }
        __syncthreads();
        // A operand: lane l holds x^[row 2 kk + (l >> 5)][channel a0 + 32 wi + (l & 31)], B likewise on the other tile
        const int kr = lane >> 5, col = lane & 31;
#pragma unroll
        for (int kk = 0; kk < MK / 2; ++kk) {
            const float a = A[(2 * kk + kr) * MPITCH + 32 * wi + col];
            const float b = Bs[(2 * kk + kr) * MPITCH + 32 * wj + col];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        if (diag && tid < MT) {
#pragma unroll 8
            for (int r = 0; r < MK; ++r) csum += (double)A[r * MPITCH + tid];
        }
        if ((s0 - s_beg + MK) % SUB_ROWS == 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                accd[r] += (double)acc[r];
                acc[r] = 0.f;
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) accd[r] += (double)acc[r];  // the last, shorter chain (zero when the chunk ended on a boundary)
    // accumulator register r of lane l: row (r & 3) + 8 (r >> 2) + 4 (l >> 5) of the A tile, column l & 31 of the B tile
    float *dst = partial + (int64_t)blockIdx.y * c * c;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int i = a0 + 32 * wi + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        const int j = b0 + 32 * wj + (lane & 31);
        if (i < c && j < c) dst[(int64_t)i * c + j] = (float)accd[r];
    }
    if (diag && tid < MT && a0 + tid < c) psum[(int64_t)blockIdx.y * c + a0 + tid] = csum;
}

// gram[a, b] = sum over chunks (in chunk order, float64) of the partial tiles; tiles below the diagonal are read mirrored
__global__ __launch_bounds__(256) void moments_reduce_kernel(int c, int n_chunks, const float *__restrict__ partial,
                                                             const double *__restrict__ psum, double *__restrict__ gram,
                                                             double *__restrict__ sum)
{
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < c * c) {
        int a = idx / c, b = idx - a * c;
        if (a / MT > b / MT) {
            const int t = a;
            a = b;
            b = t;
        }
        double s = 0.0;
        for (int k = 0; k < n_chunks; ++k) s += (double)partial[((int64_t)k * c + a) * c + b];
        gram[idx] = s;
    } else if (idx < c * c + c) {
        const int ch = idx - c * c;
        double s = 0.0;
        for (int k = 0; k < n_chunks; ++k) s += psum[(int64_t)k * c + ch];
        sum[ch] = s;
    }
}

template <int LAYOUT>
__global__ __launch_bounds__(256) void project_kernel(int c, int64_t n_pix, const float *__restrict__ x,
                                                      const float *__restrict__ mean, const float *__restrict__ comp,
                                                      float *__restrict__ t)
{
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    if (LAYOUT == 1) {
        const int lane = threadIdx.x & 63;
        const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
        if (p >= n_pix) return;  // (a whole wave)
        float v[MAX_C / 64];
        const float n = row_norm_pm(x + p * c, c, lane, v);
#pragma unroll
        for (int j = 0; j < MAX_C / 64; ++j) {
            const int ch = 64 * j + lane;
            if (ch < c) {
                const float dm = v[j] / n - mean[ch];
                d0 = fmaf(dm, comp[ch], d0); d1 = fmaf(dm, comp[c + ch], d1); d2 = fmaf(dm, comp[2 * c + ch], d2);
            }
        }
        d0 = wave_sum_xor(d0); d1 = wave_sum_xor(d1); d2 = wave_sum_xor(d2);
        if (lane == 0) { t[3 * p] = d0; t[3 * p + 1] = d1; t[3 * p + 2] = d2; }
    } else {
        const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
        if (p >= n_pix) return;
        const float n = row_norm_cm(x, n_pix, p, c);
        for (int ch = 0; ch < c; ++ch) {
            const float dm = x[(int64_t)ch * n_pix + p] / n - mean[ch];
            d0 = fmaf(dm, comp[ch], d0); d1 = fmaf(dm, comp[c + ch], d1); d2 = fmaf(dm, comp[2 * c + ch], d2);
        }
        t[3 * p] = d0; t[3 * p + 1] = d1; t[3 * p + 2] = d2;
    }
}

// ---- select ------------------------------------------------------------------------------------------------------------
struct Ranks {
    long long k[MAX_RANKS];
};

// element i of the pooled input: groups of `group` consecutive floats, `stride` floats from one group to the next
__device__ __forceinline__ unsigned pooled_key(const float *__restrict__ v, int64_t i, int64_t group, int64_t stride)
{
    const int64_t g = i / group;
    return gags_f2key(v[g * stride + (i - g * group)]);
}

// pass 0: histogram of the keys' high halves; pass 1: per rank, of the low halves of the keys in that rank's high bin
template <int PASS>
__global__ __launch_bounds__(256) void select_hist_kernel(int64_t n, const float *__restrict__ v, int64_t group, int64_t stride,
                                                          int n_ranks, const unsigned *__restrict__ bin_hi,
                                                          unsigned *__restrict__ hist)
{
    unsigned bins[MAX_RANKS];
    if (PASS == 1) {
#pragma unroll
        for (int j = 0; j < MAX_RANKS; ++j) bins[j] = j < n_ranks ? bin_hi[j] : 0xffffffffu;  // (no high half is that large)
    }
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const unsigned key = pooled_key(v, i, group, stride);
        if (PASS == 0) {
            atomicAdd(hist + (key >> 16), 1u);
        } else {
#pragma unroll
            for (int j = 0; j < MAX_RANKS; ++j)
                if ((key >> 16) == bins[j]) atomicAdd(hist + (size_t)j * BINS + (key & 0xffffu), 1u);
        }
    }
}

// block j: the bin of histogram j (all blocks share one histogram when hist_stride == 0) that holds rank r_j, and r_j's rank
// inside that bin.  dev_ranks given: r_j = dev_ranks[j] and the bin is the low half of the answer: out[j] = the float whose key
// is (bin_hi[j] << 16) | bin.
__global__ __launch_bounds__(1024) void select_locate_kernel(const unsigned *__restrict__ hist, int64_t hist_stride, Ranks host_ranks,
                                                             const long long *__restrict__ dev_ranks, unsigned *__restrict__ bin_out,
                                                             long long *__restrict__ rank_out, const unsigned *__restrict__ bin_hi,
                                                             float *__restrict__ out)
{
    __shared__ unsigned long long part[1024];
    const int j = blockIdx.x, tid = threadIdx.x;
    const unsigned *h = hist + (int64_t)j * hist_stride;
    unsigned long long s = 0;
    for (int b = 0; b < BINS / 1024; ++b) s += h[tid * (BINS / 1024) + b];
    part[tid] = s;
    __syncthreads();
    if (tid != 0) return;
    const unsigned long long r = (unsigned long long)(dev_ranks ? dev_ranks[j] : host_ranks.k[j]);
    unsigned long long cum = 0;
    int q = 0;
    while (q < 1023 && r >= cum + part[q]) cum += part[q++];
    int b = q * (BINS / 1024);
    const int b_last = b + BINS / 1024 - 1;
    while (b < b_last && r >= cum + h[b]) cum += h[b++];
    if (out) {
        out[j] = gags_key2f((bin_hi[j] << 16) | (unsigned)b);
    } else {
        bin_out[j] = (unsigned)b;
        rank_out[j] = (long long)(r - cum);
    }
}

__global__ __launch_bounds__(256) void colour_kernel(int64_t n, const float *__restrict__ t, float sub, float div,
                                                     float *__restrict__ vis, unsigned char *__restrict__ vis_u8)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float v = (t[i] - sub) / div;
    v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);  // torch.clamp: a NaN stays a NaN
    vis[i] = v;
    if (vis_u8) vis_u8[i] = (unsigned char)(int)(v * 255.0f);
}

inline bool featvis_args_ok(int c, int64_t n_pix, int layout)
{
    return c >= 16 && c <= MAX_C && c % 16 == 0 && n_pix >= 1 && n_pix <= MAX_PIXELS && (layout == 0 || layout == 1);
}
inline int64_t samples_of(int64_t n_pix) { return (n_pix + 2) / 3; }
inline int64_t chunks_of(int64_t n_pix) { return (samples_of(n_pix) + ROW_CHUNK - 1) / ROW_CHUNK; }

// (both carves: base NULL = sizes only)
struct MomentsScratch {
    float *nrm, *partial;
    double *psum;
    int64_t total;
};
inline MomentsScratch moments_carve(void *base, int c, int64_t n_pix)
{
    GagsCarve v(base);
    MomentsScratch m;
    const int64_t nch = chunks_of(n_pix);
    m.nrm = v.take<float>(samples_of(n_pix));
    m.partial = v.take<float>(nch * c * c);
    m.psum = v.take<double>(nch * c);
    m.total = v.total();
    return m;
}

struct SelectScratch {
    unsigned *hist, *bin_hi;
    long long *resid;
    int64_t total;
};
inline SelectScratch select_carve(void *base, int n_ranks)
{
    GagsCarve v(base);
    SelectScratch s;
    s.hist = v.take<unsigned>((int64_t)(1 + n_ranks) * BINS);
    s.bin_hi = v.take<unsigned>(MAX_RANKS);
    s.resid = v.take<long long>(MAX_RANKS);
    s.total = v.total();
    return s;
}

}  // namespace

extern "C" int gags_featvis_row_chunk(void) { return ROW_CHUNK; }

extern "C" int64_t gags_featvis_moments_scratch_bytes(int c, int64_t n_pix)
{
    return featvis_args_ok(c, n_pix, 0) ? moments_carve(nullptr, c, n_pix).total : 0;
}

extern "C" int gags_featvis_moments(int c, int64_t n_pix, const float *x, int layout, double *sum, double *gram, void *scratch,
                                    int64_t scratch_bytes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (!featvis_args_ok(c, n_pix, layout) || samples_of(n_pix) < 4 || !x || !sum || !gram || !scratch) return GAGS_EINVAL;
    const MomentsScratch m = moments_carve(scratch, c, n_pix);
    if (scratch_bytes < m.total) return GAGS_ESCRATCH;
    const hipStream_t st = (hipStream_t)stream;
    const int64_t S = samples_of(n_pix);
    const int nch = (int)chunks_of(n_pix), nt = (c + MT - 1) / MT;
    float *nrm = m.nrm, *partial = m.partial;
    double *psum = m.psum;
    const dim3 grid(nt * (nt + 1) / 2, nch);
    if (layout == 1) {
        hipLaunchKernelGGL(sample_norm_kernel<1>, dim3((unsigned)((S + 3) / 4)), dim3(256), 0, st, c, n_pix, S, x, nrm);
        hipLaunchKernelGGL(moments_kernel<1>, grid, dim3(256), 0, st, c, n_pix, S, x, nrm, partial, psum);
    } else {
        hipLaunchKernelGGL(sample_norm_kernel<0>, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, c, n_pix, S, x, nrm);
        hipLaunchKernelGGL(moments_kernel<0>, grid, dim3(256), 0, st, c, n_pix, S, x, nrm, partial, psum);
    }
    hipLaunchKernelGGL(moments_reduce_kernel, dim3((c * c + c + 255) / 256), dim3(256), 0, st, c, nch, partial, psum, gram, sum);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_featvis_project(int c, int64_t n_pix, const float *x, int layout, const float *mean, const float *components,
                                    float *t, void *stream)
{
    GAGS_CLEAR_ERR();
    if (!featvis_args_ok(c, n_pix, layout) || !x || !mean || !components || !t) return GAGS_EINVAL;
    const hipStream_t st = (hipStream_t)stream;
    if (layout == 1)
        hipLaunchKernelGGL(project_kernel<1>, dim3((unsigned)((n_pix + 3) / 4)), dim3(256), 0, st, c, n_pix, x, mean, components, t);
    else
        hipLaunchKernelGGL(project_kernel<0>, dim3((unsigned)((n_pix + 255) / 256)), dim3(256), 0, st, c, n_pix, x, mean, components, t);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int64_t gags_featvis_select_scratch_bytes(int n_ranks)
{
    return n_ranks >= 1 && n_ranks <= MAX_RANKS ? select_carve(nullptr, n_ranks).total : 0;
}

extern "C" int gags_featvis_select(int64_t n, const float *values, int64_t group, int64_t stride, int n_ranks, const int64_t *ranks,
                                   float *out, void *scratch, int64_t scratch_bytes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n < 1 || n >= (1ll << 31) || group < 1 || stride < group || n_ranks < 1 || n_ranks > MAX_RANKS || !values || !ranks || !out ||
        !scratch)
        return GAGS_EINVAL;
    Ranks r = {};
    for (int j = 0; j < n_ranks; ++j) {
        if (ranks[j] < 0 || ranks[j] >= n) return GAGS_EINVAL;
        r.k[j] = ranks[j];
    }
    const SelectScratch s = select_carve(scratch, n_ranks);
    if (scratch_bytes < s.total) return GAGS_ESCRATCH;
    const hipStream_t st = (hipStream_t)stream;
    unsigned *hist = s.hist, *bin_hi = s.bin_hi;
    long long *resid = s.resid;
    if (hipMemsetAsync(hist, 0, (size_t)(1 + n_ranks) * BINS * 4, st) != hipSuccess) return GAGS_ELAUNCH;
    const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(select_hist_kernel<0>, dim3(blocks), dim3(256), 0, st, n, values, group, stride, n_ranks,
                       (const unsigned *)nullptr, hist);
    hipLaunchKernelGGL(select_locate_kernel, dim3(n_ranks), dim3(1024), 0, st, (const unsigned *)hist, (int64_t)0, r,
                       (const long long *)nullptr, bin_hi, resid, (const unsigned *)nullptr, (float *)nullptr);
    hipLaunchKernelGGL(select_hist_kernel<1>, dim3(blocks), dim3(256), 0, st, n, values, group, stride, n_ranks,
                       (const unsigned *)bin_hi, hist + BINS);
    hipLaunchKernelGGL(select_locate_kernel, dim3(n_ranks), dim3(1024), 0, st, (const unsigned *)(hist + BINS), (int64_t)BINS, r,
                       (const long long *)resid, (unsigned *)nullptr, (long long *)nullptr, (const unsigned *)bin_hi, out);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_featvis_colour(int64_t n, const float *t, float sub, float div, float *vis, unsigned char *vis_u8, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n < 1 || !t || !vis) return GAGS_EINVAL;
    hipLaunchKernelGGL(colour_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n, t, sub, div, vis,
                       vis_u8);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
