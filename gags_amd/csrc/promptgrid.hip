// N13 (include/gags_next.h): the crop statistics behind SAM's depth-aware prompt grids (preprocess.py:114-149
// build_depth_point_grid, utils/SAM_utils.py:294-353 sample_based_mapping / build_mindepth_point_grid).
//
// An image is cut into n x n crops; every crop needs the sum of its rendered depths, the sum and the number of its
// non-zero depth samples, and the number of non-zero samples in each of its 10 x 10 sub-crops.  The reference does this
// with 64 + 64 means and 6400 torch.sum(crop != 0) calls per image on the host; here it is one segmented reduction over
// [C, H, W] for all cameras at once.
//
// Geometry is INTEGER and comes from the host (gags_amd/prompts.py crop_layout: numpy's float64 linspace cast to int32,
// the reference's own arithmetic): tab = x0[n], y0[n], sx[10], sy[10] in device memory.  The kernel clamps every start
// into the image and every window into its crop, so no table can make it read outside depths / samples.
//
// stats_kernel: one workgroup (4 waves) per (camera, crop, row slab).  Rows go across the waves (two rows per wave in
// flight), columns across the lanes in chunks of 64, so a wave's load is 256 contiguous bytes; crop starts have no
// alignment, so the loads are plain dwords.  Each lane keeps float64 partial sums, and ten integer counters: its non-zero
// samples in each sub-crop ROW band (the row's 10-bit band mask is wave-uniform; a row belongs to at most two bands: the
// windows may overlap by one pixel).  Once per column chunk the lane adds them to the 100 LDS counters of the one or two
// sub-crop COLUMNS its column belongs to, with integer LDS atomics: exact and order-independent.  No floating-point atomic
// anywhere.  (A first version took one ballot per sub-crop column for every row chunk: 2.0 ms for 200 cameras of 1080p
// against 1.34 ms now; docs/LAB_NOTES.md.)
// The lanes meet in a __shfl_xor tree (offsets 32 .. 1), the waves in the order 0, 1, 2, 3.  With one slab the workgroup
// writes the results; otherwise it leaves a partial in scratch and finish_kernel adds the slabs in ascending order.  The
// number of slabs depends on the sizes alone, so equal inputs give equal bits.
#include <algorithm>
#include "common.h"
#include "gags_next.h"
#include "launch.h"

namespace {

constexpr int THREADS = 256, WAVES = 4, SUB = 10, NSUB = SUB * SUB;
constexpr int64_t TARGET_BLOCKS = 2048;  // 8 workgroups for each of the 256 CUs
constexpr int ROWS = 2;                  // rows a wave has in flight (4 measured 6 % slower at 200 x 1080p)
constexpr int MAX_SLABS = 256, MIN_SLAB_ROWS = ROWS * WAVES;

struct Shape {
    int n2, slabs, rows_per_slab;
    int64_t blocks;  // n_cams * n2
};

bool bad_sizes(int n_cams, int h, int w, int n, int crop_w, int crop_h)
{
    return n_cams < 1 || h < 1 || w < 1 || (int64_t)h * w > INT32_MAX || n < 1 || n > 4096 || crop_w < 0 || crop_w > w ||
           crop_h < 0 || crop_h > h || (int64_t)n_cams * n * n > (INT32_MAX / MAX_SLABS);
}

Shape shape(int n_cams, int n, int crop_h)
{
    Shape s;
    s.n2 = n * n;
    s.blocks = (int64_t)n_cams * s.n2;
    int64_t want = std::min<int64_t>((TARGET_BLOCKS + s.blocks - 1) / s.blocks, MAX_SLABS);
    want = std::max<int64_t>(1, std::min<int64_t>(want, crop_h / MIN_SLAB_ROWS));
    s.rows_per_slab = std::max(1, (int)((crop_h + want - 1) / want));
    s.slabs = std::max(1, (crop_h + s.rows_per_slab - 1) / s.rows_per_slab);
    return s;
}

// the per-slab partial sums (base NULL: sizes only); a single slab writes the outputs themselves and needs no scratch
struct Scratch {
    double *dsum, *ssum;
    int *scount, *sub;
    int64_t total;
};

Scratch carve(void *base, const Shape &s)
{
    const int64_t parts = s.blocks * s.slabs;
    GagsCarve c(base);
    Scratch L;
    L.dsum = c.take<double>(parts);
    L.ssum = c.take<double>(parts);
    L.scount = c.take<int>(parts);
    L.sub = c.take<int>(parts * NSUB);
    L.total = s.slabs > 1 ? c.total() : 0;
    return L;
}

// the sub-crop windows [lo, hi) along one axis that hold position p of a crop side `len`, as a 10-bit mask
__device__ __forceinline__ unsigned sub_mask(const int *__restrict__ starts, int len, int p)
{
    const int step = len / SUB, last = max(len - 1, 0);
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < SUB; ++j) {
        const int lo = starts[j], hi = min(last, lo + step);
        m |= (p >= lo && p < hi) ? 1u << j : 0u;
    }
    return m;
}

template <bool HAS_S>
__global__ __launch_bounds__(THREADS) void stats_kernel(int n, int slabs, int rows_per_slab, int h, int w, int crop_w,
                                                        int crop_h, const float *__restrict__ depths,
                                                        const float *__restrict__ samples, const int *__restrict__ tab,
                                                        double *__restrict__ dsum_out, int *__restrict__ dcount_out,
                                                        double *__restrict__ ssum_out, int *__restrict__ scount_out,
                                                        int *__restrict__ sub_out)
{
    __shared__ int cnt[NSUB];
    __shared__ double red_d[WAVES], red_s[WAVES];
    __shared__ int red_c[WAVES];
    const int n2 = n * n;
    const int64_t part = blockIdx.x;  // (camera, crop, slab)
    const int slab = (int)(part % slabs);
    const int64_t ck = part / slabs;
    const int k = (int)(ck % n2);
    const int64_t cam = ck / n2;
    const int x0 = min(max(tab[k / n], 0), w), y0 = min(max(tab[n + k % n], 0), h);
    const int wc = min(crop_w, w - x0), hc = min(crop_h, h - y0);
    const int r_begin = slab * rows_per_slab, r_end = min(r_begin + rows_per_slab, hc);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    int sx[SUB], sy[SUB];  // (wave-uniform: scalar registers)
#pragma unroll
    for (int j = 0; j < SUB; ++j) {
        sx[j] = tab[2 * n + j];
        sy[j] = tab[2 * n + SUB + j];
    }

    if (HAS_S) {
        if (threadIdx.x < NSUB) cnt[threadIdx.x] = 0;
        __syncthreads();
    }
    const int64_t base = (cam * h + y0) * (int64_t)w + x0;
    const float *dbase = depths + base;
    const float *sbase = HAS_S ? samples + base : nullptr;
    double ds = 0.0, ss = 0.0;
    int sc = 0;

    for (int c0 = 0; c0 < wc; c0 += 64) {
        const int col = c0 + lane;
        const bool inc = col < wc;
        const unsigned colmask = HAS_S && inc ? sub_mask(sx, wc, col) : 0u;
        int band[SUB];  // this lane's non-zero samples in each sub-crop row band, over the wave's rows of this chunk
#pragma unroll
        for (int j = 0; j < SUB; ++j) band[j] = 0;
        for (int r0 = r_begin + wave; r0 < r_end; r0 += ROWS * WAVES) {
            float d[ROWS], s[ROWS];
            bool in[ROWS];
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                const int r = r0 + i * WAVES;
                in[i] = inc && r < r_end;
                const int64_t o = (int64_t)r * w + col;
                d[i] = in[i] ? dbase[o] : 0.f;
                s[i] = HAS_S && in[i] ? sbase[o] : 0.f;
            }
#pragma unroll
            for (int i = 0; i < ROWS; ++i) {
                if (in[i]) ds += (double)d[i];
                if (HAS_S) {
                    const int nz = in[i] && s[i] != 0.f ? 1 : 0;  // NaN != 0: counted, as torch counts it
                    if (nz) ss += (double)s[i];
                    sc += nz;
                    const unsigned rowmask = sub_mask(sy, hc, r0 + i * WAVES);  // (wave-uniform; 0 past the crop)
#pragma unroll
                    for (int j = 0; j < SUB; ++j) band[j] += (rowmask >> j) & 1u ? nz : 0;
                }
            }
        }
        if (HAS_S && colmask) {  // once per chunk: the lane's column belongs to one or two sub-crop columns
            const int jxa = __ffs(colmask) - 1, jxb = __ffs(colmask & (colmask - 1)) - 1;
#pragma unroll
            for (int j = 0; j < SUB; ++j) {
                if (band[j]) {
                    atomicAdd(&cnt[j * SUB + jxa], band[j]);
                    if (jxb >= 0) atomicAdd(&cnt[j * SUB + jxb], band[j]);
                }
            }
        }
    }

    for (int off = 32; off > 0; off >>= 1) {
        ds += __shfl_xor(ds, off, 64);
        if (HAS_S) {
            ss += __shfl_xor(ss, off, 64);
            sc += __shfl_xor(sc, off, 64);
        }
    }
    if (lane == 0) {
        red_d[wave] = ds;
        red_s[wave] = ss;
        red_c[wave] = sc;
    }
    __syncthreads();
    const bool last = slabs == 1;
    const int64_t o = last ? ck : part;
    if (threadIdx.x == 0) {
        dsum_out[o] = ((red_d[0] + red_d[1]) + red_d[2]) + red_d[3];
        if (slab == 0) dcount_out[ck] = hc * wc;
        if (HAS_S) {
            ssum_out[o] = ((red_s[0] + red_s[1]) + red_s[2]) + red_s[3];
            scount_out[o] = red_c[0] + red_c[1] + red_c[2] + red_c[3];
        }
    }
    if (HAS_S && threadIdx.x < NSUB)
        sub_out[o * NSUB + threadIdx.x] = cnt[threadIdx.x];
}

// the slabs of one (camera, crop), added in ascending order: thread 0 the depth sum, 64 the sample sum and count, the
// threads below 100 one sub-crop counter each
__global__ __launch_bounds__(128) void finish_kernel(int slabs, bool has_s, const double *__restrict__ pd,
                                                     const double *__restrict__ ps, const int *__restrict__ pc,
                                                     const int *__restrict__ psub, double *__restrict__ depth_sum,
                                                     double *__restrict__ sample_sum, int *__restrict__ sample_count,
                                                     int *__restrict__ sub_count)
{
    const int64_t ck = blockIdx.x, p0 = ck * slabs;
    const int t = threadIdx.x;
    if (t == 0) {
        double a = 0.0;
        for (int s = 0; s < slabs; ++s) a += pd[p0 + s];
        depth_sum[ck] = a;
    }
    if (!has_s) return;
    if (t == 64) {
        double a = 0.0;
        int cnt = 0;
        for (int s = 0; s < slabs; ++s) {
            a += ps[p0 + s];
            cnt += pc[p0 + s];
        }
        sample_sum[ck] = a;
        sample_count[ck] = cnt;
    }
    if (t < NSUB) {
        int cnt = 0;
        for (int s = 0; s < slabs; ++s) cnt += psub[(p0 + s) * NSUB + t];
        sub_count[ck * NSUB + t] = cnt;
    }
}

}  // namespace

extern "C" int64_t gags_promptgrid_scratch_bytes(int n_cams, int h, int w, int n_per_side, int crop_h)
{
    if (bad_sizes(n_cams, h, w, n_per_side, 0, crop_h)) return 0;
    return carve(nullptr, shape(n_cams, n_per_side, crop_h)).total;
}

extern "C" int gags_promptgrid_stats(int n_cams, int h, int w, int n_per_side, int crop_w, int crop_h, const float *depths,
                                     const float *samples, const int32_t *tab, double *depth_sum, int32_t *depth_count,
                                     double *sample_sum, int32_t *sample_count, int32_t *sub_count, void *scratch,
                                     int64_t scratch_bytes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (bad_sizes(n_cams, h, w, n_per_side, crop_w, crop_h)) return GAGS_EINVAL;
    if (!depths || !tab || !depth_sum || !depth_count) return GAGS_EINVAL;
    if (samples && (!sample_sum || !sample_count || !sub_count)) return GAGS_EINVAL;
    const Shape s = shape(n_cams, n_per_side, crop_h);
    const Scratch L = carve(scratch, s);
    if (L.total > 0 && (!scratch || scratch_bytes < L.total)) return GAGS_ESCRATCH;
    hipStream_t st = (hipStream_t)stream;
    const bool slabbed = s.slabs > 1;
    double *pd = slabbed ? L.dsum : depth_sum;
    double *ps = slabbed ? L.ssum : sample_sum;
    int *pc = slabbed ? L.scount : sample_count;
    int *psub = slabbed ? L.sub : sub_count;
    const dim3 grid((unsigned)(s.blocks * s.slabs));
    if (samples)
        hipLaunchKernelGGL(stats_kernel<true>, grid, dim3(THREADS), 0, st, n_per_side, s.slabs, s.rows_per_slab, h, w, crop_w,
                           crop_h, depths, samples, tab, pd, depth_count, ps, pc, psub);
    else
        hipLaunchKernelGGL(stats_kernel<false>, grid, dim3(THREADS), 0, st, n_per_side, s.slabs, s.rows_per_slab, h, w, crop_w,
                           crop_h, depths, samples, tab, pd, depth_count, ps, pc, psub);
    if (slabbed)
        hipLaunchKernelGGL(finish_kernel, dim3((unsigned)s.blocks), dim3(128), 0, st, s.slabs, samples != nullptr, pd, ps, pc,
                           psub, depth_sum, sample_sum, sample_count, sub_count);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
