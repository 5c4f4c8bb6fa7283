// N8: adaptive density control (include/gags_next.h "N8"; scene/gaussian_model.py:261-264, 321-482 of the reference).
// densify_and_prune is a pure function of per-Gaussian data: one decision kernel, the library's prefix sum on each of four
// flag arrays, a plan (source row and class of every OUTPUT row), ONE gather of every tensor, and a small kernel for the
// split children's positions and scales.  fp32 throughout, no atomics: two runs are bit-identical.
#include <math.h>
#include "launch.h"
#include "gags_next.h"

namespace {

constexpr int DN_THREADS = 256;
constexpr int DN_GATHER_BLOCKS = 4096;  // grid-stride: 16 workgroups per CU

// the activations as project.hip's stored-parameter path evaluates them (bit for bit torch's on this device, DESIGN)
__device__ __forceinline__ float dn_exp(float s) { return expf(s); }
__device__ __forceinline__ float dn_sigmoid(float o) { return 1.0f / (1.0f + expf(-o)); }

inline int dn_blocks(int64_t n) { return (int)((n + DN_THREADS - 1) / DN_THREADS); }

__global__ __launch_bounds__(DN_THREADS) void densify_stats_kernel(int n, const float *__restrict__ v_means2d,
                                                                   const int32_t *__restrict__ radii,
                                                                   const unsigned char *__restrict__ update_filter,
                                                                   const unsigned char *__restrict__ visibility_filter,
                                                                   float half_w, float half_h, float *__restrict__ accum,
                                                                   float *__restrict__ denom, float *__restrict__ max_radii)
{
    const int i = blockIdx.x * DN_THREADS + threadIdx.x;
    if (i >= n) return;
    const int r = radii ? radii[i] : 0;
    if (v_means2d) {
        if (update_filter ? update_filter[i] != 0 : r > 0) {
            const float gx = v_means2d[2 * i] * half_w, gy = v_means2d[2 * i + 1] * half_h;
            accum[i] = accum[i] + sqrtf(gx * gx + gy * gy);
            denom[i] = denom[i] + 1.0f;
        }
    }
    if (max_radii) {
        if (visibility_filter ? visibility_filter[i] != 0 : r > 0) max_radii[i] = fmaxf(max_radii[i], (float)r);
    }
}

__global__ __launch_bounds__(DN_THREADS) void densify_decide_kernel(int n, const float *__restrict__ accum,
                                                                    const float *__restrict__ denom,
                                                                    const float *__restrict__ scaling,
                                                                    const float *__restrict__ opacity, float max_grad,
                                                                    float dense_thr, float min_opacity, float world_thr,
                                                                    float max_screen_size, int use_screen,
                                                                    int32_t *__restrict__ flags)
{
    const int i = blockIdx.x * DN_THREADS + threadIdx.x;
    if (i >= n) return;
    float g = accum[i] / denom[i];
    if (g != g) g = 0.0f;
    const float m = fmaxf(fmaxf(dn_exp(scaling[3 * i]), dn_exp(scaling[3 * i + 1])), dn_exp(scaling[3 * i + 2]));
    const bool clone = fabsf(g) >= max_grad && m <= dense_thr;
    const bool split = g >= max_grad && m > dense_thr;
    const bool faint = dn_sigmoid(opacity[i]) < min_opacity;
    bool prune = faint, prune_child = faint;
    if (use_screen) {
        // max_radii2D was zeroed by the clone step before this test reads it (the reference's behaviour)
        const bool big_vs = 0.0f > max_screen_size;
        prune = prune || big_vs || m > world_thr;
        prune_child = prune_child || big_vs || m / 1.6f > world_thr;
    }
    flags[i] = !split && !prune;
    flags[(int64_t)n + i] = clone && !prune;
    flags[2 * (int64_t)n + i] = split;
    flags[3 * (int64_t)n + i] = split && !prune_child;
}

// flags / cum: [4, n] (keep, clone, split-selected, children survive) and their inclusive prefix sums; totals: the four sums
__global__ __launch_bounds__(DN_THREADS) void densify_plan_kernel(int n, const int32_t *__restrict__ flags,
                                                                  const int32_t *__restrict__ cum,
                                                                  const int32_t *__restrict__ totals, int64_t n_out,
                                                                  int32_t *__restrict__ src, unsigned char *__restrict__ kind,
                                                                  int32_t *__restrict__ zrow)
{
    const int i = blockIdx.x * DN_THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t tk = totals[0], tc = totals[1], ts = totals[2], th = totals[3];
    const int64_t N = n;
    if (flags[i]) {
        const int64_t j = (int64_t)cum[i] - 1;
        if (j >= 0 && j < n_out) { src[j] = i; kind[j] = 0; zrow[j] = -1; }
    }
    if (flags[N + i]) {
        const int64_t j = tk + cum[N + i] - 1;
        if (j >= 0 && j < n_out) { src[j] = i; kind[j] = 1; zrow[j] = -1; }
    }
    if (flags[3 * N + i]) {
        const int64_t rank = (int64_t)cum[2 * N + i] - 1;  // among the split-selected, before pruning
        const int64_t ja = tk + tc + cum[3 * N + i] - 1, jb = ja + th;
        if (ja >= 0 && ja < n_out) { src[ja] = i; kind[ja] = 2; zrow[ja] = (int32_t)rank; }
        if (jb >= 0 && jb < n_out) { src[jb] = i; kind[jb] = 3; zrow[jb] = (int32_t)(rank + ts); }
    }
}

struct GatherItem {
    const float *in;
    float *out;
    int32_t row;   // elements per row: floats, or float4s when vec
    int32_t flags; // bit 0: moment (zero unless kind == keep); bit 1: 16-byte lanes
};
struct GatherTable {
    GatherItem t[GAGS_GATHER_MAX_DESC];
};

// blockIdx.y = tensor.  Lanes cover consecutive elements of consecutive OUTPUT rows (full coalesced stores); the flat element
// index is 64-bit, the (row, column) pair is carried along the grid stride instead of divided out every time.
__global__ __launch_bounds__(DN_THREADS) void densify_gather_kernel(int64_t n_out, const int32_t *__restrict__ src,
                                                                    const unsigned char *__restrict__ kind, GatherTable tab)
{
    const GatherItem it = tab.t[blockIdx.y];
    const int64_t row = it.row;
    const int64_t total = n_out * row;
    const int64_t stride = (int64_t)gridDim.x * DN_THREADS;
    int64_t e = (int64_t)blockIdx.x * DN_THREADS + threadIdx.x;
    if (e >= total) return;
    int64_t j = e / row, c = e - j * row;
    const int64_t dj = stride / row, dc = stride - dj * row;
    const bool moment = it.flags & 1;
    if (it.flags & 2) {
        const float4 *in = (const float4 *)it.in;
        float4 *out = (float4 *)it.out;
        for (; e < total; e += stride) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (!moment || kind[j] == 0) v = in[(int64_t)src[j] * row + c];
            out[e] = v;
            j += dj; c += dc;
            if (c >= row) { c -= row; ++j; }
        }
    } else {
        for (; e < total; e += stride) {
            float v = 0.f;
            if (!moment || kind[j] == 0) v = it.in[(int64_t)src[j] * row + c];
            it.out[e] = v;
            j += dj; c += dc;
            if (c >= row) { c -= row; ++j; }
        }
    }
}

// Operation order of a child row (header N8): norm = sqrt(((w w + x x) + y y) + z z), q = stored / norm (four divisions),
// R as utils/general_utils.py:78-99 writes it, t = exp(s) * z_k per axis, xyz = ((R[r][0] t0 + R[r][1] t1) + R[r][2] t2) + xyz,
// scaling = log(exp(s) / 1.6f).
__global__ __launch_bounds__(DN_THREADS) void densify_children_kernel(int64_t first, int64_t n_out, int n_src, int64_t n_z,
                                                                      const int32_t *__restrict__ src,
                                                                      const int32_t *__restrict__ zrow,
                                                                      const float *__restrict__ xyz_in,
                                                                      const float *__restrict__ scaling_in,
                                                                      const float *__restrict__ rotation_in,
                                                                      const float *__restrict__ z, float *__restrict__ xyz_out,
                                                                      float *__restrict__ scaling_out)
{
    const int64_t j = first + (int64_t)blockIdx.x * DN_THREADS + threadIdx.x;
    if (j >= n_out) return;
    const int64_t i = src[j], k = zrow[j];
    if (i < 0 || i >= n_src || k < 0 || k >= n_z) return;
    const float qw0 = rotation_in[4 * i], qx0 = rotation_in[4 * i + 1], qy0 = rotation_in[4 * i + 2], qz0 = rotation_in[4 * i + 3];
    const float norm = sqrtf(((qw0 * qw0 + qx0 * qx0) + qy0 * qy0) + qz0 * qz0);
    const float r = qw0 / norm, x = qx0 / norm, y = qy0 / norm, zq = qz0 / norm;
    const float e0 = dn_exp(scaling_in[3 * i]), e1 = dn_exp(scaling_in[3 * i + 1]), e2 = dn_exp(scaling_in[3 * i + 2]);
    const float t0 = e0 * z[3 * k], t1 = e1 * z[3 * k + 1], t2 = e2 * z[3 * k + 2];
    const float R00 = 1.f - 2.f * (y * y + zq * zq), R01 = 2.f * (x * y - r * zq), R02 = 2.f * (x * zq + r * y);
    const float R10 = 2.f * (x * y + r * zq), R11 = 1.f - 2.f * (x * x + zq * zq), R12 = 2.f * (y * zq - r * x);
    const float R20 = 2.f * (x * zq - r * y), R21 = 2.f * (y * zq + r * x), R22 = 1.f - 2.f * (x * x + y * y);
    xyz_out[3 * j] = ((R00 * t0 + R01 * t1) + R02 * t2) + xyz_in[3 * i];
    xyz_out[3 * j + 1] = ((R10 * t0 + R11 * t1) + R12 * t2) + xyz_in[3 * i + 1];
    xyz_out[3 * j + 2] = ((R20 * t0 + R21 * t1) + R22 * t2) + xyz_in[3 * i + 2];
    scaling_out[3 * j] = logf(e0 / 1.6f);
    scaling_out[3 * j + 1] = logf(e1 / 1.6f);
    scaling_out[3 * j + 2] = logf(e2 / 1.6f);
}

__global__ __launch_bounds__(DN_THREADS) void reset_opacity_kernel(int64_t n, float *__restrict__ opacity,
                                                                   float *__restrict__ exp_avg, float *__restrict__ exp_avg_sq)
{
    const int64_t i = (int64_t)blockIdx.x * DN_THREADS + threadIdx.x;
    if (i >= n) return;
    const float s = dn_sigmoid(opacity[i]);
    const float x = s > 0.01f ? 0.01f : s;  // torch.min: a NaN stays a NaN
    opacity[i] = logf(x / (1.0f - x));
    if (exp_avg) exp_avg[i] = 0.f;
    if (exp_avg_sq) exp_avg_sq[i] = 0.f;
}

}  // namespace

extern "C" {

int gags_densify_stats(int n, const float *v_means2d, const int32_t *radii, const unsigned char *update_filter,
                       const unsigned char *visibility_filter, float half_w, float half_h, float *accum, float *denom,
                       float *max_radii, void *stream)
{
    if (n < 0) return GAGS_EINVAL;
    if (n == 0) return GAGS_OK;
    if (!v_means2d && !max_radii) return GAGS_EINVAL;
    if (v_means2d && (!accum || !denom || (!update_filter && !radii))) return GAGS_EINVAL;
    if (max_radii && !radii) return GAGS_EINVAL;
    GAGS_CLEAR_ERR();
    densify_stats_kernel<<<dn_blocks(n), DN_THREADS, 0, (hipStream_t)stream>>>(n, v_means2d, radii, update_filter,
                                                                                visibility_filter, half_w, half_h, accum,
                                                                                denom, max_radii);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

int gags_densify_decide(int n, const float *accum, const float *denom, const float *scaling, const float *opacity,
                        float max_grad, float dense_thr, float min_opacity, float world_thr, float max_screen_size,
                        int use_screen, int32_t *flags, void *stream)
{
    if (n < 0) return GAGS_EINVAL;
    if (n == 0) return GAGS_OK;
    if (!accum || !denom || !scaling || !opacity || !flags) return GAGS_EINVAL;
    GAGS_CLEAR_ERR();
    densify_decide_kernel<<<dn_blocks(n), DN_THREADS, 0, (hipStream_t)stream>>>(n, accum, denom, scaling, opacity, max_grad,
                                                                                 dense_thr, min_opacity, world_thr,
                                                                                 max_screen_size, use_screen != 0, flags);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

int gags_densify_plan(int n, const int32_t *flags, const int32_t *cum, const int32_t *totals, int64_t n_out, int32_t *src,
                      unsigned char *kind, int32_t *zrow, void *stream)
{
    if (n < 0 || n_out < 0 || n_out >= (1ll << 31)) return GAGS_EINVAL;
    if (n == 0 || n_out == 0) return GAGS_OK;
    if (!flags || !cum || !totals || !src || !kind || !zrow) return GAGS_EINVAL;
    GAGS_CLEAR_ERR();
    densify_plan_kernel<<<dn_blocks(n), DN_THREADS, 0, (hipStream_t)stream>>>(n, flags, cum, totals, n_out, src, kind, zrow);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

int gags_densify_gather(int64_t n_out, const int32_t *src, const unsigned char *kind, int n_desc,
                        const gags_gather_desc *descs_host, void *stream)
{
    if (n_out < 0 || n_out >= (1ll << 31) || n_desc < 0 || n_desc > GAGS_GATHER_MAX_DESC) return GAGS_EINVAL;
    if (n_desc > 0 && !descs_host) return GAGS_EINVAL;
    GatherTable tab = {};
    int64_t most = 0;
    for (int t = 0; t < n_desc; ++t) {
        const gags_gather_desc &d = descs_host[t];
        if (!d.in || !d.out || d.row_floats <= 0) return GAGS_EINVAL;
        if (d.mode != GAGS_GATHER_COPY && d.mode != GAGS_GATHER_MOMENT) return GAGS_EINVAL;
        const bool vec = d.row_floats % 4 == 0 && ((uintptr_t)d.in % 16 == 0) && ((uintptr_t)d.out % 16 == 0);
        tab.t[t].in = d.in;
        tab.t[t].out = d.out;
        tab.t[t].row = vec ? d.row_floats / 4 : d.row_floats;
        tab.t[t].flags = (d.mode == GAGS_GATHER_MOMENT ? 1 : 0) | (vec ? 2 : 0);
        const int64_t total = n_out * tab.t[t].row;
        if (total > most) most = total;
    }
    if (n_out == 0 || n_desc == 0) return GAGS_OK;
    if (!src || !kind) return GAGS_EINVAL;
    GAGS_CLEAR_ERR();
    const int64_t want = (most + DN_THREADS - 1) / DN_THREADS;
    const dim3 grid((unsigned)(want < DN_GATHER_BLOCKS ? want : DN_GATHER_BLOCKS), (unsigned)n_desc);
    densify_gather_kernel<<<grid, DN_THREADS, 0, (hipStream_t)stream>>>(n_out, src, kind, tab);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

int gags_densify_children(int64_t n_out, int64_t first_child, int n_src, const int32_t *src, const int32_t *zrow,
                          const float *xyz_in, const float *scaling_in, const float *rotation_in, const float *z, int64_t n_z,
                          float *xyz_out, float *scaling_out, void *stream)
{
    if (n_out < 0 || n_out >= (1ll << 31) || first_child < 0 || first_child > n_out || n_src < 0 || n_z < 0) return GAGS_EINVAL;
    if (first_child == n_out) return GAGS_OK;
    if (!src || !zrow || !xyz_in || !scaling_in || !rotation_in || !z || !xyz_out || !scaling_out) return GAGS_EINVAL;
    GAGS_CLEAR_ERR();
    densify_children_kernel<<<dn_blocks(n_out - first_child), DN_THREADS, 0, (hipStream_t)stream>>>(
        first_child, n_out, n_src, n_z, src, zrow, xyz_in, scaling_in, rotation_in, z, xyz_out, scaling_out);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

int gags_reset_opacity(int64_t n, float *opacity, float *exp_avg, float *exp_avg_sq, void *stream)
{
    if (n < 0 || n > ((1ll << 31) - 1) * DN_THREADS) return GAGS_EINVAL;  // the block count is an int
    if (n == 0) return GAGS_OK;
    if (!opacity) return GAGS_EINVAL;
    GAGS_CLEAR_ERR();
    reset_opacity_kernel<<<dn_blocks(n), DN_THREADS, 0, (hipStream_t)stream>>>(n, opacity, exp_avg, exp_avg_sq);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

}  // extern "C"
