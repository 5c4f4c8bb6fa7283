// N18: MCMC density control (include/gags_next.h "N18"; DESIGN.md section 7 "N18" declares the rules R1-R6).
// Sampling by binary search of a float64 cdf with integer atomic counts, the relocation rule in float64 over the drawn rows,
// the row copies of a relocation, the per-step position noise (one fp32 thread per Gaussian, one launch) and the two
// regularisers (float64 per element, a fixed-order reduction).  No float atomics: two runs are bit-identical.
#include <math.h>
#include "launch.h"
#include "gags_next.h"

namespace {

constexpr int MC_THREADS = 256;
constexpr int MC_COPY_BLOCKS = 4096;  // grid-stride: 16 workgroups per CU
constexpr int MC_R = GAGS_MCMC_MAX_RATIO;

inline int mc_blocks(int64_t n) { return (int)((n + MC_THREADS - 1) / MC_THREADS); }

// C(m, k) for m, k < 51 by Pascal's rule and 1 / sqrt(k + 1), both at compile time.  The binomials are exact doubles (the
// largest, C(50, 25) = 1.26e14, is below 2^53); the roots come from Newton's iteration and are within an ulp.
struct McTables {
    double binom[MC_R][MC_R];
    double isqrt[MC_R];
};
constexpr McTables mc_make_tables()
{
    McTables t = {};
    for (int m = 0; m < MC_R; ++m) {
        t.binom[m][0] = 1.0;
        for (int k = 1; k <= m; ++k) t.binom[m][k] = t.binom[m - 1][k - 1] + (k < m ? t.binom[m - 1][k] : 0.0);
    }
    for (int k = 0; k < MC_R; ++k) {
        const double a = (double)(k + 1);
        double x = a > 1.0 ? a * 0.5 : 1.0;
        for (int it = 0; it < 64; ++it) x = 0.5 * (x + a / x);
        t.isqrt[k] = 1.0 / x;
    }
    return t;
}
__constant__ const McTables MC_TAB = mc_make_tables();

// the fp32 activations as densify.hip and project.hip's stored-parameter path evaluate them
__device__ __forceinline__ float mc_exp(float s) { return expf(s); }
__device__ __forceinline__ float mc_sigmoid(float o) { return 1.0f / (1.0f + expf(-o)); }

// ---- R2 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_THREADS) void mcmc_sample_kernel(int n, const double *__restrict__ cdf, int n_draws,
                                                                 const double *__restrict__ u, int32_t *__restrict__ draws,
                                                                 int32_t *__restrict__ counts)
{
    const int k = blockIdx.x * MC_THREADS + threadIdx.x;
    if (k >= n_draws) return;
    const double total = cdf[n - 1];
    const double t = u[k] * total;
    int lo = 0, hi = n;  // first j with cdf[j] > t
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (cdf[mid] > t) hi = mid; else lo = mid + 1;
    }
    if (lo >= n) {  // nothing exceeds t: the first j that holds the total
        lo = 0; hi = n - 1;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (cdf[mid] >= total) hi = mid; else lo = mid + 1;
        }
    }
    draws[k] = lo;
    atomicAdd(&counts[lo], 1);
}

// ---- R1 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_THREADS) void mcmc_relocation_kernel(int n, const int32_t *__restrict__ kk, int bias,
                                                                     double min_opacity, float *__restrict__ opacity,
                                                                     float *__restrict__ scaling)
{
    const int i = blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= n) return;
    const int k0 = kk[i];
    if (k0 <= 0) return;
    const int r = min(max(min(k0, MC_R) + bias, 1), MC_R);
    const double top = 1.0 - 0x1p-23;
    const double q = fmax(1.0 / (1.0 + exp((double)opacity[i])), 0x1p-23);
    const double o = 1.0 - q;
    const double o_new = -expm1(log(q) / (double)r);
    if (r > 1) {
        double denom = 0.0;
        for (int a = 1; a <= r; ++a) {
            double p = 1.0, sign = 1.0;
            for (int b = 0; b < a; ++b) {
                p *= o_new;
                denom += MC_TAB.binom[a - 1][b] * sign * p * MC_TAB.isqrt[b];
                sign = -sign;
            }
        }
        const double shift = log(o / denom);
        for (int a = 0; a < 3; ++a) scaling[3 * (int64_t)i + a] = (float)((double)scaling[3 * (int64_t)i + a] + shift);
    }
    const double c = fmin(fmax(o_new, min_opacity), top);
    opacity[i] = (float)log(c / (1.0 - c));
}

// ---- R3 ---------------------------------------------------------------------------------------------------------------
struct CopyItem {
    float *data;
    int32_t row;   // elements per row: floats, or float4s when vec
    int32_t flags; // bit 0: moment (zero the source rows); bit 1: 16-byte lanes
};
struct CopyTable {
    CopyItem t[GAGS_GATHER_MAX_DESC];
};

template <class T>
__device__ __forceinline__ void mc_copy_rows(T *data, int64_t row, bool moment, int64_t n_pairs, const int64_t *dst_rows,
                                             const int32_t *src_rows, int64_t n_rows, T zero)
{
    const int64_t total = n_pairs * row;
    const int64_t stride = (int64_t)gridDim.x * MC_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * MC_THREADS + threadIdx.x; e < total; e += stride) {
        const int64_t p = e / row, c = e - p * row;
        const int64_t s = src_rows[p], d = dst_rows[p];
        if (s < 0 || s >= n_rows || d < 0 || d >= n_rows) continue;
        if (moment) data[s * row + c] = zero;
        else data[d * row + c] = data[s * row + c];
    }
}

// blockIdx.y = tensor; lanes cover consecutive elements of consecutive pairs
__global__ __launch_bounds__(MC_THREADS) void mcmc_copy_rows_kernel(int64_t n_pairs, const int64_t *__restrict__ dst_rows,
                                                                    const int32_t *__restrict__ src_rows, int64_t n_rows,
                                                                    CopyTable tab)
{
    const CopyItem it = tab.t[blockIdx.y];
    if (it.flags & 2)
        mc_copy_rows<float4>((float4 *)it.data, it.row, it.flags & 1, n_pairs, dst_rows, src_rows, n_rows,
                             make_float4(0.f, 0.f, 0.f, 0.f));
    else
        mc_copy_rows<float>(it.data, it.row, it.flags & 1, n_pairs, dst_rows, src_rows, n_rows, 0.f);
}

// ---- R5 ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MC_THREADS) void mcmc_noise_kernel(int n, const float *__restrict__ opacity,
                                                                const float *__restrict__ scaling,
                                                                const float *__restrict__ rotation,
                                                                const float *__restrict__ z, float scaler,
                                                                float *__restrict__ xyz)
{
    const int i = blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= n) return;
    const int64_t i3 = 3 * (int64_t)i;
    const float o = mc_sigmoid(opacity[i]);
    const float gate = 1.0f / (1.0f + expf(-100.0f * ((1.0f - o) - 0.995f)));
    const float4 qs = *(const float4 *)(rotation + 4 * (int64_t)i);
    const float norm = sqrtf(((qs.x * qs.x + qs.y * qs.y) + qs.z * qs.z) + qs.w * qs.w);
    const float r = qs.x / norm, x = qs.y / norm, y = qs.z / norm, zq = qs.w / norm;
    const float e0 = mc_exp(scaling[i3]), e1 = mc_exp(scaling[i3 + 1]), e2 = mc_exp(scaling[i3 + 2]);
    float M[3][3];
    M[0][0] = (1.f - 2.f * (y * y + zq * zq)) * e0; M[0][1] = (2.f * (x * y - r * zq)) * e1; M[0][2] = (2.f * (x * zq + r * y)) * e2;
    M[1][0] = (2.f * (x * y + r * zq)) * e0; M[1][1] = (1.f - 2.f * (x * x + zq * zq)) * e1; M[1][2] = (2.f * (y * zq - r * x)) * e2;
    M[2][0] = (2.f * (x * zq - r * y)) * e0; M[2][1] = (2.f * (y * zq + r * x)) * e1; M[2][2] = (1.f - 2.f * (x * x + y * y)) * e2;
    const float v0 = (z[i3] * gate) * scaler, v1 = (z[i3 + 1] * gate) * scaler, v2 = (z[i3 + 2] * gate) * scaler;
    _Pragma("unroll") for (int a = 0; a < 3; ++a) {
        const float s0 = (M[a][0] * M[0][0] + M[a][1] * M[0][1]) + M[a][2] * M[0][2];
        const float s1 = (M[a][0] * M[1][0] + M[a][1] * M[1][1]) + M[a][2] * M[1][2];
        const float s2 = (M[a][0] * M[2][0] + M[a][1] * M[2][1]) + M[a][2] * M[2][2];
        xyz[i3 + a] = xyz[i3 + a] + ((s0 * v0 + s1 * v1) + s2 * v2);
    }
}

// ---- R6 ---------------------------------------------------------------------------------------------------------------
// float64 sum over the 64 lanes, a fixed butterfly: every lane ends with the same bits
__device__ __forceinline__ double mc_wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ __launch_bounds__(MC_THREADS) void mcmc_reg_fwd_kernel(int n, const float *__restrict__ opacity,
                                                                  const float *__restrict__ scaling, double co, double cs,
                                                                  float *__restrict__ partials)
{
    __shared__ double red[2][4];
    const int i = blockIdx.x * MC_THREADS + threadIdx.x;
    double so = 0.0, ss = 0.0;
    if (i < n) {
        const int64_t i3 = 3 * (int64_t)i;
        so = 1.0 / (1.0 + exp(-(double)opacity[i]));
        ss = (exp((double)scaling[i3]) + exp((double)scaling[i3 + 1])) + exp((double)scaling[i3 + 2]);
    }
    so = mc_wave_sum(so);
    ss = mc_wave_sum(ss);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = so; red[1][threadIdx.x >> 6] = ss; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        const double b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        partials[blockIdx.x] = (float)(co * a + cs * b);
    }
}

__global__ __launch_bounds__(MC_THREADS) void mcmc_reg_bwd_kernel(int n, const float *__restrict__ opacity,
                                                                  const float *__restrict__ scaling, double co, double cs,
                                                                  const float *__restrict__ v_out, float *__restrict__ v_opacity,
                                                                  float *__restrict__ v_scaling)
{
    const int i = blockIdx.x * MC_THREADS + threadIdx.x;
    if (i >= n) return;
    const double g = (double)v_out[0];
    const int64_t i3 = 3 * (int64_t)i;
    const double o = 1.0 / (1.0 + exp(-(double)opacity[i]));
    v_opacity[i] = (float)(g * co * (o * (1.0 - o)));
    for (int a = 0; a < 3; ++a) v_scaling[i3 + a] = (float)(g * cs * exp((double)scaling[i3 + a]));
}

}  // namespace

extern "C" {

int gags_mcmc_sample(int n, const double *cdf, int64_t n_draws, const double *u, int32_t *draws, int32_t *counts, void *stream)
{
    if (n < 0 || n_draws < 0 || n_draws >= (1ll << 31)) return GAGS_EINVAL;
    if (n_draws == 0) return GAGS_OK;
    if (n == 0 || !cdf || !u || !draws || !counts) return GAGS_EINVAL;
    GAGS_CLEAR_ERR();
    mcmc_sample_kernel<<<mc_blocks(n_draws), MC_THREADS, 0, (hipStream_t)stream>>>(n, cdf, (int)n_draws, u, draws, counts);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

int gags_mcmc_relocation(int n, const int32_t *k, int ratio_bias, double min_opacity, float *opacity, float *scaling,
                         void *stream)
{
    if (n < 0 || (ratio_bias != 0 && ratio_bias != 1) || !(min_opacity > 0.0 && min_opacity < 1.0)) return GAGS_EINVAL;
    if (n == 0) return GAGS_OK;
    if (!k || !opacity || !scaling) return GAGS_EINVAL;
    GAGS_CLEAR_ERR();
    mcmc_relocation_kernel<<<mc_blocks(n), MC_THREADS, 0, (hipStream_t)stream>>>(n, k, ratio_bias, min_opacity, opacity,
                                                                                 scaling);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

int gags_mcmc_copy_rows(int64_t n_pairs, const int64_t *dst_rows, const int32_t *src_rows, int n_rows, int n_desc,
                        const gags_gather_desc *descs_host, void *stream)
{
    if (n_pairs < 0 || n_pairs >= (1ll << 31) || n_rows < 0 || n_desc < 0 || n_desc > GAGS_GATHER_MAX_DESC) return GAGS_EINVAL;
    if (n_desc > 0 && !descs_host) return GAGS_EINVAL;
    CopyTable tab = {};
    int64_t most = 0;
    for (int t = 0; t < n_desc; ++t) {
        const gags_gather_desc &d = descs_host[t];
        if (!d.in || d.in != d.out || d.row_floats <= 0) return GAGS_EINVAL;
        if (d.mode != GAGS_GATHER_COPY && d.mode != GAGS_GATHER_MOMENT) return GAGS_EINVAL;
        const bool vec = d.row_floats % 4 == 0 && ((uintptr_t)d.out % 16 == 0);
        tab.t[t].data = d.out;
        tab.t[t].row = vec ? d.row_floats / 4 : d.row_floats;
        tab.t[t].flags = (d.mode == GAGS_GATHER_MOMENT ? 1 : 0) | (vec ? 2 : 0);
        const int64_t total = n_pairs * tab.t[t].row;
        if (total > most) most = total;
    }
    if (n_pairs == 0 || n_desc == 0 || n_rows == 0) return GAGS_OK;
    if (!dst_rows || !src_rows) return GAGS_EINVAL;
    GAGS_CLEAR_ERR();
    const int64_t want = (most + MC_THREADS - 1) / MC_THREADS;
    const dim3 grid((unsigned)(want < MC_COPY_BLOCKS ? want : MC_COPY_BLOCKS), (unsigned)n_desc);
    mcmc_copy_rows_kernel<<<grid, MC_THREADS, 0, (hipStream_t)stream>>>(n_pairs, dst_rows, src_rows, n_rows, tab);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

int gags_mcmc_noise(int n, const float *opacity, const float *scaling, const float *rotation, const float *z, float scaler,
                    float *xyz, void *stream)
{
    if (n < 0 || !isfinite(scaler)) return GAGS_EINVAL;
    if (n == 0) return GAGS_OK;
    if (!opacity || !scaling || !rotation || !z || !xyz) return GAGS_EINVAL;
    GAGS_CLEAR_ERR();
    mcmc_noise_kernel<<<mc_blocks(n), MC_THREADS, 0, (hipStream_t)stream>>>(n, opacity, scaling, rotation, z, scaler, xyz);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

int64_t gags_mcmc_reg_partials(int n) { return n > 0 ? ((int64_t)n + MC_THREADS - 1) / MC_THREADS : 1; }

int gags_mcmc_reg_fwd(int n, const float *opacity, const float *scaling, float opacity_reg, float scale_reg, float *partials,
                      int64_t partials_bytes, float *out, void *stream)
{
    if (n < 0 || !out || !isfinite(opacity_reg) || !isfinite(scale_reg)) return GAGS_EINVAL;
    if (n > 0 && (!opacity || !scaling || !partials)) return GAGS_EINVAL;
    if (n > 0 && partials_bytes < gags_mcmc_reg_partials(n) * (int64_t)sizeof(float)) return GAGS_EINVAL;
    GAGS_CLEAR_ERR();
    if (n == 0) return hipMemsetAsync(out, 0, sizeof(float), (hipStream_t)stream) == hipSuccess ? GAGS_OK : GAGS_ELAUNCH;
    const int rows = mc_blocks(n);
    mcmc_reg_fwd_kernel<<<rows, MC_THREADS, 0, (hipStream_t)stream>>>(n, opacity, scaling, (double)opacity_reg / (double)n,
                                                                      (double)scale_reg / (3.0 * (double)n), partials);
    GAGS_CHECK_LAUNCH();
    return gags_colsum_f32(rows, 1, partials, 1.0f, out, 1, stream);
}

int gags_mcmc_reg_bwd(int n, const float *opacity, const float *scaling, float opacity_reg, float scale_reg, const float *v_out,
                      float *v_opacity, float *v_scaling, void *stream)
{
    if (n < 0 || !isfinite(opacity_reg) || !isfinite(scale_reg)) return GAGS_EINVAL;
    if (n == 0) return GAGS_OK;
    if (!opacity || !scaling || !v_out || !v_opacity || !v_scaling) return GAGS_EINVAL;
    GAGS_CLEAR_ERR();
    mcmc_reg_bwd_kernel<<<mc_blocks(n), MC_THREADS, 0, (hipStream_t)stream>>>(n, opacity, scaling, (double)opacity_reg / (double)n,
                                                                              (double)scale_reg / (3.0 * (double)n), v_out,
                                                                              v_opacity, v_scaling);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

}  // extern "C"
