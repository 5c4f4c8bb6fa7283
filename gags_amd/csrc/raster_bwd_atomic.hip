// K10 colours-only backward on the matrix cores, the single-kernel fallback (the GAD flow consumes only d loss / d colors:
// scene/gaussian_model.py:192-208):     v_colors[g, :] = sum_px w[px, g] * v_out[px, :],  w = alpha*T.
//
// Per wave the cotangent slab of its pixel block x 128 channels lives in VGPRs as MFMA B operands (K = pixel
// pairs, N = channels); A operands are 32-slot weight tiles (rows = slots); a tile costs (pixels/2) K-steps x
// 4 channel tiles of v_mfma_f32_32x32x2_f32 and yields 32 partial gradient rows of 128 channels.
//
// This variant recomputes alpha itself (it needs neither scratch nor the forward's slot counts) and adds its rows to
// v_colors with float atomics -- which are executed at the memory side on a multi-XCD MI355X (TCC_EA0_ATOMIC ==
// TCC_ATOMIC, ~1.2 TB/s measured) while plain stores of the same rows are almost free: the default is the staged path
// without atomics (raster_bwd_rows.hip); this kernel is kept as the fallback.
#include "raster_mfma_common.h"
#include "launch.h"

using namespace gags_mfma;

namespace {

constexpr int NBB = 4;         // channel tiles per wave
constexpr int CSB = 32 * NBB;  // 128 channels per wave

__device__ __forceinline__ void atomic_add_f32(float *p, float v)
{
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// cotangent slab as B operands: V[s][j] = v_out[pixel q = 2s+k][ch0 + 32j + p]
__device__ __forceinline__ void load_slab(float (&V)[16][NBB], const float *__restrict__ v_out, const BlockGeom &g,
                                          int width, int height, int d, int ch0)
{
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int q = 2 * s + g.k;
        const int qj = g.bx0 + (q & 7), qi = g.by0 + (q >> 3);
        const bool ok = (qi < height) && (qj < width);
        const float *src = v_out + ((size_t)(ok ? qi : 0) * width + (ok ? qj : 0)) * d + ch0 + g.p;
#pragma unroll
        for (int j = 0; j < NBB; ++j) V[s][j] = ok ? src[32 * j] : 0.f;
    }
}

__device__ __forceinline__ void tile_mfma(f32x16 (&acc)[NBB], const float (&A)[16], const float (&V)[16][NBB])
{
#pragma unroll
    for (int j = 0; j < NBB; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
    for (int s = 0; s < 16; ++s)
#pragma unroll
        for (int j = 0; j < NBB; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[s], V[s][j], acc[j], 0, 0, 0);
}

__global__ __launch_bounds__(64, 2) void raster_bwd_atomic(
    int d, int width, int height, int tile_w, int n_tiles, int n_slices, const GRec *__restrict__ packed,
    const int32_t *__restrict__ offsets, const int32_t *__restrict__ flatten_ids, int n_isects,
    const float *__restrict__ v_render_colors, float *__restrict__ v_colors, int by_gauss)
{
    __shared__ __attribute__((aligned(16))) HRec ring[RING];
    __shared__ __attribute__((aligned(16))) float Wt[32 * WT_STRIDE];
    __shared__ int32_t slot_id[32];

    const int logical = gags_xcd_remap(blockIdx.x, n_tiles * 8 * n_slices);
    const int slice = logical % n_slices, rest = logical / n_slices;
    const int blk = rest & 7;
    const int tile = gags_tile_of_order(rest >> 3, tile_w, n_tiles / tile_w);
    const int ch0 = slice * CSB;
    const int lane = threadIdx.x;
    BlockGeom g;
    g.init(tile, blk, tile_w, width, height, lane);
    const int p = g.p, k = g.k;
    const int start = offsets[tile];
    const int end = offsets[tile + 1]  /* n_tiles + 1 entries: the last one is the intersection count */;

    float V[16][NBB];
    load_slab(V, v_render_colors, g, width, height, d, ch0);

    PixState st;
    st.T = 1.0f; st.cur = 0; st.done = !g.inside;
    HitStream hs;
    hs.by_gauss = by_gauss != 0;
    hs.init(ring, packed, flatten_ids, start, end, lane, g);

    int nh = 0;
    const int wpos = (p & 1) * 16 + (p >> 1);
    auto flush = [&](int count) {
        float A[16];
        const float4 *rowp = reinterpret_cast<const float4 *>(Wt + p * WT_STRIDE + k * 16);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const float4 v = rowp[t];
            A[4 * t] = v.x; A[4 * t + 1] = v.y; A[4 * t + 2] = v.z; A[4 * t + 3] = v.w;
        }
        f32x16 acc[NBB];
        tile_mfma(acc, A, V);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int slot = (r & 3) + 8 * (r >> 2) + 4 * k;
            const int gid = slot_id[slot];
            if (slot < count && gid >= 0) {
                float *dst = v_colors + (size_t)gid * d + ch0 + p;
#pragma unroll
                for (int j = 0; j < NBB; ++j) atomic_add_f32(dst + 32 * j, acc[j][r]);
            }
        }
    };

    hs.refill(6);
    if (!__all(st.done) && hs.rd < hs.nq) {
        bool v_n;
        HRec h_n = hs.at(hs.rd, k, v_n);
        float a_n = eval_alpha(h_n, g.px, g.py, v_n);
        int gid_n = v_n ? h_n.gid : -1;
        bool go = true;
        while (go) {
            const float a_c = a_n;
            const int gid_c = gid_n;
            hs.rd += 2;
            if ((hs.nq - hs.rd) < 6 && hs.pending) hs.refill(6);
            const bool more = hs.rd < hs.nq;
            h_n = hs.at(hs.rd, k, v_n);
            a_n = eval_alpha(h_n, g.px, g.py, v_n);
            gid_n = v_n ? h_n.gid : -1;
            const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(a_c), __float_as_uint(a_c), false, false);
            bool blended;
            const float wgt = step_pair(st, __uint_as_float(sw[0]), __uint_as_float(sw[1]), k, blended);
            if (__any(wgt != 0.f)) {
                Wt[(nh + k) * WT_STRIDE + wpos] = wgt;
                if (p == 0) slot_id[nh + k] = gid_c;
                nh += 2;
                if (nh == 32) { flush(32); nh = 0; }
            }
            go = more && !__all(st.done);
        }
    }
    if (nh > 0) flush(nh);
}

}  // namespace

// 1 = width not eligible (d % 128 != 0)
int gags_raster_bwd_atomic_launch(int d, int width, int height, const void *packed, const int32_t *offsets,
                                  const int32_t *flat, int n_isects, const float *v_out, float *v_colors,
                                  int by_gauss, hipStream_t st)
{
    GAGS_CLEAR_ERR();
    if (d < CSB || d % CSB != 0) return 1;
    const GagsTiles T = gags_tiles(width, height);
    const int n_slices = d / CSB;
    hipLaunchKernelGGL(raster_bwd_atomic, dim3(T.n * 8 * n_slices), dim3(64), 0, st, d, width, height, T.w,
                       T.n, n_slices, reinterpret_cast<const GRec *>(packed), offsets, flat, n_isects, v_out,
                       v_colors, by_gauss);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
