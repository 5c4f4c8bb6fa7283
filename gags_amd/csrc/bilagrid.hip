// N24: bilateral grid colour correction -- per training image a [12, L, Gh, Gw] grid of 3 x 4 colour transforms,
// sliced per pixel at (column, row, the pixel's own luminance) and applied to the pixel; a total-variation term keeps the
// grids smooth.  Written with torch this is a 5-D grid_sample (whose backward scatters 96 float atomics per pixel into a grid
// of ~100 KB), about ten element-wise passes over [H, W, 3] and six strided passes for the TV term.  The rule is stated in
// include/gags_next.h ("N24") and DESIGN.md 7 "N24"; tests/bilagrid_ref.py is its float64 restatement.
//
// Layout: the image and the cotangent of the output are addressed through element strides (plane, row, column), so the
// [H, W, 3] memory the rasterizer writes and a contiguous [3, H, W] tensor are both read where they lie; the output and v_rgb
// are written as [H, W, 3] memory.
//
// Numerics: a pixel's cell and its three fractions (bg_axis, bg_guide) are formed in double from the integer pixel position and the
// float colour -- the same function in the forward and in both backward kernels, so a weight that is exactly zero in one is
// exactly zero in all -- and rounded to float once; the eight weights, the 3 x 4 transform, its z-slope and every sum are
// fp32 with explicit fmaf.
//
// Slice forward, v_rgb: one thread per pixel.  A workgroup first copies the grid nodes its 256 pixels can touch into LDS,
// node-major (below: "the workgroup's part of the grid in LDS"), and a pixel reads its eight corners' twelve channels as 16-byte
// LDS reads; where that part does not fit (a small image under a large grid) the 96 values come through the cache as 48
// 8-byte loads.  HBM traffic: 12 B in, 12 B out per pixel (v_rgb: 24 B in).
//
// v_grid: a gather, no atomics.  A workgroup owns one xy-node (m, n) and one of S row chunks of the node's support -- the
// pixels whose tent(x - n) tent(y - m) can be non-zero, a box of about (2 W / (Gw - 1)) x (2 H / (Gh - 1)) pixels.  A thread
// keeps all L x 12 sums of its pixels in registers: the tent in z is evaluated for every level l (zero for all but two), so
// the register index is a compile-time constant.  Lanes are added by a shuffle tree, the four waves in order, and the
// workgroup writes its L x 12 values -- zeros when no pixel reached the node -- into slab `chunk` of the scratch; a second
// small kernel adds the S slabs in order.  Every element of v_grid is written exactly once, by plain stores.
//
// TV: one pass over [B, 12, L, Gh, Gw] that leaves three doubles per workgroup (the squared differences along L, Gh, Gw),
// added in a fixed order by one more workgroup, as the photometric loss does; the backward is the closed form (second
// differences), one launch.
#include "common.h"
#include "gags_next.h"

namespace {

constexpr int BG_MAX_L = 16, BG_MAX_G = 64;
constexpr int BG_MAX_CHUNKS = 64, BG_TARGET_WGS = 2048;
constexpr int BG_TV_MAX_BLOCKS = 1024;

struct BgGeom {
    int L, gh, gw, h, w;
};

struct BgView {  // a strided [3, h, w] view
    const float *p;
    int64_t sp, sr, sc;
};

// cell and fraction of pixel centre i of n along an axis of g nodes: x = ((i + 0.5) / n) (g - 1) lies in (0, g - 1)
__device__ __forceinline__ void bg_axis(int i, int n, int g, int &c0, float &f)
{
    const double x = (((double)i + 0.5) / (double)n) * (double)(g - 1);
    int c = (int)x;
    c = c < 0 ? 0 : (c > g - 2 ? g - 2 : c);
    c0 = c;
    f = (float)(x - (double)c);
}

// cell and fraction along z of a colour, and m: 1 where the guide's gradient passes (0 < gray (L - 1) < L - 1), else 0
__device__ __forceinline__ void bg_guide(float r, float g, float b, int L, int &z0, float &fz, float &m)
{
    const double gray = (0.299 * (double)r + 0.587 * (double)g) + 0.114 * (double)b;
    const double top = (double)(L - 1);
    const double zc = fmin(fmax(gray, 0.0), 1.0) * top;  // (a NaN colour lands in cell 0)
    int c = (int)zc;
    c = c < 0 ? 0 : (c > L - 2 ? L - 2 : c);
    z0 = c;
    fz = (float)(zc - (double)c);
    const double zu = gray * top;
    m = (zu > 0.0 && zu < top) ? 1.f : 0.f;
}

// weight of node k for a pixel in cell c0 with fraction f: tent(x - k)
__device__ __forceinline__ float bg_tent(int k, int c0, float f) { return k == c0 ? 1.f - f : (k == c0 + 1 ? f : 0.f); }

__device__ __forceinline__ void bg_load3(const BgView &v, int i, int j, float &a, float &b, float &c)
{
    const float *q = v.p + (int64_t)i * v.sr + (int64_t)j * v.sc;
    a = q[0]; b = q[v.sp]; c = q[2 * v.sp];
}

// A[ch] = sum over the 8 corners of w g, and (SLOPE) D[ch] = sum over the 4 xy-corners of wxy (g[z0 + 1] - g[z0])
template <bool SLOPE>
__device__ __forceinline__ void bg_slice(const BgGeom &G, const float *__restrict__ grid, int x0, int y0, int z0, float fx, float fy,
                                         float fz, float *A, float *D)
{
    const float wx[2] = {1.f - fx, fx}, wy[2] = {1.f - fy, fy}, wz[2] = {1.f - fz, fz};
    const int64_t plane = (int64_t)G.gh * G.gw, chan = plane * G.L;
    const float *g0 = grid + ((int64_t)z0 * G.gh + y0) * G.gw + x0;
#pragma unroll
    for (int ch = 0; ch < 12; ++ch) {
        const float *g = g0 + ch * chan;
        float a = 0.f, d = 0.f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy) {
            // the two x-neighbours of a row are adjacent: one 8-byte load each (4-byte aligned: x0 may be odd)
            float lo2[2], hi2[2];
            __builtin_memcpy(lo2, g + dy * G.gw, 8);
            __builtin_memcpy(hi2, g + plane + dy * G.gw, 8);
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const float wxy = wy[dy] * wx[dx];
                const float lo = lo2[dx], hi = hi2[dx];
                a = fmaf(wz[0] * wxy, lo, a);
                a = fmaf(wz[1] * wxy, hi, a);
                if (SLOPE) d = fmaf(wxy, hi - lo, d);
            }
        }
        A[ch] = a;
        if (SLOPE) D[ch] = d;
    }
}

// ---- the workgroup's part of the grid in LDS ----------------------------------------------------------------------------------
// A workgroup's 256 consecutive pixels lie in a few xy-cells, but their luminances spread over all L levels: read from the
// [12, L, Gh, Gw] grid their 96 values are 24 cache lines per wave and channel pair, and the per-pixel kernels then run at the
// rate the L2 hands lines to the L1.  The workgroup therefore copies the nodes its pixels can touch -- rows ya .. yb + 1,
// columns xa .. xb + 1, every level -- into LDS once, node-major ([ny][nx][L][12]: a corner's twelve channels are three
// 16-byte reads), when they fit BG_TILE_FLOATS; otherwise (a small image under a large grid) every pixel reads the grid itself,
// as bg_slice does.  Both paths add the same terms in the same order: the same bits.
constexpr int BG_TILE_FLOATS = 6144;  // 24 KB: six workgroups per CU

struct BgTile {
    int xa, ya, nx, ny;
    bool staged;
};

// the node box of the pixels [pix0, pix0 + 255] (clipped to the image); cells are monotonic in the pixel index along an axis
__device__ __forceinline__ BgTile bg_tile_box(const BgGeom &G, int64_t pix0)
{
    const int64_t n_pix = (int64_t)G.h * G.w;
    const int64_t pixl = pix0 + 255 < n_pix ? pix0 + 255 : n_pix - 1;
    const int ia = (int)(pix0 / G.w), ib = (int)(pixl / G.w);
    int ya, yb, xa = 0, xb = G.gw - 2;
    float f;
    bg_axis(ia, G.h, G.gh, ya, f);
    bg_axis(ib, G.h, G.gh, yb, f);
    if (ia == ib) {  // (one image row: its columns only)
        bg_axis((int)(pix0 - (int64_t)ia * G.w), G.w, G.gw, xa, f);
        bg_axis((int)(pixl - (int64_t)ia * G.w), G.w, G.gw, xb, f);
    }
    BgTile t;
    t.xa = xa; t.ya = ya; t.nx = xb - xa + 2; t.ny = yb - ya + 2;
    t.staged = t.ny * t.nx * G.L * 12 <= BG_TILE_FLOATS;
    return t;
}

__device__ __forceinline__ void bg_tile_fill(const BgGeom &G, const BgTile &t, const float *__restrict__ grid, float *tile)
{
    const int size = t.ny * t.nx * G.L * 12;
    for (int idx = threadIdx.x; idx < size; idx += 256) {
        const int xx = idx % t.nx;
        int r = idx / t.nx;
        const int yy = r % t.ny;
        r /= t.ny;
        const int l = r % G.L, ch = r / G.L;  // (ch < 12: size = 12 L ny nx)
        tile[((yy * t.nx + xx) * G.L + l) * 12 + ch] = grid[((int64_t)(ch * G.L + l) * G.gh + (t.ya + yy)) * G.gw + (t.xa + xx)];
    }
}

// bg_slice from the tile: (xx, yy) = the pixel's cell relative to the tile's first node
template <bool SLOPE>
__device__ __forceinline__ void bg_slice_tile(const BgGeom &G, const BgTile &t, const float *tile, int xx, int yy, int z0, float fx,
                                              float fy, float fz, float *A, float *D)
{
    const float wx[2] = {1.f - fx, fx}, wy[2] = {1.f - fy, fy}, wz[2] = {1.f - fz, fz};
#pragma unroll
    for (int ch = 0; ch < 12; ++ch) {
        A[ch] = 0.f;
        if (SLOPE) D[ch] = 0.f;
    }
#pragma unroll
    for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
        for (int dx = 0; dx < 2; ++dx) {
            const float wxy = wy[dy] * wx[dx];
            const float w0 = wz[0] * wxy, w1 = wz[1] * wxy;
            const float4 *q = (const float4 *)(tile + (((yy + dy) * t.nx + (xx + dx)) * G.L + z0) * 12);  // (48-byte nodes: aligned)
            float lo[12], hi[12];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const float4 a = q[k], b = q[3 + k];
                lo[4 * k] = a.x; lo[4 * k + 1] = a.y; lo[4 * k + 2] = a.z; lo[4 * k + 3] = a.w;
                hi[4 * k] = b.x; hi[4 * k + 1] = b.y; hi[4 * k + 2] = b.z; hi[4 * k + 3] = b.w;
            }
#pragma unroll
            for (int ch = 0; ch < 12; ++ch) {
                A[ch] = fmaf(w0, lo[ch], A[ch]);
                A[ch] = fmaf(w1, hi[ch], A[ch]);
                if (SLOPE) D[ch] = fmaf(wxy, hi[ch] - lo[ch], D[ch]);
            }
        }
    }
}

__global__ __launch_bounds__(256) void bg_slice_fwd_kernel(BgGeom G, const float *__restrict__ grid, BgView rgb, float *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float tile[BG_TILE_FLOATS];
    const BgTile t = bg_tile_box(G, (int64_t)blockIdx.x * 256);  // (the same for every thread of the workgroup)
    if (t.staged) {
        bg_tile_fill(G, t, grid, tile);
        __syncthreads();
    }
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (int64_t)G.h * G.w) return;
    const int i = (int)(pix / G.w), j = (int)(pix - (int64_t)i * G.w);
    float r, g, b, fx, fy, fz, m, A[12];
    int x0, y0, z0;
    bg_load3(rgb, i, j, r, g, b);
    bg_axis(j, G.w, G.gw, x0, fx);
    bg_axis(i, G.h, G.gh, y0, fy);
    bg_guide(r, g, b, G.L, z0, fz, m);
    if (t.staged) bg_slice_tile<false>(G, t, tile, x0 - t.xa, y0 - t.ya, z0, fx, fy, fz, A, nullptr);
    else bg_slice<false>(G, grid, x0, y0, z0, fx, fy, fz, A, nullptr);
    float *o = out + 3 * pix;
#pragma unroll
    for (int q = 0; q < 3; ++q) o[q] = fmaf(A[4 * q], r, fmaf(A[4 * q + 1], g, fmaf(A[4 * q + 2], b, A[4 * q + 3])));
}

// v_p[c] = sum_r A[r][c] v_out[r] + m (L - 1) w_c sum_ch D[ch] v_out[r(ch)] (p, 1)[c(ch)]
__global__ __launch_bounds__(256) void bg_slice_bwd_rgb_kernel(BgGeom G, const float *__restrict__ grid, BgView rgb, BgView vout,
                                                               float *__restrict__ v_rgb)
{
    __shared__ __attribute__((aligned(16))) float tile[BG_TILE_FLOATS];
    const BgTile t = bg_tile_box(G, (int64_t)blockIdx.x * 256);
    if (t.staged) {
        bg_tile_fill(G, t, grid, tile);
        __syncthreads();
    }
    const int64_t pix = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (pix >= (int64_t)G.h * G.w) return;
    const int i = (int)(pix / G.w), j = (int)(pix - (int64_t)i * G.w);
    float p[4], v[3], fx, fy, fz, m, A[12], D[12];
    int x0, y0, z0;
    bg_load3(rgb, i, j, p[0], p[1], p[2]);
    p[3] = 1.f;
    bg_load3(vout, i, j, v[0], v[1], v[2]);
    bg_axis(j, G.w, G.gw, x0, fx);
    bg_axis(i, G.h, G.gh, y0, fy);
    bg_guide(p[0], p[1], p[2], G.L, z0, fz, m);
    if (t.staged) bg_slice_tile<true>(G, t, tile, x0 - t.xa, y0 - t.ya, z0, fx, fy, fz, A, D);
    else bg_slice<true>(G, grid, x0, y0, z0, fx, fy, fz, A, D);
    float dz = 0.f;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
#pragma unroll
        for (int c = 0; c < 4; ++c) dz = fmaf(D[4 * q + c], v[q] * p[c], dz);
    }
    dz *= m * (float)(G.L - 1);
    const float wc[3] = {0.299f, 0.587f, 0.114f};
    float *o = v_rgb + 3 * pix;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = fmaf(wc[c], dz, fmaf(A[c], v[0], fmaf(A[4 + c], v[1], A[8 + c] * v[2])));
}

// first and one-past-last pixel index along an axis of n pixels and g nodes whose tent about node k can be non-zero, one
// pixel generous on both sides (the weights decide): x_i in (k - 1, k + 1) <=> i + 0.5 in ((k - 1) n / (g - 1), (k + 1) n / (g - 1))
__device__ __forceinline__ void bg_support(int k, int n, int g, int &lo, int &hi)
{
    const double s = (double)n / (double)(g - 1);
    const int a = (int)floor((double)(k - 1) * s) - 1, b = (int)ceil((double)(k + 1) * s) + 1;
    lo = a < 0 ? 0 : a;
    hi = b > n ? n : b;
}

// grid (Gh Gw nodes, S chunks).  slabs [S][12, L, Gh, Gw]
template <int LMAX>
__global__ __launch_bounds__(256) void bg_slice_bwd_grid_kernel(BgGeom G, BgView rgb, BgView vout, float *__restrict__ slabs)
{
    __shared__ float red[4][LMAX * 12];
    const int tid = threadIdx.x, node = blockIdx.x, chunk = blockIdx.y, n_chunks = gridDim.y;
    const int nm = node / G.gw, nn = node - nm * G.gw;
    int j0, j1, i0, i1;
    bg_support(nn, G.w, G.gw, j0, j1);
    bg_support(nm, G.h, G.gh, i0, i1);
    const int per = (i1 - i0 + n_chunks - 1) / n_chunks;
    const int r0 = i0 + chunk * per, r1 = min(i1, r0 + per);
    const int ncols = j1 - j0;
    const int total = (r1 > r0 && ncols > 0) ? (r1 - r0) * ncols : 0;  // (<= h w <= 2^30)
    float acc[LMAX][12];
#pragma unroll
    for (int l = 0; l < LMAX; ++l) {
#pragma unroll
        for (int ch = 0; ch < 12; ++ch) acc[l][ch] = 0.f;
    }
    for (int idx = tid; idx < total; idx += 256) {
        const int ri = idx / ncols;
        const int i = r0 + ri, j = j0 + (idx - ri * ncols);
        int x0, y0, z0;
        float fx, fy, fz, m;
        bg_axis(j, G.w, G.gw, x0, fx);
        bg_axis(i, G.h, G.gh, y0, fy);
        const float wxy = bg_tent(nm, y0, fy) * bg_tent(nn, x0, fx);
        if (wxy == 0.f) continue;  // (outside the support: its values are not even read)
        float p[4], v[3];
        bg_load3(rgb, i, j, p[0], p[1], p[2]);
        p[3] = 1.f;
        bg_load3(vout, i, j, v[0], v[1], v[2]);
        bg_guide(p[0], p[1], p[2], G.L, z0, fz, m);
        float val[12];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
#pragma unroll
            for (int c = 0; c < 4; ++c) val[4 * q + c] = v[q] * p[c];
        }
#pragma unroll
        for (int l = 0; l < LMAX; ++l) {
            const float wgt = bg_tent(l, z0, fz) * wxy;
#pragma unroll
            for (int ch = 0; ch < 12; ++ch) acc[l][ch] = fmaf(wgt, val[ch], acc[l][ch]);
        }
    }
    // lanes by a shuffle tree, then the four waves in order
#pragma unroll
    for (int l = 0; l < LMAX; ++l) {
#pragma unroll
        for (int ch = 0; ch < 12; ++ch) {
            float a = acc[l][ch];
            for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
            if ((tid & 63) == 0) red[tid >> 6][l * 12 + ch] = a;
        }
    }
    __syncthreads();
    if (tid < G.L * 12) {
        const int l = tid / 12, ch = tid - l * 12;
        const float s = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        const int64_t n_el = (int64_t)12 * G.L * G.gh * G.gw;
        slabs[(int64_t)chunk * n_el + ((int64_t)(ch * G.L + l) * G.gh + nm) * G.gw + nn] = s;
    }
}

__global__ __launch_bounds__(256) void bg_slab_sum_kernel(int64_t n_el, int n_slabs, const float *__restrict__ slabs,
                                                          float *__restrict__ v_grid)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_el) return;
    float s = slabs[e];
    for (int k = 1; k < n_slabs; ++k) s += slabs[(int64_t)k * n_el + e];
    v_grid[e] = s;
}

// ---- TV ----------------------------------------------------------------------------------------------------------------------

// block-wide sums of three doubles in a fixed order (lanes by a shuffle tree, then the four waves in order); thread 0 holds them
__device__ __forceinline__ void bg_block_sum3(double &a, double &b, double &c, double (*red)[4])
{
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off, 64); b += __shfl_down(b, off, 64); c += __shfl_down(c, off, 64);
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; red[2][threadIdx.x >> 6] = c; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        b = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
        c = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
    }
}

// partials [gridDim.x][3]: the squared forward differences along L, Gh, Gw of the elements this workgroup strides over
__global__ __launch_bounds__(256) void bg_tv_fwd_kernel(int64_t n_el, int L, int gh, int gw, const float *__restrict__ g,
                                                        double *__restrict__ partials)
{
    __shared__ double red[3][4];
    const int64_t plane = (int64_t)gh * gw;
    double sl = 0.0, sh = 0.0, sw = 0.0;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n_el; e += (int64_t)gridDim.x * 256) {
        const int x = (int)(e % gw), y = (int)((e / gw) % gh), z = (int)((e / plane) % L);
        const double c = (double)g[e];
        if (z + 1 < L) { const double d = (double)g[e + plane] - c; sl = fma(d, d, sl); }
        if (y + 1 < gh) { const double d = (double)g[e + gw] - c; sh = fma(d, d, sh); }
        if (x + 1 < gw) { const double d = (double)g[e + 1] - c; sw = fma(d, d, sw); }
    }
    bg_block_sum3(sl, sh, sw, red);
    if (threadIdx.x == 0) {
        double *p = partials + 3 * (int64_t)blockIdx.x;
        p[0] = sl; p[1] = sh; p[2] = sw;
    }
}

// one workgroup: thread t adds partials t, t + 256, ...; thread 0 adds the 256 runs in thread order
__global__ __launch_bounds__(256) void bg_tv_sum_kernel(int n_partials, const double *__restrict__ partials, double kl, double kh,
                                                        double kw, float *__restrict__ out)
{
    __shared__ double run[3][256];
    const int tid = threadIdx.x;
    double a[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < n_partials; i += 256) { a[0] += partials[3 * i]; a[1] += partials[3 * i + 1]; a[2] += partials[3 * i + 2]; }
    run[0][tid] = a[0]; run[1][tid] = a[1]; run[2][tid] = a[2];
    __syncthreads();
    if (tid == 0) {
        double s[3] = {0.0, 0.0, 0.0};
        for (int t = 0; t < 256; ++t) { s[0] += run[0][t]; s[1] += run[1][t]; s[2] += run[2][t]; }
        out[0] = (float)((kl * s[0] + kh * s[1]) + kw * s[2]);
    }
}

// v_g = v sum_d k_d ((g - g[-1_d]) - (g[+1_d] - g)), a term absent where the neighbour is
__global__ __launch_bounds__(256) void bg_tv_bwd_kernel(int64_t n_el, int L, int gh, int gw, const float *__restrict__ g,
                                                        const float *__restrict__ v, double kl, double kh, double kw,
                                                        float *__restrict__ v_g)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n_el) return;
    const int64_t plane = (int64_t)gh * gw;
    const int x = (int)(e % gw), y = (int)((e / gw) % gh), z = (int)((e / plane) % L);
    const double c = (double)g[e];
    double dl = 0.0, dh = 0.0, dw = 0.0;
    if (z > 0) dl += c - (double)g[e - plane];
    if (z + 1 < L) dl -= (double)g[e + plane] - c;
    if (y > 0) dh += c - (double)g[e - gw];
    if (y + 1 < gh) dh -= (double)g[e + gw] - c;
    if (x > 0) dw += c - (double)g[e - 1];
    if (x + 1 < gw) dw -= (double)g[e + 1] - c;
    v_g[e] = (float)((double)v[0] * ((kl * dl + kh * dh) + kw * dw));
}

inline bool bg_grid_ok(int L, int gh, int gw)
{
    return L >= 2 && L <= BG_MAX_L && gh >= 2 && gh <= BG_MAX_G && gw >= 2 && gw <= BG_MAX_G;
}

inline bool bg_image_ok(int h, int w) { return h >= 1 && w >= 1 && (int64_t)h * w <= ((int64_t)1 << 30); }

inline bool bg_view_ok(const float *p, int64_t sp, int64_t sr, int64_t sc) { return p && sp >= 0 && sr >= 0 && sc >= 0; }

inline int bg_chunks(int gh, int gw)
{
    const int nodes = gh * gw;
    const int s = (BG_TARGET_WGS + nodes - 1) / nodes;
    return s < 1 ? 1 : (s > BG_MAX_CHUNKS ? BG_MAX_CHUNKS : s);
}

inline int64_t bg_tv_blocks(int64_t n_el)
{
    const int64_t b = (n_el + 255) / 256;
    return b > BG_TV_MAX_BLOCKS ? BG_TV_MAX_BLOCKS : b;
}

inline bool bg_tv_ok(int n_images, int L, int gh, int gw) { return n_images >= 1 && n_images <= (1 << 16) && bg_grid_ok(L, gh, gw); }

// the weights k_d = scale / (B n_d) of the three axes, n_d = the differences of one image along d
inline void bg_tv_weights(double scale, int n_images, int L, int gh, int gw, double &kl, double &kh, double &kw)
{
    const double b = (double)n_images;
    kl = scale / (b * (12.0 * (L - 1) * gh * gw));
    kh = scale / (b * (12.0 * L * (gh - 1) * gw));
    kw = scale / (b * (12.0 * L * gh * (gw - 1)));
}

}  // namespace

extern "C" int64_t gags_bilagrid_scratch_bytes(int L, int gh, int gw)
{
    if (!bg_grid_ok(L, gh, gw)) return 0;
    return (int64_t)bg_chunks(gh, gw) * 12 * L * gh * gw * (int64_t)sizeof(float);
}

extern "C" int64_t gags_bilagrid_tv_partials(int n_images, int L, int gh, int gw)
{
    if (!bg_tv_ok(n_images, L, gh, gw)) return 0;
    return bg_tv_blocks((int64_t)n_images * 12 * L * gh * gw);
}

extern "C" int gags_bilagrid_slice_fwd(int L, int gh, int gw, int h, int w, const float *grid, const float *rgb, int64_t sp,
                                       int64_t sr, int64_t sc, float *out, void *stream)
{
    GAGS_CLEAR_ERR();
    if (!bg_grid_ok(L, gh, gw) || !bg_image_ok(h, w) || !grid || !bg_view_ok(rgb, sp, sr, sc) || !out) return GAGS_EINVAL;
    const BgGeom G{L, gh, gw, h, w};
    const unsigned blocks = (unsigned)(((int64_t)h * w + 255) / 256);
    hipLaunchKernelGGL(bg_slice_fwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, G, grid, BgView{rgb, sp, sr, sc}, out);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_bilagrid_slice_bwd(int L, int gh, int gw, int h, int w, const float *grid, const float *rgb, int64_t sp,
                                       int64_t sr, int64_t sc, const float *v_out, int64_t v_sp, int64_t v_sr, int64_t v_sc,
                                       float *v_rgb, float *v_grid, void *scratch, int64_t scratch_bytes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (!bg_grid_ok(L, gh, gw) || !bg_image_ok(h, w) || !grid || !bg_view_ok(rgb, sp, sr, sc) || !bg_view_ok(v_out, v_sp, v_sr, v_sc))
        return GAGS_EINVAL;
    if (!v_rgb && !v_grid) return GAGS_EINVAL;
    if (v_grid && !scratch) return GAGS_EINVAL;
    if (v_grid && scratch_bytes < gags_bilagrid_scratch_bytes(L, gh, gw)) return GAGS_ESCRATCH;
    const BgGeom G{L, gh, gw, h, w};
    const BgView pv{rgb, sp, sr, sc}, vv{v_out, v_sp, v_sr, v_sc};
    hipStream_t s = (hipStream_t)stream;
    if (v_rgb) {
        const unsigned blocks = (unsigned)(((int64_t)h * w + 255) / 256);
        hipLaunchKernelGGL(bg_slice_bwd_rgb_kernel, dim3(blocks), dim3(256), 0, s, G, grid, pv, vv, v_rgb);
        GAGS_CHECK_LAUNCH();
    }
    if (v_grid) {
        const int chunks = bg_chunks(gh, gw);
        const dim3 grd(gh * gw, chunks);
        float *slabs = (float *)scratch;
        if (L <= 4) hipLaunchKernelGGL(bg_slice_bwd_grid_kernel<4>, grd, dim3(256), 0, s, G, pv, vv, slabs);
        else if (L <= 8) hipLaunchKernelGGL(bg_slice_bwd_grid_kernel<8>, grd, dim3(256), 0, s, G, pv, vv, slabs);
        else hipLaunchKernelGGL(bg_slice_bwd_grid_kernel<16>, grd, dim3(256), 0, s, G, pv, vv, slabs);
        GAGS_CHECK_LAUNCH();
        const int64_t n_el = (int64_t)12 * L * gh * gw;
        hipLaunchKernelGGL(bg_slab_sum_kernel, dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, s, n_el, chunks,
                           (const float *)slabs, v_grid);
        GAGS_CHECK_LAUNCH();
    }
    return GAGS_OK;
}

extern "C" int gags_bilagrid_tv_fwd(int n_images, int L, int gh, int gw, const float *grids, double *partials, float *out,
                                    void *stream)
{
    GAGS_CLEAR_ERR();
    if (!bg_tv_ok(n_images, L, gh, gw) || !grids || !partials || !out) return GAGS_EINVAL;
    const int64_t n_el = (int64_t)n_images * 12 * L * gh * gw;
    const int blocks = (int)bg_tv_blocks(n_el);
    double kl, kh, kw;
    bg_tv_weights(2.0, n_images, L, gh, gw, kl, kh, kw);
    hipLaunchKernelGGL(bg_tv_fwd_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, n_el, L, gh, gw, grids, partials);
    GAGS_CHECK_LAUNCH();
    hipLaunchKernelGGL(bg_tv_sum_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, blocks, (const double *)partials, kl, kh, kw, out);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_bilagrid_tv_bwd(int n_images, int L, int gh, int gw, const float *grids, const float *v, float *v_grids,
                                    void *stream)
{
    GAGS_CLEAR_ERR();
    if (!bg_tv_ok(n_images, L, gh, gw) || !grids || !v || !v_grids) return GAGS_EINVAL;
    const int64_t n_el = (int64_t)n_images * 12 * L * gh * gw;
    double kl, kh, kw;
    bg_tv_weights(4.0, n_images, L, gh, gw, kl, kh, kw);
    hipLaunchKernelGGL(bg_tv_bwd_kernel, dim3((unsigned)((n_el + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_el, L, gh, gw,
                       grids, v, kl, kh, kw, v_grids);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
