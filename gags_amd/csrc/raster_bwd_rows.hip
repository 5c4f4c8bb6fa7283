// K10 colours-only backward on the matrix cores, staged (the GAD flow consumes only d loss / d colors:
// scene/gaussian_model.py:192-208):     v_colors[g, :] = sum_px w[px, g] * v_out[px, :],  w = alpha*T.
//
// A tile's weights against its cotangent slab yield partial gradient rows, one per (tile, Gaussian).  What happens to
// those rows is the whole story on this part: float atomics are executed at the memory side on a multi-XCD MI355X
// (TCC_EA0_ATOMIC == TCC_ATOMIC, ~1.2 TB/s measured) while plain stores of the same rows are almost free.  So the
// default ("staged") path has NO atomics and is bit-reproducible:
//   rows    one wave per (tile, 8x8 block, slice of 128 / 64 / 32 channels): weight tile from the forward's
//           scratch (wt), 32 MFMAs per 32 channels, 32 rows stored at fixed addresses (prefix sum of the forward's slot counts);
//   sort    (Gaussian id, row) pairs, radix sort on 32-bit keys; per-Gaussian offsets;
//   reduce  v_colors[g] = sum of its rows, written once (no zero-fill of v_colors needed).
// This file: the rows kernels and the driver of the three stages; sort and reduce: rows_reduce.hip.  The single-kernel
// atomic variant (raster_bwd_atomic.hip) is kept as the fallback.
#include <cstdlib>
#include "raster_mfma_common.h"
#include "launch.h"

using namespace gags_mfma;

namespace {

// ---- staged: rows ------------------------------------------------------------------------------------
// One workgroup per (tile, channel slice); wave b of its four owns the tile's 8x8 pixel block b.  K = the block's 64
// pixels in the order of the weight rows raster_weights wrote (32 (upper, lower) pairs): K-step t pairs element t of
// the row's first half (k = 0) with element t of its second half (k = 1).  The wave's cotangent slab (64 px x 32*NBR
// channels) sits in 32*NBR VGPRs as B operands for the whole tile.
//
// A Gaussian that blends into several blocks of the tile leaves ONE gradient row for the tile, not one per block:
// the tile's rows -- numbered by trow[] = exclusive prefix sum of the forward's hit[] flags, i.e. in sorted order --
// are produced in chunks.  A chunk [r0, r1) ends where a block would need a 33rd slot (its run of slots inside the
// chunk is one 32-row MFMA tile) or after CMAX rows.  Per chunk every wave multiplies its run (the 128-MFMA burst
// of one weight tile), parks the partial rows in LDS, and after a barrier the workgroup adds the up to four partial
// rows of every tile row in a fixed order (block 0..3: bit-reproducible) and stores the merged row once, 128 B
// per lane-quad.  Compared with one row per (block, Gaussian) this halves the rows written, sorted and reduced
// (C3: 4.44 M -> ~2 M rows of 2 KB) for ~10 % more MFMA issue (runs are on average 27 of 32 slots long).
constexpr int CMAX = 64;  // merged rows per chunk (bounds pos[] and the merge loop)

template <int NBR>
__global__ __launch_bounds__(256, (NBR == 4 ? 2 : (NBR == 2 ? 3 : 4))) void raster_bwd_rows(
    int d, int width, int height, int tile_w, int n_tiles, int ch_base, int n_slices,
    const float *__restrict__ v_render_colors, const int32_t *__restrict__ offsets, int n_isects,
    const int32_t *__restrict__ blk_rows, const int32_t *__restrict__ trow, const float *__restrict__ wt,
    const int32_t *__restrict__ gid_s, const int32_t *__restrict__ trow_s, float *__restrict__ prow, int prow_pitch,
    uint32_t *__restrict__ row_key, int32_t *__restrict__ row_idx, int rows_cap)
{
    constexpr int CW = 32 * NBR;  // channels per slice; this launch covers channels ch_base .. ch_base + n_slices * CW - 1 (clipped to d)
    constexpr int C4 = CW / 4;    // float4 columns per row of the slice
    __shared__ __attribute__((aligned(16))) float stage[4][32][CW];  // partial rows of the chunk, per block
    __shared__ __attribute__((aligned(4))) uint8_t pos[2][CMAX][4];  // pos[parity][row - r0][b] = slot of block b's run holding that tile row, 0xff: none (one 32-bit read per row)
    __shared__ int cand[2][4];
    __shared__ __attribute__((aligned(16))) float zrow[CW];  // a row of zeros for the merge

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (threadIdx.x < CW) zrow[threadIdx.x] = 0.f;  // (visible after the first chunk's barrier)
    const int logical = gags_xcd_remap(blockIdx.x, n_tiles * n_slices);
    const int tile = gags_tile_of_order(logical / n_slices, tile_w, n_tiles / tile_w);
    const int start = offsets[tile];
    const int end = offsets[tile + 1]  /* n_tiles + 1 entries: the last one is the intersection count */;
    const int R0 = trow[start], R1 = trow[end];
    if (R1 == R0) return;  // nothing blended in this tile (uniform over the workgroup)
    const int blk = wave;
    const int cnt = blk_rows[tile * GAGS_BLOCKS_PER_TILE + blk];
    const int sb = gags_slot_base(start, end, tile, blk);
    const int ch0 = ch_base + (logical % n_slices) * CW;
    BlockGeom64 g;
    g.init(tile, blk, tile_w, width, height, lane);
    const int p = g.p, k = g.k;

    // V[t][j] = v_out[pixel t of half k][ch0 + NBR*p + j]  ("strided-NBR" channel tiles: one vector load / store)
    float V[32][NBR];
    if (cnt > 0) {
#pragma unroll
        for (int t = 0; t < 32; ++t) {
            // K-step t of half-wave k = pixel 16k + t/2 of the 8x4 half t%2: the order of the weight rows
            const int px = 16 * k + (t >> 1);
            const int qj = g.bx0 + (px & 7), qi = g.by0 + 4 * (t & 1) + (px >> 3);
            const bool ok = (qi < height) && (qj < width);
            // NBR == 1 also serves a ragged last slice (D % 32 != 0): lanes past the row are clamped here, masked below
            const float *src = v_render_colors + ((size_t)min(qi, height - 1) * width + min(qj, width - 1)) * d +
                               (NBR == 1 ? min(ch0 + p, d - 1) : ch0 + NBR * p);
            if constexpr (NBR == 4) {
                const float4 v = *reinterpret_cast<const float4 *>(src);
                V[t][0] = ok ? v.x : 0.f; V[t][1] = ok ? v.y : 0.f; V[t][2] = ok ? v.z : 0.f; V[t][3] = ok ? v.w : 0.f;
            } else if constexpr (NBR == 2) {
                const float2 v = *reinterpret_cast<const float2 *>(src);
                V[t][0] = ok ? v.x : 0.f; V[t][1] = ok ? v.y : 0.f;
            } else {
                const float v = src[0];
                V[t][0] = ok ? v : 0.f;
            }
        }
    } else {
#pragma unroll
        for (int t = 0; t < 32; ++t)
#pragma unroll
            for (int j = 0; j < NBR; ++j) V[t][j] = 0.f;
    }

    int pb = 0;  // slots of this block already consumed
    int r0 = R0;
    // tile rows (and Gaussians) of this block's next 33 slots: sorted, hence increasing; 0x7fffffff past the end and
    // for the pad slot of an odd count.  Always fetched one chunk ahead.
    int tr = 0x7fffffff, gid = 0;
    if (lane <= 32 && lane < cnt) {
        tr = trow_s[sb + lane];
        gid = gid_s[sb + lane];
    }
    // weight tile: slots sb+pb .. +31; lane (i = p, k) owns the 32 floats of half k of row i.  Rows past the run (the
    // next chunk's slots, or memory past the block) only produce accumulator rows nobody stores.  Also requested one
    // chunk ahead: right after the previous burst has consumed the registers.
    float A[32];
    auto load_A = [&](int first) {
        const float4 *src = reinterpret_cast<const float4 *>(wt + (size_t)(sb + first + p) * 64 + k * 32);
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            const float4 v = src[t];
            A[4 * t] = v.x; A[4 * t + 1] = v.y; A[4 * t + 2] = v.z; A[4 * t + 3] = v.w;
        }
    };
    if (cnt > 0) load_A(0);
    for (int it = 0; r0 < R1; ++it) {
        const int par = it & 1;
        if (threadIdx.x < CMAX) reinterpret_cast<uint32_t *>(&pos[par][0][0])[threadIdx.x] = 0xffffffffu;
        const int tr32 = __builtin_amdgcn_readlane(tr, 32);
        if (lane == 0) cand[par][wave] = tr32;
        gags_lds_barrier();  // LDS traffic only: __syncthreads() would also wait for the loads in flight (next chunk's weight tile) and the row stores
        const int r1 = min(min(min(cand[par][0], cand[par][1]), min(cand[par][2], cand[par][3])), min(r0 + CMAX, R1));
        const bool mine = lane < 32 && tr < r1;
        const int run = __popcll(__ballot(mine));  // this block's slots pb .. pb+run-1 fall into [r0, r1)
        const int tr_c = tr, gid_c = gid;
        const int pbn = pb + run;
        if (run > 0) {
            if (mine) pos[par][tr_c - r0][wave] = (uint8_t)lane;
            // The 32*NBR MFMAs of a weight tile are issued as ONE uninterrupted burst: everything they read is waited
            // for up front and nothing else is scheduled into the burst, so that the waves sharing a SIMD alternate
            // (one multiplies while the other loads / merges) instead of stalling and resuming in lock step.
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            f32x16 acc[NBR];
#pragma unroll
            for (int j = 0; j < NBR; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
            for (int t = 0; t < 32; ++t)
#pragma unroll
                for (int j = 0; j < NBR; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(A[t], V[t][j], acc[j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (mine && ch0 == 0 && tr_c < rows_cap) {  // row -> Gaussian map for the sort (every block of the row stores the same pair; the call that covers channel 0 writes it)
                row_key[tr_c] = (uint32_t)gid_c;
                row_idx[tr_c] = tr_c;
            }
            // next chunk's operands: in flight while this chunk is parked and merged
            tr = 0x7fffffff;
            if (lane <= 32 && pbn + lane < cnt) {
                tr = trow_s[sb + pbn + lane];
                gid = gid_s[sb + pbn + lane];
            }
            if (pbn < cnt) load_A(pbn);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int slot = (r & 3) + 8 * (r >> 2) + 4 * k;
                if (slot < run) {
                    float *dst = &stage[wave][slot][NBR * p];
                    if constexpr (NBR == 4) *reinterpret_cast<float4 *>(dst) = make_float4(acc[0][r], acc[1][r], acc[2][r], acc[3][r]);
                    else if constexpr (NBR == 2) *reinterpret_cast<float2 *>(dst) = make_float2(acc[0][r], acc[1][r]);
                    else dst[0] = acc[0][r];
                }
            }
        }
        gags_lds_barrier();  // LDS traffic only: __syncthreads() would also wait for the loads in flight (next chunk's weight tile) and the row stores
        // merged rows of the chunk: sum over the blocks that hold the row, in block order; one float4 per thread and item
        const int items = (r1 - r0) * C4;
        // branch-free, fully unrolled (at most CMAX * C4 / 256 trips): see raster_bwd_rows_pair
        int gt = threadIdx.x;
        asm volatile("" : "+v"(gt));
#pragma unroll
        for (int trip = 0; trip < CMAX * C4 / 256; ++trip) {
            const int item = gt + 256 * trip;
            if (item < items) {
                const int row = item / C4, c4 = item - row * C4;
                // a block that does not hold the row reads a row of zeros instead (one select on the address, not
                // four on the values: x + 0 is exact)
                float4 v[4];
                const uint32_t q4 = *reinterpret_cast<const uint32_t *>(&pos[par][row][0]);
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int q = (q4 >> (8 * b)) & 0xff;
                    v[b] = *(q != 0xff ? reinterpret_cast<const float4 *>(&stage[b][q][4 * c4]) : reinterpret_cast<const float4 *>(&zrow[4 * c4]));
                }
                float4 sum;
                sum.x = ((v[0].x + v[1].x) + v[2].x) + v[3].x; sum.y = ((v[0].y + v[1].y) + v[2].y) + v[3].y;
                sum.z = ((v[0].z + v[1].z) + v[2].z) + v[3].z; sum.w = ((v[0].w + v[1].w) + v[2].w) + v[3].w;
                float *dst = prow + (size_t)(r0 + row) * prow_pitch + ch0 + 4 * c4;
                if (r0 + row >= rows_cap) {
                    // (capacity-sized scratch and more rows than it holds: nothing is stored; the caller sees the count
                    // afterwards and runs the backward again with the right size)
                } else if (NBR != 1 || ch0 + 4 * c4 + 3 < d) {
                    *reinterpret_cast<float4 *>(dst) = sum;
                } else {  // ragged last slice (D % 32 != 0), possibly D % 4 != 0: never store past the row
                    const float sv[4] = {sum.x, sum.y, sum.z, sum.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (ch0 + 4 * c4 + e < d) dst[e] = sv[e];
                }
            }
            if (trip & 1) __builtin_amdgcn_sched_barrier(0);
        }
        pb = pbn;
        r0 = r1;
        // no third barrier: the next chunk's stores into stage[] / pos[par ^ 1] / cand[par ^ 1] come after ITS first
        // barrier, which every thread reaches only after finishing the loop above
    }
}

// ---- staged: rows on the 16-bit matrix cores, fp32-equivalent (the DEFAULT; GAGS_BWD_F32MFMA selects the kernel above) ----
// The same kernel with the contraction on v_mfma_f32_32x32x16_f16 (16x the fp32 MFMA rate).  Operands are written as sums of
// fp16 terms, each obtained by round-to-nearest of what the previous terms left over, after an exact power-of-two scaling:
//   weights    w = (a0 + a1 + a2) / rs   three terms: 33 significand bits >= fp32's 24, i.e. EXACT; rs = one power of two
//                                        per slot row (its largest weight -> [2^14, 2^15): heads and tails of the weights
//                                        that matter are normal fp16 numbers);
//   cotangent  v = (b0 + b1) / cs        two terms: |v cs - b0 - b1| <= 2^-24 |v cs| (each rounding leaves at most half an
//                                        ulp of an 11-bit significand): ONE fp32 rounding of the input; cs = one power of two
//                                        per (pixel block, channel), from the column's largest magnitude;
// and a product as the five terms of order <= 2:   w v ~ a0 b0 + a0 b1 + a1 b0 + a1 b1 + a2 b0   (dropped: a2 b1, 2^-36).
// Every partial product of two fp16 numbers is exact in the fp32 accumulator.  Net effect: each product w v enters the sum
// with a relative error <= 2^-24 -- the cotangent rounded once -- which is below the rounding an fp32 dot product of these
// 64-pixel columns commits in its own additions.  Against float64 (tests/test_fullsize_gpu.py
// ::test_colour_gradient_accuracy_against_float64) it is at least as close as the fp32-MFMA kernel; no atomics, fixed
// order: bit-reproducible.  A burst is 80 MFMAs of 32 cycles instead of 128 of 64.

// Phase clocks of the rows kernel's waves (tools/probe/: a SEPARATE probe build, -DGAGS_PROBE; never the shipped library)
#ifdef GAGS_PROBE
}  // namespace
__device__ unsigned long long *gags_probe_buf_bwd = nullptr;
extern "C" __attribute__((visibility("default"))) int gags_probe_set_bwd(void *p)
{
    return hipMemcpyToSymbol(HIP_SYMBOL(gags_probe_buf_bwd), &p, sizeof(p)) == hipSuccess ? 0 : -2;
}
namespace {
#define GAGS_PH_DECL unsigned long long pt_[8] = {0, 0, 0, 0, 0, 0, 0, 0}; unsigned long long tl_ = __builtin_readcyclecounter()
#define GAGS_PH(i) do { const unsigned long long now_ = __builtin_readcyclecounter(); pt_[i] += now_ - tl_; tl_ = now_; } while (0)
#define GAGS_PH_WRITE()                                                                                                  \
    do {                                                                                                                 \
        if (gags_probe_buf_bwd && lane == 0)                                                                             \
            for (int i_ = 0; i_ < 8; ++i_) gags_probe_buf_bwd[((size_t)blockIdx.x * 4 + wave) * 8 + i_] = pt_[i_];        \
    } while (0)
#else
#define GAGS_PH_DECL ((void)0)
#define GAGS_PH(i) ((void)0)
#define GAGS_PH_WRITE() ((void)0)
#endif

__device__ __forceinline__ void split8(const float (&x)[8], float scale, f16x8 &hi, f16x8 &lo)
{
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float v = x[i] * scale;
        const _Float16 h = (_Float16)v;
        hi[i] = h;
        lo[i] = (_Float16)(v - (float)h);
    }
}

__global__ __launch_bounds__(256, 2) void raster_bwd_rows_f16(
    int d, int width, int height, int tile_w, int n_tiles, int ch_base, int n_slices,
    const float *__restrict__ v_render_colors, const int32_t *__restrict__ offsets, int n_isects,
    const int32_t *__restrict__ blk_rows, const int32_t *__restrict__ trow, const float *__restrict__ wt,
    const int32_t *__restrict__ gid_s, const int32_t *__restrict__ trow_s, float *__restrict__ prow, int prow_pitch,
    uint32_t *__restrict__ row_key, int32_t *__restrict__ row_idx, int rows_cap)
{
    constexpr int NBR = 4, CW = 128, C4 = 32;
    __shared__ __attribute__((aligned(16))) float stage[4][32][CW];
    __shared__ __attribute__((aligned(4))) uint8_t pos[2][CMAX][4];
    __shared__ int cand[2][4];
    __shared__ __attribute__((aligned(16))) float zrow[CW];

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    GAGS_PH_DECL;
    if (threadIdx.x < CW) zrow[threadIdx.x] = 0.f;
    const int logical = gags_xcd_remap(blockIdx.x, n_tiles * n_slices);
    const int tile = gags_tile_of_order(logical / n_slices, tile_w, n_tiles / tile_w);
    const int start = offsets[tile];
    const int end = offsets[tile + 1]  /* n_tiles + 1 entries: the last one is the intersection count */;
    const int R0 = trow[start], R1 = trow[end];
    if (R1 == R0) return;
    const int blk = wave;
    const int cnt = blk_rows[tile * GAGS_BLOCKS_PER_TILE + blk];
    const int sb = gags_slot_base(start, end, tile, blk);
    const int ch0 = ch_base + (logical % n_slices) * CW;
    BlockGeom64 g;
    g.init(tile, blk, tile_w, width, height, lane);
    const int p = g.p, k = g.k;  // p: channel group (channels ch0 + 4p + j) / slot; k: which 8 of a K-step's 16 pixels

    // cotangent slab as B operands: K element e = 16 s + 8 k + i of the weight rows' order = pixel e >> 1 of the 8x4 half
    // e & 1; Bh / Bl[s][j] = the 8 elements of K-step s for channel ch0 + 4 p + j, head and tail, scaled by cs[j]
    f16x8 Bh[4][NBR], Bl[4][NBR];
    float inv[NBR];
    {
        float raw[4][8][NBR];
        float mx[NBR] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int e = 16 * s4 + 8 * k + i;
                const int pp = e >> 1, hh = e & 1;
                const int qj = g.bx0 + (pp & 7), qi = g.by0 + 4 * hh + (pp >> 3);
                const bool ok = (qi < height) && (qj < width) && cnt > 0;
                const float4 v = *reinterpret_cast<const float4 *>(
                    v_render_colors + ((size_t)min(qi, height - 1) * width + min(qj, width - 1)) * d + ch0 + NBR * p);
                raw[s4][i][0] = ok ? v.x : 0.f; raw[s4][i][1] = ok ? v.y : 0.f;
                raw[s4][i][2] = ok ? v.z : 0.f; raw[s4][i][3] = ok ? v.w : 0.f;
#pragma unroll
                for (int j = 0; j < NBR; ++j) mx[j] = fmaxf(mx[j], fabsf(raw[s4][i][j]));
            }
#pragma unroll
        for (int j = 0; j < NBR; ++j) {
            mx[j] = fmaxf(mx[j], __shfl_xor(mx[j], 32));  // the column's other 32 pixels live in the other half-wave
            // largest magnitude -> [2^14, 2^15); an all-zero (or non-finite) column keeps scale 1
            const float cs = (mx[j] > 0.f && mx[j] < 3.0e38f) ? ldexpf(1.0f, min(14 - ilogbf(mx[j]), 126)) : 1.0f;  // (clamped: no inf scale for a column below 2^-112)
            inv[j] = 1.0f / cs;
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                float col[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) col[i] = raw[s4][i][j];
                split8(col, cs, Bh[s4][j], Bl[s4][j]);
            }
        }
    }

    GAGS_PH(0);  // prologue: metadata, cotangent slab loaded, scaled and split
    int pb = 0;
    int r0 = R0;
    int tr = 0x7fffffff, gid = 0;
    if (lane <= 32 && lane < cnt) {
        tr = trow_s[sb + lane];
        gid = gid_s[sb + lane];
    }
    // weight tile, raw: lane (slot p, k) holds elements 16 s + 8 k + i of its slot's row
    float A[32];
    auto load_A = [&](int first) {
        const float4 *src = reinterpret_cast<const float4 *>(wt + (size_t)(sb + first + p) * 64 + k * 8);
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
            const float4 u = src[4 * s4], v = src[4 * s4 + 1];
            A[8 * s4] = u.x; A[8 * s4 + 1] = u.y; A[8 * s4 + 2] = u.z; A[8 * s4 + 3] = u.w;
            A[8 * s4 + 4] = v.x; A[8 * s4 + 5] = v.y; A[8 * s4 + 6] = v.z; A[8 * s4 + 7] = v.w;
        }
    };
    if (cnt > 0) load_A(0);
    for (int it = 0; r0 < R1; ++it) {
        const int par = it & 1;
        if (threadIdx.x < CMAX) reinterpret_cast<uint32_t *>(&pos[par][0][0])[threadIdx.x] = 0xffffffffu;
        const int tr32 = __builtin_amdgcn_readlane(tr, 32);
        if (lane == 0) cand[par][wave] = tr32;
        gags_lds_barrier();  // LDS traffic only: __syncthreads() would also wait for the loads in flight (next chunk's weight tile) and the row stores
        GAGS_PH(1);  // chunk bookkeeping + first barrier
        const int r1 = min(min(min(cand[par][0], cand[par][1]), min(cand[par][2], cand[par][3])), min(r0 + CMAX, R1));
        const bool mine = lane < 32 && tr < r1;
        const int run = __popcll(__ballot(mine));
        const int tr_c = tr, gid_c = gid;
        const int pbn = pb + run;
        if (run > 0) {
            if (mine) pos[par][tr_c - r0][wave] = (uint8_t)lane;
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            GAGS_PH(2);  // wait for the weight tile (and everything else in flight: the previous chunk's row stores)
            // power-of-two scale of this lane's slot row: its largest weight (weights are >= 0) -> [2^14, 2^15); exponent
            // arithmetic on the bits.  A row of zeros (pad slot, rows past the run: never stored) keeps scale 1.
            float wmx = 0.f;
#pragma unroll
            for (int i = 0; i < 32; ++i) wmx = fmaxf(wmx, A[i]);
            wmx = fmaxf(wmx, __shfl_xor(wmx, 32));
            const int ebits = (int)((__float_as_uint(wmx) >> 23) & 0xffu);
            const bool sane = ebits >= 15 && ebits <= 200;  // alpha*T lies in (4e-7, 1]; anything else (0, garbage past the block): 1
            const float rs = sane ? __uint_as_float((unsigned)(268 - ebits) << 23) : 1.0f;       // 2^(14 - exponent)
            const unsigned rinv = sane ? ((unsigned)(ebits - 14) << 23) : 0x3f800000u;           // its inverse, as bits
            f32x16 acc[NBR];
#pragma unroll
            for (int j = 0; j < NBR; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
                float a8[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) a8[i] = A[8 * s4 + i];
                f16x8 a0, a1, a2;
                split8x3(a8, rs, a0, a1, a2);
#pragma unroll
                for (int j = 0; j < NBR; ++j) {  // smallest terms first
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a2, Bh[s4][j], acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, Bl[s4][j], acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a1, Bh[s4][j], acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, Bl[s4][j], acc[j], 0, 0, 0);
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a0, Bh[s4][j], acc[j], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);  // one K-step's terms at a time (hoisted together they spill)
            }
            __builtin_amdgcn_sched_barrier(0);
            GAGS_PH(3);  // row scale, split, 80 MFMAs
            if (mine && ch0 == 0 && tr_c < rows_cap) {
                row_key[tr_c] = (uint32_t)gid_c;
                row_idx[tr_c] = tr_c;
            }
            tr = 0x7fffffff;
            if (lane <= 32 && pbn + lane < cnt) {
                tr = trow_s[sb + pbn + lane];
                gid = gid_s[sb + pbn + lane];
            }
            if (pbn < cnt) load_A(pbn);
            __builtin_amdgcn_sched_barrier(0);
            GAGS_PH(4);  // keys, next chunk's loads issued
            // this lane's four column unscales as two packed pairs: the row's inverse scale multiplies them with two
            // v_pk_mul_f32, the accumulators with two more
            typedef float pk2 __attribute__((ext_vector_type(2)));
            const pk2 inv01 = {inv[0], inv[1]}, inv23 = {inv[2], inv[3]};
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                // accumulator row r of this lane = slot (r & 3) + 8 (r >> 2) + 4 k: that row's inverse scale sits in lane `slot`
                const int s0 = (r & 3) + 8 * (r >> 2);
                const unsigned i0 = __builtin_amdgcn_readlane(rinv, s0), i1 = __builtin_amdgcn_readlane(rinv, s0 + 4);
                const float ri = __uint_as_float(k ? i1 : i0);
                const int slot = s0 + 4 * k;
                if (slot < run) {
                    const pk2 rr = {ri, ri};
                    const pk2 a01 = {acc[0][r], acc[1][r]}, a23 = {acc[2][r], acc[3][r]};
                    const pk2 o01 = a01 * (inv01 * rr), o23 = a23 * (inv23 * rr);
                    *reinterpret_cast<float4 *>(&stage[wave][slot][NBR * p]) = make_float4(o01[0], o01[1], o23[0], o23[1]);
                }
            }
        }
        GAGS_PH(5);  // unscale + park in LDS
        gags_lds_barrier();  // LDS traffic only: __syncthreads() would also wait for the loads in flight (next chunk's weight tile) and the row stores
        GAGS_PH(6);  // second barrier
        const int items = (r1 - r0) * C4;
        int gt = threadIdx.x;
        asm volatile("" : "+v"(gt));
#pragma unroll
        for (int trip = 0; trip < CMAX * C4 / 256; ++trip) {
            const int item = gt + 256 * trip;
            if (item < items) {
                const int row = item / C4, c4 = item - row * C4;
                float4 v[4];  // (a block that does not hold the row reads the row of zeros: see raster_bwd_rows)
                const uint32_t q4 = *reinterpret_cast<const uint32_t *>(&pos[par][row][0]);
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    const int q = (q4 >> (8 * b)) & 0xff;
                    v[b] = *(q != 0xff ? reinterpret_cast<const float4 *>(&stage[b][q][4 * c4]) : reinterpret_cast<const float4 *>(&zrow[4 * c4]));
                }
                float4 sum;
                sum.x = ((v[0].x + v[1].x) + v[2].x) + v[3].x; sum.y = ((v[0].y + v[1].y) + v[2].y) + v[3].y;
                sum.z = ((v[0].z + v[1].z) + v[2].z) + v[3].z; sum.w = ((v[0].w + v[1].w) + v[2].w) + v[3].w;
                if (r0 + row < rows_cap) *reinterpret_cast<float4 *>(prow + (size_t)(r0 + row) * prow_pitch + ch0 + 4 * c4) = sum;
            }
            if (trip & 1) __builtin_amdgcn_sched_barrier(0);
        }
        GAGS_PH(7);  // merge: LDS reads, adds, row stores
        pb = pbn;
        r0 = r1;
    }
    GAGS_PH_WRITE();
}

#include "raster_bwd_rows_cw.h"  // staged rows, channel waves (round 5; the default)

// trow_s[slot] = tile row of the slot's intersection (0x7fffffff for the pad slot of an odd count): one coalesced
// stream per block for the rows kernel instead of a dependent sidx -> trow gather.  One wave per (tile, block).
__global__ __launch_bounds__(64) void slot_rows_kernel(int n_tiles, int n_isects, const int32_t *__restrict__ offsets,
                                                       const int32_t *__restrict__ blk_rows,
                                                       const int32_t *__restrict__ sidx_s,
                                                       const int32_t *__restrict__ trow, int32_t *__restrict__ trow_s)
{
    const int tile = blockIdx.x >> 2, blk = blockIdx.x & 3;
    const int cnt = blk_rows[blockIdx.x];
    const int start = offsets[tile];
    const int end = offsets[tile + 1]  /* n_tiles + 1 entries: the last one is the intersection count */;
    const int sb = gags_slot_base(start, end, tile, blk);
    for (int j = threadIdx.x; j < cnt; j += 64) {
        const int sx = sidx_s[sb + j];
        trow_s[sb + j] = sx >= 0 ? trow[sx] : 0x7fffffff;
    }
}

// the staged backward's scratch (base NULL: sizes only)
struct StagedScratch {
    uint32_t *key, *key_s;
    int32_t *idx, *idx_s, *seg;
    void *sort;
    int64_t sort_bytes;
    float *prow;
    int64_t total;
};
inline StagedScratch staged_carve(void *base, int64_t rows, int n_gauss, int d)
{
    GagsCarve c(base);
    StagedScratch L;
    L.key = c.take<uint32_t>(rows);
    L.idx = c.take<int32_t>(rows);
    L.key_s = c.take<uint32_t>(rows);
    L.idx_s = c.take<int32_t>(rows);
    L.seg = c.take<int32_t>((int64_t)n_gauss + 2);
    L.sort = c.take_bytes(gags_sort_u32_scratch_bytes(rows));
    L.sort_bytes = c.last();
    L.prow = c.take<float>(rows * (int64_t)d);
    L.total = c.total();
    return L;
}

}  // namespace

int64_t gags_bwd_staged_scratch_bytes_impl(int64_t rows, int n_gauss, int d)
{
    return staged_carve(nullptr, rows > 0 ? rows : 1, n_gauss, d).total;
}

int gags_bwd_slot_rows_launch(int width, int height, int n_isects, const int32_t *offsets, const int32_t *blk_rows,
                              const int32_t *sidx_s, const int32_t *trow, int32_t *trow_s, hipStream_t st)
{
    GAGS_CLEAR_ERR();
    const int n_tiles = gags_tiles(width, height).n;
    hipLaunchKernelGGL(slot_rows_kernel, dim3(n_tiles * GAGS_BLOCKS_PER_TILE), dim3(64), 0, st, n_tiles, n_isects, offsets, blk_rows, sidx_s, trow, trow_s);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

// GAGS_BWD_ROWSCALE=1 (experiments; read once): the rows kernel's weight scale per (row, block) instead of the view-wide 2^15
static bool rows_scale_per_block()
{
    static const bool v = [] { const char *e = getenv("GAGS_BWD_ROWSCALE"); return e && e[0] == '1'; }();
    return v;
}

int gags_raster_bwd_staged_launch(int d, int width, int height, int n_gauss, const int32_t *offsets, int n_isects,
                                  const float *v_out, const int32_t *blk_rows, const int32_t *trow, int64_t rows,
                                  const float *wt, const int32_t *gid_s, const int32_t *trow_s, void *scratch,
                                  int64_t scratch_bytes, float *v_colors, int stage_flags, int ch_begin, int ch_count,
                                  const int32_t *rows_dev, const int32_t *wire_pos, float *wire, const uint8_t *keep_prev,
                                  uint8_t *keep_cur, hipStream_t st)
{
    // stage: GAGS_STAGE_ALL = everything; _ROWS, _SORT (+ segment offsets), _REDUCE = one of them (per-kernel timing)
    GAGS_CLEAR_ERR();
    const int stage = stage_flags & GAGS_STAGE_MASK;
    if (!gags_mfma_width(d) || d > 1024) return 1;
    const bool sA = stage == GAGS_STAGE_ALL || stage == GAGS_STAGE_ROWS, sS = stage == GAGS_STAGE_ALL || stage == GAGS_STAGE_SORT,
               sR = stage == GAGS_STAGE_ALL || stage == GAGS_STAGE_REDUCE;
    const GagsTiles T = gags_tiles(width, height);
    // channel range of this call (a by-view step exchanges the gradient range by range while the next range is computed,
    // gags_amd/dist.py); the default is everything.  Ranges start on a multiple of 32 and end on one or at d.
    if (ch_count <= 0 || ch_begin < 0 || ch_begin + ch_count > d || ch_begin % 32 != 0 ||
        (ch_count % 32 != 0 && ch_begin + ch_count != d))
        return GAGS_EINVAL;
    // GAGS_STAGED_RANGE_SCRATCH: the scratch holds partial rows of THIS call's channel range only ([rows, ch_count rounded up to 4]
    // instead of [rows, d]; sized with gags_bwd_staged_scratch_bytes(rows, n, that width)): a wide gradient is then produced
    // range by range through a scratch a quarter (an eighth ...) the size -- what lets heavy views fit (C5H: 80 M rows)
    const bool narrow = (stage_flags & GAGS_STAGED_RANGE_SCRATCH) != 0;
    const int pp = narrow ? ((ch_count + 3) & ~3) : d;
    const StagedScratch L = staged_carve(scratch, rows > 0 ? rows : 1, n_gauss, pp);
    if (scratch_bytes < L.total) return GAGS_ESCRATCH;
    uint32_t *key = L.key, *key_s = L.key_s;
    int32_t *idx = L.idx, *idx_s = L.idx_s, *seg = L.seg;
    float *prow = L.prow - (narrow ? ch_begin : 0);  // (indexed by absolute channel)
    if (rows > 0 && sA) {
        // 128-channel slices, then 64, then 32-channel slices (the last one ragged when the range ends at an odd d)
#define GAGS_ROWS_LAUNCH(KERNEL, CH0, NSL)                                                                           \
    hipLaunchKernelGGL(KERNEL, dim3(T.n * (NSL)), dim3(256), 0, st, d, width, height, T.w, T.n, (CH0), (NSL),           \
                       v_out, offsets, n_isects, blk_rows, trow, wt, gid_s, trow_s, prow, pp, key, idx, (int)rows)
        int c = ch_begin;
        const int ce = ch_begin + ch_count;
        if (ce - c >= 128) {
            const int nsl = (ce - c) / 128;
            if (stage_flags & GAGS_STAGED_F32MFMA) GAGS_ROWS_LAUNCH(raster_bwd_rows<4>, c, nsl);  // the fp32 matrix instructions
            else if (stage_flags & GAGS_STAGED_BLOCKWAVES) GAGS_ROWS_LAUNCH(raster_bwd_rows_f16, c, nsl);  // round 4's shape: a wave per pixel block, rows merged in LDS
            else if (stage_flags & GAGS_STAGED_EXACT_WEIGHTS) GAGS_ROWS_LAUNCH((raster_bwd_rows_cw<3, 5>), c, nsl);  // weights as three terms (exact), five product terms
            else if (rows_scale_per_block()) GAGS_ROWS_LAUNCH((raster_bwd_rows_cw<2, 3>), c, nsl);  // (GAGS_BWD_ROWSCALE=1: round 5's scale per (row, block))
            else GAGS_ROWS_LAUNCH((raster_bwd_rows_cw<2, 3, true>), c, nsl);  // default: 16-bit matrix cores, a wave per 32 channels, three product terms, one weight scale
            c += 128 * nsl;
        }
        if (ce - c >= 64) {
            GAGS_ROWS_LAUNCH(raster_bwd_rows<2>, c, 1);
            c += 64;
        }
        if (ce - c > 0) GAGS_ROWS_LAUNCH(raster_bwd_rows<1>, c, (ce - c + 31) / 32);
#undef GAGS_ROWS_LAUNCH
    }
    if (sS) {
        const int rc = gags_rows_group_launch(rows, n_gauss, rows_dev, key, idx, key_s, idx_s, seg, L.sort, L.sort_bytes, st);
        if (rc != GAGS_OK) return rc;
    }
    if (sR) {
        const bool half = (stage_flags & GAGS_STAGED_OUT_F16) != 0;  // v_colors is an fp16 tensor
        const int sparse = (stage_flags & GAGS_STAGED_PREZEROED) ? 1 : 0;  // v_colors arrives zero-filled: rows of Gaussians that blended nothing are skipped
        const int rc = gags_rows_reduce_launch(n_gauss, d, ch_begin, ch_count, seg, idx_s, prow, pp, v_colors, half, st, sparse, wire_pos,
                                               wire, keep_prev, keep_cur);
        if (rc != GAGS_OK) return rc;
    }
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
