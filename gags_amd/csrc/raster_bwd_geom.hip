// Geometry gradients at wide D.  The only D-proportional term of d loss / d alpha,
//     v_alpha(g, px) = T_g <c_g, v_px>  -  ra_g SUM_{g' behind g} f_g' <c_g', v_px>  +  T_f ra_g (v_a - <bg, v_px>),
// needs the dot products S[g, px] = <c_g, v_px> and nothing else: the "buffer" term is a running sum of f S over the
// Gaussians behind (linearity).  So:
//   1. raster_bwd_sdot: S[slot][64 px] for every slot of every 8x8 block on the fp32 matrix cores -- the contraction runs
//      over the CHANNELS, 256 per pass (wider tables: accumulating passes); the block's cotangent slab [64 px][256 ch]
//      sits in LDS (66 KB: two workgroups per CU, one loads its slab while the other multiplies), the four waves take
//      the block's 32-slot tiles in turn, the slots' feature rows are streamed from L2 / HBM eight float4 ahead;
//   2. raster_bwd_geom: one wave per block walks its slots back to front, one pixel per lane: alpha again from the packed
//      record, T = f / alpha from the forward's weight, v_alpha from S, the six geometry partials summed over the wave
//      and stored as ONE 32-byte row per slot (no atomics);
//   3. the rows are sorted by Gaussian and summed with the kernels of the colours backward (rows_reduce.hip, d = 8).
#include <algorithm>
#include "raster_mfma_common.h"
#include "launch.h"
#include "reduce.h"

using namespace gags_mfma;

constexpr int SD_PAD = 4;        // floats of padding per slab row: b128 reads of 32 rows then cover all 64 banks
constexpr int SD_MAXCH = 256;    // channels per pass (LDS); wider tables take several accumulating passes

template <int DCH>  // channels of this pass, compile-time for the full 256 (everything unrolled), 0 = use `dch`
__global__ __launch_bounds__(256, 2) void raster_bwd_sdot(int d, int ch0, int dch_rt, int width, int height, int tile_w, int n_tiles,
                                                       int n_gauss, const float *__restrict__ v_out,
                                                       const float *__restrict__ colors, const float *__restrict__ backgrounds,
                                                       const int32_t *__restrict__ offsets, int n_isects,
                                                       const int32_t *__restrict__ blk_rows, const int32_t *__restrict__ gid_s,
                                                       float *__restrict__ S, float *__restrict__ bgdot, int accumulate,
                                                       const int32_t *__restrict__ row_base)
{
    extern __shared__ __attribute__((aligned(16))) float slab[];  // [64 pixels in wt order e = 2 p + h][dch + SD_PAD]
    __shared__ float bred[4][64];
    __shared__ __attribute__((aligned(16))) float bgs[SD_MAXCH];  // the pass's slice of the background
    const int dch = DCH ? DCH : dch_rt;
    const int logical = gags_xcd_remap(blockIdx.x, n_tiles * GAGS_BLOCKS_PER_TILE);
    const int blk = logical & 3;
    const int tile = gags_tile_of_order(logical >> 2, tile_w, n_tiles / tile_w);
    const int cnt = blk_rows[tile * GAGS_BLOCKS_PER_TILE + blk];
    if (cnt == 0) return;
    const int start = offsets[tile];
    const int end = offsets[tile + 1]  /* n_tiles + 1 entries: the last one is the intersection count */;
    const int sb = gags_slot_base(start, end, tile, blk);
    // S rows: compact numbering (row_base = exclusive prefix sum of blk_rows: S is n_rows x 256 B) or the sparse slot index
    const int srb = row_base ? row_base[tile * GAGS_BLOCKS_PER_TILE + blk] : sb;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int pitch = dch + SD_PAD;
    const int ty = tile / tile_w, tx = tile - ty * tile_w;
    const int bx0 = tx * GAGS_TILE + (blk & 1) * 8, by0 = ty * GAGS_TILE + (blk >> 1) * 8;
    {
        // slab load, eight float4 per thread in flight (a load-then-store loop would wait for every single one)
        const int q4 = dch >> 2;  // float4 per pixel row
        const int total = 64 * q4;
        for (int i0 = tid; i0 < total; i0 += 8 * 256) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = min(i0 + u * 256, total - 1);
                const int e = i / q4, c4 = i - e * q4;
                const int pp = e >> 1, h = e & 1;
                const int pj = bx0 + (pp & 7), pi = by0 + (pp >> 3) + 4 * h;
                const bool in = pi < height && pj < width;
                v[u] = *reinterpret_cast<const float4 *>(v_out + ((size_t)min(pi, height - 1) * width + min(pj, width - 1)) * d + ch0 + 4 * c4);
                if (!in) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + u * 256;
                if (i < total) {
                    const int e = i / q4, c4 = i - e * q4;
                    *reinterpret_cast<float4 *>(slab + e * pitch + 4 * c4) = v[u];
                }
            }
        }
    }
    if (backgrounds && tid < dch) bgs[tid] = backgrounds[ch0 + tid];
    __syncthreads();
    if (backgrounds) {  // <bg, v_px> per pixel of the block, for the background term of v_alpha (background slice from LDS)
        const int e = tid & 63, part = tid >> 6;
        float acc = 0.f;
        for (int c = 4 * part; c < dch; c += 16) {
            const float4 x = *reinterpret_cast<const float4 *>(slab + e * pitch + c), b = *reinterpret_cast<const float4 *>(bgs + c);
            acc = fmaf(b.x, x.x, acc); acc = fmaf(b.y, x.y, acc); acc = fmaf(b.z, x.z, acc); acc = fmaf(b.w, x.w, acc);
        }
        bred[part][e] = acc;
        __syncthreads();
        if (tid < 64) {
            const int pp = tid >> 1, h = tid & 1;
            const int pj = bx0 + (pp & 7), pi = by0 + (pp >> 3) + 4 * h;
            if (pi < height && pj < width) {
                const float t = (bred[0][tid] + bred[1][tid]) + (bred[2][tid] + bred[3][tid]);
                float *dst = bgdot + (size_t)pi * width + pj;
                *dst = accumulate ? *dst + t : t;
            }
        }
    }
    const int m = lane & 31, kh = lane >> 5;
    const int nj = dch >> 3;  // steps of 8 channels: lane (m, kh) takes channels 8 j + 4 kh .. + 3 of slot m's row
    // work units = (32-slot tile, 32-pixel half of the block), dealt round-robin to the four waves: with whole tiles as
    // units a block of ~4.75 tiles kept the waves 59 % busy, with half-tiles 79 % (the second reader of a feature row
    // finds it in the CU's L1)
    const int n_units = 2 * ((cnt + 31) >> 5);
    for (int unit = wave; unit < n_units; unit += 4) {
        const int t0 = (unit >> 1) * 32, hh = unit & 1;
        const int slot = sb + min(t0 + m, cnt - 1);
        const int gid = min(gid_s[slot], n_gauss - 1);  // the pad slot's row is computed and never used (its weights are 0)
        const float *crow = colors + (size_t)gid * d + ch0 + 4 * kh;
        const float *b0 = slab + (32 * hh + m) * pitch + 4 * kh;
        f32x16 acc0;
        if (accumulate) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = min(t0 + (r & 3) + 8 * (r >> 2) + 4 * kh, cnt - 1);
                acc0[r] = S[(size_t)(srb + row) * 64 + 32 * hh + m];
            }
        } else {
#pragma unroll
            for (int r = 0; r < 16; ++r) acc0[r] = 0.f;
        }
        float4 a[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] = *reinterpret_cast<const float4 *>(crow + 8 * min(u, nj - 1));
        auto step = [&](int j, int u) __attribute__((always_inline)) {
            const float4 av = a[u];
            a[u] = *reinterpret_cast<const float4 *>(crow + 8 * min(j + 8, nj - 1));
            const float4 x0 = *reinterpret_cast<const float4 *>(b0 + 8 * j);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, x0.x, acc0, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, x0.y, acc0, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, x0.z, acc0, 0, 0, 0);
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, x0.w, acc0, 0, 0, 0);
        };
        if constexpr (DCH != 0) {  // one basic block: no loop back-edge for the compiler to drain the prefetches at
#pragma unroll
            for (int j = 0; j < DCH / 8; ++j) {
                step(j, j & 7);
                __builtin_amdgcn_sched_barrier(0);  // (or every LDS read of the tile is hoisted to the top: 256 VGPRs + spills)
            }
        } else {
            for (int jb = 0; jb < nj; jb += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (jb + u < nj) step(jb + u, u);
            }
        }
        // accumulator: column = pixel element m of half hh, rows = slots (r & 3) + 8 (r >> 2) + 4 kh
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = t0 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (row < cnt) S[(size_t)(srb + row) * 64 + 32 * hh + m] = acc0[r];
        }
    }
}

// ---- the same dot pass on the fp16 matrix cores with split operands (round 3; the default) --------------------------------
// S = <c_g, v_px> is a plain contraction over the channels, so the scheme of raster_bwd_rows_f16 applies with the roles
// swapped: the FEATURE rows get one power-of-two scale per Gaussian row (largest magnitude -> [2^14, 2^15)), the COTANGENT
// slab one scale per 8x8 block and pass (the geometry rows sum S over the block's 64 pixels, so an error relative to the
// block's largest cotangent is an error relative to the row's largest term).  Since round 5 both operands are TWO fp16 terms
// (one fp32-level rounding each) and a product is a0 b0 + a0 b1 + a1 b0 (SF_TA = 2; rounds 3-4: feature rows as three terms,
// exact, five product terms: SF_TA = 3) -- against float64 autograd the geometry gradients did not move (v_opacities 2.3e-7,
// v_means2d 2.5e-7; five terms: 2.7e-7 / 2.4e-7), the pass went 1.37 -> 1.16 ms.  Matrix terms at the 16-bit rate
// instead of one at the fp32 rate.
// What bounds this pass is not the arithmetic but the GATHER of the feature rows: every lane of an A operand reads
// another Gaussian's row, and the vector L1 looks up one 128-byte line per cycle -- 32x32 tiles (two lanes per row, 32 B
// per row and instruction) delivered 16-32 B/clk/CU and ran SLOWER with the 16-bit cores than the fp32 kernel (3.0 vs
// 2.1 ms per pass at C3).  Hence v_mfma_f32_16x16x32_f16: FOUR lanes per row, 64 contiguous bytes of one row per
// instruction, 16 lines per wave load.
//   feat_split_kernel: once per pass, every BLENDED Gaussian's 256-channel slice -> SF_TA fp16 terms in operand order
//     ([32-channel step][term][32 halves]) + 1 / scale per row; the split costs ~13 VALU instructions per two values and
//     a row is read by ~16 units, so it is done once, not per unit;
//   raster_bwd_sdot_f16: slab -> registers -> block maximum -> two fp16 planes in LDS (67.6 KB: two workgroups per CU);
//     units of 16 slots x 64 pixels (four 16x16 accumulators), per 32-channel step SF_TA x 16 B from the table (four steps
//     ahead), 8 x 16 B from LDS, 12 MFMAs (20 with three terms), no VALU work in the loop; the accumulators leave scaled back by
//     (row scale x block scale) -- S holds plain dot products, as before.
constexpr int SF_TA = 2;    // fp16 terms of a feature value in the table (2: one fp32-level rounding; 3: exact, five product terms)
constexpr int SF_PADH = 8;  // halves of padding per slab row (one 2-way conflict per ds_read_b128 lane group; 16 is conflict-free and measured the same)
constexpr int SF_PF = 4;    // 32-channel steps of table rows in flight
constexpr int SF_STAGE = 1024;  // slots of a block whose ids and scales are staged in LDS (8 KB; mean block: ~140 slots)
typedef float f32x4_t __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void feat_split_kernel(int, int, int, int, const float *, const unsigned char *, uint4 *, float *);  // (prototype: -Wmissing-prototypes)
__global__ __launch_bounds__(256) void feat_split_kernel(int n_gauss, int d, int ch0, int ks, const float *__restrict__ colors,
                                                         const unsigned char *__restrict__ mask, uint4 *__restrict__ table,
                                                         float *__restrict__ rinv)
{
    const int row = blockIdx.x * 8 + (threadIdx.x >> 5), l = threadIdx.x & 31;  // half a wave per row, 8 channels per lane
    if (row >= n_gauss || !mask[row]) return;
    const int dch = min(32 * ks, d - ch0);
    float x[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) x[i] = 0.f;
    if (8 * l < dch) {
        const float4 *src = reinterpret_cast<const float4 *>(colors + (size_t)row * d + ch0 + 8 * l);
        const float4 u = src[0], v = src[1];
        x[0] = u.x; x[1] = u.y; x[2] = u.z; x[3] = u.w; x[4] = v.x; x[5] = v.y; x[6] = v.z; x[7] = v.w;
    }
    float mx = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) mx = fmaxf(mx, fabsf(x[i]));
#pragma unroll
    for (int o = 1; o < 32; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    const int ebits = (int)((__float_as_uint(mx) >> 23) & 0xffu);
    const bool sane = ebits >= 16 && ebits <= 240;  // zero rows, denormals, non-finite values: scale 1
    const float rs = sane ? __uint_as_float((unsigned)(268 - ebits) << 23) : 1.0f;  // 2^(14 - exponent)
    if (l < 4 * ks) {
        f16x8 t0, t1, t2;
        uint4 *dst = table + (size_t)row * (4 * SF_TA * ks) + 4 * SF_TA * (l >> 2) + (l & 3);  // step l / 4, k quarter l % 4; term t: + 4 t
        if constexpr (SF_TA == 3) {
            split8x3(x, rs, t0, t1, t2);
            dst[8] = *reinterpret_cast<const uint4 *>(&t2);
        } else {
            split8x2(x, rs, t0, t1);
        }
        dst[0] = *reinterpret_cast<const uint4 *>(&t0);
        dst[4] = *reinterpret_cast<const uint4 *>(&t1);
    }
    if (l == 0) rinv[row] = sane ? __uint_as_float((unsigned)(ebits - 14) << 23) : 1.0f;
}

template <int KS>  // 32-channel steps of this pass: 8 = the full 256 channels, everything unrolled; 0 = `ks_rt`
__global__ __launch_bounds__(256, 2) void raster_bwd_sdot_f16(int d, int ch0, int ks_rt, int width, int height, int tile_w, int n_tiles,
                                                           int n_gauss, const float *__restrict__ v_out,
                                                           const uint4 *__restrict__ table, const float *__restrict__ rinv,
                                                           const float *__restrict__ backgrounds,
                                                           const int32_t *__restrict__ offsets, int n_isects,
                                                           const int32_t *__restrict__ blk_rows, const int32_t *__restrict__ gid_s,
                                                           float *__restrict__ S, float *__restrict__ bgdot,
                                                           const int32_t *__restrict__ row_base)
{
    extern __shared__ __attribute__((aligned(16))) _Float16 planes[];  // hi [64 pixels e = 2 p + h][pitch], then lo
    __shared__ float bred[4][64];
    __shared__ float wmax[4];
    __shared__ __attribute__((aligned(16))) float bgs[SD_MAXCH];  // the pass's slice of the background
    __shared__ int gids[SF_STAGE];                                 // the block's first SF_STAGE slots: Gaussian id, 1 / row scale
    __shared__ float rinvs[SF_STAGE];
    const int ks = KS ? KS : ks_rt;
    const int dch = min(32 * ks, d - ch0);  // channels of the pass that exist (a multiple of 8); the rest of the last step is 0
    const int pitch = 32 * ks + SF_PADH;
    _Float16 *hi = planes, *lo = planes + 64 * pitch;
    const int logical = gags_xcd_remap(blockIdx.x, n_tiles * GAGS_BLOCKS_PER_TILE);
    const int blk = logical & 3;
    const int tile = gags_tile_of_order(logical >> 2, tile_w, n_tiles / tile_w);
    const int cnt = blk_rows[tile * GAGS_BLOCKS_PER_TILE + blk];
    if (cnt == 0) return;
    const int start = offsets[tile];
    const int end = offsets[tile + 1]  /* n_tiles + 1 entries: the last one is the intersection count */;
    const int sb = gags_slot_base(start, end, tile, blk);
    const int srb = row_base ? row_base[tile * GAGS_BLOCKS_PER_TILE + blk] : sb;  // S rows: compact or sparse numbering
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ty = tile / tile_w, tx = tile - ty * tile_w;
    const int bx0 = tx * GAGS_TILE + (blk & 1) * 8, by0 = ty * GAGS_TILE + (blk >> 1) * 8;
    const int m = lane & 15, kq = lane >> 4;
    // work units = 16 slots x the block's 64 pixels, dealt round-robin to the four waves (a block of ~150 slots: ten units)
    const int n_units = (cnt + 15) >> 4;
    // The (unit, step) pairs of a wave form ONE stream: the table rows are requested SF_PF steps ahead ACROSS unit
    // boundaries.  NOTHING else is loaded from global memory inside that stream: loads return in order, so one HBM miss
    // (an id, a scale, an earlier pass's sum) in front of a row request stalls the MFMAs for its whole latency -- the ids
    // and scales of the block's slots are staged in LDS up front (requested before the slab, their latency passes under
    // the slab's), and every pass writes its own S / bgdot buffer (raster_bwd_geom adds them up; no read-modify-write).
    auto slot_gid = [&](int j) __attribute__((always_inline)) { return min(gid_s[sb + min(j, cnt - 1)], n_gauss - 1); };  // (pad slot: clamped, unused)
    const int n_stage = min(cnt, SF_STAGE);
    int sg[SF_STAGE / 256];
#pragma unroll
    for (int q = 0; q < SF_STAGE / 256; ++q) sg[q] = (q * 256 < n_stage) ? slot_gid(tid + q * 256) : 0;
    int gid = 0;
    // Row requests are made in QUAD order -- lane 4 r + q asks for quarter q (16 bytes) of row r's 64-byte step, four
    // consecutive lanes one contiguous 64 bytes -- and the registers are then permuted into the MFMA's operand order
    // (lane 16 q + r): the address coalescer works on neighbouring lanes, and in operand order (neighbours = different
    // Gaussians) a 16-byte-per-lane gather went through at one lane per cycle, which bounded the whole pass.
    const int lr = lane >> 2, lq = lane & 3;
    const int perm_src = 4 * (4 * m + kq);  // ds_bpermute address: operand lane (m, kq) takes from request lane 4 m + kq
    if (wave < n_units) gid = slot_gid(wave * 16 + lr);  // the wave's first unit: its rows are requested before the slab is waited for
    uint4 a[SF_PF][SF_TA];
    float ibs;  // 1 / block scale
    {
        // the whole slab in registers (<= 16 float4 per thread, all requested at once), its largest magnitude, then
        // scaled and split into the two planes
        const int q4 = 8 * ks;  // float4 per padded pixel row
        const int total = 64 * q4;
        float4 v[16];
        float mx = 0.f;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (u * 256 < total) {  // (uniform)
                const int i = min(tid + u * 256, total - 1);
                const int e = i / q4, c4 = i - e * q4;
                const int pp = e >> 1, h = e & 1;
                const int pj = bx0 + (pp & 7), pi = by0 + (pp >> 3) + 4 * h;
                const bool in = pi < height && pj < width && 4 * c4 < dch && tid + u * 256 < total;
                v[u] = *reinterpret_cast<const float4 *>(v_out + ((size_t)min(pi, height - 1) * width + min(pj, width - 1)) * d +
                                                         ch0 + min(4 * c4, dch - 4));
                if (!in) v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (wave < n_units) {  // (the ids were requested before the slab: they are here first)
            const uint4 *arow = table + (size_t)gid * (4 * SF_TA * ks) + lq;
#pragma unroll
            for (int u = 0; u < SF_PF; ++u)
#pragma unroll
                for (int t = 0; t < SF_TA; ++t) a[u][t] = arow[4 * SF_TA * min(u, ks - 1) + 4 * t];
        }
        float sr[SF_STAGE / 256];
#pragma unroll
        for (int q = 0; q < SF_STAGE / 256; ++q) sr[q] = (q * 256 < n_stage) ? rinv[sg[q]] : 0.f;
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int u = 0; u < 16; ++u) mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v[u].x), fabsf(v[u].y))), fmaxf(fabsf(v[u].z), fabsf(v[u].w)));
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
        if (lane == 0) wmax[wave] = mx;
        if (backgrounds && tid < dch) bgs[tid] = backgrounds[ch0 + tid];
#pragma unroll
        for (int q = 0; q < SF_STAGE / 256; ++q)
            if (q * 256 < n_stage) { gids[tid + q * 256] = sg[q]; rinvs[tid + q * 256] = sr[q]; }
        __syncthreads();
        mx = fmaxf(fmaxf(wmax[0], wmax[1]), fmaxf(wmax[2], wmax[3]));
        const int ebits = (int)((__float_as_uint(mx) >> 23) & 0xffu);
        const bool sane = ebits >= 16 && ebits <= 240;  // an all-zero (or non-finite) slab keeps scale 1
        const float bs = sane ? __uint_as_float((unsigned)(268 - ebits) << 23) : 1.0f;  // largest magnitude -> [2^14, 2^15)
        ibs = sane ? __uint_as_float((unsigned)(ebits - 14) << 23) : 1.0f;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
            const int i = tid + u * 256;
            if (i < total) {
                const int e = i / q4, c4 = i - e * q4;
                const f32x2v_t a = {v[u].x * bs, v[u].y * bs}, b = {v[u].z * bs, v[u].w * bs};
                const f16x2_t ah = __builtin_convertvector(a, f16x2_t), bh = __builtin_convertvector(b, f16x2_t);
                const f16x2_t al = __builtin_convertvector(a - __builtin_convertvector(ah, f32x2v_t), f16x2_t);
                const f16x2_t bl = __builtin_convertvector(b - __builtin_convertvector(bh, f32x2v_t), f16x2_t);
                typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
                const f16x4_t h4 = {ah[0], ah[1], bh[0], bh[1]}, l4 = {al[0], al[1], bl[0], bl[1]};
                *reinterpret_cast<f16x4_t *>(hi + e * pitch + 4 * c4) = h4;
                *reinterpret_cast<f16x4_t *>(lo + e * pitch + 4 * c4) = l4;
            }
        }
    }
    __syncthreads();
    if (backgrounds) {  // <bg, v_px> per pixel of the block, for the background term of v_alpha (from the two planes)
        // eight channels at a time, the background slice from LDS (a global load per channel, waited for one by one,
        // was 12.8 of this workgroup's 30 microseconds)
        const int e = tid & 63, part = tid >> 6;
        float acc = 0.f;
        for (int c = 8 * part; c < dch; c += 32) {
            const f16x8 h8 = *reinterpret_cast<const f16x8 *>(hi + e * pitch + c), l8 = *reinterpret_cast<const f16x8 *>(lo + e * pitch + c);
            const float4 b0 = *reinterpret_cast<const float4 *>(bgs + c), b1 = *reinterpret_cast<const float4 *>(bgs + c + 4);
            acc = fmaf(b0.x, (float)h8[0] + (float)l8[0], acc); acc = fmaf(b0.y, (float)h8[1] + (float)l8[1], acc);
            acc = fmaf(b0.z, (float)h8[2] + (float)l8[2], acc); acc = fmaf(b0.w, (float)h8[3] + (float)l8[3], acc);
            acc = fmaf(b1.x, (float)h8[4] + (float)l8[4], acc); acc = fmaf(b1.y, (float)h8[5] + (float)l8[5], acc);
            acc = fmaf(b1.z, (float)h8[6] + (float)l8[6], acc); acc = fmaf(b1.w, (float)h8[7] + (float)l8[7], acc);
        }
        bred[part][e] = acc;
        __syncthreads();
        if (tid < 64) {
            const int pp = tid >> 1, h = tid & 1;
            const int pj = bx0 + (pp & 7), pi = by0 + (pp >> 3) + 4 * h;
            if (pi < height && pj < width) {
                const float t = ((bred[0][tid] + bred[1][tid]) + (bred[2][tid] + bred[3][tid])) * ibs;
                bgdot[(size_t)pi * width + pj] = t;
            }
        }
    }
    auto unit_gid = [&](int unit) __attribute__((always_inline)) {  // staged; a block of more than SF_STAGE slots: the rest from memory
        const int j = min(min(unit, n_units - 1) * 16 + lr, cnt - 1);
        return j < SF_STAGE ? gids[j] : slot_gid(j);
    };
    int gid_n = unit_gid(wave + 4);
    for (int unit = wave; unit < n_units; unit += 4) {
        const int t0 = unit * 16;
        const uint4 *arow = table + (size_t)gid * (4 * SF_TA * ks) + lq;      // step j, term t: + 4 SF_TA j + 4 t
        const uint4 *arow_n = table + (size_t)gid_n * (4 * SF_TA * ks) + lq;  // the wave's next unit (the last one: itself again)
        const int jm = min(t0 + m, cnt - 1);
        const float ri = (jm < SF_STAGE ? rinvs[jm] : rinv[slot_gid(jm)]) * ibs;
        const int gid_nn = unit_gid(unit + 8);
        const _Float16 *bh0 = hi + m * pitch + 8 * kq, *bl0 = lo + m * pitch + 8 * kq;  // pixel group pg: + 16 pg pitch
        f32x4_t acc[4];
#pragma unroll
        for (int pg = 0; pg < 4; ++pg) acc[pg] = f32x4_t{0.f, 0.f, 0.f, 0.f};
        auto step = [&](int j, int u) __attribute__((always_inline)) {
            uint4 pa[3];
#pragma unroll
            for (int t = 0; t < SF_TA; ++t) {
                pa[t].x = (unsigned)__builtin_amdgcn_ds_bpermute(perm_src, (int)a[u][t].x);
                pa[t].y = (unsigned)__builtin_amdgcn_ds_bpermute(perm_src, (int)a[u][t].y);
                pa[t].z = (unsigned)__builtin_amdgcn_ds_bpermute(perm_src, (int)a[u][t].z);
                pa[t].w = (unsigned)__builtin_amdgcn_ds_bpermute(perm_src, (int)a[u][t].w);
            }
            if constexpr (SF_TA == 2) pa[2] = pa[1];
            const f16x8 a0 = *reinterpret_cast<const f16x8 *>(&pa[0]);
            const f16x8 a1 = *reinterpret_cast<const f16x8 *>(&pa[1]);
            const f16x8 a2 = *reinterpret_cast<const f16x8 *>(&pa[2]);
            {   // slot u next holds step j + SF_PF of this unit, or -- past its end -- step u of the next one
                const uint4 *src = (j + SF_PF < ks) ? arow + 4 * SF_TA * (j + SF_PF) : arow_n + 4 * SF_TA * min(u, ks - 1);
#pragma unroll
                for (int t = 0; t < SF_TA; ++t) a[u][t] = src[4 * t];
            }
            f16x8 bh[4], bl[4];
#pragma unroll
            for (int pg = 0; pg < 4; ++pg) {
                bh[pg] = *reinterpret_cast<const f16x8 *>(bh0 + 16 * pg * pitch + 32 * j);
                bl[pg] = *reinterpret_cast<const f16x8 *>(bl0 + 16 * pg * pitch + 32 * j);
            }
            // One scheduling fence per step, BETWEEN its reads and its MFMAs: the next step's permutes and LDS reads may
            // rise into this step's MFMAs (and no further; without any fence every read of the unit went to the top: 96 spills).
            __builtin_amdgcn_sched_barrier(0);
            // smallest terms first; the four accumulators in turn (no MFMA waits for the one before it)
            if constexpr (SF_TA == 3) {
#pragma unroll
                for (int pg = 0; pg < 4; ++pg) acc[pg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a2, bh[pg], acc[pg], 0, 0, 0);
#pragma unroll
                for (int pg = 0; pg < 4; ++pg) acc[pg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, bl[pg], acc[pg], 0, 0, 0);
            }
#pragma unroll
            for (int pg = 0; pg < 4; ++pg) acc[pg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, bh[pg], acc[pg], 0, 0, 0);
#pragma unroll
            for (int pg = 0; pg < 4; ++pg) acc[pg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, bl[pg], acc[pg], 0, 0, 0);
#pragma unroll
            for (int pg = 0; pg < 4; ++pg) acc[pg] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, bh[pg], acc[pg], 0, 0, 0);
        };
        if constexpr (KS != 0) {
#pragma unroll
            for (int j = 0; j < KS; ++j) {
                step(j, j % SF_PF);
            }
        } else {
            for (int jb = 0; jb < ks; jb += SF_PF) {
#pragma unroll
                for (int u = 0; u < SF_PF; ++u)
                    if (jb + u < ks) step(jb + u, u);
            }
        }
        gid = gid_n;
        gid_n = gid_nn;
        // accumulator pg: column = pixel element 16 pg + m, rows = slots 4 kq + i; lane m holds the scale of slot m's row
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float sc = __shfl(ri, 4 * kq + i);
            const int row = t0 + 4 * kq + i;
            if (row < cnt) {
#pragma unroll
                for (int pg = 0; pg < 4; ++pg) S[(size_t)(srb + row) * 64 + 16 * pg + m] = acc[pg][i] * sc;
            }
        }
    }
}

// mask[g] = 1 for every Gaussian that blended into at least one pixel of the view (the rows of the feature gradient
// that can be non-zero): hit flag of the forward per sorted intersection -> its Gaussian.  Benign race (all write 1).
__global__ __launch_bounds__(256) void blended_mask_kernel(int, const int32_t *, const int32_t *, unsigned char *);  // (prototype: -Wmissing-prototypes)
__global__ __launch_bounds__(256) void blended_mask_kernel(int n_isects, const int32_t *__restrict__ hit,
                                                           const int32_t *__restrict__ flatten_ids, unsigned char *__restrict__ mask)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_isects && hit[i]) mask[flatten_ids[i]] = 1;
}

int gags_blended_mask_launch(int n_isects, const int32_t *hit, const int32_t *flatten_ids, unsigned char *mask, hipStream_t st)
{
    GAGS_CLEAR_ERR();
    hipLaunchKernelGGL(blended_mask_kernel, dim3((n_isects + 255) / 256), dim3(256), 0, st, n_isects, hit, flatten_ids, mask);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

// ABS (GAGS_GEOM_ABSGRAD): lanes 6 and 7 of the row carry the wave sums of |g3| and |g4|, the per-pixel terms of v_means2d before
// any reduction across pixels (absgrad, include/gags_raster.h); without it they are the zeros they always were.
template <bool ABS>
__global__ __launch_bounds__(64) void raster_bwd_geom(int width, int height, int tile_w, int n_tiles, int n_gauss,
                                                      const GRec *__restrict__ packed, const int32_t *__restrict__ offsets,
                                                      int n_isects, const int32_t *__restrict__ blk_rows,
                                                      const float *__restrict__ wt, const int32_t *__restrict__ gid_s,
                                                      const int32_t *__restrict__ sidx_s, const float *__restrict__ S,
                                                      const float *__restrict__ Tbuf, const float *__restrict__ v_alphas,
                                                      const float *__restrict__ bgdot, float *__restrict__ grow,
                                                      uint32_t *__restrict__ key, int32_t *__restrict__ idx, int by_gauss,
                                                      const int32_t *__restrict__ row_base, int n_pass, size_t s_stride,
                                                      size_t bg_stride)
{   // n_pass > 1: the dot pass left one S / bgdot buffer per 256-channel pass (s_stride, bg_stride floats apart): summed here
    const int logical = gags_xcd_remap(blockIdx.x, n_tiles * GAGS_BLOCKS_PER_TILE);
    const int blk = logical & 3;
    const int tile = gags_tile_of_order(logical >> 2, tile_w, n_tiles / tile_w);
    const int cnt = blk_rows[tile * GAGS_BLOCKS_PER_TILE + blk];
    if (cnt == 0) return;
    const int start = offsets[tile];
    const int end = offsets[tile + 1]  /* n_tiles + 1 entries: the last one is the intersection count */;
    const int sb = gags_slot_base(start, end, tile, blk);
    // row of slot j: compact numbering (row_base = exclusive prefix sum of blk_rows) or the sparse slot index itself
    const int rb = row_base ? row_base[tile * GAGS_BLOCKS_PER_TILE + blk] : sb;
    const int lane = threadIdx.x;  // = element e of the weight rows: pixel p = e >> 1 of the 8x4 half h = e & 1
    const int ty = tile / tile_w, tx = tile - ty * tile_w;
    const int pj = tx * GAGS_TILE + (blk & 1) * 8 + ((lane >> 1) & 7);
    const int pi = ty * GAGS_TILE + (blk >> 1) * 8 + (lane >> 4) + 4 * (lane & 1);
    const bool inside = pi < height && pj < width;
    const size_t pix = inside ? (size_t)pi * width + pj : 0;
    const float px = (float)pj + 0.5f, py = (float)pi + 0.5f;
    const float T_final = inside ? Tbuf[pix] : 1.f;
    // T_f ra (v_a - <bg, v>): everything but ra is per pixel
    float bgd = 0.f;
    if (bgdot && inside) {
        bgd = bgdot[pix];
        for (int p = 1; p < n_pass; ++p) bgd += bgdot[p * bg_stride + pix];
    }
    const float k0 = inside ? T_final * ((v_alphas ? v_alphas[pix] : 0.f) - bgd) : 0.f;
    float behind = 0.f;  // SUM f S over the slots behind the current one
    // two-deep software pipeline over the slots (back to front): the slot's ids and rows are requested two slots ahead,
    // its packed record (addressed by the id) one slot ahead
    struct Ids { int sx, g; float f, sd; };
    auto fetch_ids = [&](int j) __attribute__((always_inline)) {
        Ids q;
        const int slot = sb + max(j, 0);
        q.sx = sidx_s[slot]; q.g = gid_s[slot];
        q.f = wt[(size_t)slot * 64 + lane];
        const size_t so = (size_t)(rb + max(j, 0)) * 64 + lane;  // S is numbered like the per-slot rows (compact or sparse)
        q.sd = S[so];
        if (n_pass > 1) {  // (uniform; at most four passes: D <= 1024)
            q.sd += S[s_stride + so];
            if (n_pass > 2) q.sd += S[2 * s_stride + so];
            if (n_pass > 3) q.sd += S[3 * s_stride + so];
        }
        return q;
    };
    auto fetch_rec = [&](const Ids &q) __attribute__((always_inline)) {  // (the pad slot's gid is n_gauss: clamped, unused)
        return packed[by_gauss ? min(__builtin_amdgcn_readfirstlane(q.g), n_gauss - 1) : max(__builtin_amdgcn_readfirstlane(q.sx), 0)];
    };
    Ids i1 = fetch_ids(cnt - 1), i2 = fetch_ids(cnt - 2);
    GRec r1 = fetch_rec(i1);
    for (int j = cnt - 1; j >= 0; --j) {
        const Ids cur = i1;
        const GRec r = r1;
        i1 = i2;
        r1 = fetch_rec(i1);
        i2 = fetch_ids(j - 2);
        __builtin_amdgcn_sched_barrier(0);  // keep the requests above the arithmetic of the current slot
        const int row = rb + j;
        const int sx = __builtin_amdgcn_readfirstlane(cur.sx);
        if (sx < 0) {  // pad slot: sorts behind every Gaussian
            if (lane == 0) { key[row] = (uint32_t)n_gauss; idx[row] = row; }
            continue;
        }
        const int g = __builtin_amdgcn_readfirstlane(cur.g);
        const float f = cur.f, sdot = cur.sd;
        const float dx = r.x - px, dy = r.y - py;
        const float sigma = 0.5f * (r.a * dx * dx + r.c * dy * dy) + r.b * dx * dy;
        const float vis = gags_exp_neg(sigma);
        const float alpha = fminf(GAGS_ALPHA_MAX, r.o * vis);
        float g0 = 0.f, g1 = 0.f, g2 = 0.f, g3 = 0.f, g4 = 0.f, g5 = 0.f;
        if (f != 0.f) {  // blended (f = alpha T with alpha >= 1/255 and T > 1e-4)
            const float ra = 1.0f / (1.0f - alpha);
            const float T = f / alpha;
            const float v_alpha = T * sdot - ra * behind + k0 * ra;
            behind = fmaf(f, sdot, behind);
            if (r.o * vis <= GAGS_ALPHA_MAX) {
                const float v_sigma = -r.o * vis * v_alpha;
                g0 = 0.5f * v_sigma * dx * dx;
                g1 = v_sigma * dx * dy;
                g2 = 0.5f * v_sigma * dy * dy;
                g3 = v_sigma * (r.a * dx + r.b * dy);
                g4 = v_sigma * (r.b * dx + r.c * dy);
                g5 = vis * v_alpha;
            }
        }
        g0 = gags_wave_sum(g0); g1 = gags_wave_sum(g1); g2 = gags_wave_sum(g2);
        float g6 = 0.f, g7 = 0.f;
        if constexpr (ABS) { g6 = gags_wave_sum(fabsf(g3)); g7 = gags_wave_sum(fabsf(g4)); }
        g3 = gags_wave_sum(g3); g4 = gags_wave_sum(g4); g5 = gags_wave_sum(g5);
        if (lane < 8) {
            const float v = lane == 0 ? g0 : lane == 1 ? g1 : lane == 2 ? g2 : lane == 3 ? g3 : lane == 4 ? g4 : lane == 5 ? g5
                            : !ABS ? 0.f : lane == 6 ? g6 : g7;
            grow[(size_t)row * 8 + lane] = v;
        }
        if (lane == 0) { key[row] = (uint32_t)g; idx[row] = row; }
    }
}

namespace {
struct GeomScratch {
    float *S, *bgdot, *grow, *rinv;
    size_t s_stride, bg_stride;  // floats from one pass's S / bgdot buffer to the next
    uint32_t *key, *key_s;
    int32_t *idx, *idx_s, *seg;
    uint4 *table;
    unsigned char *mask;
    void *sort;
    int64_t sort_bytes, total;
};
// n_rows < 0: one row per slot of the sparse slot space; else the compact row count (sum of blk_rows).  base NULL: sizes only
inline GeomScratch geom_carve(void *base, int64_t n_isects, int width, int height, int n_gauss, int d, int64_t n_rows)
{
    const int64_t slots = gags_slot_count(n_isects, gags_tiles(width, height).n);
    const int64_t rows = n_rows < 0 ? slots : (n_rows > 0 ? n_rows : 1);
    GagsCarve c(base);
    GeomScratch L;
    const int64_t n_pass = std::max(1, (d + SD_MAXCH - 1) / SD_MAXCH);  // the split-f16 dot pass: one S / bgdot buffer per pass
    L.s_stride = (size_t)al256((rows + 64) * 256) / 4;  // numbered like the per-slot rows: compact (n_rows) or the sparse slot space
    L.bg_stride = (size_t)al256((int64_t)width * height * 4) / 4;
    L.S = c.take<float>(n_pass * (int64_t)L.s_stride);
    L.bgdot = c.take<float>(n_pass * (int64_t)L.bg_stride);
    L.grow = c.take<float>(rows * 8);
    L.key = c.take<uint32_t>(rows);
    L.idx = c.take<int32_t>(rows);
    L.key_s = c.take<uint32_t>(rows);
    L.idx_s = c.take<int32_t>(rows);
    L.seg = c.take<int32_t>((int64_t)n_gauss + 2);
    // split feature table of one pass (<= 256 channels: 6 bytes per channel), 1 / row scale, blended mask
    const int64_t ks = (std::min(d, SD_MAXCH) + 31) / 32;  // 32-channel steps, 192 bytes each
    L.table = c.take<uint4>((int64_t)n_gauss * ks * 12);
    L.rinv = c.take<float>(n_gauss);
    L.mask = c.take<unsigned char>(n_gauss);
    L.sort = c.take_bytes(gags_sort_u32_scratch_bytes(rows));
    L.sort_bytes = c.last();
    L.total = c.total();
    return L;
}
}  // namespace

int64_t gags_raster_bwd_geom_scratch_bytes_impl(int64_t n_isects, int width, int height, int n_gauss, int d, int64_t n_rows)
{
    return geom_carve(nullptr, n_isects, width, height, n_gauss, d, n_rows).total;
}

int gags_raster_bwd_geom_launch(int d, int n_gauss, int width, int height, const float *colors, const float *backgrounds,
                                const int32_t *offsets, int n_isects, const void *packed, const float *v_out,
                                const float *v_alphas, const int32_t *blk_rows, const float *wt, const int32_t *gid_s,
                                const int32_t *sidx_s, const float *Tbuf, void *scratch, int64_t scratch_bytes, float *v_geo,
                                int by_gauss, const int32_t *row_base, int64_t n_rows, const int32_t *hit,
                                const int32_t *flatten_ids, int f32mfma, int absgrad, hipStream_t st)
{
    GAGS_CLEAR_ERR();
    if (d < 16 || d % 8 != 0) return 1;
    if (!row_base) n_rows = -1;
    const GeomScratch L = geom_carve(scratch, n_isects, width, height, n_gauss, d, n_rows);
    if (scratch_bytes < L.total) return GAGS_ESCRATCH;
    const int tile_w = gags_tiles(width, height).w, n_tiles = gags_tiles(width, height).n;
    const int64_t slots = n_rows < 0 ? gags_slot_count(n_isects, n_tiles) : n_rows;  // rows to sort
    float *S = L.S, *bgdot = backgrounds ? L.bgdot : nullptr, *grow = L.grow;
    uint32_t *key = L.key, *key_s = L.key_s;
    int32_t *idx = L.idx, *idx_s = L.idx_s, *seg = L.seg;
    // unused slots of the sparse slot space sort behind every Gaussian (the compact numbering has none)
    if (n_rows < 0 && hipMemsetD32Async((hipDeviceptr_t)key, n_gauss, (size_t)slots, st) != hipSuccess) return GAGS_ELAUNCH;
    static bool raised[GAGS_MAX_DEVICES];
    if (!gags_raise_dynamic_lds(raised, {(const void *)raster_bwd_sdot<SD_MAXCH>, (const void *)raster_bwd_sdot<0>}, 64 * (SD_MAXCH + SD_PAD) * 4))
        return GAGS_ELAUNCH;
    const bool split16 = !f32mfma && hit && flatten_ids;
    // the split-f16 dot pass writes one S / bgdot buffer per 256-channel pass (the fp32 one accumulates in the first)
    const size_t s_stride = L.s_stride, bg_stride = L.bg_stride;
    const int n_pass = split16 ? (d + SD_MAXCH - 1) / SD_MAXCH : 1;
    if (split16) {
        static bool raised16[GAGS_MAX_DEVICES];
        if (!gags_raise_dynamic_lds(raised16, {(const void *)raster_bwd_sdot_f16<SD_MAXCH / 32>, (const void *)raster_bwd_sdot_f16<0>},
                                    2 * 64 * (SD_MAXCH + SF_PADH) * 2))
            return GAGS_ELAUNCH;
        unsigned char *mask = L.mask;
        uint4 *table = L.table;
        float *rinv = L.rinv;
        if (hipMemsetAsync(mask, 0, (size_t)n_gauss, st) != hipSuccess) return GAGS_ELAUNCH;
        if (n_isects > 0) {
            const int rc = gags_blended_mask_launch(n_isects, hit, flatten_ids, mask, st);
            if (rc != GAGS_OK) return rc;
        }
        for (int ch0 = 0; ch0 < d; ch0 += SD_MAXCH) {
            const int ks = (min(SD_MAXCH, d - ch0) + 31) / 32;
            float *S_p = S + (size_t)(ch0 / SD_MAXCH) * s_stride, *bg_p = bgdot ? bgdot + (size_t)(ch0 / SD_MAXCH) * bg_stride : nullptr;
            hipLaunchKernelGGL(feat_split_kernel, dim3((n_gauss + 7) / 8), dim3(256), 0, st, n_gauss, d, ch0, ks, colors, mask, table, rinv);
            const dim3 grid(n_tiles * GAGS_BLOCKS_PER_TILE);
            const size_t lds = (size_t)2 * 64 * (32 * ks + SF_PADH) * 2;
            if (ks == SD_MAXCH / 32)
                hipLaunchKernelGGL(raster_bwd_sdot_f16<SD_MAXCH / 32>, grid, dim3(256), lds, st, d, ch0, ks, width, height, tile_w, n_tiles,
                                   n_gauss, v_out, table, rinv, backgrounds, offsets, n_isects, blk_rows, gid_s, S_p, bg_p, row_base);
            else
                hipLaunchKernelGGL(raster_bwd_sdot_f16<0>, grid, dim3(256), lds, st, d, ch0, ks, width, height, tile_w, n_tiles,
                                   n_gauss, v_out, table, rinv, backgrounds, offsets, n_isects, blk_rows, gid_s, S_p, bg_p, row_base);
        }
    }
    for (int ch0 = 0; ch0 < d && !split16; ch0 += SD_MAXCH) {
        const int dch = min(SD_MAXCH, d - ch0);
        const dim3 grid(n_tiles * GAGS_BLOCKS_PER_TILE);
        const size_t lds = (size_t)64 * (dch + SD_PAD) * 4;
        if (dch == SD_MAXCH)
            hipLaunchKernelGGL(raster_bwd_sdot<SD_MAXCH>, grid, dim3(256), lds, st, d, ch0, dch, width, height, tile_w, n_tiles, n_gauss,
                               v_out, colors, backgrounds, offsets, n_isects, blk_rows, gid_s, S, bgdot, ch0 > 0 ? 1 : 0, row_base);
        else
            hipLaunchKernelGGL(raster_bwd_sdot<0>, grid, dim3(256), lds, st, d, ch0, dch, width, height, tile_w, n_tiles, n_gauss,
                               v_out, colors, backgrounds, offsets, n_isects, blk_rows, gid_s, S, bgdot, ch0 > 0 ? 1 : 0, row_base);
    }
    hipLaunchKernelGGL(absgrad ? raster_bwd_geom<true> : raster_bwd_geom<false>, dim3(n_tiles * GAGS_BLOCKS_PER_TILE), dim3(64), 0, st,
                       width, height, tile_w, n_tiles, n_gauss, reinterpret_cast<const GRec *>(packed), offsets, n_isects, blk_rows, wt,
                       gid_s, sidx_s, S, Tbuf, v_alphas, bgdot, grow, key, idx, by_gauss, row_base, n_pass, s_stride, bg_stride);
    GAGS_CHECK_LAUNCH();
    int rc = gags_rows_group_launch(slots, n_gauss, nullptr, key, idx, key_s, idx_s, seg, L.sort, L.sort_bytes, st);
    if (rc != GAGS_OK) return rc;
    rc = gags_rows_reduce_launch(n_gauss, 8, 0, 8, seg, idx_s, grow, 8, v_geo, false, st);
    if (rc != GAGS_OK) return rc;
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
