// The 64-pixel tile machinery of CNN_decoder's fused chains, shared by csrc/decoder_fused.hip (training: forward + input-gradient
// chain) and csrc/decoder_query.hip (inference: forward chain + relevancy head): the LDS tile type, the weight-fragment stream
// (WFrag / wprefetch / layer_main), the hidden-layer epilogue and the in-place residual sum.  One copy, so that the query
// kernel's hidden layers are the training forward's arithmetic bit for bit.  Like decoder_common.h: only types, constants and
// forceinline device functions (internal linkage: both files are compiled twice, csrc/half16.h).
#pragma once
#include "decoder_common.h"

namespace {

typedef float ff32x2_t __attribute__((ext_vector_type(2)));
// (pairs are packed with h16_pack_sat throughout: both kernels set the mode first, csrc/half16.h)

#ifndef GAGS_ABL
#define GAGS_ABL 0  // timing-only ablations of the fused kernels (tools/chain_bench.py; results are WRONG with any of them): 1 no HBM
                    // stores (64 masks / 128 tiles / 256 logits alone), 2 no weight refills, 4 no MFMAs, 16 no B reads, 32 plain stores, 512 tile stores into 2 MB per tensor;
                    // csrc/decoder_query.hip (tools/query_bench.py --lib): 1024 no phrase dots, 2048 no head reads of the logits patch at all
#endif
constexpr int FT = 64;        // pixels per tile and group of four waves; a workgroup holds PH such groups (tile = 64 PH pixels)
constexpr int FH = 256;       // hidden width
constexpr int FLD = FH + 8;   // LDS row pitch in bf16 (528 B: 16-byte aligned rows, consecutive rows 4 banks apart)
constexpr int FPD = 8;        // weight fragments are requested this many K-steps ahead

typedef unsigned short (*Tile)[FLD];

// the tiles' HBM stores are non-temporal (`nt`): 10.6 GB per 1080p forward that nothing reads before the kernel ends stream past
// the L2 the weight fragments live in (round 6: -2 %; GAGS_ABL & 32 restores plain stores)
template <class V>  // uint4 or float4
__device__ __forceinline__ void stream_store(V *dst, V v)
{
    if (!(GAGS_ABL & 32)) nt_store(dst, v);
    else *dst = v;
}

// Weights arrive in MFMA-FRAGMENT order (gags_amd/decoders.py: _frag_layout): Wf[n_tile][k_step][lane][8] with lane =
// 32 kh + n and the eight values k = 16 k_step + 8 kh + 0..7 of row 32 n_tile + n -- the A operand of one MFMA is one
// contiguous, fully coalesced kilobyte, and every weight byte travels from L2 exactly once per tile.  (Read from the
// row-major matrix, a fragment is 32 row pieces of 32 bytes, one per 128-byte line: the eight waves of a CU keep 64 KB of
// such lines in flight, the L1 thrashes, and every line is fetched four times -- measured 5.8 ms instead of 2.)
// acc[i][j] (i: 32 channels of n-tile nt0 + i, j: 32 pixels 32 j..) = sum over k-steps ks0 .. ks0 + ksteps - 1 of W[n][k] in[p][k]
struct WFrag {
    bf16x8 a0[FPD], a1[FPD];
};

// the first FPD K-steps' weight fragments of a layer: issued BEFORE the epilogue of the layer above (and before its tile
// stores), so that their L2 latency hides behind that epilogue instead of opening every layer
__device__ __forceinline__ void wprefetch(WFrag &f, const unsigned short *__restrict__ Wf, int ksteps_total, int nt0, int ks0, int ksteps,
                                          int lane)
{
    const unsigned short *w0 = Wf + ((size_t)nt0 * ksteps_total + ks0) * 512 + lane * 8;
    const unsigned short *w1 = w0 + (size_t)ksteps_total * 512;
#pragma unroll
    for (int q = 0; q < FPD; ++q) {
        const int ks = min(q, ksteps - 1);
        f.a0[q] = *reinterpret_cast<const bf16x8 *>(w0 + 512 * ks);
        f.a1[q] = *reinterpret_cast<const bf16x8 *>(w1 + 512 * ks);
    }
}

__device__ __forceinline__ void layer_main(f32x16 (&acc)[2][2], WFrag &f, const unsigned short *__restrict__ Wf, int ksteps_total, int nt0,
                                           int ks0, int ksteps, Tile in, int lane, bool zero, int poff)
{
    if (zero) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    }
    const unsigned short *w0 = Wf + ((size_t)nt0 * ksteps_total + ks0) * 512 + lane * 8;
    const unsigned short *w1 = w0 + (size_t)ksteps_total * 512;
    for (int k0 = 0; k0 < ksteps; k0 += FPD) {
#pragma unroll
        for (int q = 0; q < FPD; ++q) {
            const int ks = k0 + q;
            const bf16x8 c0 = f.a0[q], c1 = f.a1[q];
            const int kn = min(ks + FPD, ksteps - 1);  // (past the end: a harmless re-read)
            if (!(GAGS_ABL & 2)) {
            f.a0[q] = *reinterpret_cast<const bf16x8 *>(w0 + 512 * kn);
            f.a1[q] = *reinterpret_cast<const bf16x8 *>(w1 + 512 * kn);
            }
            if (ks < ksteps) {  // (uniform)
                bf16x8 b0 = c0, b1 = c1;
                if (!(GAGS_ABL & 16)) {
                b0 = *reinterpret_cast<const bf16x8 *>(&in[poff + (lane & 31)][16 * ks + 8 * (lane >> 5)]);
                b1 = *reinterpret_cast<const bf16x8 *>(&in[poff + 32 + (lane & 31)][16 * ks + 8 * (lane >> 5)]);
                }
                if (!(GAGS_ABL & 4)) {
                acc[0][0] = h16_mfma(c0, b0, acc[0][0]);
                acc[0][1] = h16_mfma(c0, b1, acc[0][1]);
                acc[1][0] = h16_mfma(c1, b0, acc[1][0]);
                acc[1][1] = h16_mfma(c1, b1, acc[1][1]);
                } else { acc[0][0][0] += (float)b0[0] + (float)c0[0]; acc[1][1][0] += (float)b1[0] + (float)c1[0]; }
            }
            __builtin_amdgcn_sched_barrier(0);  // keep the prefetch FPD steps ahead (the scheduler sinks loads to their use)
        }
    }
}

// accumulator element (i, j, 4 g + e) of lane (p = lane & 31, h = lane >> 5): pixel 32 j + p, channel n_base + 32 i + 8 g + 4 h + e
// hidden-layer epilogue: out[p][n] = bf16(relu(acc + bias[n])); and, for the backward, the ReLU decisions as BITS:
// word n / 32 of a pixel holds [out > 0] of 32 channels (channel 8 g + 4 h + e of the word at bit 8 h + 2 g + (e >> 1) + 16 (e & 1));
// words are stored word-major inside 64-pixel groups, mask[(group * 8 + word) * 64 + pixel % 64]: both private to these two kernels -- 32 bytes per pixel and layer instead of the 512-byte activation row
// the input-gradient chain would otherwise re-read just for its sign.
__device__ __forceinline__ void epilogue_hidden(const f32x16 (&acc)[2][2], const float *__restrict__ bias, int n_base, Tile out,
                                                int lane, unsigned *__restrict__ mask, int64_t p0, int64_t P, int poff)
{
    // 64 values per lane and layer: this epilogue costs more issue slots than the layer's MFMAs (timestamps, round 3), so
    // it runs on packed instructions: v_pk_add_f32 (bias), v_cvt_pk_bf16_f32, then the ReLU on the PAIR -- v_pk_max_i16
    // with 0 (a negative bf16 is a negative int16; rounding first and clamping second gives the same bits) -- and the
    // ReLU decisions from v_pk_min_u16(pair, 1).  (Written as inline asm: the builtins' IEEE semantics expand to compares.)
    const int p = lane & 31, h = lane >> 5;
    unsigned bits[2][2] = {{0u, 0u}, {0u, 0u}};
    const unsigned one2 = 0x00010001u;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int n = n_base + 32 * i + 8 * g + 4 * h;
            const float4 b = *reinterpret_cast<const float4 *>(bias + n);
            const ff32x2_t b01 = {b.x, b.y}, b23 = {b.z, b.w};
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const ff32x2_t a01 = {acc[i][j][4 * g], acc[i][j][4 * g + 1]}, a23 = {acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
                const ff32x2_t v01 = a01 + b01, v23 = a23 + b23;
                unsigned u0 = h16_pack_sat(v01[0], v01[1]);
                unsigned u1 = h16_pack_sat(v23[0], v23[1]);
                unsigned m0, m1;
                asm("v_pk_max_i16 %0, %1, 0" : "=v"(u0) : "v"(u0));
                asm("v_pk_max_i16 %0, %1, 0" : "=v"(u1) : "v"(u1));
                asm("v_pk_min_u16 %0, %1, %2" : "=v"(m0) : "v"(u0), "v"(one2));
                asm("v_pk_min_u16 %0, %1, %2" : "=v"(m1) : "v"(u1), "v"(one2));
                *reinterpret_cast<uint2 *>(&out[poff + 32 * j + p][n]) = make_uint2(u0, u1);
                // m0 / m1 carry the decisions of elements (0, 1) / (2, 3) at bits 0 and 16: shifted in as they are, two
                // v_lshl_or per group (round 6; assembling a nibble per group first cost eight) -- the word's layout is private to
                // the two fused kernels: element e of group g of half h at bit 8 h + 2 g + (e >> 1) + 16 (e & 1)
                bits[i][j] |= m0 << (2 * g);
                bits[i][j] |= m1 << (2 * g + 1);
            }
        }
    if (mask) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const unsigned mine = bits[i][j] << (8 * h);  // this half-wave's bits sit at 8 h + 0..7 and 8 h + 16..23
                const auto sw = __builtin_amdgcn_permlane32_swap(mine, mine, false, false);
                const unsigned word = sw[0] | sw[1];
                const int64_t pg = p0 + poff + 32 * j + p;
                // word-major inside a 64-pixel group (round 6): the 32 lanes of a store write 128 contiguous bytes (pixel-major,
                // 8 words per pixel, they wrote 4 bytes every 32: the masks were 5 % of the kernel's bytes and 5 % of its time)
                if (h == 0 && pg < P && !(GAGS_ABL & (1 | 64)))
                    mask[(((p0 + poff) >> 6) * 8 + (n_base >> 5) + i) * 64 + 32 * j + p] = word;
            }
    }
}

// the sum of eight packed values: added in fp32, rounded once (add_h16x2 with the mode's saturation)
__device__ __forceinline__ uint4 add_sat_h16x8(uint4 x, uint4 y)
{
    return make_uint4(h16_pack_sat(h16_lo(x.x) + h16_lo(y.x), h16_hi(x.x) + h16_hi(y.x)), h16_pack_sat(h16_lo(x.y) + h16_lo(y.y), h16_hi(x.y) + h16_hi(y.y)),
                      h16_pack_sat(h16_lo(x.z) + h16_lo(y.z), h16_hi(x.z) + h16_hi(y.z)), h16_pack_sat(h16_lo(x.w) + h16_lo(y.w), h16_hi(x.w) + h16_hi(y.w)));
}

// dst[p][:] = bf16(dst + add) element-wise in LDS (fp32 add, one rounding: what gags_decoder_layer does with two sources)
template <int NT>
__device__ __forceinline__ void add_tile(Tile dst, Tile add, int tid)
{
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int id = tid + NT * q, row = id >> 5, c = (id & 31) * 8;
        const uint4 x = *reinterpret_cast<const uint4 *>(&dst[row][c]), y = *reinterpret_cast<const uint4 *>(&add[row][c]);
        *reinterpret_cast<uint4 *>(&dst[row][c]) = add_sat_h16x8(x, y);
    }
}

}  // namespace
