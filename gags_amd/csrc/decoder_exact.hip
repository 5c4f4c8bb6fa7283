// N1 at the reference's precision (VERDICT r2 "a decoder mode at the reference's precision").
// models/networks.py:109-248 are fp32 Conv2d stacks; gfx950 has no TF32 and its fp32 matrix rate (157 TFLOP/s) would cost
// >= 50 ms per iteration.  Here every fp32 operand is written as THREE bfloat16 terms,
//     a = h + m + l,   h = bf16(a),  m = bf16(a - h),  l = bf16(a - h - m)        (exact: 3 x 8 significand bits >= 24)
// and a product as the six MFMA terms of order <= 2,
//     a b ~ h h' + h m' + m h' + h l' + m m' + l h'                               (dropped: <= 2^-24 |a b|, below fp32 rounding)
// on v_mfma_f32_32x32x16_bf16 with fp32 accumulation: the arithmetic of an fp32 GEMM at 2.6x the fp32 matrix rate.
// Activations, gradients and weights are fp32 in memory; the split happens on the way into LDS.
// One tile kernel serves
//   layers / input gradients   Y[p, n] = (act(sum_k (A1 + A2)[p, k] W[n, k] + bias[n]) + E[p, n]) * (mask_src[p, n] > 0)
//   weight gradients           dW[n, k] = sum_p dZ[p, n] (A1 + A2)[p, k]   (contraction over the SLOW index of both operands:
//                              the loader transposes; pixel chunks -> partial matrices -> summed in chunk order: NO atomics,
//                              bit-reproducible)
// plus the bias gradient (column sums, same two deterministic stages) and the output heads' backward in fp32.
//
// A second tier, NT = 2 (gags_decoder_layer_split / gags_decoder_wgrad_split with terms = 2; round 4): every operand as TWO
// bfloat16 terms, a = h + m + O(2^-17 |a|) (16 significand bits), a product as its three terms of order <= 1,
//     a b ~ h h' + h m' + m h'                                                    (dropped: m m' <= 2^-18 |a b|)
// i.e. a relative error <= ~2^-16 per product -- 32x tighter than the TF32 arithmetic (10-bit significands) torch runs the
// reference's nn.Conv2d stacks in by default on the GPU its README names -- at half the matrix work and two thirds of the
// split / LDS work of the exact tier.  fp32 tensors in memory, fp32 accumulation, the same deterministic reductions.
#include "decoder_common.h"
#include "launch.h"
#ifdef GAGS_H16
#error "decoder_exact.hip splits fp32 into bfloat16 terms: it is compiled once, without -DGAGS_H16"
#endif

namespace {

constexpr int XM = 128, XN = 128, XK = 32;  // workgroup tile: 128 x 128 outputs, 32 contraction elements per step
constexpr int XLD = XK + 8;                 // LDS row pitch in bf16 (80 B: 16-byte aligned rows, banks spread)
// (the kernels are templates over the number of bf16 terms per operand, NT in {3: exact, 2: bf16x2})

// (a, b) -> NT packed bf16 pairs t[s] = (term s of a) | (term s of b) << 16; NT = 3: x = h + m + l exactly; NT = 2: h + m
template <int NT>
__device__ __forceinline__ void split3x2(float a, float b, unsigned (&t)[NT])
{
    t[0] = h16_pack(a, b);
    float ra = a - __uint_as_float(t[0] << 16), rb = b - __uint_as_float(t[0] & 0xffff0000u);
    t[1] = h16_pack(ra, rb);
    if constexpr (NT == 3) {
        ra -= __uint_as_float(t[1] << 16); rb -= __uint_as_float(t[1] & 0xffff0000u);
        t[2] = h16_pack(ra, rb);
    }
}

struct XArgs {
    const float *A1, *A2;   // NT: [M, K] rows contiguous in K.   TN: [P, M] (the contraction index p is the slow one)
    const float *B;         // NT: [N, K].                        TN: [P, N]
    const float *B2;        // TN only: second activation source, summed with B
    const float *bias, *mask_src, *E;
    float *Y, *Ypre;
    int64_t M;              // NT: rows of Y (pixels).  TN: unused
    int N, K;               // NT: columns of Y, contraction length.  TN: output is [Mo, No]
    int lda, ldb, ldy, relu;
    int Mo, No;             // TN: output rows (n_out) / columns (k_in)
    int64_t P, chunk;       // TN: contraction length and pixels per workgroup
    float *part;            // TN: partial outputs [n_chunks][Mo * No]
    unsigned m_tiles, n_tiles;  // NT: tile counts (the workgroup index is decoded XCD-aware)
    float *bias_part;       // TN: partial column sums of A1 (the bias gradient) [n_chunks][Mo], or null
    int vout;               // NT: the epilogue may move float4 pieces of rows (N % 4 == 0, ldy % 4 == 0, aligned outputs)
};

// Staging is split in two so that the global loads of step s + 1 are in flight while step s multiplies:
//   fetch_*  : global -> registers (4 x float4 per thread and operand; addresses clamped, out-of-range elements zeroed)
//   commit_* : registers -> split into three bf16 planes -> LDS
// rows [r0, r0 + 128) x contraction [k0, k0 + 32) of a row-major fp32 matrix (+ optional second summand)
// Every load is unconditional (addresses clamped into the matrix, out-of-range elements replaced by zero afterwards): a
// guarded load is a branch and a wait of its own, and eight of them in a row serialise the whole prefetch.
// VEC: K % 4 == 0, ld % 4 == 0 and 16-byte aligned bases (checked by the entry) -> one float4 per row piece.
template <bool TWO, bool VEC>
__device__ __forceinline__ void fetch_rows(float (&v)[4][4], const float *__restrict__ a1, const float *__restrict__ a2, int ld,
                                           int64_t r0, int64_t rows, int k0, int K, int tid)
{
    const int kc = k0 + (tid & 7) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int64_t rg = r0 + (tid >> 3) + 32 * q;
        const bool rok = rg < rows;
        const size_t base = (size_t)(rok ? rg : rows - 1) * ld;
        if constexpr (VEC) {
            const bool ok = rok && kc < K;  // K % 4 == 0: the piece is inside or outside as a whole
            const size_t o = base + (kc < K ? kc : 0);
            float4 u = *reinterpret_cast<const float4 *>(a1 + o);
            if constexpr (TWO) {
                const float4 w = *reinterpret_cast<const float4 *>(a2 + o);
                u.x += w.x; u.y += w.y; u.z += w.z; u.w += w.w;
            }
            v[q][0] = ok ? u.x : 0.f; v[q][1] = ok ? u.y : 0.f; v[q][2] = ok ? u.z : 0.f; v[q][3] = ok ? u.w : 0.f;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool ok = rok && kc + e < K;
                const size_t o = base + (kc + e < K ? kc + e : 0);
                float x = a1[o];
                if constexpr (TWO) x += a2[o];
                v[q][e] = ok ? x : 0.f;
            }
        }
    }
}

template <int NT>
__device__ __forceinline__ void commit_rows(unsigned short (*S)[XM][XLD], const float (&v)[4][4], int tid)
{
    const int kc = (tid & 7) * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int r = (tid >> 3) + 32 * q;
        unsigned t01[NT], t23[NT];
        split3x2<NT>(v[q][0], v[q][1], t01);
        split3x2<NT>(v[q][2], v[q][3], t23);
#pragma unroll
        for (int s = 0; s < NT; ++s) *reinterpret_cast<uint2 *>(&S[s][r][kc]) = make_uint2(t01[s], t23[s]);
    }
}

// TN: pixels [p0, p0 + 32) x columns [c0, c0 + 128) of src [P, C]: thread = ONE column x 16 consecutive pixels.  The
// lanes of a wave read 64 consecutive floats of a pixel row (coalesced) and later write 64 consecutive LDS rows (banks
// spread); with four columns per thread the rows written by a wave were 320 B apart: 8-way bank conflicts.
template <bool TWO>
__device__ __forceinline__ void fetch_cols(float (&v)[16], const float *__restrict__ s1, const float *__restrict__ s2, int ld,
                                           int64_t p0, int64_t p_end, int c0, int C, int tid)
{
    const int c = c0 + (tid & 127);
    const int64_t pg0 = p0 + 16 * (tid >> 7);
    const bool cin = c < C;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t pg = pg0 + i;
        const bool ok = cin && pg < p_end;
        const size_t o = (size_t)(ok ? pg : p_end - 1) * ld + (cin ? c : c0);  // clamped: the load itself is unconditional
        float x = s1[o];
        if constexpr (TWO) x += s2[o];
        v[i] = ok ? x : 0.f;
    }
}

// ... -> S[term][column][pixel]: four 8-byte stores per term (four consecutive pixels each: the transposition)
template <int NT>
__device__ __forceinline__ void commit_cols(unsigned short (*S)[XM][XLD], const float (&v)[16], int tid)
{
    const int c = tid & 127, sp = 16 * (tid >> 7);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        unsigned t01[NT], t23[NT];
        split3x2<NT>(v[4 * j], v[4 * j + 1], t01);
        split3x2<NT>(v[4 * j + 2], v[4 * j + 3], t23);
#pragma unroll
        for (int s = 0; s < NT; ++s) *reinterpret_cast<uint2 *>(&S[s][c][sp + 4 * j]) = make_uint2(t01[s], t23[s]);
    }
}

// one 32-wide contraction step from LDS: each wave owns 64 x 64 outputs (2 x 2 MFMA tiles)
template <int NT>
__device__ __forceinline__ void tile_step(f32x16 (&acc)[2][2], unsigned short (*Xs)[XM][XLD], unsigned short (*Ys)[XN][XLD], int wy,
                                          int wx, int lane)
{
#pragma unroll
    for (int ks = 0; ks < XK; ks += 16) {
        bf16x8 a[2][NT], b[2][NT];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int s = 0; s < NT; ++s) {
                a[i][s] = *reinterpret_cast<const bf16x8 *>(&Xs[s][wy * 64 + i * 32 + (lane & 31)][ks + 8 * (lane >> 5)]);
                b[i][s] = *reinterpret_cast<const bf16x8 *>(&Ys[s][wx * 64 + i * 32 + (lane & 31)][ks + 8 * (lane >> 5)]);
            }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                // smallest terms first
                if constexpr (NT == 3) {
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][2], b[j][0], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][1], b[j][1], acc[i][j], 0, 0, 0);
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][2], acc[i][j], 0, 0, 0);
                }
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][1], b[j][0], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][1], acc[i][j], 0, 0, 0);
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i][0], b[j][0], acc[i][j], 0, 0, 0);
            }
    }
}

constexpr int XOP = XN + 4;  // output tile pitch in floats (528 B rows: 16-byte aligned)
// (NT = 2 with three workgroups per CU, its 40 KB of operand images would allow it: measured 1.46 -> 2.28 ms per 256 x 256
// layer -- the 170-register budget spills the accumulators -- and no change for the weight-gradient kernel; two it stays)
template <bool TWO, bool VEC, int NT>
__global__ __launch_bounds__(256, 2) void gemm_x3_nt_kernel(XArgs g)
{
    // one buffer: the operand images during the K loop (2 x 3 x 128 x 40 bf16 = 60 KB), then the fp32 output tile of the
    // epilogue (128 x 132 floats = 66 KB); two workgroups per CU either way
    constexpr int OPER = 2 * NT * XM * XLD * 2, OUTB = XM * XOP * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[OPER > OUTB ? OPER : OUTB];
    unsigned short (*Xs)[XM][XLD] = reinterpret_cast<unsigned short (*)[XM][XLD]>(smem);
    unsigned short (*Ys)[XN][XLD] = reinterpret_cast<unsigned short (*)[XN][XLD]>(smem + NT * XM * XLD * 2);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wy = wave >> 1, wx = wave & 1;
    // the column tiles of one pixel tile run back to back on the SAME XCD (workgroups are dealt round-robin over the 8
    // XCDs, each with its own L2): the second one finds the activation rows in that L2 instead of re-reading HBM
    const unsigned xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const unsigned mt = (slot / g.n_tiles) * 8 + xcd;
    if (mt >= g.m_tiles) return;
    const int64_t m0 = (int64_t)mt * XM;
    const int n0 = (int)(slot % g.n_tiles) * XN;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    float va[4][4], vb[4][4];
    fetch_rows<TWO, VEC>(va, g.A1, g.A2, g.lda, m0, g.M, 0, g.K, tid);
    fetch_rows<false, VEC>(vb, g.B, nullptr, g.ldb, n0, g.N, 0, g.K, tid);
    for (int k0 = 0; k0 < g.K; k0 += XK) {
        commit_rows<NT>(Xs, va, tid);
        commit_rows<NT>(Ys, vb, tid);
        __syncthreads();
        // next step's operands: in flight while this one multiplies (past the end: clamped re-reads, never committed)
        fetch_rows<TWO, VEC>(va, g.A1, g.A2, g.lda, m0, g.M, k0 + XK, g.K, tid);
        fetch_rows<false, VEC>(vb, g.B, nullptr, g.ldb, n0, g.N, k0 + XK, g.K, tid);
        __builtin_amdgcn_sched_barrier(0);  // (the scheduler would sink the loads to their use after the MFMAs)
        tile_step<NT>(acc, Xs, Ys, wy, wx, lane);
        __syncthreads();
    }
    if (g.vout) {  // (uniform)
        // Epilogue through LDS (N % 4 == 0, ldy % 4 == 0, 16-byte aligned outputs): the accumulators (+ bias, ReLU) go to a fp32 tile in the buffer the operand
        // images no longer need, then every thread handles whole float4 pieces of rows -- residual, pre-mask copy, mask and
        // the result move as 16-byte accesses of full lines.  (Straight from the accumulators every access is 4 bytes per
        // lane, 64 stores and up to 128 loads per lane: 38 % of this kernel's time, timestamps of round 3.)
        float (*T)[XOP] = reinterpret_cast<float (*)[XOP]>(smem);
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int nl = wx * 64 + j * 32 + (lane & 31);
                const float bv = g.bias ? g.bias[min(n0 + nl, g.N - 1)] : 0.f;
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int pl = wy * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                    float v = acc[i][j][r] + bv;
                    if (g.relu) v = fmaxf(v, 0.f);
                    T[pl][nl] = v;
                }
            }
        __syncthreads();
#pragma unroll
        for (int q0 = 0; q0 < 16; q0 += 8) {  // two batches of eight pieces: every load of a batch before its first store
            float4 ev[8], mv[8];
            size_t o[8];
            bool in[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int id = tid + 256 * (q0 + q), row = id >> 5, c = (id & 31) * 4;
                const int64_t p = m0 + row;
                in[q] = p < g.M && n0 + c < g.N;  // (N % 4 == 0: a piece is inside or outside as a whole)
                o[q] = (size_t)min(p, g.M - 1) * g.ldy + min(n0 + c, g.N - 4);
            }
            if (g.E) {
#pragma unroll
                for (int q = 0; q < 8; ++q) ev[q] = *reinterpret_cast<const float4 *>(g.E + o[q]);
            }
            if (g.mask_src) {
#pragma unroll
                for (int q = 0; q < 8; ++q) mv[q] = *reinterpret_cast<const float4 *>(g.mask_src + o[q]);
            }
            if (g.E) {
#pragma unroll
                for (int q = 0; q < 8; ++q) { asm volatile("" : "+v"(ev[q].x)); asm volatile("" : "+v"(ev[q].y)); asm volatile("" : "+v"(ev[q].z)); asm volatile("" : "+v"(ev[q].w)); }
            }
            if (g.mask_src) {
#pragma unroll
                for (int q = 0; q < 8; ++q) { asm volatile("" : "+v"(mv[q].x)); asm volatile("" : "+v"(mv[q].y)); asm volatile("" : "+v"(mv[q].z)); asm volatile("" : "+v"(mv[q].w)); }
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const int id = tid + 256 * (q0 + q), row = id >> 5, c = (id & 31) * 4;
                float4 v = *reinterpret_cast<const float4 *>(&T[row][c]);
                if (g.E) { v.x += ev[q].x; v.y += ev[q].y; v.z += ev[q].z; v.w += ev[q].w; }
                if (g.Ypre && in[q]) *reinterpret_cast<float4 *>(g.Ypre + o[q]) = v;
                if (g.mask_src) {
                    v.x = mv[q].x > 0.f ? v.x : 0.f; v.y = mv[q].y > 0.f ? v.y : 0.f;
                    v.z = mv[q].z > 0.f ? v.z : 0.f; v.w = mv[q].w > 0.f ? v.w : 0.f;
                }
                if (g.Y && in[q]) *reinterpret_cast<float4 *>(g.Y + o[q]) = v;
            }
        }
        return;
    }
    // accumulator of tile (i, j): column = lane & 31 -> n, rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -> pixel.
    // The residual / mask rows of a tile are requested together, unconditionally (clamped addresses), before any of
    // them is used: sixteen guarded loads in a row would cost sixteen memory latencies.
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wx * 64 + j * 32 + (lane & 31);
            const int nc = min(n, g.N - 1);
            const float bv = g.bias ? g.bias[nc] : 0.f;
            size_t o[16];
            float ev[16], mv[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t p = m0 + wy * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                o[r] = (size_t)min(p, g.M - 1) * g.ldy + nc;
            }
            if (g.E) {
#pragma unroll
                for (int r = 0; r < 16; ++r) ev[r] = g.E[o[r]];
            }
            if (g.mask_src) {
#pragma unroll
                for (int r = 0; r < 16; ++r) mv[r] = g.mask_src[o[r]];
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t p = m0 + wy * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                float v = acc[i][j][r] + bv;
                if (g.relu) v = fmaxf(v, 0.f);
                if (g.E) v += ev[r];
                const bool in = p < g.M && n < g.N;
                if (g.Ypre && in) g.Ypre[o[r]] = v;
                if (g.mask_src) v = mv[r] > 0.f ? v : 0.f;
                if (g.Y && in) g.Y[o[r]] = v;
            }
        }
}

template <bool TWO, int NT>
__global__ __launch_bounds__(256, 2) void gemm_x3_tn_kernel(XArgs g)
{
    __shared__ __attribute__((aligned(16))) unsigned short Xs[NT][XM][XLD];
    __shared__ __attribute__((aligned(16))) unsigned short Ys[NT][XN][XLD];
    __shared__ float bsh[2][XM];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wy = wave >> 1, wx = wave & 1;
    const int64_t pa = (int64_t)blockIdx.x * g.chunk, pb = min(pa + g.chunk, g.P);
    const int m0 = blockIdx.y * XM, n0 = blockIdx.z * XN;
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // bias gradient on the way: column sums of dz over the chunk, this thread's column and pixel half, in pixel order
    const bool do_bias = g.bias_part != nullptr && blockIdx.z == 0;
    float bsum = 0.f;
    float va[16], vb[16];
    fetch_cols<false>(va, g.A1, nullptr, g.lda, pa, pb, m0, g.Mo, tid);
    fetch_cols<TWO>(vb, g.B, g.B2, g.ldb, pa, pb, n0, g.No, tid);
    for (int64_t p0 = pa; p0 < pb; p0 += XK) {
        commit_cols<NT>(Xs, va, tid);
        commit_cols<NT>(Ys, vb, tid);
        if (do_bias) {
#pragma unroll
            for (int i = 0; i < 16; ++i) bsum += va[i];
        }
        __syncthreads();
        // next step's operands: in flight while this one multiplies (past the end: clamped re-reads, never committed)
        fetch_cols<false>(va, g.A1, nullptr, g.lda, p0 + XK, pb, m0, g.Mo, tid);
        fetch_cols<TWO>(vb, g.B, g.B2, g.ldb, p0 + XK, pb, n0, g.No, tid);
        __builtin_amdgcn_sched_barrier(0);
        tile_step<NT>(acc, Xs, Ys, wy, wx, lane);
        __syncthreads();
    }
    float *out = g.part + (size_t)blockIdx.x * g.Mo * g.No;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = n0 + wx * 64 + j * 32 + (lane & 31);
            if (k >= g.No) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = m0 + wy * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (n < g.Mo) out[(size_t)n * g.No + k] = acc[i][j][r];
            }
        }
    if (do_bias) {  // (uniform over the workgroup)
        bsh[tid >> 7][tid & 127] = bsum;
        __syncthreads();
        if (tid < XM && m0 + tid < g.Mo) g.bias_part[(size_t)blockIdx.x * g.Mo + m0 + tid] = bsh[0][tid] + bsh[1][tid];
    }
}

// out[e] = sum over the chunks, in chunk order (fixed => reproducible); the loads of 16 chunks are issued together (a
// plain loop waited one memory latency per chunk: 0.14 ms per call with 512 chunks)
__global__ __launch_bounds__(256) void sum_parts_kernel(int n_chunks, int64_t elems, const float *__restrict__ part,
                                                        float *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= elems) return;
    float s = 0.f;
    int c = 0;
    for (; c + 16 <= n_chunks; c += 16) {
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = part[(size_t)(c + i) * elems + e];
#pragma unroll
        for (int i = 0; i < 16; ++i) s += v[i];
    }
    for (; c < n_chunks; ++c) s += part[(size_t)c * elems + e];
    out[e] = s;
}

// backward of the output heads in fp32 (see decoder_head.hip head_bwd_kernel): one wave per pixel
//   mode 0 (y = x / max(||x||, eps)):  dz = (g - y <y, g>) / max(||x||, eps);   mode 1 (softmax):  dz = y (g - <y, g>)
constexpr int HX_MAX = 16;  // values of a row per lane: C <= 1024
__global__ __launch_bounds__(256) void head_bwd_exact_kernel(int64_t P, int C, int ldx, int mode, const float *__restrict__ x,
                                                             const float *__restrict__ G, int layout, float *__restrict__ dz,
                                                             int lddz)
{
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= P) return;
    float xv[HX_MAX], gv[HX_MAX];  // the logits and the cotangent of this pixel: read once
    float s = 0.f, m = -3.0e38f;
#pragma unroll
    for (int q = 0; q < HX_MAX; ++q) {
        const int c = lane + 64 * q;
        xv[q] = gv[q] = 0.f;
        if (c < C) {
            xv[q] = x[p * ldx + c];
            gv[q] = layout == 1 ? G[p * C + c] : G[(size_t)c * P + p];
            s = fmaf(xv[q], xv[q], s);
            m = fmaxf(m, xv[q]);
        }
    }
    for (int off = 32; off > 0; off >>= 1) { s += __shfl_xor(s, off, 64); m = fmaxf(m, __shfl_xor(m, off, 64)); }
    float z = 0.f;
    if (mode == 1) {
#pragma unroll
        for (int q = 0; q < HX_MAX; ++q)
            if (lane + 64 * q < C) z += expf(xv[q] - m);
        for (int off = 32; off > 0; off >>= 1) z += __shfl_xor(z, off, 64);
    }
    const float nrm = fmaxf(sqrtf(s), 1e-12f);
    float dot = 0.f;
#pragma unroll
    for (int q = 0; q < HX_MAX; ++q)
        if (lane + 64 * q < C) dot = fmaf(mode == 0 ? xv[q] / nrm : expf(xv[q] - m) / z, gv[q], dot);
    for (int off = 32; off > 0; off >>= 1) dot += __shfl_xor(dot, off, 64);
#pragma unroll
    for (int q = 0; q < HX_MAX; ++q) {
        const int c = lane + 64 * q;
        if (c >= lddz) continue;
        float d = 0.f;
        if (c < C) d = mode == 0 ? (gv[q] - (xv[q] / nrm) * dot) / nrm : (expf(xv[q] - m) / z) * (gv[q] - dot);
        dz[p * lddz + c] = d;
    }
}

inline int64_t wgrad_chunk(int64_t n_pix)
{
    // ~512 pixel chunks (two workgroups per CU), whole 32-pixel steps
    return ((n_pix + 511) / 512 + XK - 1) / XK * XK;
}

}  // namespace

extern "C" int gags_decoder_layer_split(int64_t n_pix, int n_out, int k_in, const float *a1, const float *a2, int lda,
                                        const float *w, const float *bias, int relu, const float *mask_src,
                                        const float *residual, float *y, float *y_premask, int ldy, int terms, void *stream)
{
    GAGS_CLEAR_ERR();
    if (terms != 2 && terms != 3) return GAGS_EINVAL;
    if (n_pix < 0 || n_out <= 0 || k_in <= 0 || lda < k_in || ldy < n_out || !a1 || !w || (!y && !y_premask)) return GAGS_EINVAL;
    if (n_pix == 0) return GAGS_OK;
    XArgs g = {};
    g.A1 = a1; g.A2 = a2; g.B = w; g.bias = bias; g.mask_src = mask_src; g.E = residual; g.Y = y; g.Ypre = y_premask;
    g.M = n_pix; g.N = n_out; g.K = k_in; g.lda = lda; g.ldb = k_in; g.ldy = ldy; g.relu = relu;
    g.m_tiles = (unsigned)((n_pix + XM - 1) / XM);
    g.n_tiles = (unsigned)((n_out + XN - 1) / XN);
    const dim3 grid((g.m_tiles + 7) / 8 * 8 * g.n_tiles);
    const bool vec = k_in % 4 == 0 && lda % 4 == 0 && ((reinterpret_cast<uintptr_t>(a1) | reinterpret_cast<uintptr_t>(a2) |
                                                          reinterpret_cast<uintptr_t>(w)) & 15) == 0;
    g.vout = (n_out % 4 == 0 && ldy % 4 == 0 &&
              ((reinterpret_cast<uintptr_t>(y) | reinterpret_cast<uintptr_t>(y_premask) | reinterpret_cast<uintptr_t>(mask_src) |
                reinterpret_cast<uintptr_t>(residual)) & 15) == 0) ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
#define GO(NT)                                                                                              \
    do {                                                                                                    \
        if (a2) {                                                                                           \
            if (vec) hipLaunchKernelGGL((gemm_x3_nt_kernel<true, true, NT>), grid, dim3(256), 0, st, g);    \
            else hipLaunchKernelGGL((gemm_x3_nt_kernel<true, false, NT>), grid, dim3(256), 0, st, g);       \
        } else {                                                                                            \
            if (vec) hipLaunchKernelGGL((gemm_x3_nt_kernel<false, true, NT>), grid, dim3(256), 0, st, g);   \
            else hipLaunchKernelGGL((gemm_x3_nt_kernel<false, false, NT>), grid, dim3(256), 0, st, g);      \
        }                                                                                                   \
    } while (0)
    if (terms == 3) GO(3); else GO(2);
#undef GO
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_decoder_layer_exact(int64_t n_pix, int n_out, int k_in, const float *a1, const float *a2, int lda,
                                        const float *w, const float *bias, int relu, const float *mask_src,
                                        const float *residual, float *y, float *y_premask, int ldy, void *stream)
{
    return gags_decoder_layer_split(n_pix, n_out, k_in, a1, a2, lda, w, bias, relu, mask_src, residual, y, y_premask, ldy, 3,
                                    stream);
}

extern "C" int64_t gags_decoder_wgrad_exact_scratch_bytes(int64_t n_pix, int n_out, int k_in)
{
    if (n_pix <= 0 || n_out <= 0 || k_in <= 0) return 0;
    const int64_t chunk = wgrad_chunk(n_pix), n_chunks = (n_pix + chunk - 1) / chunk;
    return al256(n_chunks * ((int64_t)n_out * k_in + n_out) * 4);
}

extern "C" int gags_decoder_wgrad_split(int64_t n_pix, int n_out, int k_in, const float *dz, int lddz, const float *a1,
                                        const float *a2, int lda, float *d_w, float *d_b, void *scratch,
                                        int64_t scratch_bytes, int terms, void *stream)
{
    GAGS_CLEAR_ERR();
    if (terms != 2 && terms != 3) return GAGS_EINVAL;
    if (n_pix < 0 || n_out <= 0 || k_in <= 0 || lddz < n_out || lda < k_in || !dz || !a1 || !d_w) return GAGS_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n_pix == 0) {
        if (hipMemsetAsync(d_w, 0, sizeof(float) * (size_t)n_out * k_in, st) != hipSuccess) return GAGS_ELAUNCH;
        if (d_b && hipMemsetAsync(d_b, 0, sizeof(float) * (size_t)n_out, st) != hipSuccess) return GAGS_ELAUNCH;
        return GAGS_OK;
    }
    if (!scratch || scratch_bytes < gags_decoder_wgrad_exact_scratch_bytes(n_pix, n_out, k_in)) return GAGS_ESCRATCH;
    const int64_t chunk = wgrad_chunk(n_pix);
    const int n_chunks = (int)((n_pix + chunk - 1) / chunk);
    float *part = (float *)scratch, *part_b = part + (size_t)n_chunks * n_out * k_in;
    XArgs g = {};
    g.A1 = dz; g.lda = lddz; g.B = a1; g.B2 = a2; g.ldb = lda; g.Mo = n_out; g.No = k_in; g.P = n_pix; g.chunk = chunk; g.part = part;
    g.bias_part = d_b ? part_b : nullptr;
    const dim3 grid((unsigned)n_chunks, (unsigned)((n_out + XM - 1) / XM), (unsigned)((k_in + XN - 1) / XN));
    if (terms == 3) {
        if (a2) hipLaunchKernelGGL((gemm_x3_tn_kernel<true, 3>), grid, dim3(256), 0, st, g);
        else hipLaunchKernelGGL((gemm_x3_tn_kernel<false, 3>), grid, dim3(256), 0, st, g);
    } else {
        if (a2) hipLaunchKernelGGL((gemm_x3_tn_kernel<true, 2>), grid, dim3(256), 0, st, g);
        else hipLaunchKernelGGL((gemm_x3_tn_kernel<false, 2>), grid, dim3(256), 0, st, g);
    }
    const int64_t elems = (int64_t)n_out * k_in;
    hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)((elems + 255) / 256)), dim3(256), 0, st, n_chunks, elems, part, d_w);
    if (d_b)
        hipLaunchKernelGGL(sum_parts_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), 0, st, n_chunks, (int64_t)n_out, part_b,
                           d_b);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_decoder_wgrad_exact(int64_t n_pix, int n_out, int k_in, const float *dz, int lddz, const float *a1,
                                        const float *a2, int lda, float *d_w, float *d_b, void *scratch,
                                        int64_t scratch_bytes, void *stream)
{
    return gags_decoder_wgrad_split(n_pix, n_out, k_in, dz, lddz, a1, a2, lda, d_w, d_b, scratch, scratch_bytes, 3, stream);
}

extern "C" int gags_decoder_head_bwd_exact(int64_t n_pix, int c, int ldx, int mode, const float *x, const float *g, int layout,
                                           float *dz, int lddz, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_pix < 0 || c <= 0 || c > 64 * HX_MAX || lddz > 64 * HX_MAX || ldx < c || lddz < c || (mode != 0 && mode != 1) || (layout != 0 && layout != 1) ||
        (n_pix > 0 && (!x || !g || !dz)))
        return GAGS_EINVAL;
    if (n_pix == 0) return GAGS_OK;
    hipLaunchKernelGGL(head_bwd_exact_kernel, dim3((unsigned)((n_pix + 3) / 4)), dim3(256), 0, (hipStream_t)stream, n_pix, c, ldx, mode,
                       x, g, layout, dz, lddz);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
