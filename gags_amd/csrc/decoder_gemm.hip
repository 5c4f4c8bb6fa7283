// N1: the per-pixel decoders of models/networks.py:109-248 -- stacks of 1x1 convolutions, i.e. a
// [pixels, C_in] x [C_in, C_out] GEMM per layer over 2.07 M pixels at 1080p -- on the 16-bit matrix cores
// (v_mfma_f32_32x32x16_bf16, fp32 accumulate).  The reference runs these convolutions through cuDNN, which by
// PyTorch's default uses TF32 (10-bit mantissa) on its RTX 4090; bf16 keeps 8 bits, fp32 accumulation is the same.
//
// Layout: activations are PIXEL-major [P, C] bf16 -- what the rasterizer writes is [H, W, D] already, so the
// 16-channel render feeds layer 0 without the reference's permute -- weights [C_out, C_in] bf16 (C_in contiguous:
// both MFMA operands are then 16-byte rows).  One kernel serves every layer:
//     Y[p, n] = ( act( sum_k (A1[p, k] (+ A2[p, k])) * W[n, k] + bias[n] ) (+ E[p, n]) ) (* mask)
// with the second source for the residual sums (x1 + x2, x3 + x4 of CNN_decoder.forward) and, in the backward, the
// ReLU mask of the layer below and the residual's gradient in the epilogue.
#include "decoder_common.h"

namespace {

constexpr int TM = 128, TK = 64;             // workgroup tile: 128 pixels x (64 NJ) outputs, K step 64
constexpr int LDK = TK + 8;                  // LDS row pitch in bf16 (144 B: 16-byte aligned, spreads the banks)

struct GemmArgs {
    const unsigned short *A1, *A2;  // [P, K] bf16, A2 optional (summed with A1 in fp32, rounded once)
    const unsigned short *W;        // [N, K] bf16
    const float *bias;              // [N] or null
    const unsigned short *mask_src; // [P, N] bf16 or null: output multiplied by (mask_src > 0)
    const unsigned short *E;        // [P, N] bf16 or null: added before the mask
    unsigned short *Y;              // [P, N] bf16 or null
    unsigned short *Ypre;           // [P, N] bf16 or null: the value before the mask (a skip connection's gradient)
    float *Yf;                      // [P, N] fp32 or null
    int64_t P;
    int N, K, relu;
};

// NJ = 32-column blocks per wave: the workgroup tile is 128 pixels x TN = 64 NJ outputs (NJ = 4: a 256-wide layer in
// ONE tile, so the activations are read once).  Wider layers take several column tiles per pixel tile; the workgroup
// index is decoded so that those land on the SAME XCD back to back (hardware deals workgroups round-robin over the 8
// XCDs, each with its own L2): the second one finds the activation tile in that L2 instead of re-reading HBM.
template <int NJ, bool TWO>
__global__ __launch_bounds__(256, 2) void gemm_bf16_kernel(GemmArgs a, int n_tiles, unsigned p_tiles)
{
    constexpr int TN = 64 * NJ;
    __shared__ __attribute__((aligned(16))) unsigned short smem[(TM + TN) * LDK];
    unsigned short (*As)[LDK] = reinterpret_cast<unsigned short (*)[LDK]>(smem);
    unsigned short (*Bs)[LDK] = reinterpret_cast<unsigned short (*)[LDK]>(smem + TM * LDK);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wy = wave >> 1, wx = wave & 1;  // 2 x 2 waves, 64 x (32 NJ) outputs each
    unsigned pt = blockIdx.x;
    int nt = 0;
    if (n_tiles > 1) {
        const unsigned xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        pt = (slot / n_tiles) * 8 + xcd;
        nt = slot % n_tiles;
        if (pt >= p_tiles) return;
    }
    const int64_t p0 = (int64_t)pt * TM;
    const int n0 = nt * TN;
    f32x16 acc[2][NJ];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // staging identity: 16-byte piece tid % 8 of rows tid / 8 + 32 q (eight consecutive lanes read one row's 128
    // contiguous bytes: fully coalesced); the next K step's operands are requested into registers before the current
    // one is multiplied (the K loop is only 4-8 steps long: no deeper pipeline).  Every address is clamped into the
    // operand, so the loads are unconditional (a predicated load is a branch and a wait of its own) and what lies
    // beyond K is zeroed by a select; the second activation source is added when the tile goes to LDS, not when it is
    // requested.
    const int sr = tid >> 3, sh = (tid & 7) * 8;
    uint4 ra[4], ra2[TWO ? 4 : 1], rb[2 * NJ];
    unsigned aoff[4], boff[2 * NJ];  // element offsets: P * K < 2^31 is checked by the entry
#pragma unroll
    for (int q = 0; q < 4; ++q) aoff[q] = (unsigned)(min(p0 + sr + 32 * q, a.P - 1) * a.K);
#pragma unroll
    for (int q = 0; q < 2 * NJ; ++q) boff[q] = (unsigned)(min(n0 + sr + 32 * q, a.N - 1) * a.K);
    bool fetched_ok = true;
    auto fetch = [&](int k0) __attribute__((always_inline)) {
        fetched_ok = k0 + sh < a.K;  // K is a multiple of 32, the step is 64
        const int kc = fetched_ok ? k0 + sh : 0;
#pragma unroll
        for (int q = 0; q < 2 * NJ; ++q) rb[q] = *reinterpret_cast<const uint4 *>(a.W + boff[q] + kc);
#pragma unroll
        for (int q = 0; q < 4; ++q) ra[q] = *reinterpret_cast<const uint4 *>(a.A1 + aoff[q] + kc);
        if constexpr (TWO) {
#pragma unroll
            for (int q = 0; q < 4; ++q) ra2[q] = *reinterpret_cast<const uint4 *>(a.A2 + aoff[q] + kc);
        }
    };
    auto commit = [&]() __attribute__((always_inline)) {
        const unsigned keep = fetched_ok ? 0xffffffffu : 0u;  // (a select between two uint4 lvalues would pin them in memory)
        if constexpr (TWO) {  // residual sum of two activations: add in fp32, round once
#pragma unroll
            for (int q = 0; q < 4; ++q)
                ra[q] = make_uint4(add_h16x2(ra[q].x, ra2[q].x), add_h16x2(ra[q].y, ra2[q].y), add_h16x2(ra[q].z, ra2[q].z),
                                   add_h16x2(ra[q].w, ra2[q].w));
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<uint4 *>(&As[sr + 32 * q][sh]) =
                make_uint4(ra[q].x & keep, ra[q].y & keep, ra[q].z & keep, ra[q].w & keep);
#pragma unroll
        for (int q = 0; q < 2 * NJ; ++q) *reinterpret_cast<uint4 *>(&Bs[sr + 32 * q][sh]) =
                make_uint4(rb[q].x & keep, rb[q].y & keep, rb[q].z & keep, rb[q].w & keep);
    };
    fetch(0);
    for (int k0 = 0; k0 < a.K; k0 += TK) {
        commit();
        __syncthreads();
        if (k0 + TK < a.K) fetch(k0 + TK);
#pragma unroll
        for (int ks = 0; ks < TK; ks += 16) {
            bf16x8 af[2], bf[NJ];
#pragma unroll
            for (int i = 0; i < 2; ++i)
                af[i] = *reinterpret_cast<const bf16x8 *>(&As[wy * 64 + i * 32 + (lane & 31)][ks + 8 * (lane >> 5)]);
#pragma unroll
            for (int j = 0; j < NJ; ++j)
                bf[j] = *reinterpret_cast<const bf16x8 *>(&Bs[wx * 32 * NJ + j * 32 + (lane & 31)][ks + 8 * (lane >> 5)]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < NJ; ++j)
                    acc[i][j] = h16_mfma(bf[j], af[i], acc[i][j]);
        }
        __syncthreads();
    }
    // The operands were swapped above (weights as "A", activations as "B"): an accumulator's lane owns ONE pixel
    // (column = lane & 31) and 16 output channels (rows): channel (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of a 32-block.
    // Stored from there, every instruction would scatter 8-byte pieces 2 N bytes apart and HBM sees partial lines
    // (measured: 2.4 x the bytes, 25 B per write request).  Instead each wave passes 32 pixels x 64 channels at a time
    // through its own LDS patch in fp32 (bias and ReLU applied on the way in) and reads it back with 8 consecutive
    // channels per lane: the skip gradient E and the mask are then 16-byte reads and the results 16 / 32-byte stores,
    // eight lanes per 128-byte (bf16) or 256-byte (fp32) run of one pixel.
    constexpr int SP = 68;  // patch pitch in floats (272 B: conflict-free for both the b128 writes and reads)
    static_assert(4 * 32 * SP * 4 <= (TM + TN) * LDK * 2, "epilogue patches fit in the operand tiles' LDS");
    float *stg = reinterpret_cast<float *>(smem) + wave * 32 * SP;
    const int epx = lane & 31, ehalf = lane >> 5, cg = lane & 7;
    const bool full = p0 + TM <= a.P && n0 + TN <= a.N;  // workgroup-uniform: the interior needs no per-lane tests
    const float floor_ = a.relu ? 0.f : -3.4e38f;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
#pragma unroll
        for (int jp = 0; jp < NJ / 2; ++jp) {
            const int nb = n0 + wx * 32 * NJ + jp * 64;  // first channel of this pass (wave-uniform)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj)
#pragma unroll
                for (int rq = 0; rq < 4; ++rq) {
                    const int r0 = 4 * rq;
                    const f32x16 &c = acc[i][2 * jp + jj];
                    *reinterpret_cast<float4 *>(stg + epx * SP + jj * 32 + 8 * rq + 4 * ehalf) =
                        make_float4(c[r0], c[r0 + 1], c[r0 + 2], c[r0 + 3]);
                }
            __builtin_amdgcn_wave_barrier();
            const int n = nb + cg * 8;           // this lane's 8 channels: the same in all four pixel groups
            const int nc = min(n, a.N - 8);
            float bs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (a.bias) {
                const float4 b0 = *reinterpret_cast<const float4 *>(a.bias + nc), b1 = *reinterpret_cast<const float4 *>(a.bias + nc + 4);
                bs[0] = b0.x; bs[1] = b0.y; bs[2] = b0.z; bs[3] = b0.w; bs[4] = b1.x; bs[5] = b1.y; bs[6] = b1.z; bs[7] = b1.w;
            }
#pragma unroll
            for (int t2 = 0; t2 < 4; ++t2) {
                const int px = t2 * 8 + (lane >> 3);
                const float4 lo = *reinterpret_cast<const float4 *>(stg + px * SP + cg * 8);
                const float4 hi = *reinterpret_cast<const float4 *>(stg + px * SP + cg * 8 + 4);
                float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
                for (int q = 0; q < 8; ++q) v[q] = fmaxf(v[q] + bs[q], floor_);
                const int64_t p = p0 + wy * 64 + i * 32 + px;
                const bool live = full || (p < a.P && n < a.N);
                const size_t o = (size_t)min(p, a.P - 1) * a.N + nc;  // always a valid address: loads are unconditional
                if (a.E) {
                    const uint4 e = *reinterpret_cast<const uint4 *>(a.E + o);
                    v[0] += h16_lo(e.x); v[1] += h16_hi(e.x); v[2] += h16_lo(e.y); v[3] += h16_hi(e.y);
                    v[4] += h16_lo(e.z); v[5] += h16_hi(e.z); v[6] += h16_lo(e.w); v[7] += h16_hi(e.w);
                }
                if (a.Ypre && live)
                    *reinterpret_cast<uint4 *>(a.Ypre + o) =
                        make_uint4(h16_pack(v[0], v[1]), h16_pack(v[2], v[3]), h16_pack(v[4], v[5]), h16_pack(v[6], v[7]));
                if (a.mask_src) {
                    const uint4 m = *reinterpret_cast<const uint4 *>(a.mask_src + o);
                    const unsigned mw[4] = {m.x, m.y, m.z, m.w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        v[2 * q] = h16_lo(mw[q]) > 0.f ? v[2 * q] : 0.f;
                        v[2 * q + 1] = h16_hi(mw[q]) > 0.f ? v[2 * q + 1] : 0.f;
                    }
                }
                if (a.Y && live)
                    *reinterpret_cast<uint4 *>(a.Y + o) =
                        make_uint4(h16_pack(v[0], v[1]), h16_pack(v[2], v[3]), h16_pack(v[4], v[5]), h16_pack(v[6], v[7]));
                if (a.Yf && live) {
                    *reinterpret_cast<float4 *>(a.Yf + o) = make_float4(v[0], v[1], v[2], v[3]);
                    *reinterpret_cast<float4 *>(a.Yf + o + 4) = make_float4(v[4], v[5], v[6], v[7]);
                }
            }
            __builtin_amdgcn_wave_barrier();
        }
    }
}

}  // namespace

extern "C" int GAGS_DEC(gags_decoder_layer)(int64_t n_pix, int n_out, int k_in, const void *a1, const void *a2, const void *w,
                                  const float *bias, int relu, const void *mask_src, const void *residual, void *y_bf16,
                                  void *y_premask_bf16, float *y_f32, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_pix < 0 || n_out <= 0 || k_in <= 0 || k_in % 32 != 0 || n_out % 8 != 0 || n_pix * k_in >= ((int64_t)1 << 31) || !a1 || !w ||
        (!y_bf16 && !y_f32 && !y_premask_bf16))
        return GAGS_EINVAL;
    if (n_pix == 0) return GAGS_OK;
    GemmArgs g;
    g.A1 = (const unsigned short *)a1; g.A2 = (const unsigned short *)a2; g.W = (const unsigned short *)w; g.bias = bias;
    g.mask_src = (const unsigned short *)mask_src; g.E = (const unsigned short *)residual;
    g.Y = (unsigned short *)y_bf16; g.Ypre = (unsigned short *)y_premask_bf16; g.Yf = y_f32; g.P = n_pix; g.N = n_out; g.K = k_in; g.relu = relu;
    const unsigned p_tiles = (unsigned)((n_pix + TM - 1) / TM);
    if (n_out > 128) {
        const int n_tiles = (n_out + 255) / 256;
        const unsigned grid = n_tiles == 1 ? p_tiles : (p_tiles + 7) / 8 * 8 * n_tiles;
        if (a2) hipLaunchKernelGGL((gemm_bf16_kernel<4, true>), dim3(grid), dim3(256), 0, (hipStream_t)stream, g, n_tiles, p_tiles);
        else hipLaunchKernelGGL((gemm_bf16_kernel<4, false>), dim3(grid), dim3(256), 0, (hipStream_t)stream, g, n_tiles, p_tiles);
    } else {
        if (a2) hipLaunchKernelGGL((gemm_bf16_kernel<2, true>), dim3(p_tiles), dim3(256), 0, (hipStream_t)stream, g, 1, p_tiles);
        else hipLaunchKernelGGL((gemm_bf16_kernel<2, false>), dim3(p_tiles), dim3(256), 0, (hipStream_t)stream, g, 1, p_tiles);
    }
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
