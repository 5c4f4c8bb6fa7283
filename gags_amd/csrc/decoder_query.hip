// N15: the open-vocabulary query of one view (evaluate_iou_loc.py:258-288, compute_relvancy.py:243-269, 333-361)
// as ONE forward-only kernel:  rasterized features [P, c_in] -> CNN_decoder's nine layers -> F.normalize ->
// OpenCLIPNetwork.get_relevancy for every positive phrase -> probs [n_pos, P, 2].
//
// The nine layers run per 64-pixel tile with the activations in LDS exactly as decoder_fwd_fused_kernel runs them
// (csrc/decoder_tile.h: the same operand rounding, ascending-k fp32 accumulation, bias + ReLU + one rounding, in-place residual
// sums), but nothing the backward would need is kept: no activation, mask or logits stores, and the normalised [P, n_last] map
// the relevancy kernel (csrc/activate.hip) used to read is never formed.  HBM sees the input (4 c_in bytes per pixel) and the
// result (8 n_pos bytes per pixel); the weights and phrases live in L2.
//
// The head ("direct" design).  The last layer leaves its fp32 logits z = acc + b8 -- the very bits
// gags_decoder_fwd_fused stores -- in the LDS patch it stages them through, 128 channels at a time.  There thread
// (pixel = tid & 63, slice = wave) multiplies its 32 channels of its pixel's row with the same 32 channels of every phrase
// (per phrase one ascending fp32 fmaf chain of 32 per half-pass, the half-passes' sums added in order: short chains keep the
// rounding error near the wave-tree sum of relevancy_kernel; the phrase values are wave-uniform: they come through the scalar
// cache and are FMA operands as they are) and sums their squares the same way.  After the last pass the four slices'
// partials meet in LDS ((s0 + s1) + (s2 + s3)),
//     sim_j = z . t_j / max(sqrt(z . z), 1e-12)          (F.normalize's clamp; all-zero logits give sim = 0, p = 0.5)
// and per positive j the pair softmax(10 (sim_j, sim_neg_k)) of the negative k with the smallest positive probability, the
// first minimum winning -- relevancy_kernel's arithmetic line by line.  Error against the float64 head on the same logits: a
// dot passes through at most 32 + n_last / 128 + 2 fp32 roundings, far inside the gamma_516 of a single n_last-long chain the
// test ceiling is derived from.
#include "decoder_tile.h"

namespace {

constexpr int QMAX = 32;  // phrases (positives + negatives): gags_relevancy's cap
constexpr int QC = 4;     // phrases per unrolled group: a call computes ceil(n_text / QC) QC chains, the extra ones on the last phrase's row

struct QueryArgs {
    const float *x;              // [P, c_in] fp32 pixel-major, c_in <= 32
    const unsigned short *W[9];  // the forward's fragment-order weights
    const float *b[9];
    float *probs;                // [n_pos, P, 2]
    int64_t P;
    int c_in, n_last, n_pos, n_neg;
};

__global__ __launch_bounds__(256, 2) void decoder_query_kernel(QueryArgs a, const float *__restrict__ text)
{
    gags_h16::h16_saturate_mode();  // (f16 tier: conversions saturate in hardware; half16.h)
    __shared__ __attribute__((aligned(16))) unsigned short bufA[FT][FLD];
    __shared__ __attribute__((aligned(16))) unsigned short bufB[FT][FLD];
    constexpr int NT = 256;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t p0 = (int64_t)blockIdx.x * FT;
    const int n_base = 64 * wave;
    __shared__ __attribute__((aligned(16))) float bias_s[8][FH];  // (staged once: decoder_fwd_fused_kernel)
    {
        float bv[8 * FH / NT];
#pragma unroll
        for (int q = 0; q < 8 * FH / NT; ++q) { const int e = tid + NT * q; bv[q] = a.b[e >> 8][e & (FH - 1)]; }
#pragma unroll
        for (int q = 0; q < 8 * FH / NT; ++q) { const int e = tid + NT * q; bias_s[e >> 8][e & (FH - 1)] = bv[q]; }
    }
    f32x16 acc[2][2];
    WFrag wf;
    wprefetch(wf, a.W[0], 2, 2 * wave, 0, 2, lane);

    // input tile -> bufB[p][0..31], zero-padded (addresses clamped: rows past the image are computed and never stored)
    {
        float xv[FT * 32 / NT];
#pragma unroll
        for (int q = 0; q < FT * 32 / NT; ++q) {
            const int e = tid + NT * q, row = e >> 5, c = e & 31;
            xv[q] = a.x[min(p0 + row, a.P - 1) * a.c_in + min(c, a.c_in - 1)];
        }
#pragma unroll
        for (int q = 0; q < FT * 32 / NT; ++q) {
            const int e = tid + NT * q, row = e >> 5, c = e & 31;
            const float v = (p0 + row < a.P && c < a.c_in) ? xv[q] : 0.f;
            bufB[row][c] = (unsigned short)(h16_pack_sat(v, 0.f) & 0xffffu);
        }
    }
    __syncthreads();
    // the hidden layers, buffer by buffer as decoder_fwd_fused_kernel (no mask words: epilogue_hidden's mask is null)
    layer_main(acc, wf, a.W[0], 2, 2 * wave, 0, 2, bufB, lane, true, 0);  // L0: a0 (B) -> x1 (A)
    wprefetch(wf, a.W[1], 16, 2 * wave, 0, 16, lane);
    epilogue_hidden(acc, bias_s[0], n_base, bufA, lane, nullptr, p0, a.P, 0);
    __syncthreads();
    layer_main(acc, wf, a.W[1], 16, 2 * wave, 0, 16, bufA, lane, true, 0);  // L1: x1 (A) -> t1 (B)
    wprefetch(wf, a.W[2], 16, 2 * wave, 0, 16, lane);
    epilogue_hidden(acc, bias_s[1], n_base, bufB, lane, nullptr, p0, a.P, 0);
    __syncthreads();
    layer_main(acc, wf, a.W[2], 16, 2 * wave, 0, 16, bufB, lane, true, 0);  // L2: t1 (B) -> x2 over t1; A = x1 + x2
    wprefetch(wf, a.W[3], 16, 2 * wave, 0, 16, lane);
    __syncthreads();
    epilogue_hidden(acc, bias_s[2], n_base, bufB, lane, nullptr, p0, a.P, 0);
    __syncthreads();
    add_tile<NT>(bufA, bufB, tid);
    __syncthreads();
    layer_main(acc, wf, a.W[3], 16, 2 * wave, 0, 16, bufA, lane, true, 0);  // L3: x1 + x2 (A) -> x3 (B)
    wprefetch(wf, a.W[4], 16, 2 * wave, 0, 16, lane);
    epilogue_hidden(acc, bias_s[3], n_base, bufB, lane, nullptr, p0, a.P, 0);
    __syncthreads();
    layer_main(acc, wf, a.W[4], 16, 2 * wave, 0, 16, bufB, lane, true, 0);  // L4: x3 (B) -> t4 (A)
    wprefetch(wf, a.W[5], 16, 2 * wave, 0, 16, lane);
    epilogue_hidden(acc, bias_s[4], n_base, bufA, lane, nullptr, p0, a.P, 0);
    __syncthreads();
    layer_main(acc, wf, a.W[5], 16, 2 * wave, 0, 16, bufA, lane, true, 0);  // L5: t4 (A) -> x4 over t4; B = x3 + x4
    wprefetch(wf, a.W[6], 16, 2 * wave, 0, 16, lane);
    __syncthreads();
    epilogue_hidden(acc, bias_s[5], n_base, bufA, lane, nullptr, p0, a.P, 0);
    __syncthreads();
    add_tile<NT>(bufB, bufA, tid);
    __syncthreads();
    layer_main(acc, wf, a.W[6], 16, 2 * wave, 0, 16, bufB, lane, true, 0);  // L6: x3 + x4 (B) -> t6 (A)
    wprefetch(wf, a.W[7], 16, 2 * wave, 0, 16, lane);
    epilogue_hidden(acc, bias_s[6], n_base, bufA, lane, nullptr, p0, a.P, 0);
    __syncthreads();
    layer_main(acc, wf, a.W[7], 16, 2 * wave, 0, 16, bufA, lane, true, 0);  // L7: t6 (A) -> t7 (B)
    epilogue_hidden(acc, bias_s[7], n_base, bufB, lane, nullptr, p0, a.P, 0);
    __syncthreads();

    // L8: t7 (B) -> fp32 logits, 256 channels per pass, staged through bufA in halves of 128 channels as the forward stages them
    // for its row stores; here the head reads them instead.
    float (*patch)[FLD / 2] = reinterpret_cast<float (*)[FLD / 2]>(&bufA[0][0]);  // [64][132] floats, the tiles' 528-byte pitch
    const int p = lane & 31, h = lane >> 5;
    const int n_text = a.n_pos + a.n_neg;
    const int slice = __builtin_amdgcn_readfirstlane(wave);  // (uniform, and known to be: the phrase loads below are scalar loads)
    float dots[QMAX], n2 = 0.f;
#pragma unroll
    for (int j = 0; j < QMAX; ++j) dots[j] = 0.f;
    for (int nb = 0; nb < a.n_last; nb += FH) {
        wprefetch(wf, a.W[8], 16, nb / 32 + 2 * wave, 0, 16, lane);
        layer_main(acc, wf, a.W[8], 16, nb / 32 + 2 * wave, 0, 16, bufB, lane, true, 0);
        for (int half = 0; half < 2; ++half) {
            if ((wave >> 1) == half) {  // waves 2 half, 2 half + 1 hold channels 128 half .. + 127 of the pass
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const int nl = (n_base & 127) + 32 * i + 8 * g + 4 * h;
                        const float4 b = *reinterpret_cast<const float4 *>(a.b[8] + nb + 128 * half + nl);
#pragma unroll
                        for (int j = 0; j < 2; ++j)
                            *reinterpret_cast<float4 *>(&patch[32 * j + p][nl]) =
                                make_float4(acc[i][j][4 * g] + b.x, acc[i][j][4 * g + 1] + b.y, acc[i][j][4 * g + 2] + b.z,
                                            acc[i][j][4 * g + 3] + b.w);
                    }
            }
            __syncthreads();
            // this thread's 32 logits: row `lane` of the patch, channels 32 slice .. + 31 (the lanes of a 16-byte read are 4 banks
            // apart: conflict-free)
            float z[32], zz = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                const float4 v = (GAGS_ABL & 2048) ? make_float4(0.f, 0.f, 0.f, 0.f) : *reinterpret_cast<const float4 *>(&patch[lane][32 * slice + 4 * q]);
                z[4 * q] = v.x; z[4 * q + 1] = v.y; z[4 * q + 2] = v.z; z[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int c = 0; c < 32; ++c) zz = fmaf(z[c], z[c], zz);
            n2 += zz;
            const float *tb = text + nb + 128 * half + 32 * slice;
#pragma unroll
            for (int jc = 0; jc < QMAX / QC; ++jc) {
                if (QC * jc < n_text && !(GAGS_ABL & (1024 | 2048))) {  // (uniform)
                    float dd[QC];  // this half-pass's 32 channels: a chain of its own, added to the running sum once
#pragma unroll
                    for (int jj = 0; jj < QC; ++jj) dd[jj] = 0.f;
#pragma unroll
                    for (int cg = 0; cg < 4; ++cg)
#pragma unroll
                        for (int jj = 0; jj < QC; ++jj) {
                            const int j = QC * jc + jj;
                            const float *tj = tb + (size_t)min(j, n_text - 1) * a.n_last + 8 * cg;
                            const float4 t0 = *reinterpret_cast<const float4 *>(tj), t1 = *reinterpret_cast<const float4 *>(tj + 4);
                            float d = dd[jj];
                            d = fmaf(z[8 * cg], t0.x, d); d = fmaf(z[8 * cg + 1], t0.y, d);
                            d = fmaf(z[8 * cg + 2], t0.z, d); d = fmaf(z[8 * cg + 3], t0.w, d);
                            d = fmaf(z[8 * cg + 4], t1.x, d); d = fmaf(z[8 * cg + 5], t1.y, d);
                            d = fmaf(z[8 * cg + 6], t1.z, d); d = fmaf(z[8 * cg + 7], t1.w, d);
                            dd[jj] = d;
                        }
#pragma unroll
                    for (int jj = 0; jj < QC; ++jj) dots[QC * jc + jj] += dd[jj];
                }
            }
            __syncthreads();
        }
    }
    // the four slices' partials meet in bufA (every patch read is behind the barrier above): part[slice][j][pixel], j = QMAX: z . z
    constexpr int QS = (QMAX + 1) * FT;
    static_assert(4 * QS * sizeof(float) <= sizeof(bufA), "the partial sums live in bufA");
    float *part = reinterpret_cast<float *>(&bufA[0][0]);
#pragma unroll
    for (int j = 0; j < QMAX; ++j)
        if (j < n_text) part[slice * QS + j * FT + lane] = dots[j];
    part[slice * QS + QMAX * FT + lane] = n2;
    __syncthreads();
    // sims[j][pixel] over slice 0's dots (each entry is read and written by one thread; the z . z entries stay as they are)
    for (int e = tid; e < n_text * FT; e += NT) {
        const int px = e & (FT - 1), q = QMAX * FT + px;
        const float zz = (part[q] + part[QS + q]) + (part[2 * QS + q] + part[3 * QS + q]);
        const float d = (part[e] + part[QS + e]) + (part[2 * QS + e] + part[3 * QS + e]);
        part[e] = d / fmaxf(sqrtf(zz), 1e-12f);
    }
    __syncthreads();
    // positives j = wave, wave + 4, ...: lane = pixel, so a wave's float2 stores cover 512 contiguous bytes
    const int64_t pg = p0 + lane;
    if (pg >= a.P) return;
    for (int j = wave; j < a.n_pos; j += 4) {
        const float sa = 10.f * part[j * FT + lane];
        float best0 = 0.f, best1 = 0.f;
        for (int k = 0; k < a.n_neg; ++k) {
            const float sb = 10.f * part[(a.n_pos + k) * FT + lane];
            const float m = fmaxf(sa, sb);
            const float ea = expf(sa - m), eb = expf(sb - m);
            const float q0 = ea / (ea + eb), q1 = eb / (ea + eb);
            if (k == 0 || q0 < best0) { best0 = q0; best1 = q1; }  // argmin keeps the first minimum (csrc/activate.hip)
        }
        *reinterpret_cast<float2 *>(a.probs + ((size_t)j * a.P + pg) * 2) = make_float2(best0, best1);
    }
}

}  // namespace

extern "C" int GAGS_DEC(gags_decoder_query_fused)(int64_t n_pix, int c_in, int n_last, const float *x, const void *const *w_bf16,
                                                  const float *const *bias, const float *phrases, int n_pos, int n_neg, float *probs,
                                                  void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_pix < 0 || c_in <= 0 || c_in > 32 || n_last <= 0 || n_last % FH != 0 || !w_bf16 || !bias || !phrases || n_pos <= 0 ||
        n_neg <= 0 || n_pos + n_neg > QMAX || (n_pix > 0 && (!x || !probs)))
        return GAGS_EINVAL;
    if (((uintptr_t)phrases & 15) || ((uintptr_t)probs & 7)) return GAGS_EINVAL;  // (16-byte phrase loads, 8-byte pair stores)
    QueryArgs a;
    a.x = x; a.probs = probs; a.P = n_pix; a.c_in = c_in; a.n_last = n_last; a.n_pos = n_pos; a.n_neg = n_neg;
    for (int i = 0; i < 9; ++i) {
        if (!w_bf16[i] || !bias[i]) return GAGS_EINVAL;
        a.W[i] = (const unsigned short *)w_bf16[i];
        a.b[i] = bias[i];
    }
    if (n_pix == 0) return GAGS_OK;
    hipLaunchKernelGGL(decoder_query_kernel, dim3((unsigned)((n_pix + FT - 1) / FT)), dim3(256), 0, (hipStream_t)stream, a, phrases);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
