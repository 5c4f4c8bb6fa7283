// N2: the decoder's output head fused with the distillation L1, forward and backward -- the most heavily
// tuned kernel of the image-space losses.  Numerics follow the reference's torch ops (fp32).
#include "common.h"
#include "gags_next.h"
#include "sam_taps.h"

namespace {

// CNN_decoder's output head FUSED with the distillation L1 (train.py:159-166 in one kernel each way): from the last
// layer's fp32 logits x[P][ld] straight to l1_map = mean_c |normalize(x) m - gt m| (and back: from d l1_map to the
// bf16 gradient of the logits), without writing the normalised [512,H,W] map, reading it back for the loss, writing
// the loss's [512,H,W] gradient and reading that back for the head's backward: 8.5 + 12.7 GB per iteration at 1080p.
// Workgroup = 32 pixels; eight lanes per pixel, each holding 64 of its channels (16 float4) in registers, as in
// the pixel-major heads; the taps of the 32 pixels are computed once and shared through LDS.
constexpr int FHJ = 16;  // float4 per lane (ld <= 512)

typedef __bf16 l_bf16x2 __attribute__((ext_vector_type(2)));
typedef float l_f32x2 __attribute__((ext_vector_type(2)));

// c = ld = 512 (CNN_decoder(16, 512), the reference's configuration): 16 float4 per lane, straight-line code.
// ONE_TAP: the segmentation map has the render's resolution (identity resize: every pixel has exactly one source
// pixel), the common case -- one gather per level, the gathers of step j + 1 in flight during step j.
// DZM (BWD): the logits' gradient leaves as 0 = bf16 (the bf16 mode), 1 = fp32 (the fp32-tensor decoder tiers), 2 = IEEE half
// multiplied by the power of two dz_scale[0] and saturated at +-65504 (the f16 tier: csrc/half16.h).
struct GagsLossTrue { static constexpr bool value = true; };
struct GagsLossFalse { static constexpr bool value = false; };
template <bool BWD, bool ONE_TAP, int DZM = 0>
__global__ __launch_bounds__(256, 3) void head_distill_kernel(int H, int W, int h, int w, int n_emb,
                                                              const float *__restrict__ x, const float *__restrict__ img_embed,
                                                              const float *__restrict__ seg_map, const float *__restrict__ scale_map,
                                                              const float *__restrict__ v_map, float *__restrict__ l1_map,
                                                              float *__restrict__ mask_out, unsigned short *__restrict__ dz,
                                                              float *__restrict__ v_scale, const float *__restrict__ dz_scale = nullptr)
{
    constexpr int c = 512;
    if constexpr (BWD && DZM == 2) asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 1");  // half conversions saturate
    __shared__ TapsLds tl[TPM];
    const int HW = H * W;
    const int p0 = blockIdx.x * TPM;
    const int tid = threadIdx.x;
    if (tid < TPM) {
        const int pc = min(p0 + tid, HW - 1);
        tl[tid] = make_taps_lds<BWD>(pc, c, H, W, h, w, n_emb, seg_map, scale_map, v_map);
    }
    const int px = tid >> 3, c0 = (tid & 7) * 4;
    const int pr = p0 + px, p = min(pr, HW - 1);
    float4 v[FHJ];
#pragma unroll
    for (int j = 0; j < FHJ; ++j) v[j] = *reinterpret_cast<const float4 *>(x + (size_t)p * c + c0 + 32 * j);
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < FHJ; ++j) ss = fmaf(v[j].x, v[j].x, fmaf(v[j].y, v[j].y, fmaf(v[j].z, v[j].z, fmaf(v[j].w, v[j].w, ss))));
    ss += __shfl_xor(ss, 1); ss += __shfl_xor(ss, 2); ss += __shfl_xor(ss, 4);
    const float nrm = fmaxf(sqrtf(ss), 1e-12f);  // F.normalize(dim=0), models/networks.py:192
    const float inv = 1.0f / nrm;
    __syncthreads();
    const TapsLds &t = tl[px];
    const float m = t.mask, s0 = t.sc[0], s1 = t.sc[1], s2 = t.sc[2], vm = t.v * t.mask;
    const float w0 = t.wgt[0], w1 = t.wgt[1], w2 = t.wgt[2], w3 = t.wgt[3];
    const float *er[3][4];
#pragma unroll
    for (int l = 0; l < 3; ++l)
#pragma unroll
        for (int k = 0; k < (ONE_TAP ? 1 : 4); ++k) er[l][k] = img_embed + (size_t)t.id[l][k] * c + c0;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, dot = 0.f;
    l_f32x2 a02 = {0.f, 0.f}, a12 = {0.f, 0.f}, a22 = {0.f, 0.f}, dot2 = {0.f, 0.f};  // BWD: packed partial sums
    unsigned sgn_pos[2] = {0u, 0u}, sgn_neg[2] = {0u, 0u};  // BWD: sign of diff per element (64 per lane)
    // BWD, signs: the fast pass takes copysign(1, diff) and shifts the sign bits into two words (one v_alignbit per element;
    // three instructions per element and pass instead of sixteen: 1.57 -> 1.36 ms at 1080p, round 6) and keeps the smallest
    // |diff| it met; torch.sign(0) = 0 matters for about one element in 10^7 (an exact tie of two fp32 values), and a pixel that
    // met one runs the pass again in the exact form (EXACT: signs in {-1, 0, +1} as two bit sets, as before).
    float minabs = 3.0e38f;
    auto pass1 = [&](auto exact_tag) __attribute__((always_inline)) {
    constexpr bool EXACT = decltype(exact_tag)::value;
    float4 en[3];
    if (ONE_TAP) {
#pragma unroll
        for (int l = 0; l < 3; ++l) en[l] = *reinterpret_cast<const float4 *>(er[l][0]);
    }
#pragma unroll
    for (int j = 0; j < FHJ; ++j) {
        float f[3][4];
        if (ONE_TAP) {
#pragma unroll
            for (int l = 0; l < 3; ++l) { f[l][0] = en[l].x; f[l][1] = en[l].y; f[l][2] = en[l].z; f[l][3] = en[l].w; }
            if (j + 1 < FHJ) {
#pragma unroll
                for (int l = 0; l < 3; ++l) en[l] = *reinterpret_cast<const float4 *>(er[l][0] + 32 * (j + 1));
            }
        } else {
#pragma unroll
            for (int l = 0; l < 3; ++l) {
                const float4 e0 = *reinterpret_cast<const float4 *>(er[l][0] + 32 * j), e1 = *reinterpret_cast<const float4 *>(er[l][1] + 32 * j);
                const float4 e2 = *reinterpret_cast<const float4 *>(er[l][2] + 32 * j), e3 = *reinterpret_cast<const float4 *>(er[l][3] + 32 * j);
                // the taps in order 0..3, as level_feature16 accumulates them (a zero weight adds exactly nothing)
                f[l][0] = fmaf(w3, e3.x, fmaf(w2, e2.x, fmaf(w1, e1.x, w0 * e0.x)));
                f[l][1] = fmaf(w3, e3.y, fmaf(w2, e2.y, fmaf(w1, e1.y, w0 * e0.y)));
                f[l][2] = fmaf(w3, e3.z, fmaf(w2, e2.z, fmaf(w1, e1.z, w0 * e0.z)));
                f[l][3] = fmaf(w3, e3.w, fmaf(w2, e2.w, fmaf(w1, e1.w, w0 * e0.w)));
            }
        }
        const float xe[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
        // the element-wise part on PACKED fp32 instructions (v_pk_mul_f32 / v_pk_add_f32, two elements each: this kernel is
        // bound by its VALU issue slots, ~100 per step and lane, not by its 4.25 GB of logits); same operations, same order
#pragma unroll
        for (int q = 0; q < 4; q += 2) {
            const l_f32x2 x2 = {xe[q], xe[q + 1]}, f0 = {f[0][q], f[0][q + 1]}, f1 = {f[1][q], f[1][q + 1]}, f2 = {f[2][q], f[2][q + 1]};
            const l_f32x2 y2 = x2 * inv;  // (x * (1 / n): within an ulp of F.normalize's x / n)
            const l_f32x2 gt2 = (f0 * s0 + f1 * s1) + f2 * s2;
            // (m is 0 or 1: y m - gt m = (y - gt) m exactly; the factor rides on the pixel's sum / on v m instead of on every element)
            const l_f32x2 d2 = y2 - gt2;
            if (!BWD) {
                a0 += fabsf(d2[0]);
                a0 += fabsf(d2[1]);
            } else {
                // sign(diff) in {-1, 0, +1} by integer arithmetic on the bits (a float compare per element keeps a lane
                // mask in an SGPR pair alive until the bit sets are assembled: 128 pairs, spilled)
                l_f32x2 sg2;
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    const unsigned u = __float_as_uint(d2[e]);
                    const int bit = 4 * j + q + e;
                    if constexpr (!EXACT) {
                        // the sign bit shifted into the word (v_alignbit: (word << 1) | (u >> 31); element i of a word ends
                        // at bit 31 - i), copysign(1, d) as the factor
                        sgn_neg[bit >> 5] = __builtin_amdgcn_alignbit(sgn_neg[bit >> 5], u, 31);
                        sg2[e] = __uint_as_float((u & 0x80000000u) | 0x3f800000u);
                    } else {
                        const unsigned neg = u >> 31, mag = min(u & 0x7fffffffu, 1u);
                        sgn_neg[bit >> 5] |= (mag & neg) << (bit & 31);
                        sgn_pos[bit >> 5] |= (mag & (neg ^ 1u)) << (bit & 31);
                        sg2[e] = __uint_as_float((u & 0x80000000u) | 0x3f800000u) * (float)mag;  // sign(diff)
                    }
                }
                if constexpr (!EXACT) minabs = fminf(minabs, fminf(fabsf(d2[0]), fabsf(d2[1])));
                const l_f32x2 gg2 = sg2 * vm;  // d l1 / d y = sign(diff) v m
                dot2 = __builtin_elementwise_fma(x2, gg2, dot2);  // (even / odd elements in the two halves, added at the end)
                a02 = __builtin_elementwise_fma(-gg2, f0, a02); a12 = __builtin_elementwise_fma(-gg2, f1, a12);
                a22 = __builtin_elementwise_fma(-gg2, f2, a22);
            }
        }
        __builtin_amdgcn_sched_barrier(0);  // one step at a time (unfenced, every gather of the pixel is hoisted: 256 VGPRs)
    }
    };
    pass1(GagsLossFalse{});
    bool exact_signs = false;
    if (BWD) {
        minabs = fminf(minabs, __shfl_xor(minabs, 1)); minabs = fminf(minabs, __shfl_xor(minabs, 2));
        minabs = fminf(minabs, __shfl_xor(minabs, 4));  // (the eight lanes of a pixel decide together: their sums are shared)
        if (minabs == 0.f && vm != 0.f) {
            exact_signs = true;
            a02 = a12 = a22 = dot2 = l_f32x2{0.f, 0.f};
            sgn_neg[0] = sgn_neg[1] = 0u;
            pass1(GagsLossTrue{});
        }
        a0 = a02[0] + a02[1]; a1 = a12[0] + a12[1]; a2 = a22[0] + a22[1]; dot = dot2[0] + dot2[1];
    }
    a0 += __shfl_xor(a0, 1); a0 += __shfl_xor(a0, 2); a0 += __shfl_xor(a0, 4);
    if (!BWD) {
        if ((tid & 7) == 0 && pr < HW) {
            l1_map[pr] = (a0 * m) / (float)c;
            mask_out[pr] = m;
        }
        return;
    }
    a1 += __shfl_xor(a1, 1); a1 += __shfl_xor(a1, 2); a1 += __shfl_xor(a1, 4);
    a2 += __shfl_xor(a2, 1); a2 += __shfl_xor(a2, 4); a2 += __shfl_xor(a2, 2);
    dot += __shfl_xor(dot, 1); dot += __shfl_xor(dot, 2); dot += __shfl_xor(dot, 4);
    if (pr >= HW) return;
    if ((tid & 7) == 0) {
        v_scale[pr] = a0; v_scale[(size_t)HW + pr] = a1; v_scale[2 * (size_t)HW + pr] = a2;
    }
    // y = x / n:  dz = (g - y <y, g>) / n = g / n - x <x, g> / n^3;  g = sign(diff) v m, the signs kept as two bit sets
    float k1 = dot * inv * inv * inv, gmag = vm * inv;
    if constexpr (DZM == 2) { const float sc = dz_scale[0]; k1 *= sc; gmag *= sc; }  // (a power of two: exact)
    auto pass2 = [&](auto exact_tag) __attribute__((always_inline)) {
    constexpr bool EXACT = decltype(exact_tag)::value;
#pragma unroll
    for (int j = 0; j < FHJ; ++j) {
        const float xe[4] = {v[j].x, v[j].y, v[j].z, v[j].w};
        unsigned pk[2];
        float df[4];
#pragma unroll
        for (int q = 0; q < 4; q += 2) {
            l_f32x2 sg2;
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int bit = 4 * j + q + e;
                if constexpr (!EXACT)
                    sg2[e] = __uint_as_float(((sgn_neg[bit >> 5] << (bit & 31)) & 0x80000000u) | 0x3f800000u);
                else
                    sg2[e] = (float)((int)((sgn_pos[bit >> 5] >> (bit & 31)) & 1u) - (int)((sgn_neg[bit >> 5] >> (bit & 31)) & 1u));
            }
            const l_f32x2 x2 = {xe[q], xe[q + 1]};
            const l_f32x2 dq2 = __builtin_elementwise_fma(-x2, l_f32x2{k1, k1}, sg2 * gmag);
            if constexpr (DZM == 2) {
                typedef _Float16 l_f16x2 __attribute__((ext_vector_type(2)));
                // (saturating at +-65504: MODE.FP16_OVFL is set at the top of this instantiation -- csrc/half16.h has the story)
                pk[q >> 1] = __builtin_bit_cast(unsigned, __builtin_convertvector(dq2, l_f16x2));
            } else
            pk[q >> 1] = __builtin_bit_cast(unsigned, __builtin_convertvector(dq2, l_bf16x2));
            df[q] = dq2[0]; df[q + 1] = dq2[1];
        }
        // (streaming stores: 2.1 GB that the input-gradient chain and the last layer's weight gradient read from HBM later)
        typedef float nt_f4 __attribute__((ext_vector_type(4)));
        typedef unsigned nt_u2 __attribute__((ext_vector_type(2)));
        if constexpr (DZM == 1)
            __builtin_nontemporal_store(nt_f4{df[0], df[1], df[2], df[3]},
                                        reinterpret_cast<nt_f4 *>(reinterpret_cast<float *>(dz) + (size_t)pr * c + c0 + 32 * j));
        else
            __builtin_nontemporal_store(nt_u2{pk[0], pk[1]}, reinterpret_cast<nt_u2 *>(dz + (size_t)pr * c + c0 + 32 * j));
    }
    };
    if (exact_signs) pass2(GagsLossTrue{});  // (rare: the pixel met an exact tie)
    else pass2(GagsLossFalse{});
}

// One launch of the fused head: ONE_TAP when the segmentation map has the render's resolution.  Pointers a direction does
// not use are null (forward: v_map, dz, v_scale; backward: l1_map, mask; dz_scale: the f16 tier, DZM 2, only).
template <bool BWD, int DZM>
int launch_head_distill(int H, int W, int h, int w, int n_emb, const float *x, const float *img_embed, const float *seg_map,
                        const float *scale_map, const float *v_map, float *l1_map, float *mask, void *dz, float *v_scale,
                        const float *dz_scale, hipStream_t st)
{
    const auto kernel = (H == h && W == w) ? head_distill_kernel<BWD, true, DZM> : head_distill_kernel<BWD, false, DZM>;
    hipLaunchKernelGGL(kernel, dim3((H * W + TPM - 1) / TPM), dim3(256), 0, st, H, W, h, w, n_emb, x, img_embed, seg_map,
                       scale_map, v_map, l1_map, mask, (unsigned short *)dz, v_scale, dz_scale);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

// (the reference's CNN_decoder(16, 512); other widths take the two-step route)
inline bool head_args_ok(int c, int ld, int H, int W, int h, int w, int n_emb)
{
    return sam_args_ok(c, H, W, h, w, n_emb) && c == 512 && ld == 512;
}

}  // namespace

extern "C" int gags_decoder_head_distill_fwd(int c, int ld, int H, int W, int h, int w, int n_emb, const float *x,
                                             const float *img_embed, const float *seg_map, const float *scale_map,
                                             float *l1_map, float *mask, void *stream)
{
    GAGS_CLEAR_ERR();
    if (!head_args_ok(c, ld, H, W, h, w, n_emb) || !x || !img_embed || !seg_map || !scale_map || !l1_map || !mask) return GAGS_EINVAL;
    return launch_head_distill<false, 0>(H, W, h, w, n_emb, x, img_embed, seg_map, scale_map, nullptr, l1_map, mask, nullptr,
                                         nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int gags_decoder_head_distill_bwd(int c, int ld, int H, int W, int h, int w, int n_emb, const float *x,
                                             const float *img_embed, const float *seg_map, const float *scale_map,
                                             const float *v_map, void *dz_bf16, float *v_scale, void *stream)
{
    GAGS_CLEAR_ERR();
    if (!head_args_ok(c, ld, H, W, h, w, n_emb) || !x || !img_embed || !seg_map || !scale_map || !v_map || !dz_bf16 || !v_scale)
        return GAGS_EINVAL;
    return launch_head_distill<true, 0>(H, W, h, w, n_emb, x, img_embed, seg_map, scale_map, v_map, nullptr, nullptr, dz_bf16,
                                        v_scale, nullptr, (hipStream_t)stream);
}

extern "C" int gags_decoder_head_distill_bwd_h16(int c, int ld, int H, int W, int h, int w, int n_emb, const float *x,
                                                 const float *img_embed, const float *seg_map, const float *scale_map,
                                                 const float *v_map, void *dz_f16, const float *dz_scale, float *v_scale,
                                                 void *stream)
{
    GAGS_CLEAR_ERR();
    if (!head_args_ok(c, ld, H, W, h, w, n_emb) || !x || !img_embed || !seg_map || !scale_map || !v_map || !dz_f16 || !dz_scale ||
        !v_scale)
        return GAGS_EINVAL;
    return launch_head_distill<true, 2>(H, W, h, w, n_emb, x, img_embed, seg_map, scale_map, v_map, nullptr, nullptr, dz_f16,
                                        v_scale, dz_scale, (hipStream_t)stream);
}

extern "C" int gags_decoder_head_distill_bwd_f32(int c, int ld, int H, int W, int h, int w, int n_emb, const float *x,
                                                 const float *img_embed, const float *seg_map, const float *scale_map,
                                                 const float *v_map, float *dz, float *v_scale, void *stream)
{
    GAGS_CLEAR_ERR();
    if (!head_args_ok(c, ld, H, W, h, w, n_emb) || !x || !img_embed || !seg_map || !scale_map || !v_map || !dz || !v_scale)
        return GAGS_EINVAL;
    return launch_head_distill<true, 1>(H, W, h, w, n_emb, x, img_embed, seg_map, scale_map, v_map, nullptr, nullptr, dz, v_scale,
                                        nullptr, (hipStream_t)stream);
}
