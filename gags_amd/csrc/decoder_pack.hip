// Packing and unpacking around the 16-bit decoder chains: the fp32 input rows padded to 16-bit rows, a layer's (or a whole
// decoder's) parameters in every form the kernels read, and the input gradient back to fp32.
#include "decoder_common.h"

namespace {

// fp32 [P, C] (pixel-major: the rasterizer's own [H, W, D] output) -> bf16 [P, Cp], zero-padded to Cp >= C
__global__ __launch_bounds__(256) void to_bf16_pad_kernel(int64_t P, int C, int Cp, const float *__restrict__ x,
                                                          unsigned short *__restrict__ y)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P * Cp) return;
    const int64_t p = i / Cp;
    const int c = (int)(i - p * Cp);
    y[i] = c < C ? h16_from(x[p * C + c]) : (unsigned short)0;
}

// bf16 [P, ld] -> fp32 [P, C] (first C columns): the input gradient in the rasterizer's [H, W, D] layout
__global__ __launch_bounds__(256) void unpack_f32_kernel(int64_t P, int C, int ld, const unsigned short *__restrict__ x,
                                                         float *__restrict__ y)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P * C) return;
    const int64_t p = i / C;
    y[i] = h16_to(x[p * ld + (i - p * C)]);
}

// one layer's parameters in every form the kernels read, in ONE launch (torch: zeros + slice copy + cast + transpose +
// two permuted copies + the bias pair = ~10 tiny kernels per layer, ~150 per iteration for the two decoders)
__global__ __launch_bounds__(256) void pack_layer_kernel(int co, int ci, int np, int kp, const float *__restrict__ w,
                                                         const float *__restrict__ b, unsigned short *__restrict__ wr,
                                                         unsigned short *__restrict__ wtr, unsigned short *__restrict__ wf,
                                                         unsigned short *__restrict__ wtf, float *__restrict__ bp)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < np) bp[e] = e < co ? b[e] : 0.f;
    if (e >= np * kp) return;
    const int n = e / kp, k = e - n * kp;
    const float v = (n < co && k < ci) ? w[(size_t)n * ci + k] : 0.f;
    const unsigned short h = h16_from(v);  // RN-even, as torch
    wr[(size_t)n * kp + k] = h;
    wtr[(size_t)k * np + n] = h;
    // fragment order of a [R, C] matrix: [R / 32][C / 16][2][32][8] (gags_amd/decoders.py: _frag_layout)
    wf[((((size_t)(n >> 5) * (kp >> 4) + (k >> 4)) * 2 + ((k >> 3) & 1)) * 32 + (n & 31)) * 8 + (k & 7)] = h;
    wtf[((((size_t)(k >> 5) * (np >> 4) + (n >> 4)) * 2 + ((n >> 3) & 1)) * 32 + (k & 31)) * 8 + (n & 7)] = h;
}
}  // namespace

extern "C" int GAGS_DEC(gags_decoder_pack_layer)(int co, int ci, const float *w, const float *b, void *w_bf16, void *wt_bf16, void *w_frag,
                                       void *wt_frag, float *bias_pad, void *stream)
{
    GAGS_CLEAR_ERR();
    if (co <= 0 || ci <= 0 || !w || !b || !w_bf16 || !wt_bf16 || !w_frag || !wt_frag || !bias_pad) return GAGS_EINVAL;
    const int np = (co + 31) / 32 * 32, kp = (ci + 31) / 32 * 32;
    hipLaunchKernelGGL(pack_layer_kernel, dim3((unsigned)((np * kp + 255) / 256)), dim3(256), 0, (hipStream_t)stream, co, ci, np, kp, w, b,
                       (unsigned short *)w_bf16, (unsigned short *)wt_bf16, (unsigned short *)w_frag, (unsigned short *)wt_frag, bias_pad);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

// every layer of a decoder in ONE launch (round 6: nine + six launches of ~5 us per iteration before): blockIdx.y = layer
namespace {
constexpr int PACK_MAX_LAYERS = 12;
struct PackArgs {
    int co[PACK_MAX_LAYERS], ci[PACK_MAX_LAYERS];
    const float *w[PACK_MAX_LAYERS], *b[PACK_MAX_LAYERS];
    unsigned short *wr[PACK_MAX_LAYERS], *wtr[PACK_MAX_LAYERS], *wf[PACK_MAX_LAYERS], *wtf[PACK_MAX_LAYERS];
    float *bp[PACK_MAX_LAYERS];
};
__global__ __launch_bounds__(256) void pack_layers_kernel(PackArgs a)
{
    const int L = blockIdx.y;
    const int co = a.co[L], ci = a.ci[L], np = (co + 31) / 32 * 32, kp = (ci + 31) / 32 * 32;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e < np) a.bp[L][e] = e < co ? a.b[L][e] : 0.f;
    if (e >= np * kp) return;
    const int n = e / kp, k = e - n * kp;
    const float v = (n < co && k < ci) ? a.w[L][(size_t)n * ci + k] : 0.f;
    const unsigned short h = h16_from(v);
    a.wr[L][(size_t)n * kp + k] = h;
    a.wtr[L][(size_t)k * np + n] = h;
    a.wf[L][((((size_t)(n >> 5) * (kp >> 4) + (k >> 4)) * 2 + ((k >> 3) & 1)) * 32 + (n & 31)) * 8 + (k & 7)] = h;
    a.wtf[L][((((size_t)(k >> 5) * (np >> 4) + (n >> 4)) * 2 + ((n >> 3) & 1)) * 32 + (k & 31)) * 8 + (n & 7)] = h;
}
}  // namespace

extern "C" int GAGS_DEC(gags_decoder_pack_layers)(int n_layers, const int *co, const int *ci, const float *const *w, const float *const *b,
                                        void *const *w_bf16, void *const *wt_bf16, void *const *w_frag, void *const *wt_frag,
                                        float *const *bias_pad, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_layers <= 0 || n_layers > PACK_MAX_LAYERS || !co || !ci || !w || !b || !w_bf16 || !wt_bf16 || !w_frag || !wt_frag || !bias_pad)
        return GAGS_EINVAL;
    PackArgs a;
    int most = 0;
    for (int i = 0; i < n_layers; ++i) {
        if (co[i] <= 0 || ci[i] <= 0 || !w[i] || !b[i] || !w_bf16[i] || !wt_bf16[i] || !w_frag[i] || !wt_frag[i] || !bias_pad[i])
            return GAGS_EINVAL;
        a.co[i] = co[i]; a.ci[i] = ci[i]; a.w[i] = w[i]; a.b[i] = b[i];
        a.wr[i] = (unsigned short *)w_bf16[i]; a.wtr[i] = (unsigned short *)wt_bf16[i];
        a.wf[i] = (unsigned short *)w_frag[i]; a.wtf[i] = (unsigned short *)wt_frag[i]; a.bp[i] = bias_pad[i];
        const int np = (co[i] + 31) / 32 * 32, kp = (ci[i] + 31) / 32 * 32;
        most = np * kp > most ? np * kp : most;
    }
    hipLaunchKernelGGL(pack_layers_kernel, dim3((unsigned)((most + 255) / 256), (unsigned)n_layers), dim3(256), 0, (hipStream_t)stream, a);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int GAGS_DEC(gags_decoder_pack_input)(int64_t n_pix, int c, int c_pad, const float *x, void *y_bf16, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_pix < 0 || c <= 0 || c_pad < c || c_pad % 32 != 0 || (n_pix > 0 && (!x || !y_bf16))) return GAGS_EINVAL;
    if (n_pix == 0) return GAGS_OK;
    hipLaunchKernelGGL(to_bf16_pad_kernel, dim3((unsigned)((n_pix * c_pad + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       n_pix, c, c_pad, x, (unsigned short *)y_bf16);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int GAGS_DEC(gags_decoder_unpack_grad)(int64_t n_pix, int c, int ld, const void *x_bf16, float *y, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_pix < 0 || c <= 0 || ld < c || (n_pix > 0 && (!x_bf16 || !y))) return GAGS_EINVAL;
    if (n_pix == 0) return GAGS_OK;
    hipLaunchKernelGGL(unpack_f32_kernel, dim3((unsigned)((n_pix * c + 255) / 256)), dim3(256), 0, (hipStream_t)stream, n_pix, c,
                       ld, (const unsigned short *)x_bf16, y);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
