// N10 (include/gags_next.h): the mask post-processing between SAM's mask generator and the CLIP tile encoder of the GAS
// stage (preprocess.py:373-489, 307-318) -- mask_nms's pair statistics and mask2segmap's painting -- on bit-packed masks.
//
// (a) pack: a wave per 64-pixel word of the flattened image, one __ballot per word; the wave takes PACK_WORDS_PER_WAVE
//     consecutive words (all their byte loads are issued before the first ballot), sums their popcounts in a register
//     and adds the sum to area[m] with one integer atomic; lane k stores word k.
// (b) pairs: inter[i, j] = sum_w popcount(bits[i, w] & bits[j, w]).  A block of 256 threads owns one 32 x 32 tile of pairs
//     (upper-triangle tiles only: an off-diagonal tile is written to both halves of the matrix) and one chunk of
//     PAIR_CHUNK_WORDS words.  The chunk is staged through LDS 64 words at a time (rows padded to 65 words: the eight rows
//     a wave reads in one instruction sit two banks apart); each of the four waves takes 16 of the 64 staged words and each
//     lane a 4 x 4 register micro-tile (rows ty + 8 r, columns tx + 8 c), so one 8-byte LDS read feeds four pairs: per word
//     8 reads against 16 AND + popcount pairs.  The four waves' partial tiles are summed through LDS and leave as one
//     integer atomicAdd per pair into the zeroed matrix: exact, and independent of the order in which blocks finish.
//     Why this shape: M is typically 30 .. 100, i.e. one to ten tiles -- the word dimension (32 400 words at 1080p, 64
//     chunks) is what fills 256 CUs; a 64 x 64 tile would waste three quarters of its work at M = 33.
// (c) colmax: a thread per column rank walks all ranks (M^2 fp32 divisions in total: negligible next to (b)).
// (d) paint: a wave per word, a lane per pixel; the wave walks the kept masks from the last to the first (the word is one
//     wave-uniform load) and stops once every pixel of the word is owned; 64 coalesced 4-byte stores per word.
// No float atomics anywhere; every index read from device memory (order, kept) is range-checked before it is used.
#include <algorithm>
#include "common.h"
#include "gags_next.h"
#include "launch.h"

namespace {

constexpr int MAX_MASKS = 8192;            // inter[M, M] int32 = 256 MiB at the cap; i * M + j < 2^26
constexpr int64_t MAX_PIXELS = 1ll << 24;  // exclusive: counts stay exact as fp32
constexpr int PACK_WORDS_PER_WAVE = 16;
constexpr int PAIR_TILE = 32;              // pairs per tile side
constexpr int PAIR_STAGE = 64;             // words staged in LDS at a time
constexpr int PAIR_PITCH = PAIR_STAGE + 1; // LDS row pitch in words
constexpr int PAIR_CHUNK_WORDS = 512;      // words per block (a multiple of PAIR_STAGE): 32 768 pixels

__global__ __launch_bounds__(256) void pack_kernel(int64_t hw, int64_t nw, const unsigned char *__restrict__ masks,
                                                   unsigned long long *__restrict__ bits, int *__restrict__ area)
{
    const int m = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t w0 = ((int64_t)blockIdx.x * 4 + wave) * PACK_WORDS_PER_WAVE;
    const unsigned char *src = masks + (int64_t)m * hw;
    // all the wave's byte loads first (16 independent loads in flight per lane), then the ballots
    unsigned char v[PACK_WORDS_PER_WAVE];
#pragma unroll
    for (int k = 0; k < PACK_WORDS_PER_WAVE; ++k) {
        const int64_t p = (w0 + k) * 64 + lane;
        v[k] = p < hw ? src[p] : (unsigned char)0;  // (p < hw implies w0 + k < nw)
    }
    int count = 0;
    unsigned long long mine = 0;  // lane k keeps word k: the words leave as one contiguous store
#pragma unroll
    for (int k = 0; k < PACK_WORDS_PER_WAVE; ++k) {
        const unsigned long long word = __ballot(v[k] != 0);
        if (lane == k) mine = word;
        count += __popcll(word);
    }
    if (lane < PACK_WORDS_PER_WAVE && w0 + lane < nw) bits[(int64_t)m * nw + w0 + lane] = mine;
    if (lane == 0 && count) atomicAdd(area + m, count);
}

// tile pair t (0-based, upper triangle, row-major) of an n x n tile grid -> (ti, tj), ti <= tj
__device__ __forceinline__ void tile_of(int t, int n, int &ti, int &tj)
{
    int i = 0;
    while (t >= n - i) {
        t -= n - i;
        ++i;
    }
    ti = i;
    tj = i + t;
}

__global__ __launch_bounds__(256) void pairs_kernel(int M, int64_t nw, const unsigned long long *__restrict__ bits,
                                                    int *__restrict__ inter)
{
    __shared__ unsigned long long lds[2 * PAIR_TILE * PAIR_PITCH];  // 33 280 B; re-used for the waves' partial tiles
    unsigned long long *A = lds, *B = lds + PAIR_TILE * PAIR_PITCH;
    int ti, tj;
    tile_of(blockIdx.x, (M + PAIR_TILE - 1) / PAIR_TILE, ti, tj);
    const int i0 = ti * PAIR_TILE, j0 = tj * PAIR_TILE;
    const int64_t wbeg = (int64_t)blockIdx.y * PAIR_CHUNK_WORDS;
    const int64_t wend = wbeg + PAIR_CHUNK_WORDS < nw ? wbeg + PAIR_CHUNK_WORDS : nw;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ty = lane >> 3, tx = lane & 7;
    int acc[4][4] = {};
    for (int64_t ws = wbeg; ws < wend; ws += PAIR_STAGE) {
        // stage 32 rows x 64 words of both sides: a wave reads 512 contiguous bytes of one row; past M or wend: zero
        for (int r = wave; r < 2 * PAIR_TILE; r += 4) {
            const int row = r < PAIR_TILE ? i0 + r : j0 + (r - PAIR_TILE);
            const int64_t w = ws + lane;
            lds[r * PAIR_PITCH + lane] = (row < M && w < wend) ? bits[(int64_t)row * nw + w] : 0ull;
        }
        __syncthreads();
        const int k0 = wave * (PAIR_STAGE / 4);
#pragma unroll 4
        for (int k = k0; k < k0 + PAIR_STAGE / 4; ++k) {
            unsigned long long a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) a[r] = A[(ty + 8 * r) * PAIR_PITCH + k];
#pragma unroll
            for (int c = 0; c < 4; ++c) b[c] = B[(tx + 8 * c) * PAIR_PITCH + k];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) acc[r][c] += __popcll(a[r] & b[c]);
        }
        __syncthreads();
    }
    // the four waves' partial tiles -> one tile (LDS as int[4][1024]; the loop's last barrier has retired every read)
    int *red = (int *)lds;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) red[wave * 1024 + (ty + 8 * r) * PAIR_TILE + (tx + 8 * c)] = acc[r][c];
    __syncthreads();
    for (int e = threadIdx.x; e < PAIR_TILE * PAIR_TILE; e += 256) {
        const int i = i0 + e / PAIR_TILE, j = j0 + e % PAIR_TILE;
        if (i >= M || j >= M) continue;
        const int s = (red[e] + red[1024 + e]) + (red[2048 + e] + red[3072 + e]);
        if (s == 0) continue;  // the matrix starts zeroed
        atomicAdd(inter + (int64_t)i * M + j, s);
        if (ti != tj) atomicAdd(inter + (int64_t)j * M + i, s);
    }
}

// colmax[0..2][c] for column rank c (the rule in gags_next.h): ranks r < c are the pairs (i = r, j = c), ranks r > c
// the pairs (i = c, j = r) whose LOWER entry inner[r, c] lies in column c
__global__ __launch_bounds__(64) void colmax_kernel(int M, const int *__restrict__ inter, const int *__restrict__ area,
                                                    const int *__restrict__ order, float *__restrict__ colmax)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= M) return;
    float m_iou = 0.f, m_up = 0.f, m_low = 0.f;
    const int oc = order[c];
    if ((unsigned)oc < (unsigned)M) {
        const int ac = area[oc];
        const float fac = (float)ac;
        for (int r = 0; r < M; ++r) {
            const int orr = order[r];
            if (r == c || (unsigned)orr >= (unsigned)M) continue;
            const int ar = area[orr];
            const int in = inter[(int64_t)orr * M + oc];
            const float fi = (float)in;
            const float rc = fi / fac, rr = fi / (float)ar;  // r_c, r_r
            if (r < c) {                                      // i = r, j = c
                const float iou = fi / (float)(ar + ac - in);
                m_iou = iou > m_iou ? iou : m_iou;
                if (rr < 0.5f && rc >= 0.85f) {
                    const float prod = rc * rr;
                    const float v = 1.f - prod;
                    m_up = v > m_up ? v : m_up;
                    if (r == c - 1) m_low = v > m_low ? v : m_low;  // tril(diagonal=1) keeps the first superdiagonal
                }
            } else if (rc >= 0.85f && rr < 0.5f) {            // i = c, j = r: inner[r, c]
                const float prod = rr * rc;
                const float v = 1.f - prod;
                m_low = v > m_low ? v : m_low;
            }
        }
    }
    colmax[c] = m_iou;
    colmax[M + c] = m_up;
    colmax[2 * M + c] = m_low;
}

__global__ __launch_bounds__(256) void paint_kernel(int M, int64_t hw, int64_t nw, const unsigned long long *__restrict__ bits,
                                                    int K, const int *__restrict__ kept, int offset, int *__restrict__ seg)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= nw) return;  // wave-uniform
    const int64_t p = w * 64 + lane;
    const int64_t left = hw - w * 64;  // >= 1
    const unsigned long long valid = left >= 64 ? ~0ull : (1ull << left) - 1;
    unsigned long long owned = 0;
    int id = -1;
    for (int k = K - 1; k >= 0 && owned != valid; --k) {
        const int m = kept[k];
        if ((unsigned)m >= (unsigned)M) continue;
        const unsigned long long word = bits[(int64_t)m * nw + w] & valid;
        if (((word & ~owned) >> lane) & 1ull) id = k + offset;
        owned |= word;
    }
    if (p < hw) seg[p] = id;
}

bool bad_sizes(int M, int64_t hw) { return M < 0 || M > MAX_MASKS || hw < 1 || hw >= MAX_PIXELS; }
inline int64_t words(int64_t hw) { return (hw + 63) / 64; }

// the NMS driver's scratch: the packed masks and the M x M intersection counts (base NULL: sizes only)
struct NmsScratch {
    void *bits;
    int *inter;
    int64_t total;
};
NmsScratch nms_carve(void *base, int M, int64_t hw)
{
    GagsCarve c(base);
    NmsScratch L;
    L.bits = c.take<unsigned long long>((int64_t)M * words(hw));
    L.inter = c.take<int>((int64_t)M * M);
    L.total = c.total();
    return L;
}

int launch_pack(int M, int64_t hw, const unsigned char *masks, void *bits, int *area, hipStream_t st)
{
    if (hipMemsetAsync(area, 0, (size_t)M * 4, st) != hipSuccess) return GAGS_ELAUNCH;
    const int64_t nw = words(hw);
    const unsigned gx = (unsigned)((nw + 4 * PACK_WORDS_PER_WAVE - 1) / (4 * PACK_WORDS_PER_WAVE));
    hipLaunchKernelGGL(pack_kernel, dim3(gx, M), dim3(256), 0, st, hw, nw, masks, (unsigned long long *)bits, area);
    return GAGS_OK;
}

int launch_pairs(int M, int64_t nw, const void *bits, int *inter, hipStream_t st)
{
    if (hipMemsetAsync(inter, 0, (size_t)M * M * 4, st) != hipSuccess) return GAGS_ELAUNCH;
    const int nt = (M + PAIR_TILE - 1) / PAIR_TILE;
    const unsigned gx = (unsigned)(nt * (nt + 1) / 2), gy = (unsigned)((nw + PAIR_CHUNK_WORDS - 1) / PAIR_CHUNK_WORDS);
    hipLaunchKernelGGL(pairs_kernel, dim3(gx, gy), dim3(256), 0, st, M, nw, (const unsigned long long *)bits, inter);
    return GAGS_OK;
}

void launch_colmax(int M, const int *inter, const int *area, const int *order, float *colmax, hipStream_t st)
{
    hipLaunchKernelGGL(colmax_kernel, dim3((M + 63) / 64), dim3(64), 0, st, M, inter, area, order, colmax);
}

}  // namespace

extern "C" int gags_masks_max_count(void) { return MAX_MASKS; }

extern "C" int gags_masks_pair_chunk_words(void) { return PAIR_CHUNK_WORDS; }

extern "C" int gags_masks_pack(int n_masks, int64_t n_pixels, const unsigned char *masks, void *bits, int32_t *area,
                               void *stream)
{
    GAGS_CLEAR_ERR();
    if (bad_sizes(n_masks, n_pixels)) return GAGS_EINVAL;
    if (n_masks == 0) return GAGS_OK;
    if (!masks || !bits || !area) return GAGS_EINVAL;
    const int rc = launch_pack(n_masks, n_pixels, masks, bits, area, (hipStream_t)stream);
    if (rc != GAGS_OK) return rc;
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_masks_pairs(int n_masks, int64_t n_pixels, const void *bits, int32_t *inter, void *stream)
{
    GAGS_CLEAR_ERR();
    if (bad_sizes(n_masks, n_pixels)) return GAGS_EINVAL;
    if (n_masks == 0) return GAGS_OK;
    if (!bits || !inter) return GAGS_EINVAL;
    const int rc = launch_pairs(n_masks, words(n_pixels), bits, inter, (hipStream_t)stream);
    if (rc != GAGS_OK) return rc;
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_masks_colmax(int n_masks, const int32_t *inter, const int32_t *area, const int32_t *order,
                                 float *colmax, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_masks < 0 || n_masks > MAX_MASKS) return GAGS_EINVAL;
    if (n_masks == 0) return GAGS_OK;
    if (!inter || !area || !order || !colmax) return GAGS_EINVAL;
    launch_colmax(n_masks, inter, area, order, colmax, (hipStream_t)stream);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int gags_masks_paint(int n_masks, int64_t n_pixels, const void *bits, int n_kept, const int32_t *kept,
                                int offset, int32_t *seg, void *stream)
{
    GAGS_CLEAR_ERR();
    if (bad_sizes(n_masks, n_pixels) || n_kept < 0 || n_kept > n_masks || offset < 0 ||
        (int64_t)offset + n_kept > INT32_MAX)
        return GAGS_EINVAL;
    if (!seg || (n_kept > 0 && (!bits || !kept))) return GAGS_EINVAL;
    if (n_kept == 0) {  // nothing to paint: every pixel is -1, and nothing is launched
        if (hipMemsetAsync(seg, 0xff, (size_t)n_pixels * 4, (hipStream_t)stream) != hipSuccess) return GAGS_ELAUNCH;
        return GAGS_OK;
    }
    const int64_t nw = words(n_pixels);
    hipLaunchKernelGGL(paint_kernel, dim3((unsigned)((nw + 3) / 4)), dim3(256), 0, (hipStream_t)stream, n_masks, n_pixels,
                       nw, (const unsigned long long *)bits, n_kept, kept, offset, seg);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int64_t gags_masks_nms_scratch_bytes(int n_masks, int64_t n_pixels)
{
    if (bad_sizes(n_masks, n_pixels) || n_masks == 0) return 0;
    return nms_carve(nullptr, n_masks, n_pixels).total;
}

extern "C" int gags_masks_nms_colmax(int n_masks, int64_t n_pixels, const unsigned char *masks, const int32_t *order,
                                     int32_t *area, float *colmax, void *scratch, int64_t scratch_bytes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (bad_sizes(n_masks, n_pixels)) return GAGS_EINVAL;
    if (n_masks == 0) return GAGS_OK;
    if (!masks || !order || !area || !colmax || !scratch) return GAGS_EINVAL;
    const NmsScratch L = nms_carve(scratch, n_masks, n_pixels);
    if (scratch_bytes < L.total) return GAGS_ESCRATCH;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nw = words(n_pixels);
    void *bits = L.bits;
    int *inter = L.inter;
    int rc = launch_pack(n_masks, n_pixels, masks, bits, area, st);
    if (rc != GAGS_OK) return rc;
    rc = launch_pairs(n_masks, nw, bits, inter, st);
    if (rc != GAGS_OK) return rc;
    launch_colmax(n_masks, inter, area, order, colmax, st);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
