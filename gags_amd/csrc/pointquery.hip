// N5 (include/gags_next.h): the 3-D open-vocabulary query of compute_relvancy.py:273-394 (`pcd_relvancy`, --pcd_mode)
// on the Gaussians themselves, after the decoder and the relevancy head have run per Gaussian.
//
// (a) per phrase the relevancy's min / max (integer atomics on order-preserving keys: exact and order-independent, no host
//     readback) and one map: normalised = clip((r - min) / (max - min + 1e-9) * 2 - 1, 0, 1), mask = normalised > thresh.
// (b) utils/pcd_utils.py:204-219 `smooth_pcd_mask` -- a Python loop over every point with one KDTree.query_ball_point
//     each -- as a masked radius-neighbour count for all phrases at once:
//       c_i = #{ j : mask[j] and ((dx*dx + dy*dy) + dz*dz) <= fl(r*r) }   (float64 from the float32 coordinates, no FMA:
//                                                                          scipy's sqeuclidean distance for m = 3)
//       out_i = c_i > threshold  or  (mask_i and c_i >= 10)
//     Only masked points are candidates, and no count is needed past cap = max(threshold + 1, 10).
//     Grid: cubic cells of edge r (1 + 2^-20) over the cloud's bounding box -- float64 rounding of the cell index can then
//     never put two points within r more than one cell apart -- clamped to 16 bits per axis (monotone: a superset of the
//     candidates survives, only the scan grows).  Candidates: (phrase, cell) keys of the masked points, unmasked points
//     under a sentinel phrase K that sorts last; one stable radix sort (csrc/sort.hip) of all K n pairs, then their
//     coordinates gathered into sorted order.  Queries: one thread per (phrase, point), points visited in cell order
//     (a second sort of the N cell keys) so that a wave's binary searches and candidate reads stay in the same cells;
//     per (dx, dy) neighbour column one range of three consecutive cells, scan stops at cap.  Each thread writes its own
//     result: no atomics on the output, bit-reproducible.
#include <algorithm>
#include <cmath>
#include "launch.h"
#include "gags_next.h"
#include "reduce.h"

namespace {

constexpr int CELL_BITS = 16;
constexpr uint64_t CELL_MAX = (1u << CELL_BITS) - 1;
constexpr int PHRASE_SHIFT = 3 * CELL_BITS;  // key = phrase << 48 | cx << 32 | cy << 16 | cz
constexpr int MAX_MASKS = 65534;            // phrase field 16 bits, value n_masks = the sentinel

__global__ void minmax_init_kernel(int n_keys, unsigned *__restrict__ keys)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i < n_keys) keys[i] = (i % 2 == 0) ? 0xffffffffu : 0u;
}

// keys[2 k] = min, keys[2 k + 1] = max of probs[k, :, 0]
__global__ __launch_bounds__(256) void rel_minmax_kernel(int64_t n, const float *__restrict__ probs, unsigned *__restrict__ keys)
{
    const int k = blockIdx.y;
    unsigned kmin = 0xffffffffu, kmax = 0u;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const unsigned u = gags_f2key(probs[((int64_t)k * n + i) * 2]);
        kmin = min(kmin, u);
        kmax = max(kmax, u);
    }
    gags_block_minmax(kmin, kmax, keys + 2 * k, keys + 2 * k + 1);
}

// compute_relvancy.py:363-367, in the reference's order (max(fl(r_i - min)) == fl(max - min): fl(. - min) is monotone)
__global__ __launch_bounds__(256) void rel_normalise_kernel(int64_t n, float thresh, const float *__restrict__ probs,
                                                            const unsigned *__restrict__ keys, float *__restrict__ normalized,
                                                            unsigned char *__restrict__ mask)
{
    const int k = blockIdx.y;
    const float mn = gags_key2f(keys[2 * k]), mx = gags_key2f(keys[2 * k + 1]);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t o = (int64_t)k * n + i;
        float r = probs[o * 2] - mn;
        r = r / ((mx - mn) + 1e-9f);
        r = r * 2.0f + -1.0f;
        r = fminf(fmaxf(r, 0.f), 1.f);
        normalized[o] = r;
        mask[o] = r > thresh ? 1 : 0;
    }
}

__global__ void bbox_init_kernel(unsigned *__restrict__ bbox)
{
    if (threadIdx.x < 3) bbox[threadIdx.x] = 0xffffffffu;
}

// bbox[a] = key of min over the points of coordinate a
__global__ __launch_bounds__(256) void bbox_kernel(int64_t n, const float *__restrict__ xyz, unsigned *__restrict__ bbox)
{
    const int a = blockIdx.y;
    unsigned kmin = 0xffffffffu;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        kmin = min(kmin, gags_f2key(xyz[i * 3 + a]));
    gags_block_minmax(kmin, 0u, bbox + a, nullptr);
}

__device__ __forceinline__ uint64_t cell_coord(float x, float lo, double cell)
{
    // fl(x - lo) >= 0 (x >= lo, rounding is monotone); NaN and overflow end up in the clamped range
    const double q = floor(((double)x - (double)lo) / cell);
    return (uint64_t)fmin(fmax(q, 0.0), (double)CELL_MAX);
}

// pcell[i] = cx << 32 | cy << 16 | cz
__global__ __launch_bounds__(256) void cell_kernel(int64_t n, const float *__restrict__ xyz, const unsigned *__restrict__ bbox,
                                                   double cell, uint64_t *__restrict__ pcell)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t cx = cell_coord(xyz[i * 3 + 0], gags_key2f(bbox[0]), cell);
    const uint64_t cy = cell_coord(xyz[i * 3 + 1], gags_key2f(bbox[1]), cell);
    const uint64_t cz = cell_coord(xyz[i * 3 + 2], gags_key2f(bbox[2]), cell);
    pcell[i] = (cx << (2 * CELL_BITS)) | (cy << CELL_BITS) | cz;
}

// key[k n + i] = k << 48 | pcell[i] for a masked point, the sentinel n_masks << 48 otherwise
__global__ __launch_bounds__(256) void cand_key_kernel(int64_t n, int n_masks, const unsigned char *__restrict__ mask,
                                                       const uint64_t *__restrict__ pcell, uint64_t *__restrict__ keys)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n_masks * n) return;
    const int64_t k = t / n, i = t - k * n;
    keys[t] = mask[t] ? (((uint64_t)k << PHRASE_SHIFT) | pcell[i]) : ((uint64_t)n_masks << PHRASE_SHIFT);
}

// the candidates' coordinates in sorted order (sentinel entries are never read: no scan range reaches them)
__global__ __launch_bounds__(256) void cand_gather_kernel(int64_t n, int n_masks, const uint64_t *__restrict__ keys,
                                                          const int32_t *__restrict__ src, const float *__restrict__ xyz,
                                                          float *__restrict__ cxyz)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)n_masks * n || (keys[t] >> PHRASE_SHIFT) >= (uint64_t)n_masks) return;
    const int64_t s = src[t];
    const int64_t i = s - (s / n) * n;
    cxyz[t * 3 + 0] = xyz[i * 3 + 0];
    cxyz[t * 3 + 1] = xyz[i * 3 + 1];
    cxyz[t * 3 + 2] = xyz[i * 3 + 2];
}

// first position in keys[lo, hi) whose key is >= v (hi if none); every probe is inside [lo, hi)
__device__ __forceinline__ int64_t lower_bound(const uint64_t *__restrict__ keys, int64_t lo, int64_t hi, uint64_t v)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void vote_kernel(int64_t n, int n_masks, const float *__restrict__ xyz,
                                                   const unsigned char *__restrict__ mask, const uint64_t *__restrict__ qcell,
                                                   const int32_t *__restrict__ qorder, const uint64_t *__restrict__ ckeys,
                                                   const float *__restrict__ cxyz, double r2, int threshold, int cap,
                                                   unsigned char *__restrict__ out, int32_t *__restrict__ counts)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n_keys = (int64_t)n_masks * n;
    if (t >= n_keys) return;
    const int64_t k = t / n, j = t - k * n;
    const int64_t i = qorder[j];
    const uint64_t cell = qcell[j];
    const int cx = (int)((cell >> (2 * CELL_BITS)) & CELL_MAX), cy = (int)((cell >> CELL_BITS) & CELL_MAX),
              cz = (int)(cell & CELL_MAX);
    const double px = xyz[i * 3 + 0], py = xyz[i * 3 + 1], pz = xyz[i * 3 + 2];
    const uint64_t zlo = (uint64_t)max(cz - 1, 0), zhi = (uint64_t)min(cz + 1, (int)CELL_MAX);
    int c = 0;
    for (int x = max(cx - 1, 0); x <= min(cx + 1, (int)CELL_MAX) && c < cap; ++x)
        for (int y = max(cy - 1, 0); y <= min(cy + 1, (int)CELL_MAX) && c < cap; ++y) {
            // cells (x, y, zlo .. zhi) are consecutive keys: one range
            const uint64_t base = ((uint64_t)k << PHRASE_SHIFT) | ((uint64_t)x << (2 * CELL_BITS)) | ((uint64_t)y << CELL_BITS);
            const int64_t lo = lower_bound(ckeys, 0, n_keys, base | zlo);
            const int64_t hi = lower_bound(ckeys, lo, n_keys, (base | zhi) + 1);
            for (int64_t p = lo; p < hi && c < cap; ++p) {
                const double dx = px - (double)cxyz[p * 3 + 0];
                const double dy = py - (double)cxyz[p * 3 + 1];
                const double dz = pz - (double)cxyz[p * 3 + 2];
                const double d2 = (dx * dx + dy * dy) + dz * dz;
                c += d2 <= r2 ? 1 : 0;
            }
        }
    const int64_t o = k * n + i;
    out[o] = ((int64_t)c > (int64_t)threshold || (mask[o] && c >= 10)) ? 1 : 0;
    if (counts) counts[o] = c;
}

inline unsigned grid_stride_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 2048); }

struct SmoothScratch {
    unsigned *bbox;
    uint64_t *pcell, *ckeys_in, *ckeys, *qcell;
    int32_t *csrc, *qorder;
    float *cxyz;
    void *sort;
    int64_t sort_bytes, total;
};

// (base NULL: sizes only)
SmoothScratch smooth_carve(void *base, int n_masks, int64_t n)
{
    const int64_t nk = (int64_t)n_masks * n;
    GagsCarve c(base);
    SmoothScratch L;
    L.bbox = c.take<unsigned>(3);
    L.pcell = c.take<uint64_t>(n);
    L.ckeys_in = c.take<uint64_t>(nk);
    L.ckeys = c.take<uint64_t>(nk);
    L.csrc = c.take<int32_t>(nk);
    L.cxyz = c.take<float>(nk * 3);
    L.qcell = c.take<uint64_t>(n);
    L.qorder = c.take<int32_t>(n);
    L.sort = c.take_bytes(gags_sort_u64_scratch_bytes(std::max(nk, n)));
    L.sort_bytes = c.last();
    L.total = c.total();
    return L;
}

}  // namespace

extern "C" int64_t gags_point_relevancy_mask_scratch_bytes(int n_phrases, int64_t n)
{
    if (n_phrases <= 0 || n <= 0) return 0;
    return al256((int64_t)n_phrases * 2 * 4);
}

extern "C" int gags_point_relevancy_mask(int n_phrases, int64_t n, const float *probs, float rel_thresh, float *normalized,
                                         unsigned char *mask, void *scratch, int64_t scratch_bytes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_phrases < 0 || n < 0 || n_phrases > 65535) return GAGS_EINVAL;
    if (n_phrases == 0 || n == 0) return GAGS_OK;
    if (!probs || !normalized || !mask || !scratch) return GAGS_EINVAL;
    if (scratch_bytes < gags_point_relevancy_mask_scratch_bytes(n_phrases, n)) return GAGS_ESCRATCH;
    hipStream_t st = (hipStream_t)stream;
    unsigned *keys = (unsigned *)scratch;
    const dim3 grid(grid_stride_blocks(n), n_phrases);
    hipLaunchKernelGGL(minmax_init_kernel, dim3((2 * n_phrases + 63) / 64), dim3(64), 0, st, 2 * n_phrases, keys);
    hipLaunchKernelGGL(rel_minmax_kernel, grid, dim3(256), 0, st, n, probs, keys);
    hipLaunchKernelGGL(rel_normalise_kernel, grid, dim3(256), 0, st, n, rel_thresh, probs, keys, normalized, mask);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

extern "C" int64_t gags_point_mask_smooth_scratch_bytes(int n_masks, int64_t n)
{
    if (n_masks <= 0 || n <= 0 || n_masks > MAX_MASKS || (int64_t)n_masks * n >= (1ll << 31)) return 0;
    return smooth_carve(nullptr, n_masks, n).total;
}

extern "C" int gags_point_mask_smooth(int n_masks, int64_t n, const float *xyz, const unsigned char *mask, double radius,
                                      int threshold, unsigned char *out, int32_t *counts, void *scratch, int64_t scratch_bytes,
                                      void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_masks < 0 || n < 0 || n_masks > MAX_MASKS || threshold < 0) return GAGS_EINVAL;
    if (!(radius > 0.0) || !std::isfinite(radius)) return GAGS_EINVAL;
    if (n_masks == 0 || n == 0) return GAGS_OK;
    const int64_t nk = (int64_t)n_masks * n;
    if (nk >= (1ll << 31)) return GAGS_EINVAL;  // the radix sort's limit (and int32 source positions)
    if (!xyz || !mask || !out || !scratch) return GAGS_EINVAL;
    const SmoothScratch L = smooth_carve(scratch, n_masks, n);
    if (scratch_bytes < L.total) return GAGS_ESCRATCH;
    hipStream_t st = (hipStream_t)stream;
    unsigned *bbox = L.bbox;
    uint64_t *pcell = L.pcell, *ckeys_in = L.ckeys_in, *ckeys = L.ckeys, *qcell = L.qcell;
    int32_t *csrc = L.csrc, *qorder = L.qorder;
    float *cxyz = L.cxyz;
    void *sort_scratch = L.sort;
    const int64_t sort_bytes = L.sort_bytes;

    const double cell = radius * (1.0 + 0x1p-20);
    const int64_t cap = std::max<int64_t>((int64_t)threshold + 1, 10);  // counts past cap change nothing
    const int cap_i = (int)std::min<int64_t>(cap, INT32_MAX);            // (a count never exceeds n < 2^31)
    int phrase_bits = 0;                                                 // phrases 0 .. n_masks - 1 and the sentinel n_masks
    while ((1ll << phrase_bits) <= n_masks) ++phrase_bits;

    hipLaunchKernelGGL(bbox_init_kernel, dim3(1), dim3(64), 0, st, bbox);
    hipLaunchKernelGGL(bbox_kernel, dim3(grid_stride_blocks(n), 3), dim3(256), 0, st, n, xyz, bbox);
    const unsigned nb = (unsigned)((n + 255) / 256), nkb = (unsigned)((nk + 255) / 256);
    hipLaunchKernelGGL(cell_kernel, dim3(nb), dim3(256), 0, st, n, xyz, bbox, cell, pcell);
    hipLaunchKernelGGL(cand_key_kernel, dim3(nkb), dim3(256), 0, st, n, n_masks, mask, pcell, ckeys_in);
    GAGS_CHECK_LAUNCH();
    // queries in cell order (argsort of the N cell keys), candidates by (phrase, cell)
    int rc = gags_sort_pairs_u64(n, 0, PHRASE_SHIFT, pcell, nullptr, qcell, qorder, sort_scratch, sort_bytes, st);
    if (rc != GAGS_OK) return rc;
    rc = gags_sort_pairs_u64(nk, 0, PHRASE_SHIFT + phrase_bits, ckeys_in, nullptr, ckeys, csrc, sort_scratch, sort_bytes, st);
    if (rc != GAGS_OK) return rc;
    hipLaunchKernelGGL(cand_gather_kernel, dim3(nkb), dim3(256), 0, st, n, n_masks, ckeys, csrc, xyz, cxyz);
    hipLaunchKernelGGL(vote_kernel, dim3(nkb), dim3(256), 0, st, n, n_masks, xyz, mask, qcell, qorder, ckeys, cxyz,
                       radius * radius, threshold, cap_i, out, counts);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
