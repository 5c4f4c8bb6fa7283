// N9 (include/gags_next.h): each point's mean squared distance to its three nearest neighbours -- simple_knn's distCUDA2,
// the one non-trivial operation of GaussianModel.create_from_pcd (scene/gaussian_model.py:151-180; the initial log-scale).
//
// Contract (the header states it; tests/knn_ref.py restates it): for point i over all j != i (by index),
//   d2_ij = (dx*dx + dy*dy) + dz*dz,  dx = x_j - x_i ...,  float32, no FMA;  b0 <= b1 <= b2 the three smallest VALUES;
//   dist2[i] = ((b0 + b1) + b2) / 3.0f, written in input order.
// The multiset of the three smallest values does not depend on the order the candidates are visited in, so any exact
// traversal gives the same bits as a float32 brute force.
//
// Traversal: bounding box -> 30-bit Morton keys (10 bits per axis) -> radix sort (csrc/sort.hip) -> the coordinates gathered
// into sorted order as float4 (w = the original index) -> boxes of KNN_BOX consecutive sorted points, each with its float32
// AABB -> one thread per point in SORTED order (the 64 lanes of a wave are spatial neighbours): the best three are seeded
// from the +-3 sorted neighbours, then the wave walks the boxes.  The walk is wave-uniform: a box is opened when any lane's
// lower bound is <= its current third-best, and then every lane reads the box's points through the same address (a
// broadcast: scalar loads).  Results scatter to dist2[orig]; no atomics on the output.
//
// Why the pruning is exact IN FLOAT32.  The bound is computed by the expression and association of d2 itself: per axis
// a = max(lo - q, 0, q - hi), then (ax*ax + ay*ay) + az*az.  For a point p of the box, lo <= p <= hi on every axis, so
// a <= |p - q| in real arithmetic (a = 0 when q is inside the slab).  Round-to-nearest float32 subtraction is monotone and
// sign-symmetric, hence fl(lo - q) <= fl(p - q) = |fl(q - p)| when q < lo (likewise above hi): a <= |dx| as FLOATS.
// Squaring a non-negative float and adding floats are monotone under round-to-nearest too, so bound <= d2(p, q) as floats,
// for every p in the box.  A box is rejected only when bound > b2 (strictly): every point in it has d2 > b2, and a value
// greater than the current third-best cannot be one of the three smallest.  Ties (bound == b2) open the box.
#include <algorithm>
#include <cmath>
#include "launch.h"
#include "gags_next.h"
#include "reduce.h"

namespace {

constexpr int KNN_BOX = 256;       // sorted points per box = threads per query workgroup (gags_amd/knn.py: BOX)
constexpr int KNN_SEED = 3;        // the best three start from sorted neighbours s - 3 .. s + 3
constexpr int KNN_CELL_MAX = 1023;  // 10 bits per axis

// bbox[0..2] = keys of the minima, bbox[3..5] = keys of the maxima
__global__ void knn_bbox_init_kernel(unsigned *__restrict__ bbox)
{
    if (threadIdx.x < 6) bbox[threadIdx.x] = threadIdx.x < 3 ? 0xffffffffu : 0u;
}

__global__ __launch_bounds__(256) void knn_bbox_kernel(int64_t n, const float *__restrict__ xyz, unsigned *__restrict__ bbox)
{
    __shared__ unsigned red[2][4];
    const int a = blockIdx.y;
    unsigned kmin = 0xffffffffu, kmax = 0u;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const unsigned u = gags_f2key(xyz[i * 3 + a]);
        kmin = min(kmin, u);
        kmax = max(kmax, u);
    }
    // (gags_block_minmax's tree, inline: with the two destinations formed at a call the compiler schedules this kernel differently)
    for (int off = 32; off > 0; off >>= 1) {
        kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, off, 64));
        kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = kmin; red[1][threadIdx.x >> 6] = kmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(bbox + a, min(min(red[0][0], red[0][1]), min(red[0][2], red[0][3])));
        atomicMax(bbox + 3 + a, max(max(red[1][0], red[1][1]), max(red[1][2], red[1][3])));
    }
}

// cell of x on an axis [lo, hi]: 0 on an axis of zero (or non-finite) extent -- no division by zero -- and CLAMPED: a NaN,
// an infinity or a rounding past the last cell all end inside 0 .. KNN_CELL_MAX (fmaxf / fminf drop a NaN operand)
__device__ __forceinline__ unsigned knn_cell(float x, float lo, float hi)
{
    const float ext = hi - lo;
    if (!(ext > 0.f) || !(ext < INFINITY)) return 0u;
    const float q = (x - lo) / ext * (float)(KNN_CELL_MAX + 1);
    return (unsigned)fminf(fmaxf(q, 0.f), (float)KNN_CELL_MAX);
}

// 10 bits -> every third bit
__device__ __forceinline__ unsigned knn_spread(unsigned v)
{
    v &= 0x3ffu;
    v = (v | (v << 16)) & 0x030000ffu;
    v = (v | (v << 8)) & 0x0300f00fu;
    v = (v | (v << 4)) & 0x030c30c3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

__global__ __launch_bounds__(256) void knn_key_kernel(int64_t n, const float *__restrict__ xyz, const unsigned *__restrict__ bbox,
                                                      uint32_t *__restrict__ keys)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const unsigned cx = knn_cell(xyz[i * 3 + 0], gags_key2f(bbox[0]), gags_key2f(bbox[3]));
    const unsigned cy = knn_cell(xyz[i * 3 + 1], gags_key2f(bbox[1]), gags_key2f(bbox[4]));
    const unsigned cz = knn_cell(xyz[i * 3 + 2], gags_key2f(bbox[2]), gags_key2f(bbox[5]));
    keys[i] = (knn_spread(cx) << 2) | (knn_spread(cy) << 1) | knn_spread(cz);
}

// pts[s] = (xyz[order[s]], bits of order[s]); order is the sort's own permutation of 0 .. n - 1
__global__ __launch_bounds__(256) void knn_gather_kernel(int64_t n, const float *__restrict__ xyz, const int32_t *__restrict__ order,
                                                         float4 *__restrict__ pts)
{
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s >= n) return;
    const int32_t o = order[s];
    const int64_t i = o;
    pts[s] = make_float4(xyz[i * 3 + 0], xyz[i * 3 + 1], xyz[i * 3 + 2], __int_as_float(o));
}

// aabb[2 b] = the minima, aabb[2 b + 1] = the maxima of sorted points [b KNN_BOX, min(n, (b + 1) KNN_BOX)); one workgroup per box
__global__ __launch_bounds__(KNN_BOX) void knn_box_kernel(int64_t n, const float4 *__restrict__ pts, float4 *__restrict__ aabb)
{
    __shared__ float red[6][KNN_BOX / 64];
    const int64_t s = (int64_t)blockIdx.x * KNN_BOX + threadIdx.x;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (s < n) {
        const float4 p = pts[s];
        lo[0] = hi[0] = p.x;
        lo[1] = hi[1] = p.y;
        lo[2] = hi[2] = p.z;
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int a = 0; a < 3; ++a) {
            lo[a] = fminf(lo[a], __shfl_xor(lo[a], off, 64));
            hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], off, 64));
        }
    if ((threadIdx.x & 63) == 0)
        for (int a = 0; a < 3; ++a) {
            red[a][threadIdx.x >> 6] = lo[a];
            red[3 + a][threadIdx.x >> 6] = hi[a];
        }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < KNN_BOX / 64; ++w)
            for (int a = 0; a < 3; ++a) {
                red[a][0] = fminf(red[a][0], red[a][w]);
                red[3 + a][0] = fmaxf(red[3 + a][0], red[3 + a][w]);
            }
        aabb[2 * (int64_t)blockIdx.x] = make_float4(red[0][0], red[1][0], red[2][0], 0.f);
        aabb[2 * (int64_t)blockIdx.x + 1] = make_float4(red[3][0], red[4][0], red[5][0], 0.f);
    }
}

// the contract's distance: (dx*dx + dy*dy) + dz*dz with dx = x_j - x_i (the build has -ffp-contract=off)
__device__ __forceinline__ float knn_d2(const float4 &pj, float qx, float qy, float qz)
{
    const float dx = pj.x - qx, dy = pj.y - qy, dz = pj.z - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// d into the sorted triple b0 <= b1 <= b2 (the caller has tested d < b2)
__device__ __forceinline__ void knn_insert(float d, float &b0, float &b1, float &b2)
{
    const float t1 = fmaxf(b0, d);
    b0 = fminf(b0, d);
    b2 = fmaxf(b1, t1);  // (<= the old b2, since d < b2)
    b1 = fminf(b1, t1);
}

__global__ __launch_bounds__(KNN_BOX) void knn_query_kernel(int n, int n_boxes, const float4 *__restrict__ pts,
                                                            const float4 *__restrict__ aabb, float *__restrict__ dist2)
{
    const int64_t s64 = (int64_t)blockIdx.x * KNN_BOX + threadIdx.x;
    const bool valid = s64 < (int64_t)n;
    const int s = valid ? (int)s64 : n - 1;  // (a lane past the end follows the walk with the last point and writes nothing)
    const float4 q = pts[s];
    float b0 = INFINITY, b1 = INFINITY, b2 = INFINITY;
    // seed: n >= 4 puts at least three other points inside the window
#pragma unroll
    for (int k = -KNN_SEED; k <= KNN_SEED; ++k) {
        const int64_t j = (int64_t)s + k;
        if (k != 0 && j >= 0 && j < (int64_t)n) {
            const float d = knn_d2(pts[j], q.x, q.y, q.z);
            if (d < b2) knn_insert(d, b0, b1, b2);
        }
    }
    for (int bx = 0; bx < n_boxes; ++bx) {
        const float4 lo = aabb[2 * (int64_t)bx], hi = aabb[2 * (int64_t)bx + 1];
        // the lower bound, in d2's own expression and association (exactness argument: the head of this file)
        const float ax = fmaxf(fmaxf(lo.x - q.x, 0.f), q.x - hi.x);
        const float ay = fmaxf(fmaxf(lo.y - q.y, 0.f), q.y - hi.y);
        const float az = fmaxf(fmaxf(lo.z - q.z, 0.f), q.z - hi.z);
        const float bound = (ax * ax + ay * ay) + az * az;
        // !(bound > b2), not bound <= b2: a NaN bound opens the box instead of pruning it
        if (!__any((valid && !(bound > b2)) ? 1 : 0)) continue;
        const int j0 = bx * KNN_BOX, j1 = j0 + min(n - j0, KNN_BOX);  // (j0 < n < 2^31; no j0 + KNN_BOX, which may not fit)
#pragma unroll 4
        for (int j = j0; j < j1; ++j) {
            const float d = knn_d2(pts[j], q.x, q.y, q.z);
            // the seed window (the point itself in its middle) was counted already
            if ((unsigned)j - (unsigned)s + (unsigned)KNN_SEED > 2u * KNN_SEED && d < b2) knn_insert(d, b0, b1, b2);
        }
    }
    if (valid) {
        const int orig = __float_as_int(q.w);
        if (orig >= 0 && orig < n) dist2[orig] = ((b0 + b1) + b2) / 3.0f;
    }
}

inline unsigned grid_stride_blocks(int64_t n) { return (unsigned)std::min<int64_t>((n + 255) / 256, 2048); }

struct KnnScratch {
    unsigned *bbox;
    uint32_t *keys_in, *keys;
    int32_t *order;
    float4 *pts, *aabb;
    void *sort;
    int64_t sort_bytes, total;
};

// (base NULL: sizes only)
KnnScratch knn_carve(void *base, int64_t n)
{
    const int64_t n_boxes = (n + KNN_BOX - 1) / KNN_BOX;
    GagsCarve c(base);
    KnnScratch L;
    L.bbox = c.take<unsigned>(6);
    L.keys_in = c.take<uint32_t>(n);
    L.keys = c.take<uint32_t>(n);
    L.order = c.take<int32_t>(n);
    L.pts = c.take<float4>(n);
    L.aabb = c.take<float4>(n_boxes * 2);
    L.sort = c.take_bytes(gags_sort_u32_scratch_bytes(n));
    L.sort_bytes = c.last();
    L.total = c.total();
    return L;
}

inline bool knn_count_ok(int64_t n) { return n >= 4 && n < (1ll << 31); }

}  // namespace

extern "C" int64_t gags_knn3_dist2_scratch_bytes(int64_t n)
{
    if (!knn_count_ok(n)) return 0;
    return knn_carve(nullptr, n).total;
}

extern "C" int gags_knn3_dist2(int64_t n, const float *xyz, float *dist2, void *scratch, int64_t scratch_bytes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (!knn_count_ok(n)) return GAGS_EINVAL;  // fewer than three neighbours (the reference's infinite scale), or past int32 positions
    if (!xyz || !dist2 || !scratch) return GAGS_EINVAL;
    const KnnScratch L = knn_carve(scratch, n);
    if (scratch_bytes < L.total) return GAGS_ESCRATCH;
    hipStream_t st = (hipStream_t)stream;
    unsigned *bbox = L.bbox;
    uint32_t *keys_in = L.keys_in, *keys = L.keys;
    int32_t *order = L.order;
    float4 *pts = L.pts, *aabb = L.aabb;
    const unsigned nb = (unsigned)((n + 255) / 256), n_boxes = (unsigned)((n + KNN_BOX - 1) / KNN_BOX);

    hipLaunchKernelGGL(knn_bbox_init_kernel, dim3(1), dim3(64), 0, st, bbox);
    hipLaunchKernelGGL(knn_bbox_kernel, dim3(grid_stride_blocks(n), 3), dim3(256), 0, st, n, xyz, bbox);
    hipLaunchKernelGGL(knn_key_kernel, dim3(nb), dim3(256), 0, st, n, xyz, bbox, keys_in);
    GAGS_CHECK_LAUNCH();
    const int rc = gags_sort_pairs_u32(n, 30, keys_in, nullptr, keys, order, L.sort, L.sort_bytes, st);  // (argsort)
    if (rc != GAGS_OK) return rc;
    hipLaunchKernelGGL(knn_gather_kernel, dim3(nb), dim3(256), 0, st, n, xyz, order, pts);
    hipLaunchKernelGGL(knn_box_kernel, dim3(n_boxes), dim3(KNN_BOX), 0, st, n, pts, aabb);
    hipLaunchKernelGGL(knn_query_kernel, dim3(n_boxes), dim3(KNN_BOX), 0, st, (int)n, (int)n_boxes, pts, aabb, dist2);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
