// Rows -> Gaussians: the tail the two staged backward drivers share (colours: raster_bwd_rows.hip, rows of D channels;
// wide-D geometry: raster_bwd_geom.hip, rows of 8).  Their kernels leave partial gradient rows at fixed addresses plus a
// (Gaussian id, row) pair per row; here the pairs are sorted by Gaussian (radix sort on 32-bit keys, sort.hip), the
// per-Gaussian offsets are found, and every Gaussian's rows are summed in sorted order and written once: no atomics,
// bit-reproducible.
#include <hip/hip_fp16.h>
#include "launch.h"

namespace {

// capacity-sized row buffers: keys [total, cap) become sentinels (key n_gauss: past every Gaussian), so that the sort and
// the segment offsets can run over the capacity without the host knowing the row count
__global__ __launch_bounds__(256) void row_tail_kernel(int64_t cap, const int32_t *__restrict__ total, int n_gauss,
                                                       uint32_t *__restrict__ row_key, int32_t *__restrict__ row_idx)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cap || i < (int64_t)total[0]) return;
    row_key[i] = (uint32_t)n_gauss;
    row_idx[i] = 0;
}

// seg[g] = first sorted position whose key is >= g, for g in [0, n_keys]
__global__ __launch_bounds__(256) void seg_offsets_kernel(int n, const uint32_t *__restrict__ sorted_keys, int n_keys,
                                                          int32_t *__restrict__ seg)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int cur = min((int)sorted_keys[i], n_keys);
    if (i == 0) {
        for (int g = 0; g <= cur; ++g) seg[g] = 0;
    } else {
        const int prev = min((int)sorted_keys[i - 1], n_keys);
        for (int g = prev + 1; g <= cur; ++g) seg[g] = i;
    }
    if (i == n - 1)
        for (int g = cur + 1; g <= n_keys; ++g) seg[g] = n;
}

__global__ void seg_fill_kernel(int n_keys, int32_t *__restrict__ seg)
{
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g <= n_keys) seg[g] = 0;
}

// v_colors[g, :] = sum over the Gaussian's rows, in sorted (= deterministic) order; VW channels per lane (4: one float4;
// 1: the 1-3 channels a width that is no multiple of 4 leaves over, e.g. the 513th).
// HALF: the sum (formed in fp32) is stored as fp16 -- the gradient of an fp16 feature table in the table's own dtype,
// instead of an fp32 tensor plus a cast pass over it (N x D x 6 bytes of traffic at C5).
constexpr int REDUCE_ITER = 8;
template <bool HALF, int VW>
__global__ __launch_bounds__(256) void reduce_rows_kernel(int n_gauss, int d, int ch_begin, int ch_count,
                                                          const int32_t *__restrict__ seg,
                                                          const int32_t *__restrict__ sorted_rows,
                                                          const float *__restrict__ prow, int prow_pitch,
                                                          void *__restrict__ v_colors_, int sparse,
                                                          const int32_t *__restrict__ wire_pos, float *__restrict__ wire,
                                                          const uint8_t *__restrict__ keep_prev, uint8_t *__restrict__ keep_cur,
                                                          int tail)
{
    // tail (VW == 4 only): the 1-3 channels an odd width leaves behind its float4 columns (the 513th of BASELINE.json configs[4])
    // ride along -- lane t < tail of a Gaussian's group also sums channel ch_begin + ch_count + t -- instead of a second launch
    // with one lane per Gaussian walking the same row lists again (0.22 ms at C5).
    // keep (round 6): v_colors is a PERSISTENT buffer of the caller's whose rows are zero except those the previous backward
    // wrote (keep_prev[g] != 0).  This launch writes the rows that have partial rows now, re-zeroes the rows that had some
    // last time and have none now, leaves every other row alone -- 73 % of the Gaussians blend nothing at C3: 2.2 GB of zero
    // rows per step are not written -- and records keep_cur[g] for the next step (two arrays, swapped by the caller: the lanes
    // of a Gaussian span two waves, a flag cleared in place could be read after it was cleared).
    // wire (by-view multi-GPU step, gags_amd/dist.py): the rows the ranks exchange -- wire_pos[g] >= 0: row wire_pos[g] of the
    // dense [rows, ch_count] fp32 block -- leave from here, next to the gradient itself, instead of being re-read by a pack
    // kernel (a union row this view did not touch gets its zeros here as well: every row of the block is written)
    // (REDUCE_ITER groups of Gaussians per workgroup, one after the other: three of four Gaussians have no rows at C3 -- as one
    // workgroup per group those were 550 k empty workgroups for the dispatcher)
    const int lpg = ch_count / VW;  // lanes per Gaussian (channels ch_begin .. ch_begin + ch_count - 1 of its row)
    const int gpb = 256 / lpg;
    const int gl = threadIdx.x / lpg;
    const int cl = ch_begin + (threadIdx.x % lpg) * VW;
    if (gl >= gpb) return;
    for (int it = 0; it < REDUCE_ITER; ++it) {
    const int g = (blockIdx.x * REDUCE_ITER + it) * gpb + gl;
    if (g >= n_gauss) return;
        const int b = seg[g], e = seg[g + 1];
        // sparse: the caller zero-filled v_colors (on a second stream, under the rows kernel): a Gaussian without rows -- 73 % of
        // them at C3 -- costs nothing here instead of a 4 D-byte row of zeros
        const bool has = b != e;
        bool write_grad = sparse ? has : true;
        const bool on_wire = wire && wire_pos[g] >= 0;
        if (keep_cur) {
            // (a row of the exchanged block will be written by the caller once the ranks' sum is known: it counts as written)
            if (threadIdx.x % lpg == 0) keep_cur[g] = (has || on_wire) ? 1 : 0;
            write_grad = has || keep_prev[g] != 0;
        }
        if (!write_grad && !on_wire) continue;
        const bool skip_grad = !write_grad;  // (only its wire row is due)
        if constexpr (VW == 1) {
            float acc = 0.f;
            for (int i = b; i < e; ++i) acc += prow[(size_t)sorted_rows[i] * prow_pitch + cl];
            if (!skip_grad) {
                if constexpr (HALF) reinterpret_cast<__half *>(v_colors_)[(size_t)g * d + cl] = __float2half_rn(acc);
                else reinterpret_cast<float *>(v_colors_)[(size_t)g * d + cl] = acc;
            }
            if (wire) {
                const int q = wire_pos[g];
                if (q >= 0) wire[(size_t)q * ch_count + (cl - ch_begin)] = acc;
            }
        } else {
            float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
            const int tl = threadIdx.x % lpg;
            const bool has_tail = tl < tail;
            const int ct = ch_begin + ch_count + (has_tail ? tl : 0);  // this lane's tail channel (same order of additions as the body)
            float acc_t = 0.f;
            // Batches of eight rows, every load of a batch requested before the first is added: the row numbers (clamped to the
            // Gaussian's last row: valid addresses, their values unused), then the rows.  A Gaussian has 4.7 rows on average at
            // C3 -- two round trips instead of one per group of four plus one per leftover row.  Same order of additions.
            for (int i = b; i < e; i += 8) {
                int r[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) r[j] = sorted_rows[min(i + j, e - 1)];
                float4 v[8];
                float vt[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    v[j] = *reinterpret_cast<const float4 *>(prow + (size_t)r[j] * prow_pitch + cl);
                    vt[j] = has_tail ? prow[(size_t)r[j] * prow_pitch + ct] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (i + j < e) {
                        acc.x += v[j].x; acc.y += v[j].y; acc.z += v[j].z; acc.w += v[j].w;
                        acc_t += vt[j];
                    }
                }
            }
            if (!skip_grad && has_tail) {
                if constexpr (HALF) reinterpret_cast<__half *>(v_colors_)[(size_t)g * d + ct] = __float2half_rn(acc_t);
                else reinterpret_cast<float *>(v_colors_)[(size_t)g * d + ct] = acc_t;
            }
            if (!skip_grad) {
                if constexpr (HALF) {
                    const __half2 lo = __floats2half2_rn(acc.x, acc.y), hi = __floats2half2_rn(acc.z, acc.w);
                    uint2 w;
                    w.x = *reinterpret_cast<const unsigned *>(&lo);
                    w.y = *reinterpret_cast<const unsigned *>(&hi);
                    *reinterpret_cast<uint2 *>(reinterpret_cast<__half *>(v_colors_) + (size_t)g * d + cl) = w;
                } else {
                    typedef float nt_f4 __attribute__((ext_vector_type(4)));
                    __builtin_nontemporal_store(nt_f4{acc.x, acc.y, acc.z, acc.w},
                                                reinterpret_cast<nt_f4 *>(reinterpret_cast<float *>(v_colors_) + (size_t)g * d + cl));
                }
            }
            if (wire) {
                const int q = wire_pos[g];
                if (q >= 0) *reinterpret_cast<float4 *>(wire + (size_t)q * ch_count + (cl - ch_begin)) = acc;
            }
        }
    }
}

}  // namespace

int gags_rows_group_launch(int64_t rows, int n_gauss, const int32_t *rows_dev, uint32_t *key, int32_t *idx, uint32_t *key_s,
                           int32_t *idx_s, int32_t *seg, void *sort_scratch, int64_t sort_scratch_bytes, hipStream_t st)
{
    if (rows <= 0) {
        hipLaunchKernelGGL(seg_fill_kernel, dim3((n_gauss + 1 + 255) / 256), dim3(256), 0, st, n_gauss, seg);
        return GAGS_OK;
    }
    const dim3 grid((unsigned)((rows + 255) / 256));
    // rows is a CAPACITY when rows_dev is given (the true count lives on the device): sentinel keys past it
    if (rows_dev) hipLaunchKernelGGL(row_tail_kernel, grid, dim3(256), 0, st, rows, rows_dev, n_gauss, key, idx);
    int nbits = 1;
    while ((1ll << nbits) <= n_gauss) ++nbits;  // keys in [0, n_gauss]
    const int rc = gags_sort_pairs_u32(rows, nbits, key, idx, key_s, idx_s, sort_scratch, sort_scratch_bytes, st);
    if (rc != GAGS_OK) return rc;
    hipLaunchKernelGGL(seg_offsets_kernel, grid, dim3(256), 0, st, (int)rows, key_s, n_gauss, seg);
    return GAGS_OK;
}

int gags_rows_reduce_launch(int n_gauss, int d, int ch_begin, int ch_count, const int32_t *seg, const int32_t *idx_s,
                            const float *prow, int pitch, void *out, bool out_f16, hipStream_t st, int sparse,
                            const int32_t *wire_pos, float *wire, const uint8_t *keep_prev, uint8_t *keep_cur)
{
    const int c4 = ch_count & ~3, c1 = ch_count & 3;  // float4 lanes + the 1-3 channels an odd width leaves over
    if (wire && (c1 != 0 || !wire_pos)) return GAGS_EINVAL;  // the wire block is [rows, ch_count], ch_count % 4 == 0
    const bool ride = c4 >= 16 && c1 > 0;  // the 1-3 leftover channels ride along with the float4 columns' launch
    // one launch of the reduce kernel over channels [c0, c0 + cw), cw / vw lanes per Gaussian: the fp16- or the fp32-output instantiation
    auto reduce = [&](auto *k_f16, auto *k_f32, int vw, int c0, int cw, int tail) {
        const int gpb = 256 / (cw / vw);
        const dim3 grid((n_gauss + gpb * REDUCE_ITER - 1) / (gpb * REDUCE_ITER));
        hipLaunchKernelGGL(out_f16 ? k_f16 : k_f32, grid, dim3(256), 0, st, n_gauss, d, c0, cw, seg, idx_s, prow, pitch, out, sparse,
                           wire_pos, wire, keep_prev, keep_cur, tail);
    };
    if (c4 > 0) reduce((reduce_rows_kernel<true, 4>), (reduce_rows_kernel<false, 4>), 4, ch_begin, c4, ride ? c1 : 0);
    if (c1 > 0 && !ride) reduce((reduce_rows_kernel<true, 1>), (reduce_rows_kernel<false, 1>), 1, ch_begin + c4, c1, 0);
    return GAGS_OK;
}
