// Internal header of libgags_hip.so: every host function that one translation unit defines and another calls is declared
// here, ONCE; the file that defines it and the files that call it include this header, so a signature that drifts is a
// compile error instead of a silently different call.  Also the few host-side helpers several drivers had private copies of.
// (The C ABI itself is include/*.h; nothing here is exported.)
#pragma once
#include "common.h"

// ---- host helpers -----------------------------------------------------------------------------------------------------
// scratch regions start on 256-byte boundaries
inline int64_t al256(int64_t x) { return (x + 255) / 256 * 256; }

// A scratch layout, written once: a cursor that hands out the regions of a buffer in order and adds up what they take.
// A driver's layout function carves with the caller's buffer as `base` and its *_scratch_bytes export with NULL, which only
// counts (offsets are integers; a pointer is formed from a real base alone).  `base` is const so that an entry which only
// reads an earlier call's scratch can carve it too.
class GagsCarve {
    char *base_;
    int64_t off_ = 0, last_ = 0;

public:
    explicit GagsCarve(const void *base) : base_((char *)base) {}
    void *take_bytes(int64_t bytes)
    {
        void *p = base_ ? base_ + off_ : nullptr;
        off_ += last_ = al256(bytes);
        return p;
    }
    template <class T>
    T *take(int64_t count) { return (T *)take_bytes(count * (int64_t)sizeof(T)); }
    int64_t last() const { return last_; }   // bytes of the region taken last (a sub-scratch handed on to another driver)
    int64_t total() const { return off_; }
};

// the 16x16 tiles of a width x height image: tiles across, tiles down, tiles in all
struct GagsTiles {
    int w, h, n;
};
inline GagsTiles gags_tiles(int width, int height)
{
    const int w = (width + GAGS_TILE - 1) / GAGS_TILE, h = (height + GAGS_TILE - 1) / GAGS_TILE;
    return {w, h, w * h};
}

// Dynamic LDS above 64 KB is an opt-in per kernel -- and HIP keeps the attribute per DEVICE: raised once per (kernel, device).
// `raised` is the call site's own static array (one per group of kernels); a device number past it is raised on every call.
// false: the runtime refused.
constexpr int GAGS_MAX_DEVICES = 16;
template <int N>
inline bool gags_raise_dynamic_lds(bool (&raised)[GAGS_MAX_DEVICES], const void *const (&kernels)[N], int bytes)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0) return false;
    if (dev < GAGS_MAX_DEVICES && raised[dev]) return true;
    for (const void *k : kernels)
        if (hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess) return false;
    if (dev < GAGS_MAX_DEVICES) raised[dev] = true;
    return true;
}

// ---- sort.hip ---------------------------------------------------------------------------------------------------------
int64_t gags_sort_u32_scratch_bytes(int64_t n);
int gags_sort_pairs_u32(int64_t n, int nbits, const uint32_t *keys_in, const int32_t *vals_in, uint32_t *keys_out,
                        int32_t *vals_out, void *scratch, int64_t scratch_bytes, hipStream_t st);
int64_t gags_sort_u64_scratch_bytes(int64_t n);
int gags_sort_pairs_u64(int64_t n, int first_bit, int nbits, const uint64_t *keys_in, const int32_t *vals_in,
                        uint64_t *keys_out, int32_t *vals_out, void *scratch, int64_t scratch_bytes, hipStream_t st);

// ---- raster_valu.hip --------------------------------------------------------------------------------------------------
int gags_raster_fwd_valu(int d, int width, int height, const float *means2d, const float *conics,
                         const float *opacities, const float *colors, const float *backgrounds,
                         const int32_t *offsets, const int32_t *flat, int n_isects, float *out, float *alphas,
                         int32_t *last_ids, hipStream_t st);
int gags_raster_bwd_valu(int d, int width, int height, const float *means2d, const float *conics,
                         const float *opacities, const float *colors, const float *backgrounds,
                         const int32_t *offsets, const int32_t *flat, int n_isects, const float *alphas,
                         const int32_t *last_ids, const float *v_out, const float *v_alpha, float *v_colors,
                         float *v_opac, float *v_m2d, float *v_con, bool geom, hipStream_t st, float *v_m2d_abs = nullptr);

// ---- raster_weights.hip -----------------------------------------------------------------------------------------------
int gags_pack_isects_launch(int n, int n_isects, const int32_t *flat, const float *means2d, const float *conics,
                            const float *opacities, const int32_t *radii, void *grec, void *packed, hipStream_t st);
int gags_raster_weights_launch(int width, int height, int n_gauss, const void *packed, int by_gauss, const int32_t *offsets,
                               const int32_t *flat, int n_isects, float *wt, int32_t *gid_s, int32_t *sidx_s,
                               int32_t *hit, int32_t *blk_rows, float *Tbuf, float *alphas, int32_t *last_ids,
                               hipStream_t st, const float *colors16 = nullptr, const float *backgrounds = nullptr,
                               float *render_colors = nullptr);
int gags_list_need_launch(int width, int height, int n_gauss, const void *packed, int by_gauss, const int32_t *offsets,
                          const int32_t *flat, int n_isects, int32_t *need, hipStream_t st);
int gags_trim_offsets_launch(int n_tiles, const int32_t *cum, int32_t *off_new, hipStream_t st);
int gags_trim_gather_launch(int n_tiles, const int32_t *off_old, const int32_t *off_new, const int32_t *flat_in, int32_t *flat_out,
                            hipStream_t st);
int gags_trim_last_ids_launch(int width, int height, const int32_t *off_old, const int32_t *off_new, const float *alphas,
                              int32_t *last_ids, hipStream_t st);

// ---- raster_fwd_mfma.hip ----------------------------------------------------------------------------------------------
int gags_raster_fwd_feat_launch(int d, int width, int height, int n_gauss, const float *colors, int colors_f16, int exact,
                                const float *backgrounds, const int32_t *offsets, int n_isects,
                                const int32_t *blk_rows, const float *wt, const int32_t *gid_s, const float *Tbuf,
                                float *out, hipStream_t st);
int gags_raster_fwd_fused_launch(int d, int width, int height, const void *packed, const float *colors,
                                 const float *backgrounds, const int32_t *offsets, const int32_t *flat, int n_isects,
                                 float *out, float *alphas, int32_t *last_ids, int by_gauss, hipStream_t st);

// ---- raster_bwd_rows.hip: staged colours backward ---------------------------------------------------------------------
int64_t gags_bwd_staged_scratch_bytes_impl(int64_t rows, int n_gauss, int d);
// 1 = width not eligible
int gags_raster_bwd_staged_launch(int d, int width, int height, int n_gauss, const int32_t *offsets, int n_isects,
                                  const float *v_out, const int32_t *blk_rows, const int32_t *trow, int64_t rows,
                                  const float *wt, const int32_t *gid_s, const int32_t *trow_s, void *scratch,
                                  int64_t scratch_bytes, float *v_colors, int stage_flags, int ch_begin, int ch_count,
                                  const int32_t *rows_dev, const int32_t *wire_pos, float *wire, const uint8_t *keep_prev,
                                  uint8_t *keep_cur, hipStream_t st);
int gags_bwd_slot_rows_launch(int width, int height, int n_isects, const int32_t *offsets, const int32_t *blk_rows,
                              const int32_t *sidx_s, const int32_t *trow, int32_t *trow_s, hipStream_t st);

// ---- rows_reduce.hip: partial rows -> per-Gaussian sums, the tail of both backward drivers ----------------------------
// Group `rows` (key = Gaussian, value = row number) pairs by Gaussian: key_s / idx_s = the pairs sorted by key, seg[g] = first
// sorted position of Gaussian g, for g in [0, n_gauss].  rows_dev given: `rows` is a capacity, the count lives on the device.
// No launch check of its own (the caller's next GAGS_CHECK_LAUNCH covers it); returns the sort's code.
int gags_rows_group_launch(int64_t rows, int n_gauss, const int32_t *rows_dev, uint32_t *key, int32_t *idx, uint32_t *key_s,
                           int32_t *idx_s, int32_t *seg, void *sort_scratch, int64_t sort_scratch_bytes, hipStream_t st);
// out[g, ch_begin .. ch_begin + ch_count) = sum of Gaussian g's rows (prow: `pitch` floats per row, indexed by absolute
// channel), out = [n_gauss, d], fp16 when out_f16.  sparse / wire / keep: reduce_rows_kernel.  No launch check of its own.
int gags_rows_reduce_launch(int n_gauss, int d, int ch_begin, int ch_count, const int32_t *seg, const int32_t *idx_s,
                            const float *prow, int pitch, void *out, bool out_f16, hipStream_t st, int sparse = 0,
                            const int32_t *wire_pos = nullptr, float *wire = nullptr, const uint8_t *keep_prev = nullptr,
                            uint8_t *keep_cur = nullptr);

// ---- raster_bwd_geom.hip: geometry backward at wide D -----------------------------------------------------------------
int64_t gags_raster_bwd_geom_scratch_bytes_impl(int64_t n_isects, int width, int height, int n_gauss, int d, int64_t n_rows);
// 1 = width not eligible (d % 8 != 0 or d < 16)
int gags_raster_bwd_geom_launch(int d, int n_gauss, int width, int height, const float *colors, const float *backgrounds,
                                const int32_t *offsets, int n_isects, const void *packed, const float *v_out,
                                const float *v_alphas, const int32_t *blk_rows, const float *wt, const int32_t *gid_s,
                                const int32_t *sidx_s, const float *Tbuf, void *scratch, int64_t scratch_bytes, float *v_geo,
                                int by_gauss, const int32_t *row_base, int64_t n_rows, const int32_t *hit,
                                const int32_t *flatten_ids, int f32mfma, int absgrad, hipStream_t st);
int gags_blended_mask_launch(int n_isects, const int32_t *hit, const int32_t *flatten_ids, unsigned char *mask, hipStream_t st);

// ---- raster_bwd_atomic.hip: single-kernel colours backward ------------------------------------------------------------
// 1 = width not eligible (d % 128 != 0)
int gags_raster_bwd_atomic_launch(int d, int width, int height, const void *packed, const int32_t *offsets,
                                  const int32_t *flat, int n_isects, const float *v_out, float *v_colors,
                                  int by_gauss, hipStream_t st);
