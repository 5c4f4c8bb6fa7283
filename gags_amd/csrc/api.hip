// C-ABI entry points of the raster stages: argument validation + dispatch onto the VALU kernels
// (narrow / odd D, full geometry gradients) and the matrix-core kernels (D >= 16, D % 4 == 0;
// the single-kernel fallbacks: D % 32 == 0).
#include <cstdlib>
#include "launch.h"
#include "scan.h"

namespace {
// the split forward's scratch, written by gags_raster_fwd and read by the backward entries (base NULL: sizes only)
struct FwdScratch {
    float *wt, *tbuf;
    int32_t *gid, *sidx, *hit;
    int64_t total;
};
// slot space: gags_slot_count() slots of 64 weights (common.h)
inline FwdScratch fwd_carve(const void *base, int64_t n_isects, int width, int height)
{
    const int64_t slots = gags_slot_count(n_isects, gags_tiles(width, height).n);
    GagsCarve c(base);
    FwdScratch L;
    L.wt = c.take<float>(slots * 64);
    L.gid = c.take<int32_t>(slots);
    L.sidx = c.take<int32_t>(slots);
    L.hit = c.take<int32_t>(n_isects + 1);
    L.tbuf = c.take<float>((int64_t)width * height);
    L.total = c.total();
    return L;
}
inline bool fused_width(int d) { return d >= 32 && d % 32 == 0; }  // single-kernel forward / atomic backward
// Intersections of one view the raster kernels can index: the count itself below GAGS_MAX_ISECTS AND the slot space it
// spans (4 I + 64 tiles + 64 slots, common.h) below 2^30 -- slot numbers are multiplied by 4 in unsigned 32-bit offsets
// (the id gathers of the feature pass); near the cap the per-tile slack alone (0.5 M slots at 1080p) would wrap them.
inline bool isects_ok(int64_t n_isects, int width, int height)
{
    if (n_isects < 0 || n_isects >= GAGS_MAX_ISECTS || width <= 0 || height <= 0) return false;
    return gags_slot_count(n_isects, gags_tiles(width, height).n) < (1ll << 30);
}
}  // namespace

extern "C" int gags_pack_isects(int n, int64_t n_isects, const int32_t *flatten_ids, const float *means2d,
                                const float *conics, const float *opacities, const int32_t *radii, void *grec,
                                void *packed, void *stream)
{
    if (n < 0 || n_isects < 0 || n_isects >= (1ll << 31)) return GAGS_EINVAL;
    if (n_isects == 0) return GAGS_OK;
    if (!flatten_ids || !means2d || !conics || !opacities || (!packed && !grec)) return GAGS_EINVAL;
    return gags_pack_isects_launch(n, (int)n_isects, flatten_ids, means2d, conics, opacities, radii, grec, packed,
                                   (hipStream_t)stream);
}

extern "C" int64_t gags_raster_fwd_scratch_bytes(int64_t n_isects, int width, int height)
{
    if (n_isects < 0 || width <= 0 || height <= 0) return 0;
    return fwd_carve(nullptr, n_isects, width, height).total;
}

namespace {
// GAGS_FWD_D16_UNFUSED=1 (experiments; read once): the 16-channel feature pass as its own kernel
bool fwd_d16_unfused()
{
    static const bool v = [] { const char *e = getenv("GAGS_FWD_D16_UNFUSED"); return e && e[0] == '1'; }();
    return v;
}
}  // namespace

extern "C" int gags_raster_fwd(int d, int n, int width, int height, const float *means2d, const float *conics,
                               const float *opacities, const float *colors, const float *backgrounds,
                               const int32_t *isect_offsets, const int32_t *flatten_ids, int64_t n_isects,
                               const void *packed, float *render_colors, float *render_alphas, int32_t *last_ids,
                               void *scratch, int64_t scratch_bytes, int32_t *blk_rows, int flags, void *stream)
{
    if (d <= 0 || n < 0 || width <= 0 || height <= 0 || !isects_ok(n_isects, width, height)) return GAGS_EINVAL;
    if (!isect_offsets || !render_colors || !render_alphas || !last_ids) return GAGS_EINVAL;
    if (n_isects > 0 && (!means2d || !conics || !opacities || !colors || !flatten_ids)) return GAGS_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const bool split = scratch && blk_rows && gags_mfma_width(d);
    if ((flags & GAGS_FEAT_F16) && (!split || (flags & GAGS_FWD_NO_MFMA) || !packed || n <= 0))
        return GAGS_EINVAL;  // an fp16 feature table is only read by the feature pass of the split forward
    if (d == 16 && !scratch && !blk_rows && packed && n > 0 && n_isects > 0 && !(flags & (GAGS_FWD_NO_MFMA | GAGS_FEAT_F16)) &&
        !(reinterpret_cast<uintptr_t>(render_colors) & 15) && !fwd_d16_unfused()) {
        // a 16-channel render without scratch (nobody will differentiate it): the fused weights + feature pass alone, no tiles
        return gags_raster_weights_launch(width, height, n, packed, (flags & GAGS_RECS_BY_GAUSSIAN) ? 1 : 0, isect_offsets, flatten_ids,
                                          (int)n_isects, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, render_alphas, last_ids, st,
                                          colors, backgrounds, render_colors);
    }
    if (!(flags & GAGS_FWD_NO_MFMA) && (split || fused_width(d)) && (packed || n_isects == 0) && n > 0) {
        if (split) {  // split forward: weights once, then the feature stream
            const FwdScratch L = fwd_carve(scratch, n_isects, width, height);
            if (scratch_bytes < L.total) return GAGS_ESCRATCH;
            float *wt = L.wt, *tbuf = L.tbuf;
            int32_t *gid_s = L.gid;
            int rc = GAGS_OK;
            // an fp32 table of exactly 16 channels (the reference's own width, train.py:68): the feature pass rides along with
            // the weights pass (bit-identical to the feature kernel: raster_weights.hip); the two ONLY_* flags keep the passes apart
            const bool fuse16 = d == 16 && !(flags & (GAGS_FEAT_F16 | GAGS_FWD_ONLY_FEATURES | GAGS_FWD_ONLY_WEIGHTS)) && n_isects > 0 &&
                                !(reinterpret_cast<uintptr_t>(render_colors) & 15) && !fwd_d16_unfused();
            if (!(flags & GAGS_FWD_ONLY_FEATURES))
                rc = gags_raster_weights_launch(width, height, n, packed, (flags & GAGS_RECS_BY_GAUSSIAN) ? 1 : 0, isect_offsets, flatten_ids, (int)n_isects, wt,
                                                gid_s, L.sidx, L.hit, blk_rows, tbuf, render_alphas, last_ids, st,
                                                fuse16 ? colors : nullptr, backgrounds, render_colors);
            if (rc != GAGS_OK || (flags & GAGS_FWD_ONLY_WEIGHTS) || fuse16) return rc;
            return gags_raster_fwd_feat_launch(d, width, height, n, colors, (flags & GAGS_FEAT_F16) ? ((flags & GAGS_FWD_F16MFMA) ? 2 : 1) : 0,
                                               (flags & GAGS_FWD_EXACT) ? 1 : 0, backgrounds, isect_offsets, (int)n_isects,
                                               blk_rows, wt, gid_s, tbuf, render_colors, st);
        }
        return gags_raster_fwd_fused_launch(d, width, height, packed, colors, backgrounds, isect_offsets, flatten_ids,
                                            (int)n_isects, render_colors, render_alphas, last_ids,
                                            (flags & GAGS_RECS_BY_GAUSSIAN) ? 1 : 0, st);
    }
    return gags_raster_fwd_valu(d, width, height, means2d, conics, opacities, colors, backgrounds, isect_offsets,
                                flatten_ids, (int)n_isects, render_colors, render_alphas, last_ids, st);
}

// ---- list trimming (round 6; include/gags_raster.h) ---------------------------------------------------------------------
extern "C" int gags_raster_list_need(int n, int width, int height, const int32_t *isect_offsets, const int32_t *flatten_ids,
                                     int64_t n_isects, const void *packed, int flags, int32_t *need, void *stream)
{
    if (n < 0 || width <= 0 || height <= 0 || n_isects < 0 || n_isects >= (1ll << 31) || !need || !isect_offsets) return GAGS_EINVAL;
    if (n_isects > 0 && (!flatten_ids || !packed || n == 0)) return GAGS_EINVAL;
    return gags_list_need_launch(width, height, n, packed, (flags & GAGS_RECS_BY_GAUSSIAN) ? 1 : 0, isect_offsets, flatten_ids,
                                 (int)n_isects, need, (hipStream_t)stream);
}

extern "C" int gags_trim_lists(int width, int height, const int32_t *isect_offsets, const int32_t *need_cum,
                               const int32_t *flatten_ids, int32_t *offsets_out, int32_t *flatten_out, void *stream)
{
    if (width <= 0 || height <= 0 || !isect_offsets || !need_cum || !offsets_out) return GAGS_EINVAL;
    const int n_tiles = gags_tiles(width, height).n;
    int rc = gags_trim_offsets_launch(n_tiles, need_cum, offsets_out, (hipStream_t)stream);
    if (rc != GAGS_OK || !flatten_out) return rc;  // (flatten_out NULL: the offsets only)
    if (!flatten_ids) return GAGS_EINVAL;
    return gags_trim_gather_launch(n_tiles, isect_offsets, offsets_out, flatten_ids, flatten_out, (hipStream_t)stream);
}

extern "C" int gags_trim_last_ids(int width, int height, const int32_t *isect_offsets, const int32_t *offsets_trimmed,
                                  const float *render_alphas, int32_t *last_ids, void *stream)
{
    if (width <= 0 || height <= 0 || !isect_offsets || !offsets_trimmed || !render_alphas || !last_ids) return GAGS_EINVAL;
    return gags_trim_last_ids_launch(width, height, isect_offsets, offsets_trimmed, render_alphas, last_ids, (hipStream_t)stream);
}

extern "C" int gags_raster_bwd(int d, int width, int height, const float *means2d, const float *conics,
                               const float *opacities, const float *colors, const float *backgrounds,
                               const int32_t *isect_offsets, const int32_t *flatten_ids, int64_t n_isects,
                               const void *packed, const float *render_alphas, const int32_t *last_ids,
                               const float *v_render_colors, const float *v_render_alphas, float *v_colors,
                               float *v_opacities, float *v_means2d, float *v_conics, int flags, void *stream)
{
    return gags_raster_bwd_abs(d, width, height, means2d, conics, opacities, colors, backgrounds, isect_offsets, flatten_ids,
                               n_isects, packed, render_alphas, last_ids, v_render_colors, v_render_alphas, v_colors, v_opacities,
                               v_means2d, v_conics, nullptr, flags, stream);
}

extern "C" int gags_raster_bwd_abs(int d, int width, int height, const float *means2d, const float *conics,
                                   const float *opacities, const float *colors, const float *backgrounds,
                                   const int32_t *isect_offsets, const int32_t *flatten_ids, int64_t n_isects,
                                   const void *packed, const float *render_alphas, const int32_t *last_ids,
                                   const float *v_render_colors, const float *v_render_alphas, float *v_colors,
                                   float *v_opacities, float *v_means2d, float *v_conics, float *v_means2d_abs, int flags,
                                   void *stream)
{
    if (d <= 0 || width <= 0 || height <= 0 || !isects_ok(n_isects, width, height)) return GAGS_EINVAL;
    if (v_means2d_abs && (d > 32 || (flags & GAGS_BWD_COLORS_ONLY))) return GAGS_EINVAL;
    if (n_isects == 0) return GAGS_OK;
    if (!means2d || !conics || !opacities || !colors || !isect_offsets || !flatten_ids || !render_alphas ||
        !last_ids || !v_render_colors || !v_colors)
        return GAGS_EINVAL;
    const bool geom = !(flags & GAGS_BWD_COLORS_ONLY);
    if (geom && (!v_opacities || !v_means2d || !v_conics)) return GAGS_EINVAL;
    if (!geom && !(flags & GAGS_FWD_NO_MFMA) && packed) {
        const int rc = gags_raster_bwd_atomic_launch(d, width, height, packed, isect_offsets, flatten_ids,
                                                     (int)n_isects, v_render_colors, v_colors,
                                                     (flags & GAGS_RECS_BY_GAUSSIAN) ? 1 : 0, (hipStream_t)stream);
        if (rc != 1) return rc;
    }
    return gags_raster_bwd_valu(d, width, height, means2d, conics, opacities, colors, backgrounds, isect_offsets,
                                flatten_ids, (int)n_isects, render_alphas, last_ids, v_render_colors,
                                v_render_alphas, v_colors, v_opacities, v_means2d, v_conics, geom,
                                (hipStream_t)stream, v_means2d_abs);
}

extern "C" int64_t gags_bwd_staged_scratch_bytes(int64_t rows, int n, int d)
{
    if (rows < 0 || n < 0 || d <= 0) return 0;
    return gags_bwd_staged_scratch_bytes_impl(rows, n, d);
}

namespace {
// rowmap = trow[n_isects + 1] (exclusive prefix sum of the forward's hit flags) followed, 256-B aligned, by
// trow_s[slots] (tile row of every K-step slot of the forward's slot space)
inline int64_t rowmap_slot_off(int64_t n_isects) { return al256((n_isects + 1) * 4) / 4; }
inline int64_t slot_count(int64_t n_isects, int width, int height)
{
    return gags_slot_count(n_isects, gags_tiles(width, height).n);
}
}  // namespace

extern "C" int64_t gags_bwd_rowmap_elems(int64_t n_isects, int width, int height)
{
    if (n_isects < 0 || width <= 0 || height <= 0) return 0;
    return rowmap_slot_off(n_isects) + slot_count(n_isects, width, height);
}

extern "C" int64_t gags_bwd_rowmap_scratch_bytes(int64_t n_isects)
{
    return n_isects < 0 ? 0 : gags_scan::scratch_bytes(n_isects > 0 ? n_isects : 1);
}

extern "C" int gags_bwd_rowmap(int64_t n_isects, int width, int height, const int32_t *isect_offsets,
                               const int32_t *blk_rows, const void *fwd_scratch, int64_t fwd_scratch_bytes,
                               int32_t *rowmap, int64_t rowmap_elems, int32_t *total, void *scratch,
                               int64_t scratch_bytes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (!isects_ok(n_isects, width, height) || !fwd_scratch || !rowmap || !total ||
        !isect_offsets || !blk_rows)
        return GAGS_EINVAL;
    if (rowmap_elems < gags_bwd_rowmap_elems(n_isects, width, height)) return GAGS_ESCRATCH;
    const FwdScratch L = fwd_carve(fwd_scratch, n_isects, width, height);
    if (fwd_scratch_bytes < L.total) return GAGS_ESCRATCH;
    hipStream_t st = (hipStream_t)stream;
    int32_t *trow = rowmap;
    if (hipMemsetAsync(trow, 0, sizeof(int32_t), st) != hipSuccess) return GAGS_ELAUNCH;
    if (n_isects == 0) return hipMemsetAsync(total, 0, sizeof(int32_t), st) == hipSuccess ? GAGS_OK : GAGS_ELAUNCH;
    if (!scratch || scratch_bytes < gags_scan::scratch_bytes(n_isects)) return GAGS_ESCRATCH;
    gags_scan::launch<false>((int)n_isects, L.hit, trow + 1, total, (int32_t *)scratch, st);
    GAGS_CHECK_LAUNCH();
    return gags_bwd_slot_rows_launch(width, height, (int)n_isects, isect_offsets, blk_rows,
                                     L.sidx, trow, rowmap + rowmap_slot_off(n_isects), st);
}

extern "C" int64_t gags_raster_bwd_geom_scratch_bytes(int64_t n_isects, int width, int height, int n, int d, int64_t n_rows)
{
    if (n_isects < 0 || width <= 0 || height <= 0 || n < 0 || d <= 0) return 0;
    return gags_raster_bwd_geom_scratch_bytes_impl(n_isects, width, height, n, d, n_rows);
}

extern "C" int gags_raster_bwd_geom(int d, int n, int width, int height, const float *colors, const float *backgrounds,
                                    const int32_t *isect_offsets, int64_t n_isects, const void *packed,
                                    const float *v_render_colors, const float *v_render_alphas, const int32_t *blk_rows,
                                    const void *fwd_scratch, int64_t fwd_scratch_bytes, void *scratch, int64_t scratch_bytes,
                                    float *v_geo, const int32_t *flatten_ids, const int32_t *row_base, int64_t n_rows,
                                    int flags, void *stream)
{
    if (d <= 0 || width <= 0 || height <= 0 || n < 0 || !isects_ok(n_isects, width, height)) return GAGS_EINVAL;
    if (n == 0) return GAGS_OK;
    if (!colors || !isect_offsets || !packed || !v_render_colors || !blk_rows || !fwd_scratch || !scratch || !v_geo)
        return GAGS_EINVAL;
    const FwdScratch L = fwd_carve(fwd_scratch, n_isects, width, height);
    if (fwd_scratch_bytes < L.total) return GAGS_ESCRATCH;
    return gags_raster_bwd_geom_launch(d, n, width, height, colors, backgrounds, isect_offsets, (int)n_isects, packed,
                                       v_render_colors, v_render_alphas, blk_rows, L.wt, L.gid, L.sidx, L.tbuf, scratch,
                                       scratch_bytes, v_geo, (flags & GAGS_RECS_BY_GAUSSIAN) ? 1 : 0, row_base, n_rows, L.hit,
                                       flatten_ids, (flags & GAGS_GEOM_F32MFMA) ? 1 : 0, (flags & GAGS_GEOM_ABSGRAD) ? 1 : 0,
                                       (hipStream_t)stream);
}

extern "C" int gags_blended_mask(int64_t n_isects, int width, int height, int n, const int32_t *flatten_ids,
                                 const void *fwd_scratch, int64_t fwd_scratch_bytes, unsigned char *mask, void *stream)
{
    if (!isects_ok(n_isects, width, height) || n < 0) return GAGS_EINVAL;
    if (n == 0) return GAGS_OK;
    if (!mask) return GAGS_EINVAL;
    if (hipMemsetAsync(mask, 0, (size_t)n, (hipStream_t)stream) != hipSuccess) return GAGS_ELAUNCH;
    if (n_isects == 0) return GAGS_OK;
    if (!flatten_ids || !fwd_scratch) return GAGS_EINVAL;
    const FwdScratch L = fwd_carve(fwd_scratch, n_isects, width, height);
    if (fwd_scratch_bytes < L.total) return GAGS_ESCRATCH;
    return gags_blended_mask_launch((int)n_isects, L.hit, flatten_ids, mask, (hipStream_t)stream);
}

extern "C" int gags_raster_bwd_colors_staged(int d, int n, int width, int height, const int32_t *isect_offsets,
                                             int64_t n_isects, const float *v_render_colors, const int32_t *blk_rows,
                                             const int32_t *rowmap, int64_t rows, const void *fwd_scratch,
                                             int64_t fwd_scratch_bytes, void *scratch, int64_t scratch_bytes,
                                             float *v_colors, int stage, int ch_begin, int ch_count,
                                             const int32_t *rows_dev, const int32_t *wire_pos, float *wire,
                                             const uint8_t *keep_prev, uint8_t *keep_cur, void *stream)
{
    if ((wire != nullptr) != (wire_pos != nullptr) || (wire && (stage & GAGS_STAGED_OUT_F16))) return GAGS_EINVAL;  // (the block is fp32)
    if ((keep_prev != nullptr) != (keep_cur != nullptr) || (keep_cur && (keep_prev == keep_cur || (stage & GAGS_STAGED_PREZEROED))))
        return GAGS_EINVAL;
    if (d <= 0 || width <= 0 || height <= 0 || n < 0 || !isects_ok(n_isects, width, height) || rows < 0 ||
        rows >= (1ll << 31) || stage < 0 || (stage & GAGS_STAGE_MASK) > GAGS_STAGE_REDUCE)
        return GAGS_EINVAL;
    if (n == 0) return GAGS_OK;
    if (!isect_offsets || !blk_rows || !rowmap || !fwd_scratch || !scratch || !v_colors || !v_render_colors)
        return GAGS_EINVAL;
    // (the rows kernel reads a tile's four slot counts as ONE 16-byte scalar load)
    if (reinterpret_cast<uintptr_t>(blk_rows) & 15) return GAGS_EINVAL;
    const FwdScratch L = fwd_carve(fwd_scratch, n_isects, width, height);
    if (fwd_scratch_bytes < L.total) return GAGS_ESCRATCH;
    return gags_raster_bwd_staged_launch(d, width, height, n, isect_offsets, (int)n_isects, v_render_colors, blk_rows,
                                         rowmap, rows, L.wt, L.gid, rowmap + rowmap_slot_off(n_isects), scratch, scratch_bytes,
                                         v_colors, stage, ch_begin, ch_count, rows_dev, wire_pos, wire, keep_prev, keep_cur,
                                         (hipStream_t)stream);
}
