/*
 * gags_raster.h -- C ABI of the MI355X-native GAGS feature rasterizer (libgags_hip.so).
 *
 * This is the drop-in boundary for ONE path of WHU-USI3DV/GAGS: the operator
 *     gsplat.rasterization(means, quats, scales, opacities, colors, viewmats, Ks,
 *                          backgrounds, width, height, packed=False, sh_degree, render_mode)
 * exactly as the reference calls it at gaussian_renderer/__init__.py:56-70, plus the
 * backward pass autograd runs for it under train.py:174 (`loss.backward()`).
 * Each entry point below is one stage of that operator; the stage <-> reference mapping
 *  is given per function.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no torch / C++ types cross the boundary.
 *  - every pointer is a DEVICE pointer unless its name ends in _host.
 *  - the caller owns all memory (outputs and scratch); nothing here allocates or frees
 *    caller-visible memory, and there is no global mutable state (re-entrant per stream).
 *  - `stream` is a hipStream_t passed as void* (NULL = the null stream).  Calls only
 *    enqueue work; they never synchronize, except gags_read_i32 which is the one
 *    explicit device->host readback (n_isects), mirroring gsplat's own sync -- avoidable: gags_tile_emit_cap.
 *  - return value: GAGS_OK (0) or a negative GAGS_E* code; gags_strerror() names it.
 *  - all floating point is fp32; indices are int32; intersection keys are int64
 *    (tile_id << 32 | float_bits(depth)), as in the reference's rasterizer.
 *  - tile size is fixed at 16 (GAGS_TILE), the gsplat default the reference relies on.
 */
#ifndef GAGS_RASTER_H
#define GAGS_RASTER_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: only what these headers declare is exported */
#pragma GCC visibility push(default)

#define GAGS_TILE 16
/* tile intersections of one view: the raster entries refuse more (GAGS_EINVAL).  4 K-step slots per intersection plus 64 per
 * tile must stay below 2^30 (32-bit byte offsets into the slot tables); 2^28 = 268 M covers a 4 M-Gaussian scene at 40+ tiles
 * per Gaussian.  The slot space is ~1 KB per intersection: the caller's memory is the practical limit. */
#define GAGS_MAX_ISECTS (1ll << 28)

#define GAGS_OK 0
#define GAGS_EINVAL (-1)   /* bad argument (null pointer, non-positive size, unsupported D) */
#define GAGS_ELAUNCH (-2)  /* HIP launch / runtime error (hipGetLastError != success) */
#define GAGS_ESCRATCH (-3) /* scratch buffer too small */
#define GAGS_ENODEV (-4)   /* no usable gfx950 device */

/* raster flags */
#define GAGS_BWD_COLORS_ONLY 1 /* backward: only v_colors (all the GAD flow consumes) */
#define GAGS_FWD_NO_MFMA 2     /* force the VALU kernels even when D allows the MFMA path */
#define GAGS_FEAT_F16 32       /* forward: `colors` points to an fp16 [N,D] table (BASELINE.json configs[4]: fp16 feature
                                  storage); widened exactly, same fp32 arithmetic.  Split matrix-core forward only. */
#define GAGS_FWD_F16MFMA 64    /* with GAGS_FEAT_F16 and D % 128 == 0, opt-in: the feature pass contracts on the 16-bit matrix
                                  cores (features exact, weights as fp16 head + tail: ~2^-22 per term, not bit-identical) */

#define GAGS_FWD_EXACT 2048    /* fp32 table, D >= 128: contract the feature pass with v_mfma_f32_32x32x2_f32 -- bit-for-bit the
                                  sequential fmaf chain of the algorithm (what the oracle computes) -- instead of the default
                                  16-bit matrix cores on operands split into three bf16 terms (exact operands, products to
                                  2^-23: as close to the float64 statement, 3x faster, not bit-identical to the chain) */

#define GAGS_FWD_ONLY_WEIGHTS 512   /* split forward: launch the weights pass only (alphas, last_ids, scratch) ... */
#define GAGS_FWD_ONLY_FEATURES 1024 /* ... or the feature pass only, on the scratch a GAGS_FWD_ONLY_WEIGHTS call left: lets a
                                  caller bracket the two kernels with its own events (bench.py's per-kernel roofline) */

#define GAGS_RECS_BY_GAUSSIAN 256 /* `packed` holds one record per GAUSSIAN (gags_pack_isects with packed = NULL) and the raster
                                  kernels gather it through flatten_ids themselves: no per-intersection copy (32 B x n_isects
                                  written and read back) and no gather kernel */

int gags_abi_version(void);
const char *gags_strerror(int code);
/* number of HIP devices visible, or a negative error; never throws */
int gags_device_count(void);

/* ---- The projection: K1 + K4 (fused projection and tile counting) forward, K2 backward -------------------------------------
 * Eleven entries, ONE contract.  gags_project_fwd_cam / gags_project_bwd_cam(camera_model, flags, ...) take the union of all
 * arguments and are what the package itself calls, for every camera; the nine entries declared behind them are compatibility
 * forms: each is the flagged entry with GAGS_CAM_PINHOLE and fixed flags, what its argument list lacks filled in (NULL, 1.0f,
 * 0) -- same launch, same bits, same return codes.
 *
 * Forward.  Replaces the projection stage of gsplat.rasterization reached from gaussian_renderer/__init__.py:56-63 (means,
 * quats wxyz, scales, viewmats, Ks) and the first pass of its tile intersection.  viewmat: row-major 4x4 world-to-camera (the
 * reference's world_view_transform.transpose(0,1), :55); K: row-major 3x3 (:31-38).  Outputs: radii[N] (0 = culled),
 * means2d[N,2], depths[N], conics[N,3], tiles_per_gauss[N].  Culled Gaussians get zeros everywhere.
 * Backward.  The chain rule of the forward for Gaussians with radii > 0 (the forward is recomputed in its operation order).
 * Inputs v_means2d[N,2], v_depths[N] (may be NULL), v_conics[N,3]; outputs (overwritten) v_means[N,3], v_quats[N,4],
 * v_scales[N,3].
 *
 * camera_model.  The model decides where a centre lands and the 2 x 3 Jacobian J of cov2d = J Sc J^T, with
 * p = (x, y, z) = Rcw mean + t and Sc = Rcw Sigma Rcw^T; near / far culling on z, depths = z, eps2d, the det <= 0 cull, conic,
 * radius, radius_clip / off-screen cull, tile count, the antialiased compensation and the pose terms are the same for every
 * model (N20).
 *   GAGS_CAM_PINHOLE  means2d = (fx x / z + cx, fy y / z + cy), J with the tangent clamp.
 *   GAGS_CAM_ORTHO    means2d = (fx x + cx, fy y + cy), J = [[fx, 0, 0], [0, fy, 0]]; fx, fy are pixels per world unit; no clamp.
 *   GAGS_CAM_FISHEYE  equidistant, no clamp; distortion coefficients with GAGS_PROJ_KB (below).  With eps = 1e-7:
 *                       rho = sqrt(x^2 + y^2) + eps, theta = atan2(rho, z + eps),
 *                       means2d = (fx x theta / rho + cx, fy y theta / rho + cy),
 *                       x2 = x^2 + eps, y2 = y^2, xy = x y, s = x2 + y2, l2 = s + z^2, b = atan2(rho, z) / rho / s, a = z / (l2 s),
 *                       J = [[fx (x2 a + y2 b), fx xy (a - b), -fx x / l2], [fy xy (a - b), fy (y2 a + x2 b), -fy y / l2]].
 *                     J IS this closed form, guards included (on the axis: [[fx / z, 0, 0], [0, fy / z, 0]]), not the derivative
 *                     of the map; the backward is the exact derivative of this forward, with d sqrt(x^2 + y^2) = 0 at x = y = 0,
 *                     so every output is finite there.  z < near_plane is culled: the field of view stays below 180 degrees.
 *
 * flags.  What a variant does not read is ignored, NULL or not.
 * GAGS_PROJ_RAW: quats / scales / opacity_logit are the STORED parameters (R2 folded into R4; SURVEY 8a R2: "4 elementwise
 *   kernels/iter over N (fusable into projection)"): rotation[N,4] un-normalised, scaling_log[N,3], opacity_logit[N] exactly
 *   as scene/gaussian_model.py:48-61 holds them; the kernel applies the getters of :116-139 -- exp (* scaling_modifier,
 *   gaussian_renderer/__init__.py:41), F.normalize, sigmoid -- bit for bit as torch evaluates them (tools/micro/actprobe.py),
 *   then projects.  Extra outputs: opacities[N] (activated: what the raster kernels read); quats_act[N,4] / scales_act[N,3]
 *   (activated; NULL = not wanted); grec (N * GAGS_PACKED_BYTES bytes, or NULL): the per-Gaussian record table of K8b for
 *   every Gaussian with radii > 0 -- the bytes gags_pack_isects(packed = NULL) would write -- so that the binning needs no
 *   record kernel.  The backward takes the gradients back to the stored parameters, v_opacities[N] (from the rasterizer;
 *   NULL = zeros) included; v_opacity_logit may be NULL.  Without RAW opacity_logit, scaling_modifier, opacities, quats_act,
 *   scales_act, grec, v_opacities and v_opacity_logit are ignored.
 * GAGS_PROJ_AA: rasterize_mode "antialiased" (Mip-Splatting's opacity compensation; N16).  The rule, in fp32:
 *   s00, s01, s11 = the 2-D covariance BEFORE eps2d is added;  det_o = s00 s11 - s01^2;  det_b = the blurred determinant
 *   (s00 + eps2d)(s11 + eps2d) - s01^2;  compensations[i] = sqrt(max(0, det_o / det_b)), and 0 for a culled Gaussian (radius 0).
 *   No constant is added to the divisor.  The opacity that reaches the binning records, the raster forward and backward is
 *   fl(opacity * compensation): the caller multiplies (without RAW), or the kernel does on the activated opacity,
 *   fl(fl(sigmoid(logit)) * compensation), in `opacities` and in the record it writes (with RAW).  Radius, conic, means2d,
 *   depth and tile count are those without AA bit for bit: the blurred covariance still decides them.  compensations[N] is
 *   written in full; without AA it is ignored.
 *   Backward: the exact derivative.  With r = det_o / det_b and (a, b, c) the conic, v_r = v_comp / (2 comp) where comp > 0,
 *   else 0, and
 *     d r / d s00 = (1 - r) a - eps2d / det_b,   d r / d s11 = (1 - r) c - eps2d / det_b,   d r / d s01 = 2 (1 - r) b
 *   are added to the covariance cotangent built from v_conics.  Without RAW v_comp is v_compensations[N] (NULL = zeros); with
 *   RAW v_opacities is the cotangent of the COMPENSATED opacity: v_comp = v_opacities * sigmoid(logit), v_opacity_logit gets
 *   the extra factor comp (0 for a culled Gaussian), and v_compensations is ignored (as it is without AA).
 * GAGS_PROJ_POSE (backward only; N17): the camera pose's cotangent on the way (pose refinement, relocalisation against a
 *   frozen scene).  v_viewmat[16] (overwritten): d loss / d viewmat, row-major 4 x 4, row 3 exactly zero.  With Rcw, t the
 *   upper 3 x 4, vp the cotangent of the camera-space point, GSc that of the camera-space covariance and A = Rcw Sigma, a
 *   Gaussian with radii > 0 contributes
 *     v_t[r] += vp[r],   v_Rcw[r][c] += vp[r] mean[c] + sum_k (GSc[r][k] + GSc[k][r]) A[k][c]
 *   and a culled one exactly zero.  K is not differentiated.  The sum over N is deterministic (no atomics): a wave sum, the
 *   four waves of a workgroup in double, one row of 12 floats per workgroup into `partials`, then gags_colsum_f32 over the
 *   rows.  partials: gags_project_pose_partials(n) rows of 12 floats, partials_bytes >= rows * 48.  With POSE v_means,
 *   v_quats / v_rotation, v_scales / v_scaling_log, v_opacity_logit may each be NULL (not wanted: not stored); where given
 *   they are bit for bit what the call without POSE writes.  Without POSE v_means, v_quats, v_scales are required and
 *   v_viewmat, partials, partials_bytes are ignored.
 * GAGS_PROJ_KB (both directions, only with GAGS_CAM_FISHEYE; N21): the fisheye's distortion coefficients, OpenCV's fisheye
 *   model / COLMAP's OPENCV_FISHEYE: theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8).  K then points to
 *   13 floats: the row-major 3 x 3 matrix, then k1, k2, k3, k4 (without the flag K is 9 floats and nothing behind them is
 *   read).  By Horner in t = theta^2:
 *     P(t) = 1 + t (k1 + t (k2 + t (k3 + t k4))),   P'(t) = 1 + t (3 k1 + t (5 k2 + t (7 k3 + t 9 k4))),
 *     g(theta) = theta P(theta^2),   g'(theta) = P'(theta^2),   g''(theta) = theta (6 k1 + t (20 k2 + t (42 k3 + t 72 k4))).
 *   The rule, with the guards of GAGS_CAM_FISHEYE (eps = 1e-7):
 *     rho = sqrt(x^2 + y^2) + eps,  theta = atan2(rho, z + eps),  tb = atan2(rho, z),
 *     means2d = (fx x g(theta) / rho + cx, fy y g(theta) / rho + cy),
 *     x2 = x^2 + eps, y2 = y^2, xy = x y, s = x2 + y2, l2 = s + z^2, b = g(tb) / rho / s, dg = g'(tb), a = dg * (z / (l2 s)),
 *     J = [[fx (x2 a + y2 b), fx xy (a - b), -fx x / l2 * dg], [fy xy (a - b), fy (y2 a + x2 b), -fy y / l2 * dg]]:
 *   the closed form above with g(theta) in the two places theta stands, and g'(tb) on a and on the third column.  With
 *   k1 .. k4 = 0, P = P' = 1 and g'' = 0 exactly, and every output, forward and backward, is bit for bit the one without the
 *   flag.  A Gaussian with dg <= 0 is culled (radius 0, zeros everywhere): there the image folds back on itself, and no lens
 *   maps that way; every other cull is shared and unchanged.  The backward is the exact derivative of this forward: the
 *   cotangents v_g (from g(theta) / rho), v_gb (from b) and v_dg (from a and the third column) return through
 *   v_theta += v_g g'(theta) and v_tb += v_gb g'(tb) + v_dg g''(tb), then the fisheye's chain.  K and the coefficients get no
 *   gradient from this entry (since N23: gags_project_bwd_calib, below).  POSE as for every model.
 *
 * GAGS_EINVAL before any launch: an unknown camera_model, unknown flag bits, GAGS_PROJ_KB with a camera_model other than
 * GAGS_CAM_FISHEYE, n < 0 (before any pointer is looked at), width or height <= 0, a missing pointer, with POSE a NULL
 * v_viewmat / partials or a short partials_bytes.  n = 0 is GAGS_OK with NULLs (with POSE v_viewmat is written, zeros). */
#define GAGS_CAM_PINHOLE 0
#define GAGS_CAM_ORTHO 1
#define GAGS_CAM_FISHEYE 2
#define GAGS_PROJ_RAW 1
#define GAGS_PROJ_AA 2
#define GAGS_PROJ_POSE 4
#define GAGS_PROJ_KB 32
int64_t gags_project_pose_partials(int n);
int gags_project_fwd_cam(int camera_model, int flags, int n, const float *means, const float *quats, const float *scales,
                         const float *opacity_logit, float scaling_modifier, const float *viewmat, const float *K,
                         int width, int height, float eps2d, float near_plane, float far_plane, float radius_clip,
                         int32_t *radii, float *means2d, float *depths, float *conics, int32_t *tiles_per_gauss,
                         float *opacities, float *quats_act, float *scales_act, void *grec, float *compensations,
                         void *stream);
int gags_project_bwd_cam(int camera_model, int flags, int n, const float *means, const float *quats, const float *scales,
                         const float *opacity_logit, float scaling_modifier, const float *viewmat, const float *K,
                         int width, int height, float eps2d, const int32_t *radii, const float *v_means2d,
                         const float *v_depths, const float *v_conics, const float *v_opacities,
                         const float *v_compensations, float *v_means, float *v_quats, float *v_scales,
                         float *v_opacity_logit, float *v_viewmat, float *partials, int64_t partials_bytes, void *stream);

/* N23: the intrinsics' gradients.  gags_project_bwd_calib is gags_project_bwd_cam -- its argument list, its variants (flags:
 * GAGS_PROJ_RAW | GAGS_PROJ_AA | GAGS_PROJ_POSE | GAGS_PROJ_KB), its scene gradients and, with POSE, its v_viewmat, bit for
 * bit -- with the cotangent of K and of the distortion coefficients on the way.  gags_project_bwd_cam itself has no flag for
 * it and is unchanged.
 *   v_K[9] (overwritten): d loss / d K, row-major 3 x 3; the entries of fx, cx, fy, cy, and exact zeros in the five others.
 *   v_coeffs[4] (overwritten; required with GAGS_PROJ_KB, neither read nor written without): d loss / d (k1, k2, k3, k4).
 * The rule.  The cotangent is the exact derivative of the projection forward as it is written above, summed over the
 * Gaussians with radii > 0; a culled Gaussian contributes exact zeros.  The culls, radii and tile decisions are not
 * differentiated (nowhere are they).  With vm2 the cotangent of means2d, vJ that of J (the antialiased compensation reaches K
 * through vJ; v_depths does not depend on K), rz = 1 / z, the y row mirroring the x row:
 *   every model      v_cx += vm2x.
 *   GAGS_CAM_PINHOLE v_fx += vm2x x rz + vJ[0][0] rz - [x inside the clamp] vJ[0][2] tx rz^2.  The clamp limits are functions
 *                    of K, x_pos = (1.15 W - cx) / fx and x_neg = (cx + 0.15 W) / fx, so past the clamp J[0][2] = -(fx lim) / z
 *                    does not depend on fx, and v_cx += vJ[0][2] rz there, on either side: the derivative of the code as written.
 *   GAGS_CAM_ORTHO   v_fx += vm2x x + vJ[0][0].
 *   GAGS_CAM_FISHEYE (with or without KB) row 0 of J is linear in fx: v_fx += vm2x (x k) + sum_c vJ[0][c] (J[0][c] / fx), k =
 *                    g(theta) / rho, the unscaled row formed once, nothing divided.
 *   GAGS_PROJ_KB     with t = theta^2, tt = tb^2 and the backward's v_g, v_gb, v_dg (v_dg after both of its contributions), for
 *                    j = 1 .. 4:  v_kj += v_g theta t^j + v_gb tb tt^j + v_dg (2 j + 1) tt^j, the powers by successive
 *                    multiplication.  They do not vanish at k1 .. k4 = 0: a calibration can start from the plain fisheye.
 * The sums over N are the pose's: a wave sum per term, the four waves of a workgroup in double, one row per workgroup, then
 * the column sums of the rows in gags_colsum_f32's fixed order (one launch for all of them); no atomics, the same bits from run
 * to run.  partials:
 * gags_project_calib_partials(n) rows of GAGS_CALIB_PARTIAL_FLOATS floats (12 pose, 6 K, 4 coefficients), partials_bytes >=
 * rows * GAGS_CALIB_PARTIAL_FLOATS * 4.  The kernel always runs in the pose kernel's structure; v_viewmat is stored only with
 * GAGS_PROJ_POSE (else ignored).  v_means, v_quats, v_scales, v_opacity_logit may each be NULL (not wanted: not stored).
 * GAGS_EINVAL before any launch: what gags_project_bwd_cam refuses, a NULL v_K or partials, with KB a NULL v_coeffs, with POSE
 * a NULL v_viewmat, a short partials_bytes.  n = 0 is GAGS_OK: v_K (v_coeffs with KB, v_viewmat with POSE) is written, zeros. */
#define GAGS_CALIB_PARTIAL_FLOATS 22
int64_t gags_project_calib_partials(int n);
int gags_project_bwd_calib(int camera_model, int flags, int n, const float *means, const float *quats, const float *scales,
                           const float *opacity_logit, float scaling_modifier, const float *viewmat, const float *K,
                           int width, int height, float eps2d, const int32_t *radii, const float *v_means2d,
                           const float *v_depths, const float *v_conics, const float *v_opacities,
                           const float *v_compensations, float *v_means, float *v_quats, float *v_scales,
                           float *v_opacity_logit, float *v_viewmat, float *v_K, float *v_coeffs, float *partials,
                           int64_t partials_bytes, void *stream);

/* The compatibility forms: nothing of their own but the argument list. */
/* = gags_project_fwd_cam(GAGS_CAM_PINHOLE, 0): opacity_logit, opacities, quats_act, scales_act, grec, compensations NULL,
 * scaling_modifier 1.0f. */
int gags_project_fwd(int n, const float *means, const float *quats, const float *scales,
                     const float *viewmat, const float *K, int width, int height,
                     float eps2d, float near_plane, float far_plane, float radius_clip,
                     int32_t *radii, float *means2d, float *depths, float *conics,
                     int32_t *tiles_per_gauss, void *stream);
/* = gags_project_fwd_cam(GAGS_CAM_PINHOLE, GAGS_PROJ_AA): as gags_project_fwd, compensations passed on. */
int gags_project_fwd_aa(int n, const float *means, const float *quats, const float *scales,
                        const float *viewmat, const float *K, int width, int height,
                        float eps2d, float near_plane, float far_plane, float radius_clip,
                        int32_t *radii, float *means2d, float *depths, float *conics,
                        int32_t *tiles_per_gauss, float *compensations, void *stream);
/* = gags_project_fwd_cam(GAGS_CAM_PINHOLE, GAGS_PROJ_RAW): compensations NULL. */
int gags_project_fwd_raw(int n, const float *means, const float *rotation, const float *scaling_log,
                         const float *opacity_logit, float scaling_modifier, const float *viewmat, const float *K,
                         int width, int height, float eps2d, float near_plane, float far_plane, float radius_clip,
                         int32_t *radii, float *means2d, float *depths, float *conics, int32_t *tiles_per_gauss,
                         float *opacities, float *quats_act, float *scales_act, void *grec, void *stream);
/* = gags_project_fwd_cam(GAGS_CAM_PINHOLE, GAGS_PROJ_RAW | GAGS_PROJ_AA): every argument passed on. */
int gags_project_fwd_raw_aa(int n, const float *means, const float *rotation, const float *scaling_log,
                            const float *opacity_logit, float scaling_modifier, const float *viewmat, const float *K,
                            int width, int height, float eps2d, float near_plane, float far_plane, float radius_clip,
                            int32_t *radii, float *means2d, float *depths, float *conics, int32_t *tiles_per_gauss,
                            float *opacities, float *quats_act, float *scales_act, void *grec, float *compensations,
                            void *stream);
/* = gags_project_bwd_cam(GAGS_CAM_PINHOLE, 0): opacity_logit, v_opacities, v_compensations, v_opacity_logit, v_viewmat, partials
 * NULL, scaling_modifier 1.0f, partials_bytes 0; `conics` is not read (recomputed in the forward's operation order). */
int gags_project_bwd(int n, const float *means, const float *quats, const float *scales,
                     const float *viewmat, const float *K, int width, int height, float eps2d,
                     const int32_t *radii, const float *conics,
                     const float *v_means2d, const float *v_depths, const float *v_conics,
                     float *v_means, float *v_quats, float *v_scales, void *stream);
/* = gags_project_bwd_cam(GAGS_CAM_PINHOLE, GAGS_PROJ_AA): as gags_project_bwd, v_compensations passed on. */
int gags_project_bwd_aa(int n, const float *means, const float *quats, const float *scales,
                        const float *viewmat, const float *K, int width, int height, float eps2d,
                        const int32_t *radii, const float *v_means2d, const float *v_depths, const float *v_conics,
                        const float *v_compensations, float *v_means, float *v_quats, float *v_scales, void *stream);
/* = gags_project_bwd_cam(GAGS_CAM_PINHOLE, GAGS_PROJ_RAW): v_compensations, v_viewmat, partials NULL, partials_bytes 0. */
int gags_project_bwd_raw(int n, const float *means, const float *rotation, const float *scaling_log,
                         const float *opacity_logit, float scaling_modifier, const float *viewmat, const float *K,
                         int width, int height, float eps2d, const int32_t *radii, const float *v_means2d,
                         const float *v_depths, const float *v_conics, const float *v_opacities, float *v_means,
                         float *v_rotation, float *v_scaling_log, float *v_opacity_logit, void *stream);
/* = gags_project_bwd_cam(GAGS_CAM_PINHOLE, GAGS_PROJ_RAW | GAGS_PROJ_AA): likewise. */
int gags_project_bwd_raw_aa(int n, const float *means, const float *rotation, const float *scaling_log,
                            const float *opacity_logit, float scaling_modifier, const float *viewmat, const float *K,
                            int width, int height, float eps2d, const int32_t *radii, const float *v_means2d,
                            const float *v_depths, const float *v_conics, const float *v_opacities, float *v_means,
                            float *v_rotation, float *v_scaling_log, float *v_opacity_logit, void *stream);
/* = gags_project_bwd_cam(GAGS_CAM_PINHOLE, flags | GAGS_PROJ_POSE): every argument passed on.  flags: GAGS_POSE_RAW |
 * GAGS_POSE_AA (= GAGS_PROJ_RAW, GAGS_PROJ_AA) and nothing else -- GAGS_PROJ_POSE itself is GAGS_EINVAL here. */
#define GAGS_POSE_RAW 1
#define GAGS_POSE_AA 2
int gags_project_bwd_pose(int flags, int n, const float *means, const float *quats, const float *scales,
                          const float *opacity_logit, float scaling_modifier, const float *viewmat, const float *K,
                          int width, int height, float eps2d, const int32_t *radii, const float *v_means2d,
                          const float *v_depths, const float *v_conics, const float *v_opacities,
                          const float *v_compensations, float *v_means, float *v_quats, float *v_scales,
                          float *v_opacity_logit, float *v_viewmat, float *partials, int64_t partials_bytes, void *stream);

/* K5: inclusive prefix sum of tiles_per_gauss -> cum[N]; the grand total (n_isects) is
 * also written to total[0], or -1 when it does not fit an int32 (the caller must refuse the view; the entries of cum
 * behind the wrap are then unspecified).  Every entry must lie in [0, 2^20): the 2048 entries one workgroup sums then fit an
 * int32, which is what the overflow check builds on (a tile count is at most the grid's: 2^20 tiles is 16 384 x 16 384
 * pixels).  in == cum is allowed, total may be NULL, n = 0 writes total[0] = 0 and nothing else.
 * scratch: gags_scan_scratch_bytes(n) bytes. */
int64_t gags_scan_scratch_bytes(int n);
int gags_cumsum_i32(int n, const int32_t *in, int32_t *cum, int32_t *total,
                    void *scratch, int64_t scratch_bytes, void *stream);

/* K5 over a permuted view: cum[i] = sum_{j <= i} in[idx[j]] (the tile counts in depth order, idx = gags_depth_order's
 * `order`): no gather kernel, no permuted copy.  in != cum. */
int gags_cumsum_gather_i32(int n, const int32_t *in, const int32_t *idx, int32_t *cum, int32_t *total,
                           void *scratch, int64_t scratch_bytes, void *stream);

/* the single device->host readback of the path (n_isects); synchronizes `stream`. */
int gags_read_i32(const int32_t *src, int32_t *dst_host, void *stream);

/* K7a (optional, faster binning): order[N] = stable argsort of the Gaussians by depth bits, and -- when tiles_ordered is
 * not NULL -- tiles_ordered[i] = tiles_per_gauss[order[i]] (prefix-sum THAT, or call gags_cumsum_gather_i32 on
 * tiles_per_gauss and order; emit in that order, and K7 only has to group by tile).
 * scratch: gags_depth_order_scratch_bytes(n) bytes. */
int64_t gags_depth_order_scratch_bytes(int n);
int gags_depth_order(int n, const float *depths, const int32_t *tiles_per_gauss, int32_t *order,
                     int32_t *tiles_ordered, void *scratch, int64_t scratch_bytes, void *stream);

/* K6: emit (key, value) per (Gaussian, tile) intersection, Gaussian after Gaussian in the order given
 * (order == NULL: by index); cum = inclusive prefix sum of the tile counts IN THAT ORDER.
 * isect_ids[n_isects] int64 = tile << 32 | depth bits, flatten_ids[n_isects] int32 = Gaussian. */
int gags_tile_emit(int n, const float *means2d, const int32_t *radii, const float *depths,
                   const int32_t *cum, const int32_t *order, int tile_w, int tile_h,
                   int64_t *isect_ids, int32_t *flatten_ids, void *stream);

/* K6 into CAPACITY-sized buffers, so that the count need not reach the host before the launches: at most `cap` pairs
 * are written, and entries [total[0], cap) become sentinel keys of a tile past the last one (they sort to the end;
 * gags_sort_pairs needs tile_bits = bit length of n_tiles for them).  total = gags_cumsum_i32's device-side total.  Run
 * sort / offsets / raster with `cap` as n_isects; read total afterwards (e.g. from a second stream, once everything is
 * enqueued): if it exceeds cap the results are garbage -- nothing was written out of bounds -- and the view must be run
 * again with a larger capacity. */
int gags_tile_emit_cap(int n, const float *means2d, const int32_t *radii, const float *depths, const int32_t *cum,
                       const int32_t *order, int tile_w, int tile_h, int64_t *isect_ids, int32_t *flatten_ids, int64_t cap,
                       const int32_t *total, void *stream);

/* K7: stable radix sort of the pairs on key bits [0, 32 + tile_bits); with depth_sorted != 0 the input
 * is already in depth order (K7a + ordered K6) and only bits [32, 32 + tile_bits) are sorted -- same
 * result (ties: depth, then Gaussian index), 2 passes instead of 6 at 1080p.
 * scratch: gags_sort_scratch_bytes(n_isects) bytes. */
int64_t gags_sort_scratch_bytes(int64_t n_isects);
int gags_sort_pairs(int64_t n_isects, int tile_bits, int depth_sorted,
                    const int64_t *keys_in, const int32_t *vals_in,
                    int64_t *keys_out, int32_t *vals_out,
                    void *scratch, int64_t scratch_bytes, void *stream);

/* K8: isect_offsets[tile_h*tile_w + 1]: first sorted index of each tile, and in the LAST entry the intersection count
 * (ABI version 2: every raster entry reads a tile's end from isect_offsets[tile + 1], none needs the count from the
 * host).  With capacity-sized inputs (gags_tile_emit_cap) pass the capacity as n_isects: the last entry is where the
 * sentinel keys begin = the true count. */
int gags_tile_offsets(int64_t n_isects, const int64_t *sorted_ids, int n_tiles,
                      int32_t *isect_offsets, void *stream);

/* K8b: gather each intersection's 2-D parameters into sorted order: one 32-byte record
 * {x, y, conic a, b, c, opacity, ex, ey} per sorted intersection, (ex, ey) being the conservative
 * half-extent of the alpha >= 1/255 footprint.  The wide-D (MFMA) raster kernels stream this
 * array instead of gathering means2d/conics/opacities per tile.  packed: n_isects * 32 bytes.
 * grec (optional scratch, n * 32 bytes): when given, the record is built once per Gaussian
 * (radii > 0 only, radii may be NULL = all) and the per-intersection pass is a pure gather.
 * packed == NULL (grec required): only the per-Gaussian table is built; hand `grec` to the raster entries as
 * `packed` together with the flag GAGS_RECS_BY_GAUSSIAN. */
#define GAGS_PACKED_BYTES 32
int gags_pack_isects(int n, int64_t n_isects, const int32_t *flatten_ids, const float *means2d,
                     const float *conics, const float *opacities, const int32_t *radii, void *grec,
                     void *packed, void *stream);

/* K9 (+K11): rasterize forward, any D >= 1 in ONE pass over the sorted lists (no 32-wide
 * re-walks).  Replaces the compositing stage of gsplat.rasterization for
 * colors[N,D] / backgrounds[D] (gaussian_renderer/__init__.py:61,64).
 * backgrounds may be NULL.  Outputs render_colors[H,W,D], render_alphas[H,W],
 * last_ids[H,W] (sorted index of the last blended Gaussian per pixel).
 * Kernel choice: with `packed` given, any D >= 16 runs on the matrix cores as the split weights + feature passes
 * (128-channel slices, then 64, then 32-channel slices, the last one ragged; D = 513 is four wide slices and one lane of a
 * narrow one) when `scratch` (gags_raster_fwd_scratch_bytes) and `blk_rows` ([tile_h*tile_w*4] int32, written: slots per
 * 8x8 pixel block) are provided, else (D % 32 == 0) as one fused kernel; anything else runs the
 * VALU kernels.  The scratch and blk_rows of a split forward are what
 * gags_raster_bwd_colors_staged consumes, so keep them alive until the backward.
 * An fp32 table of exactly 16 channels (the reference's own width) is composited by the weights pass itself (round 6: one
 * kernel, bit-identical to the separate feature pass; not with GAGS_FWD_ONLY_WEIGHTS / _ONLY_FEATURES).
 * The same table with `scratch` and `blk_rows` both NULL (a render nobody differentiates) runs that kernel without writing
 * weight tiles: no scratch needed, same pixels bit for bit, ~20 % less time; there is then nothing for a backward to consume.
 */
int64_t gags_raster_fwd_scratch_bytes(int64_t n_isects, int width, int height);
int gags_raster_fwd(int d, int n, int width, int height, const float *means2d, const float *conics,
                    const float *opacities, const float *colors, const float *backgrounds,
                    const int32_t *isect_offsets, const int32_t *flatten_ids, int64_t n_isects,
                    const void *packed /* from gags_pack_isects, or NULL: VALU kernels only */,
                    float *render_colors, float *render_alphas, int32_t *last_ids,
                    void *scratch, int64_t scratch_bytes, int32_t *blk_rows,
                    int flags, void *stream);

/* List trimming (round 6): a heavy view's tiles stop -- every pixel saturated -- after a few hundred of their tens of thousands
 * of sorted entries, yet the split forward's scratch is ~1 KB per LIST ENTRY (C5H: 169 M entries = 173 GB).
 *   gags_raster_list_need: need[tile] (n_tiles int32, written in full) = how many leading entries of the tile's list any of its
 *       pixels reads before the tile is done: the weights pass's own walk (same records, extent test, pairs, stop rule) without
 *       its outputs.  flags: GAGS_RECS_BY_GAUSSIAN as for gags_raster_fwd.
 *   gags_trim_lists: from the INCLUSIVE prefix sums of need (gags_cumsum_i32; its total = the trimmed intersection count, which
 *       sizes flatten_out) the trimmed offsets (n_tiles + 1 entries, the last one = the count) and the trimmed id list
 *       (flatten_out NULL: offsets only).
 * Every raster entry run on (offsets_out, flatten_out, trimmed count) computes bit for bit what it computes on the full
 * lists -- same slots, weights, alphas, renders, gradients -- except that last_ids index the trimmed list:
 *   gags_trim_last_ids: last_ids back to indices of the full sorted list, in place (pixels with alpha == 0 keep their 0). */
int gags_raster_list_need(int n, int width, int height, const int32_t *isect_offsets, const int32_t *flatten_ids,
                          int64_t n_isects, const void *packed, int flags, int32_t *need, void *stream);
int gags_trim_lists(int width, int height, const int32_t *isect_offsets, const int32_t *need_cum,
                    const int32_t *flatten_ids, int32_t *offsets_out, int32_t *flatten_out, void *stream);
int gags_trim_last_ids(int width, int height, const int32_t *isect_offsets, const int32_t *offsets_trimmed,
                       const float *render_alphas, int32_t *last_ids, void *stream);

/* K10: rasterize backward (what autograd runs under train.py:174).
 * v_colors[N,D] (and, unless GAGS_BWD_COLORS_ONLY, v_opacities[N], v_means2d[N,2],
 * v_conics[N,3]) must be zero-filled by the caller; results are accumulated with
 * float atomics.  v_render_alphas may be NULL (treated as zeros). */
int gags_raster_bwd(int d, int width, int height, const float *means2d, const float *conics,
                    const float *opacities, const float *colors, const float *backgrounds,
                    const int32_t *isect_offsets, const int32_t *flatten_ids, int64_t n_isects,
                    const void *packed /* from gags_pack_isects, or NULL */,
                    const float *render_alphas, const int32_t *last_ids,
                    const float *v_render_colors, const float *v_render_alphas,
                    float *v_colors, float *v_opacities, float *v_means2d, float *v_conics,
                    int flags, void *stream);

/* K10 with absgrad (AbsGS; N16): gags_raster_bwd's arguments plus v_means2d_abs[N,2], zero-filled by the caller like the
 * others.  The rule: absgrad[g] = SUM over pixels of (|g3|, |g4|), g3 / g4 being the pixel's v_means2d terms over ALL of its
 * channels, before any reduction across pixels; zero for a Gaussian that blended nowhere.  Defined only where one channel chunk
 * covers D (D <= 32): above that the kernel splits the per-pixel total over chunks, and an absolute value of a partial is not
 * the rule -- GAGS_EINVAL for D > 32 (or GAGS_BWD_COLORS_ONLY) with a non-NULL pointer.  NULL: gags_raster_bwd itself. */
int gags_raster_bwd_abs(int d, int width, int height, const float *means2d, const float *conics,
                        const float *opacities, const float *colors, const float *backgrounds,
                        const int32_t *isect_offsets, const int32_t *flatten_ids, int64_t n_isects,
                        const void *packed /* from gags_pack_isects, or NULL */,
                        const float *render_alphas, const int32_t *last_ids,
                        const float *v_render_colors, const float *v_render_alphas,
                        float *v_colors, float *v_opacities, float *v_means2d, float *v_conics, float *v_means2d_abs,
                        int flags, void *stream);

/* K10, staged flavour: colours-only backward WITHOUT atomics (deterministic), 16 <= D <= 1024 (any such D).
 * Consumes the scratch + blk_rows of a split gags_raster_fwd.
 *
 * gags_bwd_rowmap: numbers the (tile, Gaussian) pairs that blended into at least one pixel -- one partial
 * gradient row each -- in sorted order: rowmap[0 .. n_isects] = exclusive prefix sum of the hit flags the
 * forward left in its scratch, followed by the row number of every K-step slot of the forward; total[0] = the
 * row count `rows` (read it with gags_read_i32).  rowmap: gags_bwd_rowmap_elems(...) int32;
 * scratch: gags_bwd_rowmap_scratch_bytes(n_isects) bytes.
 *
 * The backward itself: gags_raster_bwd_colors_staged below. */
int64_t gags_bwd_rowmap_elems(int64_t n_isects, int width, int height);
int64_t gags_bwd_rowmap_scratch_bytes(int64_t n_isects);
int gags_bwd_rowmap(int64_t n_isects, int width, int height, const int32_t *isect_offsets, const int32_t *blk_rows,
                    const void *fwd_scratch, int64_t fwd_scratch_bytes, int32_t *rowmap, int64_t rowmap_elems,
                    int32_t *total, void *scratch, int64_t scratch_bytes, void *stream);
/* K10, geometry part at wide D (D >= 32, D % 8 == 0) after a split gags_raster_fwd: v_geo[N][8] =
 * (v_conics[3], v_means2d[2], v_opacities[1], A, A) per Gaussian, written in full, no atomics, deterministic.  A = (0, 0), or
 * with flags bit GAGS_GEOM_ABSGRAD the absgrad of gags_raster_bwd_abs: SUM over pixels of (|g3|, |g4|), the per-pixel v_means2d
 * terms over all channels (both dot passes and every D the entry serves; the dot products are complete before the scalar pass).
 * The D-proportional work -- <colors[g], v_render_colors[px]> for every (slot, pixel) of the forward -- runs on the
 * matrix cores: by default the 16-bit ones with split operands (feature rows and cotangent as two fp16 terms each after
 * exact power-of-two scalings -- one per Gaussian row, one per 8x8 block -- and three product terms: as close to float64 as
 * fp32 matrix arithmetic), with
 * flags bit GAGS_GEOM_F32MFMA the fp32 matrix instructions (rounds 1-2's kernel); the per-pair chain uses the forward's own weights (T = weight / alpha: front-to-back quantities,
 * not 1 - render_alpha rebuilt back to front).  Together with gags_raster_bwd_colors_staged this replaces
 * gags_raster_bwd when geometry needs grad at wide D (gsplat's rasterize_to_pixels backward [EXT]).
 * backgrounds / v_render_alphas may be NULL.  row_base (optional, [tile_h*tile_w*4] int32 = exclusive prefix sum of
 * blk_rows) with n_rows = sum of blk_rows numbers the per-slot rows compactly, so that only n_rows keys are sorted;
 * NULL / -1: one row per slot of the sparse slot space (no host-side count needed, ~6x more keys).
 * flatten_ids: the sorted intersections' Gaussian ids (names, with the forward's hit flags, the rows to split).
 * scratch: gags_raster_bwd_geom_scratch_bytes(n_isects, w, h, n, d, n_rows): with row_base the dot products are numbered
 * like the rows (256 B per blended slot and 256-channel pass: 2.3 GB at C3, D = 512), without it they live in a copy of
 * the forward's sparse slot space (~1.1 KB per tile intersection and pass); + 1.5 KB per Gaussian for the split table.
 * Returns 1 when D is not eligible. */
#define GAGS_GEOM_F32MFMA 32 /* gags_raster_bwd_geom's `flags`, next to GAGS_RECS_BY_GAUSSIAN */
#define GAGS_GEOM_ABSGRAD 0x40 /* gags_raster_bwd_geom's `flags`: columns 6, 7 of v_geo carry absgrad (N16) */
int64_t gags_raster_bwd_geom_scratch_bytes(int64_t n_isects, int width, int height, int n, int d, int64_t n_rows);
int gags_raster_bwd_geom(int d, int n, int width, int height, const float *colors, const float *backgrounds,
                         const int32_t *isect_offsets, int64_t n_isects, const void *packed,
                         const float *v_render_colors, const float *v_render_alphas, const int32_t *blk_rows,
                         const void *fwd_scratch, int64_t fwd_scratch_bytes, void *scratch, int64_t scratch_bytes,
                         float *v_geo, const int32_t *flatten_ids, const int32_t *row_base, int64_t n_rows, int flags,
                         void *stream);

/* mask[g] (n bytes, written in full) = 1 for every Gaussian that blended into at least one pixel of the view of a
 * split gags_raster_fwd (its scratch): exactly the rows of v_colors that can be non-zero.  A by-view multi-GPU step
 * exchanges only the union of these rows over the ranks (gags_amd/dist.py; SURVEY 8e "gradients are sparse in rows"). */
int gags_blended_mask(int64_t n_isects, int width, int height, int n, const int32_t *flatten_ids,
                      const void *fwd_scratch, int64_t fwd_scratch_bytes, unsigned char *mask, void *stream);
/* K10, staged flavour, the backward itself: per tile the four pixel blocks' partial rows are merged on chip and stored once
 * per (tile, Gaussian) ("rows"), the rows are sorted by Gaussian ("sort") and summed per Gaussian ("reduce").  No atomics,
 * bit-reproducible.  The rows' contraction (128-channel slices) runs on the 16-bit matrix cores with fp32-equivalent split
 * operands (fp16 terms after exact power-of-two scalings -- per (tile, channel) for the cotangent; for the weights, which lie
 * in [2^-21.3, 1), the constant 2^15 since round 6 --, fp32 accumulation; see the bits below for the number of terms).  Shape
 * since round 5: a wave per 32 channels of the slice, the four pixel blocks' contributions to a tile row meet in its
 * accumulators (csrc/raster_bwd_rows_cw.h); it multiplies THREE product terms of two-term operands (one fp32-level rounding
 * per operand, the second-order term dropped: <= 3 * 2^-24 per product; 1.68e-7 of float64 against the fp32 matrix
 * instructions' 1.90e-7).  Returns 1 when D is not eligible (16 <= D <= 1024, any such D); GAGS_ESCRATCH when a scratch is too
 * small.  One entry; a trailing pointer that is NULL switches its feature off.  By argument:
 *
 * blk_rows, fwd_scratch
 *     as a split gags_raster_fwd left them.  blk_rows (four int32 per tile) must be 16-byte aligned: a tile's four counts
 *     are one load.
 * rowmap, rows
 *     gags_bwd_rowmap's map and the row count it left in total[0].
 * scratch
 *     gags_bwd_staged_scratch_bytes(rows, n, d) bytes; the same scratch for every call of a view.
 * v_colors
 *     [N,D], written in full (no zero-fill needed) unless a bit or pointer below says otherwise.
 * stage
 *     (stage & GAGS_STAGE_MASK): GAGS_STAGE_ALL, or one of GAGS_STAGE_ROWS / _SORT / _REDUCE (per-kernel timing, range by
 *     range production, overlap of the zero-fill below), OR-ed with any of
 *     GAGS_STAGED_F32MFMA        rows on the fp32 matrix instructions instead (rounds 1-2's kernel).
 *     GAGS_STAGED_BLOCKWAVES     rows in round 4's shape (a wave per pixel block, rows merged in LDS; weights as three terms,
 *                                five product terms).
 *     GAGS_STAGED_EXACT_WEIGHTS  the default shape with exact three-term weights and five product terms.
 *     GAGS_STAGED_OUT_F16        v_colors points to an fp16 [N,D] tensor (the gradient of an fp16 feature table in the
 *                                table's dtype; sums are formed in fp32 and rounded once).
 *     GAGS_STAGED_PREZEROED      v_colors arrives ZERO-FILLED and the reduce stage skips the Gaussians that blended nothing
 *                                (73 % at C3) instead of writing their rows of zeros -- the caller fills it on a second
 *                                stream while the rows stage runs.
 *     GAGS_STAGED_RANGE_SCRATCH  the scratch holds the partial rows of THIS call's channel range only -- [rows, ch_count]
 *                                instead of [rows, D]; size it with gags_bwd_staged_scratch_bytes(rows, n, ch_count) -- so
 *                                that a wide gradient can be produced range by range (stages rows, sort, reduce for the
 *                                first range, rows and reduce for the others) through a quarter of the memory: a heavy
 *                                view's rows (80 M x 2 KB at D = 512) need not exist at once.
 * ch_begin, ch_count
 *     channels [ch_begin, ch_begin + ch_count) only (whole 128- / 64- / 32-channel slices, as D % 128 / 64 allows; the last
 *     range may end at D): v_colors[:, ch_begin : ch_begin + ch_count] is written; (0, d) = everything.  A multi-GPU by-view
 *     step calls range after range -- stages rows, sort, reduce for the range that starts at 0 (it writes the row ->
 *     Gaussian keys the sort needs), rows and reduce for the others -- and exchanges each range while the next is computed
 *     (gags_amd/dist.py).
 * rows_dev
 *     `rows` is a CAPACITY and the true row count lives on the device (rows_dev = gags_bwd_rowmap's total; NULL: rows is
 *     exact): rows past the capacity are dropped, the keys between the count and the capacity become sentinels.  Read the
 *     count afterwards; if it exceeds the capacity run the backward again.
 * wire_pos, wire (both or neither; not with GAGS_STAGED_OUT_F16: the block is fp32)
 *     the reduce stage ALSO writes the rows a by-view multi-GPU step exchanges (gags_amd/dist.py):
 *     wire[wire_pos[g], :] = the range's gradient row of Gaussian g for every g with wire_pos[g] >= 0 -- wire is a dense
 *     fp32 [union rows, ch_count] block (ch_count % 4 == 0), wire_pos the inverse of the union's row list
 *     (gags_compact_mask_pos).  Every row of the block is written (a union row this view did not touch gets zeros), so the
 *     block needs no clearing and no pack kernel re-reads the gradient.  v_colors is written as always.
 * keep_prev, keep_cur (both or neither, two different arrays of n bytes; not with GAGS_STAGED_PREZEROED)
 *     v_colors is a PERSISTENT gradient buffer (round 6) the caller keeps between steps, all zeros except the rows the
 *     previous call wrote -- keep_prev[g] != 0 (all zeros for a freshly zeroed buffer).  The reduce stage writes the rows
 *     that have partial rows now, re-zeroes the rows that had some last time and none now, touches nothing else (the rows of
 *     Gaussians that blend nothing -- 73 % at C3, 2.2 GB of zeros per step -- are never written again), and leaves
 *     keep_cur[g] for the next call.  Same values as without, bit for bit.  With wire: a row counts as written when it has
 *     partial rows OR lies in the exchanged block (the caller writes the ranks' sum there).  The caller must know that
 *     nobody else wrote the buffer in between (gags_amd/rasterization.py checks the storage's reference count and version
 *     counter and passes NULL otherwise). */
#define GAGS_STAGE_ALL 0
#define GAGS_STAGE_ROWS 1
#define GAGS_STAGE_SORT 2
#define GAGS_STAGE_REDUCE 3
#define GAGS_STAGE_MASK 15
#define GAGS_STAGED_F32MFMA 32
#define GAGS_STAGED_OUT_F16 64
#define GAGS_STAGED_PREZEROED 128
#define GAGS_STAGED_RANGE_SCRATCH 256
#define GAGS_STAGED_BLOCKWAVES 512
#define GAGS_STAGED_EXACT_WEIGHTS 1024
int64_t gags_bwd_staged_scratch_bytes(int64_t rows, int n, int d);
int gags_raster_bwd_colors_staged(int d, int n, int width, int height, const int32_t *isect_offsets, int64_t n_isects,
                                  const float *v_render_colors, const int32_t *blk_rows, const int32_t *rowmap, int64_t rows,
                                  const void *fwd_scratch, int64_t fwd_scratch_bytes, void *scratch, int64_t scratch_bytes,
                                  float *v_colors, int stage, int ch_begin, int ch_count, const int32_t *rows_dev,
                                  const int32_t *wire_pos, float *wire, const uint8_t *keep_prev, uint8_t *keep_cur,
                                  void *stream);

/* Diagnostics (roofline model): counts[0] += (pixel,Gaussian) pairs evaluated
 * before each pixel's stop, counts[1] += pairs blended.  counts[2] int64, zeroed by caller. */
int gags_raster_stats(int width, int height, const float *means2d, const float *conics,
                      const float *opacities, const int32_t *isect_offsets, const int32_t *flatten_ids,
                      int64_t n_isects, int64_t *counts, void *stream);

/* Column sums of an fp32 table [n_rows, k], 1 <= k <= 12: out[c] = sign * sum over rows of table[r, c] for c < k, and
 * out[k .. n_out) = 0 (k <= n_out <= 256).  One workgroup, sums in double, fixed order: two calls give the same bits.
 * n_rows = 0 writes zeros.  (Second stage of gags_project_bwd_pose; v_campos = -sum of gags_sh_bwd_dirs' rows.) */
int gags_colsum_f32(int64_t n_rows, int k, const float *table, float sign, float *out, int n_out, void *stream);

/* K3: spherical-harmonics colour, used when feature_mode=False and no override colour
 * (gaussian_renderer/__init__.py:51-53).  coeffs[N,kc,3], campos[3] (device),
 * out[N,3] = max(SH(dir) + 0.5, 0) where radii>0, zeros elsewhere.  Basis and signs as
 * utils/sh_utils.py:57-112. */
int gags_sh_fwd(int n, int kc, int degree, const float *means, const float *campos,
                const float *coeffs, const int32_t *radii, float *out, void *stream);
/* v_coeffs[N,kc,3] overwritten; directions are treated as constants (geometry frozen). */
int gags_sh_bwd(int n, int kc, int degree, const float *means, const float *campos,
                const int32_t *radii, const float *colors_out, const float *v_out,
                float *v_coeffs, void *stream);

/* K3 backward, view-direction part: v_means[n,3] = d loss / d means through dir = normalize(mean - campos) (gsplat
 * propagates this gradient; it matters when the SH colour branch runs with trainable positions, train.py:142 without
 * --feature_mode).  coeffs [n,kc,3], colors_out = gags_sh_fwd's output (clamp mask), v_out [n,3]. */
int gags_sh_bwd_dirs(int n, int kc, int degree, const float *means, const float *campos, const float *coeffs,
                     const int32_t *radii, const float *colors_out, const float *v_out, float *v_means, void *stream);

/* K12: expected-depth normalisation of the last channel: c[...,d-1] /= max(alpha,1e-10)
 * (render_mode "RGB+ED", the only consumer is render.py:118,127-133). */
int gags_ed_normalize(int64_t n_pix, int d, float *render_colors, const float *render_alphas,
                      void *stream);

/* R9: one Adam step of the feature parameter, in place, torch.optim.Adam semantics without weight decay
 * or amsgrad (the reference's optimizer: scene/gaussian_model.py:192-208, eps = 1e-15; stepped at
 * train.py:221-223).  `step` is the 1-based step count; all four arrays have `numel` floats, 16-B aligned. */
int gags_adam_step(int64_t numel, float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                   double lr, double beta1, double beta2, double eps, int step, void *stream);

/* N19: row-selective Adam, every tensor of a step in ONE launch.  Tensor t is [n_rows, width_t] fp32, row-major and
 * contiguous; its four arrays share that shape.  Row r of tensor t is updated iff
 *     (row_mask == NULL || row_mask[r] != 0)  &&  (!(flags & GAGS_ADAM_SKIP_ZERO_ROWS) || grad_t[r, :] has a non-zero),
 * "non-zero" by bit pattern (bits & 0x7fffffff: -0.0 is zero, NaN is not), decided per tensor.  A row that is not updated
 * keeps param, exp_avg and exp_avg_sq bit for bit (its moments do NOT decay); an updated element holds exactly the bits
 * gags_adam_step writes (same arithmetic, same host scalars).  `step` is the global 1-based count, there is no per-row
 * counter.  GAGS_ADAM_NO_BIAS_CORRECTION: step_size = lr and sqrt(v) is not divided.
 * tensors: a HOST array of n_tensors descriptors (1 .. GAGS_ADAM_MAX_TENSORS), copied into the kernel argument: no device
 * allocation, no global state, no readback.  Pointers need 4-byte alignment only (a row slice, a view at an odd offset);
 * a tensor whose four bases are 16-byte aligned with width % 4 == 0 is accessed 16 bytes per lane.  row_mask: device,
 * n_rows bytes.  Traffic of a skipped row: the mask byte (mask), or the gradient row once (zero test); nothing else.
 * GAGS_EINVAL, nothing launched: n_rows < 0, n_tensors outside [1, 8], step < 1, unknown flag bits, width < 1, betas
 * outside [0, 1), eps < 0, a pointer not 4-byte aligned, a NULL array with n_rows > 0.  n_rows == 0: GAGS_OK. */
typedef struct {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    int64_t width;
    double lr, beta1, beta2, eps;
} gags_adam_tensor;
#define GAGS_ADAM_MAX_TENSORS 8
#define GAGS_ADAM_SKIP_ZERO_ROWS 1
#define GAGS_ADAM_NO_BIAS_CORRECTION 2
int64_t gags_adam_tensor_bytes(void); /* sizeof(gags_adam_tensor): lets a binding check its mirror of the struct */
int gags_adam_step_rows(int64_t n_rows, int32_t n_tensors, const gags_adam_tensor *tensors, const uint8_t *row_mask,
                        int32_t flags, int32_t step, void *stream);

/* Multi-GPU by-view step (north_star "RCCL all-reduce of feature/geometry gradients"): the exchange itself is
 * torch.distributed over RCCL; these two kernels move the rows that can be non-zero between the gradient [N, d] and
 * the dense wire block [n_rows, cw] of one channel range [c0, c0 + cw).  idx: int64 row numbers (device; NULL = all rows,
 * n_rows = N).  Element types: 0 fp32, 1 fp16, 2 bf16 (wire only).
 *   gags_pack_rows  : wire[r, :] = grad[idx[r], c0 : c0 + cw]                     (idx[r] < 0: a padding row, zeros)
 *   gags_unpack_rows: local == NULL: grad[idx[r], c0 : c0 + cw]  = wire[r, :]
 *                     local != NULL: grad[idx[r], c0 : c0 + cw] += wire[r, :] - local[r, :]   (local: same type as wire)
 *                     (idx[r] < 0: skipped)
 *   gags_compact_mask: the row list itself, on the device: idx[0 .. count) = ascending r with mask[r] != 0 (the union of
 *                     the ranks' blended-Gaussian masks, gags_blended_mask), idx[count .. cap) = -1, count[0] = number of
 *                     set rows (may exceed cap: the surplus is not stored).  Replaces a host-synchronising torch.nonzero. */
int64_t gags_compact_mask_scratch_bytes(int n);
int gags_compact_mask(int n, const uint8_t *mask, int64_t cap, int64_t *idx, int32_t *count, void *scratch,
                      int64_t scratch_bytes, void *stream);
/*   gags_compact_mask_pos: the same, and the inverse on the way: pos[r] (n int32, written in full) = the position of row r
 *                     in idx, -1 for rows that are not set or whose position is >= cap (gags_raster_bwd_colors_staged
 *                     writes the exchanged rows through it: wire_pos). */
int gags_compact_mask_pos(int n, const uint8_t *mask, int64_t cap, int64_t *idx, int32_t *pos, int32_t *count, void *scratch,
                          int64_t scratch_bytes, void *stream);
int gags_pack_rows(int64_t n_rows, const int64_t *idx, const void *grad, int grad_type, int d, int c0, int cw,
                   void *wire, int wire_type, void *stream);
int gags_unpack_rows(int64_t n_rows, const int64_t *idx, const void *wire, int wire_type, const void *local,
                     void *grad, int grad_type, int d, int c0, int cw, void *stream);

/* Harness helper (the build's own synthetic step): out[0] = <x, y> over `numel` floats,
 * the terminal loss `(render * G).sum()` of bench.py; reproducible (fixed grid and order).
 * scratch: gags_dot_scratch_bytes() bytes; x, y 16-B aligned. */
int64_t gags_dot_scratch_bytes(void);
int gags_dot_f32(int64_t numel, const float *x, const float *y, float *out, void *scratch,
                 int64_t scratch_bytes, void *stream);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* GAGS_RASTER_H */
