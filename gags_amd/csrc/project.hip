// K1 + K4: fused 3D->2D projection and tile counting, one lane per Gaussian.
// HBM-bound O(N) stage: reads 40 B (+ the shared 21-float camera block via scalar loads),
// writes 32 B per Gaussian.  Follows SURVEY.md Appendix A1-A6; the operation order is part
// of the numerical contract (bit-exact radii / tile counts against the oracle), so this
// translation unit must be built with -ffp-contract=off.
#include "common.h"
#include "raster_mfma_common.h"
#include "reduce.h"
#include <type_traits>

namespace {

struct Cam {
    float R00, R01, R02, t0, R10, R11, R12, t1, R20, R21, R22, t2;
    float fx, fy, cx, cy;
};

__device__ __forceinline__ Cam load_cam(const float *__restrict__ vm, const float *__restrict__ K)
{
    Cam c;
    c.R00 = vm[0]; c.R01 = vm[1]; c.R02 = vm[2]; c.t0 = vm[3];
    c.R10 = vm[4]; c.R11 = vm[5]; c.R12 = vm[6]; c.t1 = vm[7];
    c.R20 = vm[8]; c.R21 = vm[9]; c.R22 = vm[10]; c.t2 = vm[11];
    c.fx = K[0]; c.cx = K[2]; c.fy = K[4]; c.cy = K[5];
    return c;
}

// N20: the camera model.  It decides where a centre lands (means2d) and the 2 x 3 Jacobian J that carries the camera-space
// covariance to the screen (cov2d = J Sc J^T); everything else of the projection is shared.  cam_fwd / cam_bwd are the ONE place
// where each model's arithmetic stands: the forward kernel and the backward kernel (which recomputes the forward) call cam_fwd,
// the backward calls cam_bwd, in every RAW / AA / POSE variant.  The pinhole bodies are the expressions the kernels held before
// N20, token for token: same operation order, same bits.
//   ortho:    means2d = (fx x + cx, fy y + cy), J = [[fx, 0, 0], [0, fy, 0]]; no clamp.
//   fisheye:  equidistant, no clamp (with distortion coefficients: N21, below); eps = 1e-7:  rho = sqrt(x^2 + y^2) + eps, theta = atan2(rho, z + eps),
//             means2d = (fx x theta / rho + cx, fy y theta / rho + cy); x2 = x^2 + eps, y2 = y^2, xy = x y, s = x2 + y2,
//             l2 = s + z^2, b = atan2(rho, z) / rho / s, a = z / (l2 s),
//             J = [[fx (x2 a + y2 b), fx xy (a - b), -fx x / l2], [fy xy (a - b), fy (y2 a + x2 b), -fy y / l2]].
//             J is this closed form, guards included (on the axis: fx / z, fy / z, 0 elsewhere), and cam_bwd is its exact
//             derivative, d sqrt(x^2 + y^2) taken as 0 at x = y = 0.
struct CamLim { float x_pos, x_neg, y_pos, y_neg; };  // the pinhole's tangent clamp (0.3 of the half field of view past the image)

__device__ __forceinline__ CamLim cam_limits(float fx, float fy, float cx, float cy, int width, int height)
{
    const float fw = (float)width, fh = (float)height;
    const float tan_fovx = 0.5f * fw / fx;
    const float tan_fovy = 0.5f * fh / fy;
    CamLim l;
    l.x_pos = (fw - cx) / fx + 0.3f * tan_fovx;
    l.x_neg = cx / fx + 0.3f * tan_fovx;
    l.y_pos = (fh - cy) / fy + 0.3f * tan_fovy;
    l.y_neg = cy / fy + 0.3f * tan_fovy;
    return l;
}

// N21: the fisheye with distortion coefficients (GAGS_PROJ_KB: K carries k1 .. k4 behind its nine floats) is a fourth value of
// CAM, private to this file.  theta_d = g(theta) = theta P(theta^2) stands where the fisheye has theta (in k and in b), and
// dg = g'(tb) = P'(tb^2) multiplies a and the third column of J; by Horner in t = theta^2:
//   P(t) = 1 + t (k1 + t (k2 + t (k3 + t k4))),  P'(t) = 1 + t (3 k1 + t (5 k2 + t (7 k3 + t 9 k4))),
//   g''(theta) = theta (6 k1 + t (20 k2 + t (42 k3 + t 72 k4))).
// With k1 .. k4 = 0: P = P' = 1 and g'' = 0 exactly, and every expression below rounds as the plain fisheye's does (same bits,
// forward and backward).  dg <= 0 (the image folds back on itself) is a cull: cam_fwd returns dg, 1 for every other model.
// (GAGS_FISHEYE_EPS, Kb, kb_P and kb_dP stand in common.h: the min-depth mapping of depthsample.hip projects with them too.)
constexpr int GAGS_CAM_FISHEYE_KB = 3;

template <int CAM>
__device__ __forceinline__ Kb load_kb(const float *__restrict__ K)
{
    if constexpr (CAM == GAGS_CAM_FISHEYE_KB) return Kb{K[9], K[10], K[11], K[12]};
    else return Kb{0.f, 0.f, 0.f, 0.f};  // (K is nine floats: nothing behind them is read)
}
__device__ __forceinline__ float kb_ddg(const Kb &c, float theta, float t)
{
    return theta * (6.f * c.k1 + t * (20.f * c.k2 + t * (42.f * c.k3 + t * (72.f * c.k4))));
}

template <int CAM>
__device__ __forceinline__ float cam_fwd(float fx, float fy, float cx, float cy, const CamLim &lim, const Kb &kb, float x, float y,
                                         float z, float &m2x, float &m2y, float (&J)[2][3])
{
    if constexpr (CAM == GAGS_CAM_PINHOLE) {
        const float rz = 1.f / z;
        const float rz2 = rz * rz;
        const float tx = z * fminf(lim.x_pos, fmaxf(-lim.x_neg, x * rz));
        const float ty = z * fminf(lim.y_pos, fmaxf(-lim.y_neg, y * rz));
        J[0][0] = fx * rz; J[0][1] = 0.f; J[0][2] = -fx * tx * rz2;
        J[1][0] = 0.f; J[1][1] = fy * rz; J[1][2] = -fy * ty * rz2;
        m2x = fx * x * rz + cx;
        m2y = fy * y * rz + cy;
    } else if constexpr (CAM == GAGS_CAM_ORTHO) {
        J[0][0] = fx; J[0][1] = 0.f; J[0][2] = 0.f;
        J[1][0] = 0.f; J[1][1] = fy; J[1][2] = 0.f;
        m2x = fx * x + cx;
        m2y = fy * y + cy;
    } else if constexpr (CAM == GAGS_CAM_FISHEYE_KB) {
        const float rho = sqrtf(x * x + y * y) + GAGS_FISHEYE_EPS;
        const float theta = atan2f(rho, z + GAGS_FISHEYE_EPS);
        const float k = (theta * kb_P(kb, theta * theta)) / rho;
        m2x = (fx * x) * k + cx;
        m2y = (fy * y) * k + cy;
        const float x2 = x * x + GAGS_FISHEYE_EPS, y2 = y * y, xy = x * y;
        const float s = x2 + y2, l2 = s + z * z;
        const float tb = atan2f(rho, z), tt = tb * tb;
        const float dg = kb_dP(kb, tt);
        const float b = (tb * kb_P(kb, tt)) / rho / s, a = dg * (z / (l2 * s));
        const float amb = a - b;
        J[0][0] = fx * (x2 * a + y2 * b); J[0][1] = (fx * xy) * amb; J[0][2] = -fx * x / l2 * dg;
        J[1][0] = (fy * xy) * amb; J[1][1] = fy * (y2 * a + x2 * b); J[1][2] = -fy * y / l2 * dg;
        return dg;
    } else {
        const float rho = sqrtf(x * x + y * y) + GAGS_FISHEYE_EPS;
        const float theta = atan2f(rho, z + GAGS_FISHEYE_EPS);
        const float k = theta / rho;
        m2x = (fx * x) * k + cx;
        m2y = (fy * y) * k + cy;
        const float x2 = x * x + GAGS_FISHEYE_EPS, y2 = y * y, xy = x * y;
        const float s = x2 + y2, l2 = s + z * z;
        const float b = atan2f(rho, z) / rho / s, a = z / (l2 * s);
        const float amb = a - b;
        J[0][0] = fx * (x2 * a + y2 * b); J[0][1] = (fx * xy) * amb; J[0][2] = -fx * x / l2;
        J[1][0] = (fy * xy) * amb; J[1][1] = fy * (y2 * a + x2 * b); J[1][2] = -fy * y / l2;
    }
    return 1.f;
}

// (v_means2d, vJ) -> vp, the cotangent of the camera-space point; v_depth (the cotangent of depths = z, when has_depth) joins
// vp[2] where the pinhole kernel has always added it, between the means2d term and the J terms.
// CALIB (N23): cal[8] = this Gaussian's terms of the cotangents of (fx, cx, fy, cy, k1, k2, k3, k4), the exact derivative of
// cam_fwd as it is written (k1 .. k4 only with GAGS_CAM_FISHEYE_KB; the others are left as they come in).  The pinhole's clamp
// limits are functions of K -- x_pos = (1.15 W - cx) / fx, x_neg = (cx + 0.15 W) / fx -- so past the clamp, on either side,
// J[0][2] = -(fx lim) / z does not depend on fx and d J[0][2] / d cx = 1 / z.  The fisheye's rows of J are linear in fx / fy:
// the unscaled row is formed once, nothing is divided.  Everything CALIB adds stands behind `if constexpr`: without it the
// bodies, and their bits, are those of before N23.
template <int CAM, bool CALIB = false>
__device__ __forceinline__ void cam_bwd(float fx, float fy, const CamLim &lim, const Kb &kb, float x, float y, float z, float vm2x,
                                        float vm2y, const float (&vJ)[2][3], bool has_depth, float v_depth, float (&vp)[3],
                                        float *cal = nullptr)
{
    if constexpr (CAM == GAGS_CAM_PINHOLE) {
        const float rz = 1.f / z, rz2 = rz * rz, rz3 = rz2 * rz;
        const float xr = x * rz, yr = y * rz;
        const int x_in = (xr <= lim.x_pos) && (xr >= -lim.x_neg);
        const int y_in = (yr <= lim.y_pos) && (yr >= -lim.y_neg);
        const float tx = z * fminf(lim.x_pos, fmaxf(-lim.x_neg, xr));
        const float ty = z * fminf(lim.y_pos, fmaxf(-lim.y_neg, yr));
        vp[0] = fx * rz * vm2x;
        vp[1] = fy * rz * vm2y;
        vp[2] = -(fx * x * vm2x + fy * y * vm2y) * rz2;
        if (has_depth) vp[2] += v_depth;
        if (x_in) vp[0] += -fx * rz2 * vJ[0][2]; else vp[2] += -fx * rz3 * vJ[0][2] * tx;
        if (y_in) vp[1] += -fy * rz2 * vJ[1][2]; else vp[2] += -fy * rz3 * vJ[1][2] * ty;
        vp[2] += -fx * rz2 * vJ[0][0] - fy * rz2 * vJ[1][1] + 2.f * fx * tx * rz3 * vJ[0][2] + 2.f * fy * ty * rz3 * vJ[1][2];
        if constexpr (CALIB) {
            cal[0] = (vm2x * x) * rz + vJ[0][0] * rz;
            cal[1] = vm2x;
            if (x_in) cal[0] -= (vJ[0][2] * tx) * rz2; else cal[1] += vJ[0][2] * rz;
            cal[2] = (vm2y * y) * rz + vJ[1][1] * rz;
            cal[3] = vm2y;
            if (y_in) cal[2] -= (vJ[1][2] * ty) * rz2; else cal[3] += vJ[1][2] * rz;
        }
    } else if constexpr (CAM == GAGS_CAM_ORTHO) {
        vp[0] = fx * vm2x;  // (J is constant: vJ reaches nothing)
        vp[1] = fy * vm2y;
        vp[2] = has_depth ? v_depth : 0.f;
        if constexpr (CALIB) {
            cal[0] = vm2x * x + vJ[0][0];
            cal[1] = vm2x;
            cal[2] = vm2y * y + vJ[1][1];
            cal[3] = vm2y;
        }
    } else if constexpr (CAM == GAGS_CAM_FISHEYE_KB) {  // the fisheye's chain below with g, dg and their three cotangents
        const float r0 = sqrtf(x * x + y * y);
        const float rho = r0 + GAGS_FISHEYE_EPS, zt = z + GAGS_FISHEYE_EPS;
        const float theta = atan2f(rho, zt);
        const float k = (theta * kb_P(kb, theta * theta)) / rho;
        const float x2 = x * x + GAGS_FISHEYE_EPS, y2 = y * y, xy = x * y;
        const float s = x2 + y2, z2 = z * z, l2 = s + z2;
        const float tb = atan2f(rho, z), tt = tb * tb;
        const float dg = kb_dP(kb, tt);
        const float a0 = z / (l2 * s);
        const float b = (tb * kb_P(kb, tt)) / rho / s, a = dg * a0;
        // means2d = (fx x k + cx, fy y k + cy), k = g(theta) / rho
        const float v_k = (fx * x) * vm2x + (fy * y) * vm2y;
        float vx = (fx * k) * vm2x, vy = (fy * k) * vm2y, vz = has_depth ? v_depth : 0.f;
        const float v_g = v_k / rho;
        float v_rho = -(v_k * k) / rho;
        // J (the closed form): cotangents of x2, y2, xy, a, b, l2, dg
        const float g00 = fx * vJ[0][0], g01 = fx * vJ[0][1], g02 = fx * vJ[0][2];
        const float g10 = fy * vJ[1][0], g11 = fy * vJ[1][1], g12 = fy * vJ[1][2];
        const float gx = g01 + g10;
        float v_x2 = g00 * a + g11 * b;
        float v_y2 = g00 * b + g11 * a;
        const float v_a = (g00 * x2 + g11 * y2) + gx * xy;
        const float v_b = (g00 * y2 + g11 * x2) - gx * xy;
        const float v_xy = gx * (a - b);
        vx += -g02 / l2 * dg;
        vy += -g12 / l2 * dg;
        float v_l2 = (g02 * x + g12 * y) / (l2 * l2) * dg;
        float v_dg = -(g02 * x + g12 * y) / l2;
        // a = dg a0, a0 = z / (l2 s)
        vz += (v_a * dg) / (l2 * s);
        v_l2 += -(v_a * a) / l2;
        float v_s = -(v_a * a) / s;
        v_dg += v_a * a0;
        // b = g(tb) / (rho s), dg = g'(tb), tb = atan2(rho, z)
        const float v_gb = v_b / (rho * s);
        v_rho += -(v_b * b) / rho;
        v_s += -(v_b * b) / s;
        const float v_tb = v_gb * dg + v_dg * kb_ddg(kb, tb, tt);
        if constexpr (CALIB) {
            const float amb = a - b, u01 = xy * amb;  // (the rows of J without fx / fy)
            cal[0] = vm2x * (x * k) + ((vJ[0][0] * (x2 * a + y2 * b) + vJ[0][1] * u01) + vJ[0][2] * (-x / l2 * dg));
            cal[1] = vm2x;
            cal[2] = vm2y * (y * k) + ((vJ[1][0] * u01 + vJ[1][1] * (y2 * a + x2 * b)) + vJ[1][2] * (-y / l2 * dg));
            cal[3] = vm2y;
            // k_j: g(theta) = theta (1 + sum k_j t^j), likewise g(tb); dg = 1 + sum (2 j + 1) k_j tt^j (v_dg is final here)
            const float t = theta * theta, wg = v_g * theta, wgb = v_gb * tb;
            float pt = t, ptt = tt;
            cal[4] = (wg * pt + wgb * ptt) + (3.f * v_dg) * ptt;
            pt *= t; ptt *= tt;
            cal[5] = (wg * pt + wgb * ptt) + (5.f * v_dg) * ptt;
            pt *= t; ptt *= tt;
            cal[6] = (wg * pt + wgb * ptt) + (7.f * v_dg) * ptt;
            pt *= t; ptt *= tt;
            cal[7] = (wg * pt + wgb * ptt) + (9.f * v_dg) * ptt;
        }
        const float hb = rho * rho + z2;
        v_rho += v_tb * z / hb;
        vz += -(v_tb * rho) / hb;
        // l2 = s + z^2, s = x2 + y2, x2 = x^2 + eps, y2 = y^2, xy = x y
        v_s += v_l2;
        vz += 2.f * z * v_l2;
        v_x2 += v_s;
        v_y2 += v_s;
        vx += 2.f * x * v_x2 + y * v_xy;
        vy += 2.f * y * v_y2 + x * v_xy;
        // g(theta), theta = atan2(rho, z + eps)
        const float v_theta = v_g * kb_dP(kb, theta * theta);
        const float ht = rho * rho + zt * zt;
        v_rho += v_theta * zt / ht;
        vz += -(v_theta * rho) / ht;
        // rho = sqrt(x^2 + y^2) + eps; its derivative at x = y = 0 is taken as 0
        if (r0 > 0.f) {
            vx += v_rho * (x / r0);
            vy += v_rho * (y / r0);
        }
        vp[0] = vx; vp[1] = vy; vp[2] = vz;
    } else {
        const float r0 = sqrtf(x * x + y * y);
        const float rho = r0 + GAGS_FISHEYE_EPS, zt = z + GAGS_FISHEYE_EPS;
        const float theta = atan2f(rho, zt);
        const float k = theta / rho;
        const float x2 = x * x + GAGS_FISHEYE_EPS, y2 = y * y, xy = x * y;
        const float s = x2 + y2, z2 = z * z, l2 = s + z2;
        const float tb = atan2f(rho, z);
        const float b = tb / rho / s, a = z / (l2 * s);
        // means2d = (fx x k + cx, fy y k + cy), k = theta / rho
        const float v_k = (fx * x) * vm2x + (fy * y) * vm2y;
        float vx = (fx * k) * vm2x, vy = (fy * k) * vm2y, vz = has_depth ? v_depth : 0.f;
        const float v_theta = v_k / rho;
        float v_rho = -(v_k * k) / rho;
        // J (the closed form): cotangents of x2, y2, xy, a, b, l2
        const float g00 = fx * vJ[0][0], g01 = fx * vJ[0][1], g02 = fx * vJ[0][2];
        const float g10 = fy * vJ[1][0], g11 = fy * vJ[1][1], g12 = fy * vJ[1][2];
        const float gx = g01 + g10;
        float v_x2 = g00 * a + g11 * b;
        float v_y2 = g00 * b + g11 * a;
        const float v_a = (g00 * x2 + g11 * y2) + gx * xy;
        const float v_b = (g00 * y2 + g11 * x2) - gx * xy;
        const float v_xy = gx * (a - b);
        if constexpr (CALIB) {
            const float amb = a - b, u01 = xy * amb;  // (the rows of J without fx / fy)
            cal[0] = vm2x * (x * k) + ((vJ[0][0] * (x2 * a + y2 * b) + vJ[0][1] * u01) + vJ[0][2] * (-x / l2));
            cal[1] = vm2x;
            cal[2] = vm2y * (y * k) + ((vJ[1][0] * u01 + vJ[1][1] * (y2 * a + x2 * b)) + vJ[1][2] * (-y / l2));
            cal[3] = vm2y;
        }
        vx += -g02 / l2;
        vy += -g12 / l2;
        float v_l2 = (g02 * x + g12 * y) / (l2 * l2);
        // a = z / (l2 s)
        vz += v_a / (l2 * s);
        v_l2 += -(v_a * a) / l2;
        float v_s = -(v_a * a) / s;
        // b = tb / (rho s), tb = atan2(rho, z)
        const float v_tb = v_b / (rho * s);
        v_rho += -(v_b * b) / rho;
        v_s += -(v_b * b) / s;
        const float hb = rho * rho + z2;
        v_rho += v_tb * z / hb;
        vz += -(v_tb * rho) / hb;
        // l2 = s + z^2, s = x2 + y2, x2 = x^2 + eps, y2 = y^2, xy = x y
        v_s += v_l2;
        vz += 2.f * z * v_l2;
        v_x2 += v_s;
        v_y2 += v_s;
        vx += 2.f * x * v_x2 + y * v_xy;
        vy += 2.f * y * v_y2 + x * v_xy;
        // theta = atan2(rho, z + eps)
        const float ht = rho * rho + zt * zt;
        v_rho += v_theta * zt / ht;
        vz += -(v_theta * rho) / ht;
        // rho = sqrt(x^2 + y^2) + eps; its derivative at x = y = 0 is taken as 0
        if (r0 > 0.f) {
            vx += v_rho * (x / r0);
            vy += v_rho * (y / r0);
        }
        vp[0] = vx; vp[1] = vy; vp[2] = vz;
    }
}

// The activations of scene/gaussian_model.py:116-139 as torch evaluates them on this stack, bit for bit
// (tools/micro/actprobe.py: 0 of 4 M values differ): get_scaling = exp(_scaling) (* scaling_modifier in render()),
// get_rotation = F.normalize(_rotation) = q / max(|q|, 1e-12) with |q|^2 summed pairwise, get_opacity = sigmoid(_opacity).
__device__ __forceinline__ float4 gags_act_rotation(float4 q)
{
    const float nrm = fmaxf(sqrtf((q.x * q.x + q.y * q.y) + (q.z * q.z + q.w * q.w)), 1e-12f);
    return make_float4(q.x / nrm, q.y / nrm, q.z / nrm, q.w / nrm);
}
__device__ __forceinline__ float gags_act_scaling(float s, float modifier) { return expf(s) * modifier; }
__device__ __forceinline__ float gags_act_opacity(float o) { return 1.0f / (1.0f + expf(-o)); }

// RAW: quats / scales are the stored parameters (_rotation un-normalised, _scaling in log space) and the kernel applies
// the getters itself (gags_project_fwd_raw); the activated opacity -- and, for a later backward, the activated quats and
// scales when asked for -- are written on the way.
// AA (rasterize_mode "antialiased", include/gags_raster.h): compensations[i] = sqrt(max(0, det(cov2d) / det(cov2d + eps2d I))),
// 0 for a culled Gaussian; RAW folds it into the activated opacity and the record.  Nothing else changes: the blurred
// covariance still decides radius, conic and tile count.
template <bool RAW, bool AA, int CAM>
__global__ __launch_bounds__(256) void project_fwd_kernel(
    int n, const float *__restrict__ means, const float *__restrict__ quats,
    const float *__restrict__ scales, const float *__restrict__ viewmat, const float *__restrict__ Kmat,
    int width, int height, float eps2d, float near_plane, float far_plane, float radius_clip,
    int tile_w, int tile_h,
    int32_t *__restrict__ radii, float *__restrict__ means2d, float *__restrict__ depths,
    float *__restrict__ conics, int32_t *__restrict__ tiles_per_gauss,
    const float *__restrict__ opacity_logits, float scaling_modifier, float *__restrict__ opacities_out,
    float *__restrict__ quats_out, float *__restrict__ scales_out, gags_mfma::GRec *__restrict__ grec_out,
    float *__restrict__ compensations)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float4 q = reinterpret_cast<const float4 *>(quats)[i];
    float s0 = scales[3 * i], s1 = scales[3 * i + 1], s2 = scales[3 * i + 2];
    float opac = 0.f;
    if constexpr (RAW) {
        q = gags_act_rotation(q);
        s0 = gags_act_scaling(s0, scaling_modifier); s1 = gags_act_scaling(s1, scaling_modifier); s2 = gags_act_scaling(s2, scaling_modifier);
        opac = gags_act_opacity(opacity_logits[i]);
        if constexpr (!AA) opacities_out[i] = opac;
        if (quats_out) reinterpret_cast<float4 *>(quats_out)[i] = q;
        if (scales_out) { scales_out[3 * i] = s0; scales_out[3 * i + 1] = s1; scales_out[3 * i + 2] = s2; }
    }
    const Cam c = load_cam(viewmat, Kmat);
    const float fw = (float)width, fh = (float)height;
    const CamLim lim = cam_limits(c.fx, c.fy, c.cx, c.cy, width, height);

    int32_t o_rad = 0, o_tiles = 0;
    float o_mx = 0.f, o_my = 0.f, o_z = 0.f, o_a = 0.f, o_b = 0.f, o_c = 0.f;
    float o_comp = 0.f;

    const float px = means[3 * i], py = means[3 * i + 1], pz = means[3 * i + 2];
    const float x = ((c.R00 * px + c.R01 * py) + c.R02 * pz) + c.t0;
    const float y = ((c.R10 * px + c.R11 * py) + c.R12 * pz) + c.t1;
    const float z = ((c.R20 * px + c.R21 * py) + c.R22 * pz) + c.t2;
    if (!(z < near_plane || z > far_plane)) {
        float qw = q.x, qx = q.y, qy = q.z, qz = q.w;
        const float inv_norm = 1.0f / sqrtf(((qx * qx + qy * qy) + qz * qz) + qw * qw);
        qw *= inv_norm; qx *= inv_norm; qy *= inv_norm; qz *= inv_norm;
        const float x2 = qx * qx, y2 = qy * qy, z2 = qz * qz;
        const float xy = qx * qy, xz = qx * qz, yz = qy * qz;
        const float wx = qw * qx, wy = qw * qy, wz = qw * qz;
        const float r00 = 1.f - 2.f * (y2 + z2), r01 = 2.f * (xy - wz), r02 = 2.f * (xz + wy);
        const float r10 = 2.f * (xy + wz), r11 = 1.f - 2.f * (x2 + z2), r12 = 2.f * (yz - wx);
        const float r20 = 2.f * (xz - wy), r21 = 2.f * (yz + wx), r22 = 1.f - 2.f * (x2 + y2);
        const float m00 = r00 * s0, m01 = r01 * s1, m02 = r02 * s2;
        const float m10 = r10 * s0, m11 = r11 * s1, m12 = r12 * s2;
        const float m20 = r20 * s0, m21 = r21 * s1, m22 = r22 * s2;
        const float c00 = (m00 * m00 + m01 * m01) + m02 * m02;
        const float c01 = (m00 * m10 + m01 * m11) + m02 * m12;
        const float c02 = (m00 * m20 + m01 * m21) + m02 * m22;
        const float c11 = (m10 * m10 + m11 * m11) + m12 * m12;
        const float c12 = (m10 * m20 + m11 * m21) + m12 * m22;
        const float c22 = (m20 * m20 + m21 * m21) + m22 * m22;
        const float a00 = (c.R00 * c00 + c.R01 * c01) + c.R02 * c02;
        const float a01 = (c.R00 * c01 + c.R01 * c11) + c.R02 * c12;
        const float a02 = (c.R00 * c02 + c.R01 * c12) + c.R02 * c22;
        const float a10 = (c.R10 * c00 + c.R11 * c01) + c.R12 * c02;
        const float a11 = (c.R10 * c01 + c.R11 * c11) + c.R12 * c12;
        const float a12 = (c.R10 * c02 + c.R11 * c12) + c.R12 * c22;
        const float a20 = (c.R20 * c00 + c.R21 * c01) + c.R22 * c02;
        const float a21 = (c.R20 * c01 + c.R21 * c11) + c.R22 * c12;
        const float a22 = (c.R20 * c02 + c.R21 * c12) + c.R22 * c22;
        const float v00 = (a00 * c.R00 + a01 * c.R01) + a02 * c.R02;
        const float v01 = (a00 * c.R10 + a01 * c.R11) + a02 * c.R12;
        const float v02 = (a00 * c.R20 + a01 * c.R21) + a02 * c.R22;
        const float v11 = (a10 * c.R10 + a11 * c.R11) + a12 * c.R12;
        const float v12 = (a10 * c.R20 + a11 * c.R21) + a12 * c.R22;
        const float v22 = (a20 * c.R20 + a21 * c.R21) + a22 * c.R22;

        float m2x, m2y, J[2][3];
        const float dg = cam_fwd<CAM>(c.fx, c.fy, c.cx, c.cy, lim, load_kb<CAM>(Kmat), x, y, z, m2x, m2y, J);
        float s00, s01, s11;
        if constexpr (CAM != GAGS_CAM_FISHEYE && CAM != GAGS_CAM_FISHEYE_KB) {  // J[0][1] = J[1][0] = 0: the products the pinhole kernel has always formed
            const float j00 = J[0][0], j02 = J[0][2];
            const float j11 = J[1][1], j12 = J[1][2];
            const float b00 = j00 * v00 + j02 * v02;
            const float b01 = j00 * v01 + j02 * v12;
            const float b02 = j00 * v02 + j02 * v22;
            const float b11 = j11 * v11 + j12 * v12;
            const float b12 = j11 * v12 + j12 * v22;
            s00 = b00 * j00 + b02 * j02;
            s01 = b01 * j11 + b02 * j12;
            s11 = b11 * j11 + b12 * j12;
        } else {  // a full J, in the order of the backward kernel
            const float b00 = (J[0][0] * v00 + J[0][1] * v01) + J[0][2] * v02;
            const float b01 = (J[0][0] * v01 + J[0][1] * v11) + J[0][2] * v12;
            const float b02 = (J[0][0] * v02 + J[0][1] * v12) + J[0][2] * v22;
            const float b10 = (J[1][0] * v00 + J[1][1] * v01) + J[1][2] * v02;
            const float b11 = (J[1][0] * v01 + J[1][1] * v11) + J[1][2] * v12;
            const float b12 = (J[1][0] * v02 + J[1][1] * v12) + J[1][2] * v22;
            s00 = (b00 * J[0][0] + b01 * J[0][1]) + b02 * J[0][2];
            s01 = (b00 * J[1][0] + b01 * J[1][1]) + b02 * J[1][2];
            s11 = (b10 * J[1][0] + b11 * J[1][1]) + b12 * J[1][2];
        }

        float det_o = 0.f;  // (AA: the determinant before the blur)
        if constexpr (AA) det_o = s00 * s11 - s01 * s01;
        s00 += eps2d; s11 += eps2d;
        const float det = s00 * s11 - s01 * s01;
        bool keep = det > 0.f;
        if constexpr (CAM == GAGS_CAM_FISHEYE_KB) keep = keep && dg > 0.f;  // (past the fold: culled)
        if (keep) {
            const float inv_det = 1.f / det;
            const float hb = 0.5f * (s00 + s11);
            const float v1 = hb + sqrtf(fmaxf(0.01f, hb * hb - det));
            const float radius = ceilf(3.f * sqrtf(v1));
            const bool off = (radius <= radius_clip) || (m2x + radius <= 0.f) || (m2x - radius >= fw) ||
                             (m2y + radius <= 0.f) || (m2y - radius >= fh);
            if (!off) {
                o_rad = (int32_t)radius;
                o_mx = m2x; o_my = m2y; o_z = z;
                o_a = s11 * inv_det; o_b = -s01 * inv_det; o_c = s00 * inv_det;
                int x0, x1, y0, y1;
                gags_tile_aabb(m2x, m2y, o_rad, tile_w, tile_h, x0, x1, y0, y1);
                o_tiles = (y1 - y0) * (x1 - x0);
                if constexpr (AA) o_comp = sqrtf(fmaxf(0.f, det_o / det));
            }
        }
    }
    radii[i] = o_rad;
    reinterpret_cast<float2 *>(means2d)[i] = make_float2(o_mx, o_my);
    depths[i] = o_z;
    conics[3 * i] = o_a; conics[3 * i + 1] = o_b; conics[3 * i + 2] = o_c;
    tiles_per_gauss[i] = o_tiles;
    if constexpr (AA) {
        compensations[i] = o_comp;
        if constexpr (RAW) { opac = opac * o_comp; opacities_out[i] = opac; }
    }
    // K8b on the way (the activated opacity is at hand here): the per-Gaussian record of the matrix-core raster kernels
    // (gags_pack_isects with packed = NULL writes the same bytes from the arrays above)
    if constexpr (RAW) {
        if (grec_out && o_rad > 0) grec_out[i] = gags_mfma::make_grec_from(o_mx, o_my, o_a, o_b, o_c, opac);
    }
}

}  // namespace

namespace {

template <bool RAW, bool AA, int CAM>
int project_fwd_launch(int n, const float *means, const float *quats, const float *scales, const float *opacity_logit,
                       float scaling_modifier, const float *viewmat, const float *K, int width, int height, float eps2d,
                       float near_plane, float far_plane, float radius_clip, int32_t *radii, float *means2d, float *depths,
                       float *conics, int32_t *tiles_per_gauss, float *opacities, float *quats_act, float *scales_act,
                       void *grec, float *compensations, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n < 0 || width <= 0 || height <= 0) return GAGS_EINVAL;
    if (n == 0) return GAGS_OK;
    if (!means || !quats || !scales || !viewmat || !K || !radii || !means2d || !depths || !conics || !tiles_per_gauss)
        return GAGS_EINVAL;
    if (RAW && (!opacity_logit || !opacities)) return GAGS_EINVAL;
    if (AA && !compensations) return GAGS_EINVAL;
    const int tile_w = (width + GAGS_TILE - 1) / GAGS_TILE, tile_h = (height + GAGS_TILE - 1) / GAGS_TILE;
    hipLaunchKernelGGL((project_fwd_kernel<RAW, AA, CAM>), dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, means,
                       quats, scales, viewmat, K, width, height, eps2d, near_plane, far_plane, radius_clip,
                       tile_w, tile_h, radii, means2d, depths, conics, tiles_per_gauss, opacity_logit, scaling_modifier,
                       opacities, quats_act, scales_act, reinterpret_cast<gags_mfma::GRec *>(grec), compensations);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

}  // namespace

// The four named forwards: gags_project_fwd_cam for the pinhole, what a variant lacks filled in (include/gags_raster.h).
extern "C" int gags_project_fwd(int n, const float *means, const float *quats, const float *scales,
                                const float *viewmat, const float *K, int width, int height,
                                float eps2d, float near_plane, float far_plane, float radius_clip,
                                int32_t *radii, float *means2d, float *depths, float *conics,
                                int32_t *tiles_per_gauss, void *stream)
{
    return gags_project_fwd_cam(GAGS_CAM_PINHOLE, 0, n, means, quats, scales, nullptr, 1.0f, viewmat, K, width, height, eps2d,
                                near_plane, far_plane, radius_clip, radii, means2d, depths, conics, tiles_per_gauss, nullptr,
                                nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int gags_project_fwd_aa(int n, const float *means, const float *quats, const float *scales,
                                   const float *viewmat, const float *K, int width, int height,
                                   float eps2d, float near_plane, float far_plane, float radius_clip,
                                   int32_t *radii, float *means2d, float *depths, float *conics,
                                   int32_t *tiles_per_gauss, float *compensations, void *stream)
{
    return gags_project_fwd_cam(GAGS_CAM_PINHOLE, GAGS_PROJ_AA, n, means, quats, scales, nullptr, 1.0f, viewmat, K, width, height,
                                eps2d, near_plane, far_plane, radius_clip, radii, means2d, depths, conics, tiles_per_gauss,
                                nullptr, nullptr, nullptr, nullptr, compensations, stream);
}

extern "C" int gags_project_fwd_raw(int n, const float *means, const float *rotation, const float *scaling_log,
                                    const float *opacity_logit, float scaling_modifier, const float *viewmat, const float *K,
                                    int width, int height, float eps2d, float near_plane, float far_plane,
                                    float radius_clip, int32_t *radii, float *means2d, float *depths, float *conics,
                                    int32_t *tiles_per_gauss, float *opacities, float *quats_act, float *scales_act,
                                    void *grec, void *stream)
{
    return gags_project_fwd_cam(GAGS_CAM_PINHOLE, GAGS_PROJ_RAW, n, means, rotation, scaling_log, opacity_logit, scaling_modifier,
                                viewmat, K, width, height, eps2d, near_plane, far_plane, radius_clip, radii, means2d, depths,
                                conics, tiles_per_gauss, opacities, quats_act, scales_act, grec, nullptr, stream);
}

extern "C" int gags_project_fwd_raw_aa(int n, const float *means, const float *rotation, const float *scaling_log,
                                       const float *opacity_logit, float scaling_modifier, const float *viewmat, const float *K,
                                       int width, int height, float eps2d, float near_plane, float far_plane,
                                       float radius_clip, int32_t *radii, float *means2d, float *depths, float *conics,
                                       int32_t *tiles_per_gauss, float *opacities, float *quats_act, float *scales_act,
                                       void *grec, float *compensations, void *stream)
{
    return gags_project_fwd_cam(GAGS_CAM_PINHOLE, GAGS_PROJ_RAW | GAGS_PROJ_AA, n, means, rotation, scaling_log, opacity_logit,
                                scaling_modifier, viewmat, K, width, height, eps2d, near_plane, far_plane, radius_clip, radii,
                                means2d, depths, conics, tiles_per_gauss, opacities, quats_act, scales_act, grec, compensations,
                                stream);
}

namespace {

// K2: projection backward, one lane per Gaussian (same operation order as the forward).
// RAW (gags_project_bwd_raw): quats / scales are the stored parameters; the getters are re-applied (bit for bit the
// forward's), and the gradients are taken one step further, to the stored parameters: d/d _scaling = v_s * exp(_scaling) *
// modifier, d/d _rotation through q / max(|q|, 1e-12), d/d _opacity = v_o * o (1 - o) for EVERY Gaussian (the opacity's
// gradient comes from the rasterizer, not from the projection, so it is not gated by radii).
// AA: the exact derivative of comp = sqrt(max(0, r)), r = det(cov2d) / det(cov2d + eps2d I), joins the covariance cotangent
// (include/gags_raster.h has the three partials).  Its cotangent is v_compensations (may be NULL), or in RAW
// v_opacities * sigmoid(logit) -- v_opacities then being the cotangent of the COMPENSATED opacity, so that the logit's
// gradient carries the factor comp (0 for a culled Gaussian).
// POSE (gags_project_bwd_pose, N17): the cotangent of the upper 3 x 4 of viewmat on the way.  With p = Rcw mu + t and
// Sc = Rcw S3 Rcw^T (S3 symmetric, A = Rcw S3) a Gaussian on screen contributes
//   v_t[r] = vp[r],   v_Rcw[r][c] = vp[r] mu[c] + sum_k (GSc[r][k] + GSc[k][r]) A[k][c]
// (the clamp of tx / ty, the antialiased term and v_depths are inside vp and GSc already); pose[4 r + c] takes them in the
// row-major order of viewmat, pose[4 r + 3] = v_t[r], and keeps its zeros for a lane past N or a culled Gaussian.  v_means,
// v_quats, v_scales may then each be NULL (a frozen scene): the stores are skipped, the values that are stored are the
// POSE = false kernel's bit for bit (same operations, same order).
// A lane past N or on a culled Gaussian LEAVEs the per-Gaussian work: it ends there without POSE; with POSE it only leaves
// the do { } while (0) around that work, so that all 64 lanes of every wave reach the wave sums behind it.  That is the first
// stage of the deterministic sum over N: a gags_wave_sum per term, the four wave totals of the workgroup added in double in
// wave order, one row of twelve floats per workgroup into pose_partials[blockIdx.x][12].  gags_colsum_f32 adds the rows
// (second stage).  No atomics.
#define GAGS_PBWD_LEAVE()              \
    {                                  \
        if constexpr (POSE) break;     \
        else return;                   \
    }
// MODE (N23): none / pose / pose + calib.  GAGS_PBWD_CALIB is the pose kernel -- same structure, the twelve pose terms formed by
// the very same operations -- with eight more sums on the way: the cotangents of (fx, cx, fy, cy) and, with GAGS_CAM_FISHEYE_KB,
// of (k1 .. k4), per Gaussian from cam_bwd<CAM, true>, exact zeros for a lane past N or a culled Gaussian.  First stage as the
// pose's; per workgroup one row (fx, 0, cx, 0, fy, cy) into the table behind the pose rows and, with the coefficients, one row
// (k1 .. k4) into the table behind that: pose_partials is then [rows, 12] [rows, 6] [rows, 4], rows = gridDim.x.
constexpr int GAGS_PBWD_NONE = 0, GAGS_PBWD_POSE = 1, GAGS_PBWD_CALIB = 2;
// (The calib kernels ask for three waves per SIMD, at most 168 registers: the compiler meets it without scratch, where it takes
// 176 - 178 for the fisheye with coefficients when left alone.  A second launch-bound argument of 1 asks for nothing: the
// kernels of before N23 compile to the instructions they had.)
template <bool RAW, bool AA, int MODE, int CAM>
__global__ __launch_bounds__(256, MODE == GAGS_PBWD_CALIB ? 3 : 1) void project_bwd_kernel(
    int N, const float *__restrict__ means, const float *__restrict__ quats, const float *__restrict__ scales,
    const float *__restrict__ viewmat, const float *__restrict__ Kmat, int width, int height, float eps2d,
    const int32_t *__restrict__ radii, const float *__restrict__ v_means2d, const float *__restrict__ v_depths,
    const float *__restrict__ v_conics, float *__restrict__ v_means, float *__restrict__ v_quats,
    float *__restrict__ v_scales, const float *__restrict__ opacity_logits, float scaling_modifier,
    const float *__restrict__ v_opacities, float *__restrict__ v_opacity_logits, const float *__restrict__ v_compensations,
    float *__restrict__ pose_partials)
{
    constexpr bool POSE = MODE != GAGS_PBWD_NONE, CALIB = MODE == GAGS_PBWD_CALIB;
    const int i = blockIdx.x * 256 + threadIdx.x;
    float pose[12];
    if constexpr (POSE) { _Pragma("unroll") for (int k = 0; k < 12; ++k) pose[k] = 0.f; }
    float cal[CALIB ? 8 : 1];
    if constexpr (CALIB) { _Pragma("unroll") for (int k = 0; k < 8; ++k) cal[k] = 0.f; }
    do {
    if (i >= N) GAGS_PBWD_LEAVE()
    const bool w_means = !POSE || v_means, w_quats = !POSE || v_quats, w_scales = !POSE || v_scales;
    if constexpr (RAW && AA) {
        if (v_opacity_logits) v_opacity_logits[i] = 0.f;  // (rewritten below, with comp, for the Gaussians on screen)
    } else if constexpr (RAW) {
        if (v_opacity_logits) {
            const float o = gags_act_opacity(opacity_logits[i]);
            v_opacity_logits[i] = v_opacities ? (v_opacities[i] * (1.0f - o)) * o : 0.f;  // (torch: grad * (1 - y) * y)
        }
    }
    _Pragma("unroll") for (int k = 0; k < 3; ++k) {
        if (w_means) v_means[3 * i + k] = 0.f;
        if (w_scales) v_scales[3 * i + k] = 0.f;
    }
    if (w_quats) { _Pragma("unroll") for (int k = 0; k < 4; ++k) v_quats[4 * i + k] = 0.f; }
    if (radii[i] <= 0) GAGS_PBWD_LEAVE()
    const float Rc[3][3] = {{viewmat[0], viewmat[1], viewmat[2]},
                            {viewmat[4], viewmat[5], viewmat[6]},
                            {viewmat[8], viewmat[9], viewmat[10]}};
    const float tc[3] = {viewmat[3], viewmat[7], viewmat[11]};
    const float fx = Kmat[0], cx = Kmat[2], fy = Kmat[4], cy = Kmat[5];
    const CamLim lim = cam_limits(fx, fy, cx, cy, width, height);
        /* ---- recompute forward intermediates ---- */
        const float mu[3] = {means[3 * i], means[3 * i + 1], means[3 * i + 2]};
        float p[3];
        _Pragma("unroll") for (int r = 0; r < 3; ++r) p[r] = ((Rc[r][0] * mu[0] + Rc[r][1] * mu[1]) + Rc[r][2] * mu[2]) + tc[r];
        const float x = p[0], y = p[1], z = p[2];
        float q0 = quats[4 * i], q1 = quats[4 * i + 1], q2 = quats[4 * i + 2], q3 = quats[4 * i + 3];
        float raw_nrm = 1.f;
        if constexpr (RAW) {
            raw_nrm = fmaxf(sqrtf((q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3)), 1e-12f);
            const float4 qa = gags_act_rotation(make_float4(q0, q1, q2, q3));
            q0 = qa.x; q1 = qa.y; q2 = qa.z; q3 = qa.w;
        }
        const float inv_norm = 1.0f / sqrtf(((q1 * q1 + q2 * q2) + q3 * q3) + q0 * q0);
        const float qw = q0 * inv_norm, qx = q1 * inv_norm, qy = q2 * inv_norm, qz = q3 * inv_norm;
        float R[3][3];
        R[0][0] = 1.f - 2.f * (qy * qy + qz * qz); R[0][1] = 2.f * (qx * qy - qw * qz); R[0][2] = 2.f * (qx * qz + qw * qy);
        R[1][0] = 2.f * (qx * qy + qw * qz); R[1][1] = 1.f - 2.f * (qx * qx + qz * qz); R[1][2] = 2.f * (qy * qz - qw * qx);
        R[2][0] = 2.f * (qx * qz - qw * qy); R[2][1] = 2.f * (qy * qz + qw * qx); R[2][2] = 1.f - 2.f * (qx * qx + qy * qy);
        float s[3] = {scales[3 * i], scales[3 * i + 1], scales[3 * i + 2]};
        if constexpr (RAW) { _Pragma("unroll") for (int k = 0; k < 3; ++k) s[k] = gags_act_scaling(s[k], scaling_modifier); }
        float M[3][3], S3[3][3], A[3][3], Sc[3][3];
        _Pragma("unroll") for (int r = 0; r < 3; ++r) _Pragma("unroll") for (int c = 0; c < 3; ++c) M[r][c] = R[r][c] * s[c];
        _Pragma("unroll") for (int r = 0; r < 3; ++r) _Pragma("unroll") for (int c = 0; c < 3; ++c)
            S3[r][c] = (M[r][0] * M[c][0] + M[r][1] * M[c][1]) + M[r][2] * M[c][2];
        _Pragma("unroll") for (int r = 0; r < 3; ++r) _Pragma("unroll") for (int c = 0; c < 3; ++c)
            A[r][c] = (Rc[r][0] * S3[0][c] + Rc[r][1] * S3[1][c]) + Rc[r][2] * S3[2][c];
        _Pragma("unroll") for (int r = 0; r < 3; ++r) _Pragma("unroll") for (int c = 0; c < 3; ++c)
            Sc[r][c] = (A[r][0] * Rc[c][0] + A[r][1] * Rc[c][1]) + A[r][2] * Rc[c][2];
        float m2x_, m2y_, J[2][3];  // (the centre itself is not needed again)
        const Kb kb = load_kb<CAM>(Kmat);
        cam_fwd<CAM>(fx, fy, cx, cy, lim, kb, x, y, z, m2x_, m2y_, J);
        (void)m2x_; (void)m2y_;
        float B[2][3];
        _Pragma("unroll") for (int r = 0; r < 2; ++r) _Pragma("unroll") for (int c = 0; c < 3; ++c)
            B[r][c] = (J[r][0] * Sc[0][c] + J[r][1] * Sc[1][c]) + J[r][2] * Sc[2][c];
        const float s00o = (B[0][0] * J[0][0] + B[0][1] * J[0][1]) + B[0][2] * J[0][2];
        const float s01 = (B[0][0] * J[1][0] + B[0][1] * J[1][1]) + B[0][2] * J[1][2];
        const float s11o = (B[1][0] * J[1][0] + B[1][1] * J[1][1]) + B[1][2] * J[1][2];
        const float s00 = s00o + eps2d, s11 = s11o + eps2d;
        const float det = s00 * s11 - s01 * s01;
        const float inv_det = 1.f / det;
        const float ca = s11 * inv_det, cb = -s01 * inv_det, cc = s00 * inv_det;
        /* ---- 1. conic -> cov2d:  G = -X Gx X,  X = [[ca,cb],[cb,cc]], Gx = [[va, vb/2],[vb/2, vc]] ---- */
        const float va = v_conics[3 * i], vb = 0.5f * v_conics[3 * i + 1], vc = v_conics[3 * i + 2];
        const float t00 = ca * va + cb * vb, t01 = ca * vb + cb * vc;
        const float t10 = cb * va + cc * vb, t11 = cb * vb + cc * vc;
        float G00 = -(t00 * ca + t01 * cb), G01 = -(t00 * cb + t01 * cc);
        float G10 = -(t10 * ca + t11 * cb), G11 = -(t10 * cb + t11 * cc);
        if constexpr (AA) {
            const float r = (s00o * s11o - s01 * s01) / det;
            const float comp = sqrtf(fmaxf(0.f, r));
            float v_comp = 0.f;
            if constexpr (RAW) {
                const float o = opacity_logits ? gags_act_opacity(opacity_logits[i]) : 0.f;
                const float vo = v_opacities ? v_opacities[i] : 0.f;
                v_comp = vo * o;
                if (v_opacity_logits) v_opacity_logits[i] = ((vo * comp) * (1.0f - o)) * o;
            } else {
                v_comp = v_compensations ? v_compensations[i] : 0.f;
            }
            const float v_r = comp > 0.f ? v_comp / (2.f * comp) : 0.f;
            const float e = eps2d * inv_det, omr = 1.f - r;
            G00 += v_r * (omr * ca - e);
            G11 += v_r * (omr * cc - e);
            G01 += v_r * omr * cb;  // (d r / d s01 = 2 (1 - r) b, half on either side of the symmetric matrix)
            G10 += v_r * omr * cb;
        }
        const float G[2][2] = {{G00, G01}, {G10, G11}};
        /* ---- 2. cov2d = J Sc J^T:  G_Sc = J^T G J ; G_J = G J Sc^T + G^T J Sc ---- */
        float GJ[2][3], GSc[3][3], vJ[2][3];
        _Pragma("unroll") for (int r = 0; r < 2; ++r) _Pragma("unroll") for (int c = 0; c < 3; ++c) GJ[r][c] = G[r][0] * J[0][c] + G[r][1] * J[1][c];
        _Pragma("unroll") for (int r = 0; r < 3; ++r) _Pragma("unroll") for (int c = 0; c < 3; ++c) GSc[r][c] = J[0][r] * GJ[0][c] + J[1][r] * GJ[1][c];
        _Pragma("unroll") for (int r = 0; r < 2; ++r) _Pragma("unroll") for (int c = 0; c < 3; ++c) {
            const float gt0 = G[0][r], gt1 = G[1][r]; /* G^T row r */
            const float a1 = (GJ[r][0] * Sc[c][0] + GJ[r][1] * Sc[c][1]) + GJ[r][2] * Sc[c][2];
            const float gtj0 = gt0 * J[0][0] + gt1 * J[1][0], gtj1 = gt0 * J[0][1] + gt1 * J[1][1],
                        gtj2 = gt0 * J[0][2] + gt1 * J[1][2];
            const float a2 = (gtj0 * Sc[0][c] + gtj1 * Sc[1][c]) + gtj2 * Sc[2][c];
            vJ[r][c] = a1 + a2;
        }
        /* ---- 3. J and mean2d/depth -> camera-space point ---- */
        const float vm2x = v_means2d[2 * i], vm2y = v_means2d[2 * i + 1];
        float vp[3];
        if constexpr (CALIB)
            cam_bwd<CAM, true>(fx, fy, lim, kb, x, y, z, vm2x, vm2y, vJ, v_depths != nullptr, v_depths ? v_depths[i] : 0.f, vp, cal);
        else
            cam_bwd<CAM>(fx, fy, lim, kb, x, y, z, vm2x, vm2y, vJ, v_depths != nullptr, v_depths ? v_depths[i] : 0.f, vp);
        if constexpr (POSE) {
            _Pragma("unroll") for (int r = 0; r < 3; ++r) {
                _Pragma("unroll") for (int c = 0; c < 3; ++c)
                    pose[4 * r + c] = vp[r] * mu[c] + (((GSc[r][0] + GSc[0][r]) * A[0][c] + (GSc[r][1] + GSc[1][r]) * A[1][c]) +
                                                       (GSc[r][2] + GSc[2][r]) * A[2][c]);
                pose[4 * r + 3] = vp[r];
            }
        }
        /* ---- 4. camera -> world ---- */
        if (w_means) {
            _Pragma("unroll") for (int c = 0; c < 3; ++c) v_means[3 * i + c] = (Rc[0][c] * vp[0] + Rc[1][c] * vp[1]) + Rc[2][c] * vp[2];
        }
        float T1[3][3], GS[3][3];
        _Pragma("unroll") for (int r = 0; r < 3; ++r) _Pragma("unroll") for (int c = 0; c < 3; ++c)
            T1[r][c] = (Rc[0][r] * GSc[0][c] + Rc[1][r] * GSc[1][c]) + Rc[2][r] * GSc[2][c];
        _Pragma("unroll") for (int r = 0; r < 3; ++r) _Pragma("unroll") for (int c = 0; c < 3; ++c)
            GS[r][c] = (T1[r][0] * Rc[0][c] + T1[r][1] * Rc[1][c]) + T1[r][2] * Rc[2][c];
        /* ---- 5. Sigma = M M^T: G_M = (G_S + G_S^T) M ---- */
        float GM[3][3];
        _Pragma("unroll") for (int r = 0; r < 3; ++r) _Pragma("unroll") for (int c = 0; c < 3; ++c)
            GM[r][c] = ((GS[r][0] + GS[0][r]) * M[0][c] + (GS[r][1] + GS[1][r]) * M[1][c]) + (GS[r][2] + GS[2][r]) * M[2][c];
        /* ---- 6. M = R diag(s) ---- */
        float GR[3][3];
        _Pragma("unroll") for (int c = 0; c < 3; ++c) {
            const float vs = (R[0][c] * GM[0][c] + R[1][c] * GM[1][c]) + R[2][c] * GM[2][c];
            if (w_scales) v_scales[3 * i + c] = RAW ? vs * s[c] : vs;  // RAW: d/d log-scale (torch: grad * modifier, then * exp(_scaling))
            _Pragma("unroll") for (int r = 0; r < 3; ++r) GR[r][c] = GM[r][c] * s[c];
        }
        /* ---- 7. R(q^) -> q^ ---- */
        const float vqw = 2.f * (-qz * GR[0][1] + qy * GR[0][2] + qz * GR[1][0] - qx * GR[1][2] - qy * GR[2][0] + qx * GR[2][1]);
        const float vqx = 2.f * (qy * GR[0][1] + qz * GR[0][2] + qy * GR[1][0] - 2.f * qx * GR[1][1] - qw * GR[1][2] +
                                 qz * GR[2][0] + qw * GR[2][1] - 2.f * qx * GR[2][2]);
        const float vqy = 2.f * (-2.f * qy * GR[0][0] + qx * GR[0][1] + qw * GR[0][2] + qx * GR[1][0] + qz * GR[1][2] -
                                 qw * GR[2][0] + qz * GR[2][1] - 2.f * qy * GR[2][2]);
        const float vqz = 2.f * (-2.f * qz * GR[0][0] - qw * GR[0][1] + qx * GR[0][2] + qw * GR[1][0] - 2.f * qz * GR[1][1] +
                                 qy * GR[1][2] + qx * GR[2][0] + qy * GR[2][1]);
        /* ---- 8. normalisation q^ = q/|q| ---- */
        const float dotp = ((qw * vqw + qx * vqx) + qy * vqy) + qz * vqz;
        float g0 = (vqw - qw * dotp) * inv_norm, g1 = (vqx - qx * dotp) * inv_norm;
        float g2 = (vqy - qy * dotp) * inv_norm, g3 = (vqz - qz * dotp) * inv_norm;
        if constexpr (RAW) {
            // through the getter q_a = q / n, n = max(|q|, 1e-12):  v_q = (g - q_a <q_a, g>) / n  (q_a = (q0..q3) here)
            const float d2 = ((q0 * g0 + q1 * g1) + q2 * g2) + q3 * g3;
            g0 = (g0 - q0 * d2) / raw_nrm; g1 = (g1 - q1 * d2) / raw_nrm;
            g2 = (g2 - q2 * d2) / raw_nrm; g3 = (g3 - q3 * d2) / raw_nrm;
        }
        if (w_quats) { v_quats[4 * i] = g0; v_quats[4 * i + 1] = g1; v_quats[4 * i + 2] = g2; v_quats[4 * i + 3] = g3; }
    } while (0);
#undef GAGS_PBWD_LEAVE
    if constexpr (POSE) {
        __shared__ double red[4][CALIB ? 20 : 12];
        _Pragma("unroll") for (int k = 0; k < 12; ++k) {
            const float w = gags_wave_sum(pose[k]);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = (double)w;
        }
        if constexpr (CALIB) {
            _Pragma("unroll") for (int k = 0; k < (CAM == GAGS_CAM_FISHEYE_KB ? 8 : 4); ++k) {
                const float w = gags_wave_sum(cal[k]);
                if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][12 + k] = (double)w;
            }
        }
        __syncthreads();
        if (threadIdx.x < 12) {
            const int k = threadIdx.x;
            pose_partials[(int64_t)blockIdx.x * 12 + k] = (float)(((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]);
        }
        if constexpr (CALIB) {
            const int64_t rows = gridDim.x;
            const int c = (int)threadIdx.x - 64;  // (the second wave: columns 0 .. 5 of the K row, 6 .. 9 the coefficients)
            if (c >= 0 && c < 6) {
                const int k = c == 0 ? 12 : c == 2 ? 13 : c == 4 ? 14 : c == 5 ? 15 : -1;  // (fx, 0, cx, 0, fy, cy)
                pose_partials[rows * 12 + (int64_t)blockIdx.x * 6 + c] =
                    k < 0 ? 0.f : (float)(((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]);
            }
            if constexpr (CAM == GAGS_CAM_FISHEYE_KB) {
                if (c >= 6 && c < 10) {
                    const int k = 10 + c;
                    pose_partials[rows * 18 + (int64_t)blockIdx.x * 4 + (c - 6)] =
                        (float)(((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]);
                }
            }
        }
    }
}

// Column sums of an fp32 table [n_rows, k], k <= GAGS_COLSUM_MAX_K, by ONE workgroup, in double and in a fixed order: thread t adds
// rows t, t + 256, ... in that order, the 256 per-thread sums are folded pairwise through LDS (t += t + 128, 64, ... 1).
// out[c] = (float)(sign * sum_c) for c < k, and out[k .. n_out) = 0.
constexpr int GAGS_COLSUM_MAX_K = 12;
__global__ __launch_bounds__(256) void colsum_kernel(int64_t n_rows, int k, const float *__restrict__ table, float sign,
                                                     float *__restrict__ out, int n_out)
{
    __shared__ double red[256][GAGS_COLSUM_MAX_K];
    const int t = threadIdx.x;
    double acc[GAGS_COLSUM_MAX_K];
    _Pragma("unroll") for (int c = 0; c < GAGS_COLSUM_MAX_K; ++c) acc[c] = 0.0;
    for (int64_t r = t; r < n_rows; r += 256) {
        _Pragma("unroll") for (int c = 0; c < GAGS_COLSUM_MAX_K; ++c)
            if (c < k) acc[c] += (double)table[r * k + c];
    }
    _Pragma("unroll") for (int c = 0; c < GAGS_COLSUM_MAX_K; ++c) red[t][c] = acc[c];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) { _Pragma("unroll") for (int c = 0; c < GAGS_COLSUM_MAX_K; ++c) red[t][c] += red[t + s][c]; }
        __syncthreads();
    }
    if (t < n_out) out[t] = t < k ? (float)((double)sign * red[0][t]) : 0.f;
}

// N23's second stage in ONE launch: the column sums of the three tables of a calib partials buffer -- [n_rows, 12] pose,
// [n_rows, 6] = (fx, 0, cx, 0, fy, cy), [n_rows, 4] coefficients -- each column summed exactly as colsum_kernel sums it (the same
// rows per thread in the same order, the same pairwise fold, in double), so that v_viewmat has the pose entry's bits.
// v_viewmat[16] (row 3 zeros) and v_coeffs[4] are summed and written only where given; v_K[9] always (entries 6 .. 8 zeros).
constexpr int GAGS_CALIB_COLS = 22;
__global__ __launch_bounds__(256) void calib_colsum_kernel(int64_t n_rows, const float *__restrict__ partials,
                                                           float *__restrict__ v_viewmat, float *__restrict__ v_K,
                                                           float *__restrict__ v_coeffs)
{
    __shared__ double red[256][GAGS_CALIB_COLS];
    const int t = threadIdx.x;
    const float *pose = partials, *kt = partials + n_rows * 12, *ct = partials + n_rows * 18;
    double acc[GAGS_CALIB_COLS];
    _Pragma("unroll") for (int c = 0; c < GAGS_CALIB_COLS; ++c) acc[c] = 0.0;
    for (int64_t r = t; r < n_rows; r += 256) {
        if (v_viewmat) { _Pragma("unroll") for (int c = 0; c < 12; ++c) acc[c] += (double)pose[r * 12 + c]; }
        _Pragma("unroll") for (int c = 0; c < 6; ++c) acc[12 + c] += (double)kt[r * 6 + c];
        if (v_coeffs) { _Pragma("unroll") for (int c = 0; c < 4; ++c) acc[18 + c] += (double)ct[r * 4 + c]; }
    }
    _Pragma("unroll") for (int c = 0; c < GAGS_CALIB_COLS; ++c) red[t][c] = acc[c];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) { _Pragma("unroll") for (int c = 0; c < GAGS_CALIB_COLS; ++c) red[t][c] += red[t + s][c]; }
        __syncthreads();
    }
    if (t < 16) {
        if (v_viewmat) v_viewmat[t] = t < 12 ? (float)red[0][t] : 0.f;
    } else if (t >= 64 && t < 64 + 9) {
        v_K[t - 64] = t - 64 < 6 ? (float)red[0][12 + (t - 64)] : 0.f;
    } else if (t >= 128 && t < 128 + 4) {
        if (v_coeffs) v_coeffs[t - 128] = (float)red[0][18 + (t - 128)];
    }
}

}  // namespace

namespace {

template <bool RAW, bool AA, int CAM>
int project_bwd_launch(int n, const float *means, const float *quats, const float *scales, const float *opacity_logit,
                       float scaling_modifier, const float *viewmat, const float *K, int width, int height, float eps2d,
                       const int32_t *radii, const float *v_means2d, const float *v_depths, const float *v_conics,
                       const float *v_opacities, const float *v_compensations, float *v_means, float *v_quats, float *v_scales,
                       float *v_opacity_logit, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n < 0 || width <= 0 || height <= 0) return GAGS_EINVAL;
    if (n == 0) return GAGS_OK;
    if (!means || !quats || !scales || !viewmat || !K || !radii || !v_means2d || !v_conics || !v_means || !v_quats || !v_scales)
        return GAGS_EINVAL;
    if (RAW && (v_opacity_logit || (AA && v_opacities)) && !opacity_logit) return GAGS_EINVAL;
    hipLaunchKernelGGL((project_bwd_kernel<RAW, AA, GAGS_PBWD_NONE, CAM>), dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, means,
                       quats, scales, viewmat, K, width, height, eps2d, radii, v_means2d, v_depths, v_conics, v_means, v_quats,
                       v_scales, opacity_logit, scaling_modifier, v_opacities, v_opacity_logit, v_compensations, nullptr);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

int colsum_launch(int64_t n_rows, int k, const float *table, float sign, float *out, int n_out, hipStream_t st)
{
    if (n_rows < 0 || k < 1 || k > GAGS_COLSUM_MAX_K || n_out < k || n_out > 256 || !out || (n_rows > 0 && !table))
        return GAGS_EINVAL;
    hipLaunchKernelGGL(colsum_kernel, dim3(1), dim3(256), 0, st, n_rows, k, table, sign, out, n_out);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

template <bool RAW, bool AA, int CAM>
int project_bwd_pose_launch(int n, const float *means, const float *quats, const float *scales, const float *opacity_logit,
                            float scaling_modifier, const float *viewmat, const float *K, int width, int height, float eps2d,
                            const int32_t *radii, const float *v_means2d, const float *v_depths, const float *v_conics,
                            const float *v_opacities, const float *v_compensations, float *v_means, float *v_quats,
                            float *v_scales, float *v_opacity_logit, float *v_viewmat, float *partials, hipStream_t st)
{
    const int64_t rows = n > 0 ? gags_project_pose_partials(n) : 0;
    if (n > 0) {
        if (!means || !quats || !scales || !viewmat || !K || !radii || !v_means2d || !v_conics) return GAGS_EINVAL;
        if (RAW && (v_opacity_logit || (AA && v_opacities)) && !opacity_logit) return GAGS_EINVAL;
        hipLaunchKernelGGL((project_bwd_kernel<RAW, AA, GAGS_PBWD_POSE, CAM>), dim3((unsigned)rows), dim3(256), 0, st, n, means, quats, scales,
                           viewmat, K, width, height, eps2d, radii, v_means2d, v_depths, v_conics, v_means, v_quats, v_scales,
                           opacity_logit, scaling_modifier, v_opacities, v_opacity_logit, v_compensations, partials);
        GAGS_CHECK_LAUNCH();
    }
    // second stage: the rows of `partials` in row order; entries 12 .. 15 (row 3 of the 4 x 4) are written as zeros
    return colsum_launch(rows, 12, partials, 1.0f, v_viewmat, 16, st);
}

// N23: the pose launch with the calibration sums.  partials: [rows, 12] (pose), [rows, 6] (K), [rows, 4] (coefficients), as the
// kernel lays them out; second stage: calib_colsum_kernel, one launch -- the pose rows only when v_viewmat is asked for, the K
// rows straight into the row-major 3 x 3 (entries 6 .. 8 written as zeros, 1 and 3 summed from zeros), the coefficient rows with
// GAGS_CAM_FISHEYE_KB.
template <bool RAW, bool AA, int CAM>
int project_bwd_calib_launch(int n, const float *means, const float *quats, const float *scales, const float *opacity_logit,
                             float scaling_modifier, const float *viewmat, const float *K, int width, int height, float eps2d,
                             const int32_t *radii, const float *v_means2d, const float *v_depths, const float *v_conics,
                             const float *v_opacities, const float *v_compensations, float *v_means, float *v_quats,
                             float *v_scales, float *v_opacity_logit, float *v_viewmat, float *v_K, float *v_coeffs,
                             float *partials, hipStream_t st)
{
    const int64_t rows = n > 0 ? gags_project_calib_partials(n) : 0;
    if (n > 0) {
        if (!means || !quats || !scales || !viewmat || !K || !radii || !v_means2d || !v_conics) return GAGS_EINVAL;
        if (RAW && (v_opacity_logit || (AA && v_opacities)) && !opacity_logit) return GAGS_EINVAL;
        hipLaunchKernelGGL((project_bwd_kernel<RAW, AA, GAGS_PBWD_CALIB, CAM>), dim3((unsigned)rows), dim3(256), 0, st, n, means, quats,
                           scales, viewmat, K, width, height, eps2d, radii, v_means2d, v_depths, v_conics, v_means, v_quats,
                           v_scales, opacity_logit, scaling_modifier, v_opacities, v_opacity_logit, v_compensations, partials);
        GAGS_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL(calib_colsum_kernel, dim3(1), dim3(256), 0, st, rows, partials, v_viewmat, v_K,
                       CAM == GAGS_CAM_FISHEYE_KB ? v_coeffs : nullptr);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

}  // namespace

// The four named backwards and gags_project_bwd_pose: gags_project_bwd_cam for the pinhole, likewise.
extern "C" int gags_project_bwd(int n, const float *means, const float *quats, const float *scales,
                                const float *viewmat, const float *K, int width, int height, float eps2d,
                                const int32_t *radii, const float *conics, const float *v_means2d,
                                const float *v_depths, const float *v_conics, float *v_means, float *v_quats,
                                float *v_scales, void *stream)
{
    (void)conics;  // recomputed in-kernel with the forward's operation order
    return gags_project_bwd_cam(GAGS_CAM_PINHOLE, 0, n, means, quats, scales, nullptr, 1.0f, viewmat, K, width, height, eps2d, radii,
                                v_means2d, v_depths, v_conics, nullptr, nullptr, v_means, v_quats, v_scales, nullptr, nullptr,
                                nullptr, 0, stream);
}

extern "C" int gags_project_bwd_aa(int n, const float *means, const float *quats, const float *scales,
                                   const float *viewmat, const float *K, int width, int height, float eps2d,
                                   const int32_t *radii, const float *v_means2d, const float *v_depths,
                                   const float *v_conics, const float *v_compensations, float *v_means, float *v_quats,
                                   float *v_scales, void *stream)
{
    return gags_project_bwd_cam(GAGS_CAM_PINHOLE, GAGS_PROJ_AA, n, means, quats, scales, nullptr, 1.0f, viewmat, K, width, height,
                                eps2d, radii, v_means2d, v_depths, v_conics, nullptr, v_compensations, v_means, v_quats, v_scales,
                                nullptr, nullptr, nullptr, 0, stream);
}

extern "C" int gags_project_bwd_raw(int n, const float *means, const float *rotation, const float *scaling_log,
                                    const float *opacity_logit, float scaling_modifier, const float *viewmat, const float *K,
                                    int width, int height, float eps2d, const int32_t *radii, const float *v_means2d,
                                    const float *v_depths, const float *v_conics, const float *v_opacities, float *v_means,
                                    float *v_rotation, float *v_scaling_log, float *v_opacity_logit, void *stream)
{
    return gags_project_bwd_cam(GAGS_CAM_PINHOLE, GAGS_PROJ_RAW, n, means, rotation, scaling_log, opacity_logit, scaling_modifier,
                                viewmat, K, width, height, eps2d, radii, v_means2d, v_depths, v_conics, v_opacities, nullptr,
                                v_means, v_rotation, v_scaling_log, v_opacity_logit, nullptr, nullptr, 0, stream);
}

extern "C" int gags_project_bwd_raw_aa(int n, const float *means, const float *rotation, const float *scaling_log,
                                       const float *opacity_logit, float scaling_modifier, const float *viewmat, const float *K,
                                       int width, int height, float eps2d, const int32_t *radii, const float *v_means2d,
                                       const float *v_depths, const float *v_conics, const float *v_opacities, float *v_means,
                                       float *v_rotation, float *v_scaling_log, float *v_opacity_logit, void *stream)
{
    return gags_project_bwd_cam(GAGS_CAM_PINHOLE, GAGS_PROJ_RAW | GAGS_PROJ_AA, n, means, rotation, scaling_log, opacity_logit,
                                scaling_modifier, viewmat, K, width, height, eps2d, radii, v_means2d, v_depths, v_conics,
                                v_opacities, nullptr, v_means, v_rotation, v_scaling_log, v_opacity_logit, nullptr, nullptr, 0,
                                stream);
}

// ---- N17: camera pose gradients ---------------------------------------------------------------------------------------------

extern "C" int64_t gags_project_pose_partials(int n) { return n > 0 ? ((int64_t)n + 255) / 256 : 1; }

extern "C" int gags_project_bwd_pose(int flags, int n, const float *means, const float *quats, const float *scales,
                                     const float *opacity_logit, float scaling_modifier, const float *viewmat, const float *K,
                                     int width, int height, float eps2d, const int32_t *radii, const float *v_means2d,
                                     const float *v_depths, const float *v_conics, const float *v_opacities,
                                     const float *v_compensations, float *v_means, float *v_quats, float *v_scales,
                                     float *v_opacity_logit, float *v_viewmat, float *partials, int64_t partials_bytes,
                                     void *stream)
{
    static_assert(GAGS_POSE_RAW == GAGS_PROJ_RAW && GAGS_POSE_AA == GAGS_PROJ_AA, "the pose entry hands its flags on as they are");
    if (flags & ~(GAGS_POSE_RAW | GAGS_POSE_AA)) return GAGS_EINVAL;  // (GAGS_PROJ_POSE is not a flag of this entry)
    return gags_project_bwd_cam(GAGS_CAM_PINHOLE, flags | GAGS_PROJ_POSE, n, means, quats, scales, opacity_logit, scaling_modifier,
                                viewmat, K, width, height, eps2d, radii, v_means2d, v_depths, v_conics, v_opacities,
                                v_compensations, v_means, v_quats, v_scales, v_opacity_logit, v_viewmat, partials, partials_bytes,
                                stream);
}

// ---- N20: camera models -----------------------------------------------------------------------------------------------------

namespace {

// Run-time (camera_model, flag, flag ...) to compile-time constants, once for both directions: f is called with a
// std::integral_constant for the camera model and a std::bool_constant per flag, and instantiates what it names.
template <class F>
int with_flags(F &&f) { return f(); }
template <class F, class... Bs>
int with_flags(F &&f, bool b, Bs... bs)
{
    return b ? with_flags([&](auto... cs) { return f(std::true_type{}, cs...); }, bs...)
             : with_flags([&](auto... cs) { return f(std::false_type{}, cs...); }, bs...);
}
template <class F, class... Bs>
int with_camera(int camera_model, bool kb, F &&f, Bs... bs)  // (one of the three, kb only with the fisheye: the entries have checked)
{
    if (kb)
        return with_flags([&](auto... cs) { return f(std::integral_constant<int, GAGS_CAM_FISHEYE_KB>{}, cs...); }, bs...);
    if (camera_model == GAGS_CAM_ORTHO)
        return with_flags([&](auto... cs) { return f(std::integral_constant<int, GAGS_CAM_ORTHO>{}, cs...); }, bs...);
    if (camera_model == GAGS_CAM_FISHEYE)
        return with_flags([&](auto... cs) { return f(std::integral_constant<int, GAGS_CAM_FISHEYE>{}, cs...); }, bs...);
    return with_flags([&](auto... cs) { return f(std::integral_constant<int, GAGS_CAM_PINHOLE>{}, cs...); }, bs...);
}

}  // namespace

extern "C" int gags_project_fwd_cam(int camera_model, int flags, int n, const float *means, const float *quats,
                                    const float *scales, const float *opacity_logit, float scaling_modifier, const float *viewmat,
                                    const float *K, int width, int height, float eps2d, float near_plane, float far_plane,
                                    float radius_clip, int32_t *radii, float *means2d, float *depths, float *conics,
                                    int32_t *tiles_per_gauss, float *opacities, float *quats_act, float *scales_act, void *grec,
                                    float *compensations, void *stream)
{
    GAGS_CLEAR_ERR();
    if (camera_model < GAGS_CAM_PINHOLE || camera_model > GAGS_CAM_FISHEYE || (flags & ~(GAGS_PROJ_RAW | GAGS_PROJ_AA | GAGS_PROJ_KB)))
        return GAGS_EINVAL;
    const bool raw = flags & GAGS_PROJ_RAW, aa = flags & GAGS_PROJ_AA, kb = flags & GAGS_PROJ_KB;
    if (kb && camera_model != GAGS_CAM_FISHEYE) return GAGS_EINVAL;  // (the coefficients are the fisheye's)
    // what a variant does not read is ignored
    if (!raw) { opacity_logit = nullptr; scaling_modifier = 1.0f; opacities = nullptr; quats_act = nullptr; scales_act = nullptr; grec = nullptr; }
    if (!aa) compensations = nullptr;
    return with_camera(camera_model, kb, [&](auto CAM, auto RAW, auto AA) {
        return project_fwd_launch<RAW.value, AA.value, CAM.value>(
            n, means, quats, scales, opacity_logit, scaling_modifier, viewmat, K, width, height, eps2d, near_plane, far_plane,
            radius_clip, radii, means2d, depths, conics, tiles_per_gauss, opacities, quats_act, scales_act, grec, compensations,
            stream);
    }, raw, aa);
}

extern "C" int gags_project_bwd_cam(int camera_model, int flags, int n, const float *means, const float *quats,
                                    const float *scales, const float *opacity_logit, float scaling_modifier, const float *viewmat,
                                    const float *K, int width, int height, float eps2d, const int32_t *radii,
                                    const float *v_means2d, const float *v_depths, const float *v_conics, const float *v_opacities,
                                    const float *v_compensations, float *v_means, float *v_quats, float *v_scales,
                                    float *v_opacity_logit, float *v_viewmat, float *partials, int64_t partials_bytes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (camera_model < GAGS_CAM_PINHOLE || camera_model > GAGS_CAM_FISHEYE ||
        (flags & ~(GAGS_PROJ_RAW | GAGS_PROJ_AA | GAGS_PROJ_POSE | GAGS_PROJ_KB)))
        return GAGS_EINVAL;
    const bool raw = flags & GAGS_PROJ_RAW, aa = flags & GAGS_PROJ_AA, pose = flags & GAGS_PROJ_POSE, kb = flags & GAGS_PROJ_KB;
    if (kb && camera_model != GAGS_CAM_FISHEYE) return GAGS_EINVAL;
    if (n < 0 || width <= 0 || height <= 0) return GAGS_EINVAL;
    // (a short partials buffer would be written out of bounds: refused before anything is launched)
    if (pose && (!v_viewmat || !partials || partials_bytes < gags_project_pose_partials(n) * 12 * (int64_t)sizeof(float)))
        return GAGS_EINVAL;
    if (!raw) { opacity_logit = nullptr; scaling_modifier = 1.0f; v_opacities = nullptr; v_opacity_logit = nullptr; }
    if (raw || !aa) v_compensations = nullptr;
    return with_camera(camera_model, kb, [&](auto CAM, auto RAW, auto AA, auto POSE) {
        if constexpr (POSE.value)
            return project_bwd_pose_launch<RAW.value, AA.value, CAM.value>(
                n, means, quats, scales, opacity_logit, scaling_modifier, viewmat, K, width, height, eps2d, radii, v_means2d,
                v_depths, v_conics, v_opacities, v_compensations, v_means, v_quats, v_scales, v_opacity_logit, v_viewmat, partials,
                (hipStream_t)stream);
        else
            return project_bwd_launch<RAW.value, AA.value, CAM.value>(
                n, means, quats, scales, opacity_logit, scaling_modifier, viewmat, K, width, height, eps2d, radii, v_means2d,
                v_depths, v_conics, v_opacities, v_compensations, v_means, v_quats, v_scales, v_opacity_logit, stream);
    }, raw, aa, pose);
}

// ---- N23: intrinsics gradients ----------------------------------------------------------------------------------------------

extern "C" int64_t gags_project_calib_partials(int n) { return gags_project_pose_partials(n); }

extern "C" int gags_project_bwd_calib(int camera_model, int flags, int n, const float *means, const float *quats,
                                      const float *scales, const float *opacity_logit, float scaling_modifier, const float *viewmat,
                                      const float *K, int width, int height, float eps2d, const int32_t *radii,
                                      const float *v_means2d, const float *v_depths, const float *v_conics,
                                      const float *v_opacities, const float *v_compensations, float *v_means, float *v_quats,
                                      float *v_scales, float *v_opacity_logit, float *v_viewmat, float *v_K, float *v_coeffs,
                                      float *partials, int64_t partials_bytes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (camera_model < GAGS_CAM_PINHOLE || camera_model > GAGS_CAM_FISHEYE ||
        (flags & ~(GAGS_PROJ_RAW | GAGS_PROJ_AA | GAGS_PROJ_POSE | GAGS_PROJ_KB)))
        return GAGS_EINVAL;
    const bool raw = flags & GAGS_PROJ_RAW, aa = flags & GAGS_PROJ_AA, pose = flags & GAGS_PROJ_POSE, kb = flags & GAGS_PROJ_KB;
    if (kb && camera_model != GAGS_CAM_FISHEYE) return GAGS_EINVAL;
    if (n < 0 || width <= 0 || height <= 0) return GAGS_EINVAL;
    // (a short partials buffer would be written out of bounds: refused before anything is launched)
    if (!v_K || (kb && !v_coeffs) || (pose && !v_viewmat) || !partials ||
        partials_bytes < gags_project_calib_partials(n) * GAGS_CALIB_PARTIAL_FLOATS * (int64_t)sizeof(float))
        return GAGS_EINVAL;
    if (!raw) { opacity_logit = nullptr; scaling_modifier = 1.0f; v_opacities = nullptr; v_opacity_logit = nullptr; }
    if (raw || !aa) v_compensations = nullptr;
    if (!pose) v_viewmat = nullptr;  // (not asked for: not stored)
    return with_camera(camera_model, kb, [&](auto CAM, auto RAW, auto AA) {
        return project_bwd_calib_launch<RAW.value, AA.value, CAM.value>(
            n, means, quats, scales, opacity_logit, scaling_modifier, viewmat, K, width, height, eps2d, radii, v_means2d, v_depths,
            v_conics, v_opacities, v_compensations, v_means, v_quats, v_scales, v_opacity_logit, v_viewmat, v_K, v_coeffs, partials,
            (hipStream_t)stream);
    }, raw, aa);
}

extern "C" int gags_colsum_f32(int64_t n_rows, int k, const float *table, float sign, float *out, int n_out, void *stream)
{
    GAGS_CLEAR_ERR();
    return colsum_launch(n_rows, k, table, sign, out, n_out, (hipStream_t)stream);
}
