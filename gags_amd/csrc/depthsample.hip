// N6 (include/gags_next.h): depth_SAM.py -- the point-to-pixel min-depth mapping of the GAS stage -- on the GPU.
//
// For every Gaussian centre and every training camera one decision (ds_decide, steps 1-5 of the rule in gags_next.h, all
// fp32 with no FMA and IEEE division): project, round half to even, keep what lands inside the image and agrees with the
// rendered depth there.  Every kernel calls that one function, so a decision is bit-identical wherever it is made.
//
// (a) map pass: one thread per point, the cameras in chunks whose depth maps fit the 256 MiB Infinity Cache together (16
//     maps at 1080p); the thread keeps the running min of the rendered depth D_c[v, u] over the cameras that see it in a
//     register and writes min_depth once per chunk (a read-modify-write by the owning thread: no atomics).  Optionally the
//     dense mapping [N, C, 2] (v, u) and visible [N, C] that preprocess.py --pcd_mindepth_mode reads.
// (b) scatter pass: one thread per (point, camera) of a chunk re-derives the decision and takes the integer max of its
//     point index into the camera's winner map (scratch, -1 = none); a per-pixel finalise writes
//     samples = winner >= 0 ? min_depth[winner] : 0.  The max is order-independent: bit-reproducible, and the highest
//     point index wins a pixel several points land on (the reference's single-threaded index_put_).
// Offsets into the dense outputs and the [C, H, W] maps are 64-bit.  Every depth read and every map write sits behind
// the inside test (ds_visible).
//
// N22 (gags_next.h): the same two passes for a rig of any camera models.  ds_decide_cam is ds_decide with step 2 and the
// position culls of the camera's model; an all-pinhole rig runs the N6 kernels on the N6 block, any other rig the *_rig
// kernels (the same bodies, the general decision) on a widened block that carries the coefficients and the model id.
#include <algorithm>
#include <cmath>
#include "common.h"
#include "gags_next.h"
#include "launch.h"

namespace {

constexpr int CAM_FLOATS = 16;                      // rows 0..2 of the world-to-camera matrix, fx, fy, cx, cy
// N22, a rig with a non-pinhole camera: the widened block = the 16 floats, k1 .. k4, the model id (its bits), padding
constexpr int CAM_KB = 16, CAM_MODEL = 20, RIG_FLOATS = 24;
constexpr int MAX_CHUNK = 64;                       // cameras per launch (LDS: 64 x 64 B, 64 x 96 B for the widened block)
constexpr int64_t CACHE_BUDGET = 128ll << 20;       // depth maps (and winner maps) per chunk: 16 at 1920 x 1080

struct Pix {
    int v, u;
    float d;  // D_c[v, u]
};

// Step 1 of the rule: the camera-space point.
__device__ __forceinline__ void ds_cam_space(const float *__restrict__ cam, float x, float y, float z, float &xc, float &yc,
                                             float &zc)
{
    xc = cam[0] * x;
    xc = xc + cam[1] * y;
    xc = xc + cam[2] * z;
    xc = xc + cam[3];
    yc = cam[4] * x;
    yc = yc + cam[5] * y;
    yc = yc + cam[6] * z;
    yc = yc + cam[7];
    zc = cam[8] * x;
    zc = zc + cam[9] * y;
    zc = zc + cam[10] * z;
    zc = zc + cam[11];
}

// Steps 3-5 of the rule on the projected (u, v): true when the point is inside and agrees with the rendered depth; then p
// holds (v, u) and the depth read there.  No depth is read unless the pixel is inside.
__device__ __forceinline__ bool ds_visible(float u, float v, float zc, int w, int h, float cut, float vis_thresh,
                                           const float *__restrict__ depth, Pix &p)
{
    const float ur = __builtin_rintf(u), vr = __builtin_rintf(v);  // half to even (torch.round)
    // in float, before any conversion: NaN fails every comparison, and so does anything past the int32 range
    const bool inside = ur >= cut && ur < (float)w - cut && vr >= cut && vr < (float)h - cut;
    if (!inside) return false;
    p.u = (int)ur;
    p.v = (int)vr;
    p.d = depth[(int64_t)p.v * w + p.u];
    return fabsf(p.d - zc) <= vis_thresh * p.d;
}

// Steps 1-5 of the rule for a pinhole camera (N6).
__device__ __forceinline__ bool ds_decide(const float *__restrict__ cam, float x, float y, float z, int w, int h, float cut,
                                          float vis_thresh, const float *__restrict__ depth, Pix &p)
{
    float xc, yc, zc;
    ds_cam_space(cam, x, y, z, xc, yc, zc);
    float u = xc * cam[12];
    u = u / zc;
    u = u + cam[14];
    float v = yc * cam[13];
    v = v / zc;
    v = v + cam[15];
    return ds_visible(u, v, zc, w, h, cut, vis_thresh, depth, p);
}

// N22: steps 1-5 for a camera of any model.  cam is the widened block: the 16 floats above, k1 .. k4 (zero unless the camera
// is a fisheye with coefficients) and the model id.  Only step 2 and the position culls depend on the model, and the model
// is the same for every lane of a wave (the map pass walks the cameras in step, the scatter pass has one camera per block).
__device__ __forceinline__ bool ds_decide_cam(const float *__restrict__ cam, float x, float y, float z, int w, int h, float cut,
                                              float vis_thresh, const float *__restrict__ depth, Pix &p)
{
    const int model = __float_as_int(cam[CAM_MODEL]);
    if (model == GAGS_CAM_PINHOLE) return ds_decide(cam, x, y, z, w, h, cut, vis_thresh, depth, p);
    float xc, yc, zc;
    ds_cam_space(cam, x, y, z, xc, yc, zc);
    bool keep = zc >= 0.01f;  // render()'s near plane; NaN is outside
    float u, v;
    if (model == GAGS_CAM_ORTHO) {
        u = xc * cam[12];
        u = u + cam[14];
        v = yc * cam[13];
        v = v + cam[15];
    } else {  // the quantities of cam_fwd (project.hip)
        const Kb kb{cam[CAM_KB + 0], cam[CAM_KB + 1], cam[CAM_KB + 2], cam[CAM_KB + 3]};
        const float rho = sqrtf(xc * xc + yc * yc) + GAGS_FISHEYE_EPS;
        const float theta = atan2f(rho, zc + GAGS_FISHEYE_EPS);
        const float t = theta * theta;
        const float k = (theta * kb_P(kb, t)) / rho;
        keep = keep && !(kb_dP(kb, t) <= 0.f);  // the fold, where the projection kernel culls
        u = (cam[12] * xc) * k + cam[14];
        v = (cam[13] * yc) * k + cam[15];
    }
    if (!keep) return false;  // a culled point is outside: no depth is read
    return ds_visible(u, v, zc, w, h, cut, vis_thresh, depth, p);
}

// cam[c] = {M[0, 0..3], M[1, 0..3], M[2, 0..3], fx, fy, cx, cy} from viewmats [C, 4, 4] and Ks [C, 3, 3]
__global__ void pack_cams_kernel(int n_cams, const float *__restrict__ viewmats, const float *__restrict__ Ks,
                                 float *__restrict__ cams)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= n_cams) return;
    float *o = cams + (int64_t)c * CAM_FLOATS;
    for (int k = 0; k < 12; ++k) o[k] = viewmats[(int64_t)c * 16 + k];
    const float *K = Ks + (int64_t)c * 9;
    o[12] = K[0];
    o[13] = K[4];
    o[14] = K[2];
    o[15] = K[5];
}

// The model ids of up to 64 cameras, by value: the caller's host array reaches the device as a kernel argument.
struct CamIds {
    uint32_t word[MAX_CHUNK / 4];  // four ids per word
};

// The widened block of cameras c0 .. c0 + nc - 1 (one thread each): pack_cams_kernel's 16 floats, then k1 .. k4 -- read from
// radial_coeffs [C, 4] for a fisheye camera only, zero otherwise and when radial_coeffs is NULL -- and the model id.
__global__ void pack_rig_kernel(int c0, int nc, CamIds ids, const float *__restrict__ viewmats, const float *__restrict__ Ks,
                                const float *__restrict__ radial_coeffs, float *__restrict__ cams)
{
    const int cc = threadIdx.x;
    if (cc >= nc) return;
    uint32_t word = 0;
#pragma unroll
    for (int k = 0; k < MAX_CHUNK / 4; ++k) word = (cc >> 2) == k ? ids.word[k] : word;  // (constant indices: no private copy)
    const int model = (int)((word >> ((cc & 3) * 8)) & 0xffu);
    const int64_t c = (int64_t)c0 + cc;
    float *o = cams + c * RIG_FLOATS;
    for (int k = 0; k < 12; ++k) o[k] = viewmats[c * 16 + k];
    const float *K = Ks + c * 9;
    o[12] = K[0];
    o[13] = K[4];
    o[14] = K[2];
    o[15] = K[5];
    const bool kb = model == GAGS_CAM_FISHEYE && radial_coeffs;
    for (int k = 0; k < 4; ++k) o[CAM_KB + k] = kb ? radial_coeffs[c * 4 + k] : 0.f;
    o[CAM_MODEL] = __int_as_float(model);
    for (int k = CAM_MODEL + 1; k < RIG_FLOATS; ++k) o[k] = 0.f;
}

// RIG: the widened block and the decision of any model; otherwise N6's block and decision.
template <bool RIG>
__device__ __forceinline__ bool decide(const float *__restrict__ cam, float x, float y, float z, int w, int h, float cut,
                                       float vis_thresh, const float *__restrict__ depth, Pix &p)
{
    if constexpr (RIG) return ds_decide_cam(cam, x, y, z, w, h, cut, vis_thresh, depth, p);
    else return ds_decide(cam, x, y, z, w, h, cut, vis_thresh, depth, p);
}

template <bool RIG>
__device__ __forceinline__ void map_body(int64_t n, int n_cams, int c0, int nc, int w, int h, float cut, float vis_thresh,
                                         const float *__restrict__ xyz, const float *__restrict__ cams,
                                         const float *__restrict__ depths, float *__restrict__ min_depth,
                                         int2 *__restrict__ mapping, unsigned char *__restrict__ visible, float *lcam)
{
    constexpr int FLOATS = RIG ? RIG_FLOATS : CAM_FLOATS;
    for (int k = threadIdx.x; k < nc * FLOATS; k += 256) lcam[k] = cams[(int64_t)c0 * FLOATS + k];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float x = xyz[i * 3 + 0], y = xyz[i * 3 + 1], z = xyz[i * 3 + 2];
    const int64_t hw = (int64_t)h * w;
    float m = c0 == 0 ? INFINITY : min_depth[i];
    for (int cc = 0; cc < nc; ++cc) {
        const int64_t c = c0 + cc;
        Pix p;
        const bool vis = decide<RIG>(lcam + cc * FLOATS, x, y, z, w, h, cut, vis_thresh, depths + c * hw, p);
        if (vis) m = p.d < m ? p.d : m;
        if (mapping) mapping[i * n_cams + c] = vis ? make_int2(p.v, p.u) : make_int2(0, 0);
        if (visible) visible[i * n_cams + c] = vis ? 1 : 0;
    }
    min_depth[i] = m;
}

__global__ __launch_bounds__(256) void map_kernel(int64_t n, int n_cams, int c0, int nc, int w, int h, float cut,
                                                  float vis_thresh, const float *__restrict__ xyz,
                                                  const float *__restrict__ cams, const float *__restrict__ depths,
                                                  float *__restrict__ min_depth, int2 *__restrict__ mapping,
                                                  unsigned char *__restrict__ visible)
{
    __shared__ float lcam[MAX_CHUNK * CAM_FLOATS];
    map_body<false>(n, n_cams, c0, nc, w, h, cut, vis_thresh, xyz, cams, depths, min_depth, mapping, visible, lcam);
}

__global__ __launch_bounds__(256) void map_rig_kernel(int64_t n, int n_cams, int c0, int nc, int w, int h, float cut,
                                                      float vis_thresh, const float *__restrict__ xyz,
                                                      const float *__restrict__ cams, const float *__restrict__ depths,
                                                      float *__restrict__ min_depth, int2 *__restrict__ mapping,
                                                      unsigned char *__restrict__ visible)
{
    __shared__ float lcam[MAX_CHUNK * RIG_FLOATS];
    map_body<true>(n, n_cams, c0, nc, w, h, cut, vis_thresh, xyz, cams, depths, min_depth, mapping, visible, lcam);
}

// winner[cc][v, u] = max point index that camera c0 + cc sees at (v, u); blockIdx.y = cc
template <bool RIG>
__device__ __forceinline__ void scatter_body(int64_t n, int c0, int w, int h, float cut, float vis_thresh,
                                             const float *__restrict__ xyz, const float *__restrict__ cams,
                                             const float *__restrict__ depths, int *__restrict__ winner)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int cc = blockIdx.y;
    const int64_t c = c0 + cc, hw = (int64_t)h * w;
    Pix p;
    if (decide<RIG>(cams + c * (RIG ? RIG_FLOATS : CAM_FLOATS), xyz[i * 3 + 0], xyz[i * 3 + 1], xyz[i * 3 + 2], w, h, cut,
                    vis_thresh, depths + c * hw, p))
        atomicMax(winner + cc * hw + (int64_t)p.v * w + p.u, (int)i);
}

__global__ __launch_bounds__(256) void scatter_kernel(int64_t n, int c0, int w, int h, float cut, float vis_thresh,
                                                      const float *__restrict__ xyz, const float *__restrict__ cams,
                                                      const float *__restrict__ depths, int *__restrict__ winner)
{
    scatter_body<false>(n, c0, w, h, cut, vis_thresh, xyz, cams, depths, winner);
}

__global__ __launch_bounds__(256) void scatter_rig_kernel(int64_t n, int c0, int w, int h, float cut, float vis_thresh,
                                                          const float *__restrict__ xyz, const float *__restrict__ cams,
                                                          const float *__restrict__ depths, int *__restrict__ winner)
{
    scatter_body<true>(n, c0, w, h, cut, vis_thresh, xyz, cams, depths, winner);
}

__global__ __launch_bounds__(256) void finalise_kernel(int c0, int64_t hw, const int *__restrict__ winner,
                                                       const float *__restrict__ min_depth, float *__restrict__ samples)
{
    const int64_t px = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (px >= hw) return;
    const int cc = blockIdx.y;
    const int wi = winner[cc * hw + px];
    samples[(c0 + cc) * hw + px] = wi >= 0 ? min_depth[wi] : 0.f;
}

// cameras per launch: their depth maps (and the scatter's winner maps) within CACHE_BUDGET, at least 1
inline int chunk_cams(int n_cams, int h, int w)
{
    const int64_t per = (int64_t)h * w * 4;
    return (int)std::max<int64_t>(1, std::min<int64_t>({(int64_t)n_cams, (int64_t)MAX_CHUNK, CACHE_BUDGET / per}));
}

bool bad_sizes(int64_t n, int n_cams, int h, int w, int cut_bound)
{
    // h, w < 2^24: exact as floats, so the inside test in float bounds every index
    return n < 0 || n >= INT32_MAX || n_cams < 1 || h < 1 || w < 1 || h >= (1 << 24) || w >= (1 << 24) ||
           (int64_t)h * w > INT32_MAX || cut_bound < 0;
}

// packed camera constants, one chunk's winner maps (base NULL: sizes only)
struct Scratch {
    float *cams;
    int *winner;
    int64_t total;
};

// cam_floats per camera: CAM_FLOATS for the N6 entries, RIG_FLOATS for the rig entries (whatever the rig's models)
Scratch carve(void *base, int n_cams, int h, int w, int cam_floats)
{
    GagsCarve c(base);
    Scratch L;
    L.cams = c.take<float>((int64_t)n_cams * cam_floats);
    L.winner = c.take<int>((int64_t)chunk_cams(n_cams, h, w) * h * w);
    L.total = c.total();
    return L;
}

// The cameras of a call.  models NULL: all pinhole (the N6 entries, and a rig entry given NULL).  general: some camera is
// not a pinhole, and the widened block and the rig kernels run; otherwise the N6 kernels on the N6 block.
struct Rig {
    const int32_t *models;  // host, n_cams ids, or NULL
    const float *coeffs;    // device [n_cams, 4], or NULL
    int cam_floats;         // of the scratch layout
    bool general;
};

// false: an id outside the three models
bool read_rig(int n_cams, const int32_t *cam_models, const float *radial_coeffs, Rig &rig)
{
    rig = Rig{cam_models, radial_coeffs, RIG_FLOATS, false};
    if (!cam_models) return true;
    for (int c = 0; c < n_cams; ++c) {
        if (cam_models[c] < GAGS_CAM_PINHOLE || cam_models[c] > GAGS_CAM_FISHEYE) return false;
        rig.general = rig.general || cam_models[c] != GAGS_CAM_PINHOLE;
    }
    return true;
}

// the camera blocks of the whole rig into L.cams
void pack_rig(int n_cams, const float *viewmats, const float *Ks, const Rig &rig, float *cams, hipStream_t st)
{
    if (!rig.general) {
        hipLaunchKernelGGL(pack_cams_kernel, dim3((n_cams + 63) / 64), dim3(64), 0, st, n_cams, viewmats, Ks, cams);
        return;
    }
    for (int c0 = 0; c0 < n_cams; c0 += MAX_CHUNK) {
        const int nc = std::min(MAX_CHUNK, n_cams - c0);
        CamIds ids = {};
        for (int cc = 0; cc < nc; ++cc) ids.word[cc >> 2] |= (uint32_t)rig.models[c0 + cc] << ((cc & 3) * 8);
        hipLaunchKernelGGL(pack_rig_kernel, dim3(1), dim3(MAX_CHUNK), 0, st, c0, nc, ids, viewmats, Ks, rig.coeffs, cams);
    }
}

// The one driver of the map pass: the N6 entry and the rig entry differ in `rig` alone.
int map_driver(int64_t n, int n_cams, int h, int w, const float *xyz, const float *viewmats, const float *Ks, const Rig &rig,
               const float *depths, float vis_thresh, int cut_bound, float *min_depth, int32_t *mapping,
               unsigned char *visible, void *scratch, int64_t scratch_bytes, void *stream)
{
    if (n == 0) return GAGS_OK;
    if (!xyz || !viewmats || !Ks || !depths || !min_depth || !scratch) return GAGS_EINVAL;
    const Scratch L = carve(scratch, n_cams, h, w, rig.cam_floats);
    if (scratch_bytes < L.total) return GAGS_ESCRATCH;
    hipStream_t st = (hipStream_t)stream;
    float *cams = L.cams;
    pack_rig(n_cams, viewmats, Ks, rig, cams, st);
    const int chunk = chunk_cams(n_cams, h, w);
    const unsigned nb = (unsigned)((n + 255) / 256);
    for (int c0 = 0; c0 < n_cams; c0 += chunk) {
        const int nc = std::min(chunk, n_cams - c0);
        if (rig.general)
            hipLaunchKernelGGL(map_rig_kernel, dim3(nb), dim3(256), 0, st, n, n_cams, c0, nc, w, h, (float)cut_bound,
                               vis_thresh, xyz, cams, depths, min_depth, (int2 *)mapping, visible);
        else
            hipLaunchKernelGGL(map_kernel, dim3(nb), dim3(256), 0, st, n, n_cams, c0, nc, w, h, (float)cut_bound, vis_thresh,
                               xyz, cams, depths, min_depth, (int2 *)mapping, visible);
    }
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

// ... and of the scatter pass.
int scatter_driver(int64_t n, int n_cams, int h, int w, const float *xyz, const float *viewmats, const float *Ks,
                   const Rig &rig, const float *depths, float vis_thresh, int cut_bound, const float *min_depth,
                   float *samples, void *scratch, int64_t scratch_bytes, void *stream)
{
    if (!samples) return GAGS_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const int64_t hw = (int64_t)h * w;
    if (n == 0) {  // no point: every map is zero
        if (hipMemsetAsync(samples, 0, (size_t)(n_cams * hw * 4), st) != hipSuccess) return GAGS_ELAUNCH;
        return GAGS_OK;
    }
    if (!xyz || !viewmats || !Ks || !depths || !min_depth || !scratch) return GAGS_EINVAL;
    const Scratch L = carve(scratch, n_cams, h, w, rig.cam_floats);
    if (scratch_bytes < L.total) return GAGS_ESCRATCH;
    float *cams = L.cams;
    int *winner = L.winner;
    pack_rig(n_cams, viewmats, Ks, rig, cams, st);
    const int chunk = chunk_cams(n_cams, h, w);
    const unsigned nb = (unsigned)((n + 255) / 256), nbp = (unsigned)((hw + 255) / 256);
    for (int c0 = 0; c0 < n_cams; c0 += chunk) {
        const int nc = std::min(chunk, n_cams - c0);
        if (hipMemsetAsync(winner, 0xff, (size_t)(nc * hw * 4), st) != hipSuccess) return GAGS_ELAUNCH;
        if (rig.general)
            hipLaunchKernelGGL(scatter_rig_kernel, dim3(nb, nc), dim3(256), 0, st, n, c0, w, h, (float)cut_bound, vis_thresh,
                               xyz, cams, depths, winner);
        else
            hipLaunchKernelGGL(scatter_kernel, dim3(nb, nc), dim3(256), 0, st, n, c0, w, h, (float)cut_bound, vis_thresh, xyz,
                               cams, depths, winner);
        hipLaunchKernelGGL(finalise_kernel, dim3(nbp, nc), dim3(256), 0, st, c0, hw, winner, min_depth, samples);
    }
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}

const Rig N6_RIG = {nullptr, nullptr, CAM_FLOATS, false};

}  // namespace

extern "C" int64_t gags_depthsample_scratch_bytes(int64_t n, int n_cams, int h, int w)
{
    if (bad_sizes(n, n_cams, h, w, 0) || n == 0) return 0;
    return carve(nullptr, n_cams, h, w, CAM_FLOATS).total;
}

extern "C" int gags_depthsample_map(int64_t n, int n_cams, int h, int w, const float *xyz, const float *viewmats,
                                    const float *Ks, const float *depths, float vis_thresh, int cut_bound,
                                    float *min_depth, int32_t *mapping, unsigned char *visible, void *scratch,
                                    int64_t scratch_bytes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (bad_sizes(n, n_cams, h, w, cut_bound)) return GAGS_EINVAL;
    return map_driver(n, n_cams, h, w, xyz, viewmats, Ks, N6_RIG, depths, vis_thresh, cut_bound, min_depth, mapping, visible,
                      scratch, scratch_bytes, stream);
}

extern "C" int gags_depthsample_scatter(int64_t n, int n_cams, int h, int w, const float *xyz, const float *viewmats,
                                        const float *Ks, const float *depths, float vis_thresh, int cut_bound,
                                        const float *min_depth, float *samples, void *scratch, int64_t scratch_bytes,
                                        void *stream)
{
    GAGS_CLEAR_ERR();
    if (bad_sizes(n, n_cams, h, w, cut_bound)) return GAGS_EINVAL;
    return scatter_driver(n, n_cams, h, w, xyz, viewmats, Ks, N6_RIG, depths, vis_thresh, cut_bound, min_depth, samples,
                          scratch, scratch_bytes, stream);
}

// ---- N22: the same two passes for a rig of any camera models -----------------------------------------------------------------

extern "C" int64_t gags_rig_depth_scratch_bytes(int64_t n, int n_cams, int h, int w)
{
    if (bad_sizes(n, n_cams, h, w, 0) || n == 0) return 0;
    return carve(nullptr, n_cams, h, w, RIG_FLOATS).total;
}

extern "C" int gags_rig_depth_map(int64_t n, int n_cams, int h, int w, const float *xyz, const float *viewmats,
                                  const float *Ks, const int32_t *cam_models, const float *radial_coeffs, const float *depths,
                                  float vis_thresh, int cut_bound, float *min_depth, int32_t *mapping, unsigned char *visible,
                                  void *scratch, int64_t scratch_bytes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (bad_sizes(n, n_cams, h, w, cut_bound)) return GAGS_EINVAL;
    Rig rig;
    if (!read_rig(n_cams, cam_models, radial_coeffs, rig)) return GAGS_EINVAL;
    return map_driver(n, n_cams, h, w, xyz, viewmats, Ks, rig, depths, vis_thresh, cut_bound, min_depth, mapping, visible,
                      scratch, scratch_bytes, stream);
}

extern "C" int gags_rig_depth_scatter(int64_t n, int n_cams, int h, int w, const float *xyz, const float *viewmats,
                                      const float *Ks, const int32_t *cam_models, const float *radial_coeffs,
                                      const float *depths, float vis_thresh, int cut_bound, const float *min_depth,
                                      float *samples, void *scratch, int64_t scratch_bytes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (bad_sizes(n, n_cams, h, w, cut_bound)) return GAGS_EINVAL;
    Rig rig;
    if (!read_rig(n_cams, cam_models, radial_coeffs, rig)) return GAGS_EINVAL;
    return scatter_driver(n, n_cams, h, w, xyz, viewmats, Ks, rig, depths, vis_thresh, cut_bound, min_depth, samples, scratch,
                          scratch_bytes, stream);
}
