// The weight and bias gradients of the 16-bit decoder layers (gags_decoder_wgrad*): three kernels by layer shape -- narrow,
// 256 inputs, general -- each leaving one partial matrix per pixel chunk in scratch, and the fixed-order sum of those
// partials into the parameter's own shape.  The plan (which kernel, how many chunks) is the same for both operand types.
#include "decoder_common.h"
#include "launch.h"

namespace {

// Weight gradient of one layer: dW[n, k] += sum_p dz[p, n] * (a1[p, k] + a2[p, k]),  db[n] += sum_p dz[p, n].
// The contraction runs over PIXELS, the slow index of both operands, so the 32-pixel tiles are transposed on their
// way into LDS (8-byte stores of four pixels of one column) and both MFMA fragments become 16-byte rows again.
// Workgroup = (128 n) x (128 k) x (a chunk of pixels); every chunk leaves a partial matrix, summed in chunk order
// (sum_wparts_out_kernel: no atomics).
constexpr int WP = 32;          // pixels per step (8 groups of 4 x 32 groups of 4 columns = 256 threads)
constexpr int LDP2 = WP + 8;    // LDS row pitch (bf16)
constexpr int WCHUNK = 16384;   // pixels per workgroup

__global__ __launch_bounds__(256) void wgrad_bf16_kernel(int64_t P, int N, int K, const unsigned short *__restrict__ dz,
                                                         const unsigned short *__restrict__ a1,
                                                         const unsigned short *__restrict__ a2, float *__restrict__ dW,
                                                         float *__restrict__ db)
{
    __shared__ __attribute__((aligned(16))) unsigned short At[128][LDP2];  // [n][p]
    __shared__ __attribute__((aligned(16))) unsigned short Bt[128][LDP2];  // [k][p]
    __shared__ float bsh[8][128];  // bias partial sums per pixel-row group: summed in a fixed order (no atomics)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wy = wave >> 1, wx = wave & 1;
    const int n0 = blockIdx.y * 128, k0 = blockIdx.z * 128;
    const int64_t pa = (int64_t)blockIdx.x * WCHUNK, pb = min(pa + WCHUNK, P);
    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // staging: thread = 4 consecutive pixels x 4 consecutive columns; a column's four pixels go to LDS as one 8-byte
    // store (the transposition), 8 stores per thread and step instead of 32 two-byte ones
    const int sp = (tid >> 5) * 4, sc = (tid & 31) * 4;
    float bsum[4] = {0.f, 0.f, 0.f, 0.f};
    const bool do_bias = db != nullptr && blockIdx.z == 0;
    for (int64_t p0 = pa; p0 < pb; p0 += WP) {
        uint2 zr[4], xr[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t p = p0 + sp + r;
            zr[r] = xr[r] = make_uint2(0, 0);
            if (p < pb) {
                if (n0 + sc < N) zr[r] = *reinterpret_cast<const uint2 *>(dz + p * N + n0 + sc);
                if (k0 + sc < K) {
                    xr[r] = *reinterpret_cast<const uint2 *>(a1 + p * K + k0 + sc);
                    if (a2) {
                        const uint2 y = *reinterpret_cast<const uint2 *>(a2 + p * K + k0 + sc);
                        xr[r] = make_uint2(add_h16x2(xr[r].x, y.x), add_h16x2(xr[r].y, y.y));
                    }
                }
            }
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {  // column c of the thread's 4: its four pixels, packed
            auto col = [&](const uint2 (&v)[4]) {
                unsigned short e[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned wv = (c < 2) ? v[r].x : v[r].y;
                    e[r] = (unsigned short)((c & 1) ? (wv >> 16) : (wv & 0xffff));
                }
                return make_uint2((unsigned)e[0] | ((unsigned)e[1] << 16), (unsigned)e[2] | ((unsigned)e[3] << 16));
            };
            const uint2 zc = col(zr), xc = col(xr);
            *reinterpret_cast<uint2 *>(&At[sc + c][sp]) = zc;
            *reinterpret_cast<uint2 *>(&Bt[sc + c][sp]) = xc;
            if (do_bias)
                bsum[c] += (h16_to((unsigned short)(zc.x & 0xffff)) + h16_to((unsigned short)(zc.x >> 16))) +
                           (h16_to((unsigned short)(zc.y & 0xffff)) + h16_to((unsigned short)(zc.y >> 16)));
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < WP; ks += 16) {
            bf16x8 af[2], bf[2];
#pragma unroll
            for (int i = 0; i < 2; ++i)
                af[i] = *reinterpret_cast<const bf16x8 *>(&At[wy * 64 + i * 32 + (lane & 31)][ks + 8 * (lane >> 5)]);
#pragma unroll
            for (int j = 0; j < 2; ++j)
                bf[j] = *reinterpret_cast<const bf16x8 *>(&Bt[wx * 64 + j * 32 + (lane & 31)][ks + 8 * (lane >> 5)]);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
                    acc[i][j] = h16_mfma(af[i], bf[j], acc[i][j]);
        }
        __syncthreads();
    }
    // accumulator: column = lane & 31 -> k, rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -> n
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int k = k0 + wx * 64 + j * 32 + (lane & 31);
            if (k >= K) continue;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wy * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (n < N) dW[((size_t)blockIdx.x * N + n) * K + k] = acc[i][j][r];  // this pixel chunk's partial matrix
            }
        }
    if (db != nullptr && blockIdx.z == 0) {  // (uniform over the workgroup)
#pragma unroll
        for (int c = 0; c < 4; ++c) bsh[tid >> 5][sc + c] = bsum[c];
        __syncthreads();
        if (tid < 128 && n0 + tid < N) {
            float t = 0.f;
#pragma unroll
            for (int q = 0; q < 8; ++q) t += bsh[q][tid];
            db[(size_t)blockIdx.x * N + n0 + tid] = t;
        }
    }
}

// Weight gradient for the 256-input layers (8 of CNN_decoder's 9): workgroup = 128 outputs (n) x all 256 inputs (k)
// x a chunk of pixels.  Both operands stay PIXEL-major in LDS exactly as they sit in memory (16-byte loads, 16-byte
// LDS writes, no shuffling in registers) and the MFMA fragments, which want eight consecutive PIXELS of one channel
// per lane, come out of gfx950's transposing LDS read: ds_read_b64_tr_b16 hands lane l of a 16-lane group the four
// rows of column l of a [4 pixels][16 channels] block.  Row pitches of 64 B mod 256 B put the four pixel rows of a
// read on four different quarters of the 64 banks.  The LDS image is double-buffered (one barrier per 32-pixel
// step) and the operands of the step after next are in flight in registers meanwhile; two workgroups per CU.
struct GagsTrue { static constexpr bool value = true; };
struct GagsFalse { static constexpr bool value = false; };
constexpr int W2P = 32;                       // pixels per step
constexpr int W2ZP = 128 * 2 + 64;            // bytes per pixel row, dz image (128 channels)
constexpr int W2XP = 256 * 2 + 64;            // bytes per pixel row, activation image (256 channels)
typedef short v4s __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) v4s *lds_v4s;

template <bool TWO>
__global__ __launch_bounds__(256, 2) void wgrad256_kernel(int64_t P, int N, const unsigned short *__restrict__ dz,
                                                          const unsigned short *__restrict__ a1,
                                                          const unsigned short *__restrict__ a2, float *__restrict__ dW,
                                                          float *__restrict__ db, int64_t chunk, int n_tiles, unsigned n_chunks)
{
    constexpr int K = 256;
    __shared__ __attribute__((aligned(16))) unsigned char Zi[2][W2P * W2ZP];
    __shared__ __attribute__((aligned(16))) unsigned char Xi[2][W2P * W2XP];
    __shared__ float bsh[16][128];  // bias partial sums per pixel-row group: summed in a fixed order (no atomics)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wy = wave >> 1, wx = wave & 1;  // 2 x 2 waves: 64 n x 128 k each
    // the n tiles of one pixel chunk run back to back on the same XCD (they share the activation rows through its L2)
    unsigned ck = blockIdx.x;
    int nt = 0;
    if (n_tiles > 1) {
        const unsigned xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
        ck = (slot / n_tiles) * 8 + xcd;
        nt = slot % n_tiles;
        if (ck >= n_chunks) return;
    }
    const int n0 = nt * 128;
    const int64_t pa = (int64_t)ck * chunk, pb = min(pa + chunk, P);
    if (pa >= pb) return;
    f32x16 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // loads: dz piece tid & 15 (8 channels) of rows tid / 16 + 16 q; activation piece tid & 31 of rows tid / 32 + 8 q
    const int zc = (tid & 15) * 8, zr = tid >> 4, xc = (tid & 31) * 8, xr = tid >> 5;
    // a step that lies inside the chunk (all but the last one of the last chunk) is addressed by ONE uniform base per stream and
    // the lane's six fixed 32-bit byte offsets (round 6: the per-row form cost ~100 VALU instructions per step, quarter-rate
    // 64-bit multiplies among them, on the SIMD whose matrix pipe waits meanwhile), without clamps and without row masks
    uint4 rz[2], rx[4], rx2[TWO ? 4 : 1];
    unsigned zo[2], xo[4];
#pragma unroll
    for (int q = 0; q < 2; ++q) zo[q] = (unsigned)(((zr + 16 * q) * N + zc) * 2);
#pragma unroll
    for (int q = 0; q < 4; ++q) xo[q] = (unsigned)(((xr + 8 * q) * K + xc) * 2);
    auto fetch = [&](auto whole, int64_t p0) __attribute__((always_inline)) {
        if constexpr (decltype(whole)::value) {
            const char *zb = reinterpret_cast<const char *>(dz + p0 * N + n0), *xb = reinterpret_cast<const char *>(a1 + p0 * K);
            const char *xb2 = TWO ? reinterpret_cast<const char *>(a2 + p0 * K) : nullptr;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                unsigned o = zo[q];
                asm volatile("" : "+v"(o));  // (opaque: keeps the scalar-base + lane-offset form of the load)
                rz[q] = *reinterpret_cast<const uint4 *>(zb + o);
            }
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                unsigned o = xo[q];
                asm volatile("" : "+v"(o));
                rx[q] = *reinterpret_cast<const uint4 *>(xb + o);
                if constexpr (TWO) rx2[q] = *reinterpret_cast<const uint4 *>(xb2 + o);
            }
        } else {
#pragma unroll
            for (int q = 0; q < 2; ++q) rz[q] = *reinterpret_cast<const uint4 *>(dz + min(p0 + zr + 16 * q, pb - 1) * N + n0 + zc);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t o = min(p0 + xr + 8 * q, pb - 1) * K + xc;
                rx[q] = *reinterpret_cast<const uint4 *>(a1 + o);
                if constexpr (TWO) rx2[q] = *reinterpret_cast<const uint4 *>(a2 + o);
            }
        }
    };
    float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // (summed whether or not db is wanted: 24 instructions, no branch)
    auto commit = [&](auto whole, int buf, int64_t p0) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            uint4 v = rz[q];
            if constexpr (!decltype(whole)::value) {
                const unsigned keep = p0 + zr + 16 * q < pb ? 0xffffffffu : 0u;  // rows beyond the chunk contribute zero
                v = make_uint4(v.x & keep, v.y & keep, v.z & keep, v.w & keep);
            }
            *reinterpret_cast<uint4 *>(&Zi[buf][(zr + 16 * q) * W2ZP + zc * 2]) = v;
            bsum[0] += h16_lo(v.x); bsum[1] += h16_hi(v.x); bsum[2] += h16_lo(v.y); bsum[3] += h16_hi(v.y);
            bsum[4] += h16_lo(v.z); bsum[5] += h16_hi(v.z); bsum[6] += h16_lo(v.w); bsum[7] += h16_hi(v.w);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint4 v = rx[q];
            if constexpr (TWO)
                v = make_uint4(add_h16x2(v.x, rx2[q].x), add_h16x2(v.y, rx2[q].y), add_h16x2(v.z, rx2[q].z), add_h16x2(v.w, rx2[q].w));
            *reinterpret_cast<uint4 *>(&Xi[buf][(xr + 8 * q) * W2XP + xc * 2]) = v;  // (dz rows are zero there: no mask needed)
        }
    };
    constexpr GagsTrue yes{};
    constexpr GagsFalse no{};
    // fragment addresses of this lane inside an image (bytes): pixel row 8 (l >> 5) + ((l & 15) >> 2), channel
    // 16 ((l >> 4) & 1) + 4 (l & 3) of the 32-channel block; + 4 rows for the second half, + 16 rows for the second k step
    const int frow = 8 * (lane >> 5) + ((lane & 15) >> 2), fcol = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    const int zoff = frow * W2ZP + (wy * 64 + fcol) * 2, xoff = frow * W2XP + (wx * 128 + fcol) * 2;
    auto frag = [&](const unsigned char *base) __attribute__((always_inline)) {
        const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)base);
        return lo;
    };
    auto compute = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 af[2], bf[4];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const unsigned char *b = &Zi[buf][zoff + ks * 16 * W2ZP + i * 64];
                const v4s lo = frag(b), hi = frag(b + 4 * W2ZP);
                af[i] = bf16x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned char *b = &Xi[buf][xoff + ks * 16 * W2XP + j * 64];
                const v4s lo = frag(b), hi = frag(b + 4 * W2XP);
                bf[j] = bf16x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = h16_mfma(af[i], bf[j], acc[i][j]);
        }
    };
    const int64_t steps = (pb - pa + W2P - 1) / W2P, n_whole = (pb - pa) / W2P;
    if (n_whole > 0) fetch(yes, pa); else fetch(no, pa);
    if (n_whole > 0) commit(yes, 0, pa); else commit(no, 0, pa);
    if (n_whole > 1) fetch(yes, pa + W2P); else if (steps > 1) fetch(no, pa + W2P);
    __syncthreads();
    // step s computes on image s & 1 while the registers (step s + 1) go to the other image and are refilled for s + 2
    int64_t s = 0;
    for (; s + 2 < n_whole; ++s) {
        const int buf = (int)(s & 1);
        commit(yes, buf ^ 1, pa + (s + 1) * W2P);
        fetch(yes, pa + (s + 2) * W2P);
        compute(buf);
        gags_lds_barrier();  // (not __syncthreads(): that would land the fetch above before every step)
    }
    for (; s < steps; ++s) {  // the last two steps, and the chunk's ragged one
        const int buf = (int)(s & 1);
        if (s + 1 < steps) commit(no, buf ^ 1, pa + (s + 1) * W2P);
        if (s + 2 < steps) fetch(no, pa + (s + 2) * W2P);
        compute(buf);
        gags_lds_barrier();
    }
    // accumulator: column = lane & 31 -> k, rows (r & 3) + 8 (r >> 2) + 4 (lane >> 5) -> n; 32 lanes = 128 contiguous bytes
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = wx * 128 + j * 32 + (lane & 31);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int n = n0 + wy * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                dW[((size_t)ck * N + n) * K + k] = acc[i][j][r];  // this pixel chunk's partial matrix
            }
        }
    if (db != nullptr) {
#pragma unroll
        for (int q = 0; q < 8; ++q) bsh[zr][zc + q] = bsum[q];
        __syncthreads();
        if (tid < 128) {
            float t = 0.f;
#pragma unroll
            for (int q = 0; q < 16; ++q) t += bsh[q][tid];
            db[(size_t)ck * N + n0 + tid] = t;
        }
    }
}

// Weight gradient of the narrow layers (N = 32 NB outputs, K = 32 KB inputs, NB KB <= 8: the scale decoder and the
// first layer of CNN_decoder): the whole N x K gradient fits one wave's accumulators, so every WAVE runs its own
// pipeline over its own range of pixels -- 16 pixels per step, pixel-major rows into a wave-private LDS patch, fragments
// through the transposing read -- with no workgroup barrier anywhere (LDS executes a wave's accesses in order); the
// four waves of a workgroup are summed in LDS, in wave order, and stored as the workgroup's partial matrix (no atomics).
template <int NB, int KB, bool TWO>
__global__ __launch_bounds__(256) void wgrad_narrow_kernel(int64_t P, const unsigned short *__restrict__ dz,
                                                           const unsigned short *__restrict__ a1,
                                                           const unsigned short *__restrict__ a2, float *__restrict__ dW,
                                                           float *__restrict__ db, int64_t chunk)
{
    constexpr int N = 32 * NB, K = 32 * KB;
    constexpr int ZP = (N * 2 / 64 | 1) * 64, XP = (K * 2 / 64 | 1) * 64;  // row pitches: odd multiples of 64 B
    constexpr int PATCH = 16 * (ZP + XP);
    constexpr int RED = N * K * 4 + N * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem[(4 * PATCH > RED ? 4 * PATCH : RED)];
    __shared__ float bsh[4][64][8];  // bias partial sums per wave and lane: summed in a fixed order (no atomics)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    unsigned char *Zi = smem + wave * PATCH, *Xi = Zi + 16 * ZP;
    const int64_t pa = ((int64_t)blockIdx.x * 4 + wave) * chunk, pb = min(pa + chunk, P);
    f32x16 acc[NB][KB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = 0; j < KB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    // 16-byte pieces lane + 64 q of the 16 x (N / 8) resp. 16 x (K / 8) pieces of a step
    constexpr int ZQ = N / 32, XQ = K / 32, ZR = N / 8, XR = K / 8;
    uint4 rz[ZQ], rx[XQ], rx2[TWO ? XQ : 1];
    auto fetch = [&](int64_t p0) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < ZQ; ++q) {
            const int pc = lane + 64 * q;
            rz[q] = *reinterpret_cast<const uint4 *>(dz + min(p0 + pc / ZR, P - 1) * N + (pc % ZR) * 8);
        }
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int pc = lane + 64 * q;
            const int64_t o = min(p0 + pc / XR, P - 1) * K + (pc % XR) * 8;
            rx[q] = *reinterpret_cast<const uint4 *>(a1 + o);
            if constexpr (TWO) rx2[q] = *reinterpret_cast<const uint4 *>(a2 + o);
        }
    };
    float bsum[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // channels (lane % ZR) * 8 .. + 7 (the same for every q)
    const bool do_bias = db != nullptr;
    auto commit = [&](int64_t p0) __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < ZQ; ++q) {
            const int pc = lane + 64 * q;
            const unsigned keep = p0 + pc / ZR < pb ? 0xffffffffu : 0u;  // rows beyond the range contribute zero
            const uint4 v = make_uint4(rz[q].x & keep, rz[q].y & keep, rz[q].z & keep, rz[q].w & keep);
            *reinterpret_cast<uint4 *>(Zi + (pc / ZR) * ZP + (pc % ZR) * 16) = v;
            if (do_bias) {
                bsum[0] += h16_lo(v.x); bsum[1] += h16_hi(v.x); bsum[2] += h16_lo(v.y); bsum[3] += h16_hi(v.y);
                bsum[4] += h16_lo(v.z); bsum[5] += h16_hi(v.z); bsum[6] += h16_lo(v.w); bsum[7] += h16_hi(v.w);
            }
        }
#pragma unroll
        for (int q = 0; q < XQ; ++q) {
            const int pc = lane + 64 * q;
            uint4 v = rx[q];
            if constexpr (TWO)
                v = make_uint4(add_h16x2(v.x, rx2[q].x), add_h16x2(v.y, rx2[q].y), add_h16x2(v.z, rx2[q].z), add_h16x2(v.w, rx2[q].w));
            *reinterpret_cast<uint4 *>(Xi + (pc / XR) * XP + (pc % XR) * 16) = v;
        }
    };
    const int frow = 8 * (lane >> 5) + ((lane & 15) >> 2), fcol = 16 * ((lane >> 4) & 1) + 4 * (lane & 3);
    if (pa < pb) {
        fetch(pa);
        for (int64_t p0 = pa; p0 < pb; p0 += 16) {
            commit(p0);
            if (p0 + 16 < pb) fetch(p0 + 16);
            bf16x8 af[NB], bf[KB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                const unsigned char *b = Zi + frow * ZP + (i * 32 + fcol) * 2;
                const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)b), hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(b + 4 * ZP));
                af[i] = bf16x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            }
#pragma unroll
            for (int j = 0; j < KB; ++j) {
                const unsigned char *b = Xi + frow * XP + (j * 32 + fcol) * 2;
                const v4s lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)b), hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_v4s)(b + 4 * XP));
                bf[j] = bf16x8{lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
            }
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int j = 0; j < KB; ++j) acc[i][j] = h16_mfma(af[i], bf[j], acc[i][j]);
        }
    }
    // sum the four waves in LDS (the patches are done with) -- one wave at a time, in wave order, plain read-modify-
    // write: a fixed order, hence reproducible bits -- then store the workgroup's partial matrix
    __syncthreads();
    float *red = reinterpret_cast<float *>(smem);
    for (int e = tid; e < N * K; e += 256) red[e] = 0.f;
    if (do_bias) {
#pragma unroll
        for (int q = 0; q < 8; ++q) bsh[wave][lane][q] = bsum[q];
    }
    __syncthreads();
    for (int wv = 0; wv < 4; ++wv) {
        if (wave == wv) {
#pragma unroll
            for (int i = 0; i < NB; ++i)
#pragma unroll
                for (int j = 0; j < KB; ++j)
#pragma unroll
                    for (int r = 0; r < 16; ++r)
                        red[(i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * K + j * 32 + (lane & 31)] += acc[i][j][r];
        }
        __syncthreads();
    }
    for (int e = tid; e < N * K; e += 256) dW[(size_t)blockIdx.x * N * K + e] = red[e];
    if (do_bias)
        for (int c = tid; c < N; c += 256) {  // column c: lanes c / 8 + ZR m of every wave, element c % 8
            float t = 0.f;
            for (int wv = 0; wv < 4; ++wv)
                for (int l = c >> 3; l < 64; l += ZR) t += bsh[wv][l][c & 7];
            db[(size_t)blockIdx.x * N + c] = t;
        }
}

inline int64_t narrow_chunk(int64_t n_pix)
{
    const int64_t waves = 4 * 768;  // three workgroups per CU
    return ((n_pix + waves - 1) / waves + 15) / 16 * 16;
}
inline unsigned narrow_parts(int64_t n_pix) { const int64_t c = narrow_chunk(n_pix); return (unsigned)((n_pix + 4 * c - 1) / (4 * c)); }

template <int NB, int KB>
void launch_wgrad_narrow(int64_t n_pix, const void *dz, const void *a1, const void *a2, float *d_w, float *d_b, hipStream_t stream)
{
    const int64_t chunk = narrow_chunk(n_pix);
    const unsigned grid = narrow_parts(n_pix);
    if (a2)
        hipLaunchKernelGGL((wgrad_narrow_kernel<NB, KB, true>), dim3(grid), dim3(256), 0, stream, n_pix, (const unsigned short *)dz,
                           (const unsigned short *)a1, (const unsigned short *)a2, d_w, d_b, chunk);
    else
        hipLaunchKernelGGL((wgrad_narrow_kernel<NB, KB, false>), dim3(grid), dim3(256), 0, stream, n_pix, (const unsigned short *)dz,
                           (const unsigned short *)a1, (const unsigned short *)a2, d_w, d_b, chunk);
}

// out[e] = sum of the partial results over the pixel chunks, in a FIXED order (=> reproducible): sixteen groups of a
// workgroup take the chunks g, g + 16, ... of 64 consecutive elements (up to 16 loads in flight each), their sums are
// added in group order.  (One thread per element walking all 768 chunks of a narrow layer was a chain of 48 round trips:
// 17-28 us for a 4 KB matrix, 0.5 ms per iteration over the thirty sums.)
// A weight matrix AND its bias row in one launch, written in the parameter's own shape (round 6; one launch per tensor
// before): the partial matrices are [n, k] (padded to multiples of 32), the outputs out_w[co, ci] and out_b[co]; every sum is
// multiplied by scale[0] when given (the f16 tier's power of two: exact).  Blocks [0, wb) sum the matrix, the rest the bias.
__global__ __launch_bounds__(1024) void sum_wparts_out_kernel(int n_parts, int n, int k, int co, int ci, unsigned wb,
                                                              const float *__restrict__ part_w, const float *__restrict__ part_b,
                                                              float *__restrict__ out_w, float *__restrict__ out_b,
                                                              const float *__restrict__ scale)
{
    __shared__ float sm[16][64];
    const int g = threadIdx.x >> 6, l = threadIdx.x & 63;
    const bool bias = blockIdx.x >= wb;
    const int64_t n_el = bias ? co : (int64_t)co * ci, stride = bias ? n : (int64_t)n * k;
    const float *part = bias ? part_b : part_w;
    const int64_t e = (int64_t)(bias ? blockIdx.x - wb : blockIdx.x) * 64 + l;
    const int64_t ec = min(e, n_el - 1);
    const int64_t src = bias ? ec : (ec / ci) * k + ec % ci;
    float t = 0.f;
    int c = g;
    for (; c + 16 * 15 < n_parts; c += 16 * 16) {
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = part[(size_t)(c + 16 * i) * stride + src];
#pragma unroll
        for (int i = 0; i < 16; ++i) t += v[i];
    }
    for (; c < n_parts; c += 16) t += part[(size_t)c * stride + src];
    sm[g][l] = t;
    __syncthreads();
    if (g == 0 && e < n_el) {
        float r = sm[0][l];
#pragma unroll
        for (int i = 1; i < 16; ++i) r += sm[i][l];
        if (scale) r *= scale[0];
        (bias ? out_b : out_w)[e] = r;
    }
}

// which kernel serves a shape, and how many partial matrices (pixel chunks) it leaves
enum { WG_NARROW = 0, WG_256 = 1, WG_GENERAL = 2 };
inline bool narrow_shape(int n_out, int k_in)
{
    if (n_out % 32 || k_in % 32) return false;
    const int nb = n_out / 32, kb = k_in / 32;
    return (nb == 1 && (kb == 1 || kb == 2 || kb == 4 || kb == 8)) || (nb == 2 && (kb == 1 || kb == 2 || kb == 4)) ||
           (nb == 4 && (kb == 1 || kb == 2)) || (nb == 8 && kb == 1);
}
inline int64_t w256_chunk(int64_t n_pix) { return ((n_pix + 255) / 256 + W2P - 1) / W2P * W2P; }
inline int wgrad_plan(int64_t n_pix, int n_out, int k_in, int64_t &parts)
{
    if (narrow_shape(n_out, k_in)) { parts = narrow_parts(n_pix); return WG_NARROW; }
    if (k_in == 256 && n_out % 128 == 0) { const int64_t c = w256_chunk(n_pix); parts = (n_pix + c - 1) / c; return WG_256; }
    parts = (n_pix + WCHUNK - 1) / WCHUNK;
    return WG_GENERAL;
}
// bytes of the partial matrices and bias rows (what both the exported query and wgrad_impl go by)
inline int64_t wgrad_scratch_bytes(int64_t n_pix, int n_out, int k_in)
{
    if (n_pix <= 0 || n_out <= 0 || k_in <= 0) return 0;
    int64_t parts;
    wgrad_plan(n_pix, n_out, k_in, parts);
    return al256(parts * ((int64_t)n_out * k_in + n_out) * 4);
}

int wgrad_impl(int64_t n_pix, int n_out, int k_in, const void *dz, const void *a1, const void *a2, float *d_w, float *d_b, int co,
               int ci, const float *out_scale, void *scratch, int64_t scratch_bytes, void *stream)
{
    GAGS_CLEAR_ERR();
    if (n_pix < 0 || n_out <= 0 || k_in <= 0 || n_out % 16 != 0 || k_in % 16 != 0 || !dz || !a1 || !d_w || co <= 0 || ci <= 0 ||
        co > n_out || ci > k_in)
        return GAGS_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n_pix == 0) {
        if (hipMemsetAsync(d_w, 0, sizeof(float) * (size_t)co * ci, st) != hipSuccess) return GAGS_ELAUNCH;
        if (d_b && hipMemsetAsync(d_b, 0, sizeof(float) * (size_t)co, st) != hipSuccess) return GAGS_ELAUNCH;
        return GAGS_OK;
    }
    if (!scratch || scratch_bytes < wgrad_scratch_bytes(n_pix, n_out, k_in)) return GAGS_ESCRATCH;
    int64_t parts;
    const int plan = wgrad_plan(n_pix, n_out, k_in, parts);
    // every pixel chunk leaves a partial matrix (and bias row) in scratch; they are summed in chunk order: no atomics
    float *pw = (float *)scratch, *pb = d_b ? pw + (size_t)parts * n_out * k_in : nullptr;
    if (plan == WG_NARROW) {
        const int nb = n_out / 32, kb = k_in / 32;
        if (false) {}
#define GAGS_NARROW(NB_, KB_) else if (nb == NB_ && kb == KB_) launch_wgrad_narrow<NB_, KB_>(n_pix, dz, a1, a2, pw, pb, st);
        GAGS_NARROW(1, 1) GAGS_NARROW(2, 1) GAGS_NARROW(1, 2) GAGS_NARROW(2, 2) GAGS_NARROW(4, 1) GAGS_NARROW(1, 4)
        GAGS_NARROW(4, 2) GAGS_NARROW(2, 4) GAGS_NARROW(8, 1) GAGS_NARROW(1, 8)
#undef GAGS_NARROW
    } else if (plan == WG_256) {
        // one workgroup per n tile and pixel chunk, two per CU: 512 chunks of whole 32-pixel steps
        const int n_tiles = n_out / 128;
        const int64_t chunk = w256_chunk(n_pix);
        const unsigned n_chunks = (unsigned)parts;
        const unsigned grid = n_tiles == 1 ? n_chunks : (n_chunks + 7) / 8 * 8 * n_tiles;
        if (a2)
            hipLaunchKernelGGL(wgrad256_kernel<true>, dim3(grid), dim3(256), 0, st, n_pix, n_out, (const unsigned short *)dz,
                               (const unsigned short *)a1, (const unsigned short *)a2, pw, pb, chunk, n_tiles, n_chunks);
        else
            hipLaunchKernelGGL(wgrad256_kernel<false>, dim3(grid), dim3(256), 0, st, n_pix, n_out, (const unsigned short *)dz,
                               (const unsigned short *)a1, (const unsigned short *)a2, pw, pb, chunk, n_tiles, n_chunks);
    } else {
        hipLaunchKernelGGL(wgrad_bf16_kernel, dim3((unsigned)parts, (unsigned)((n_out + 127) / 128), (unsigned)((k_in + 127) / 128)),
                           dim3(256), 0, st, n_pix, n_out, k_in, (const unsigned short *)dz, (const unsigned short *)a1,
                           (const unsigned short *)a2, pw, pb);
    }
    // one launch sums the matrix and the bias row, in the caller's [co, ci] shape
    const unsigned wb = (unsigned)(((int64_t)co * ci + 63) / 64), bb = d_b ? (unsigned)((co + 63) / 64) : 0u;
    hipLaunchKernelGGL(sum_wparts_out_kernel, dim3(wb + bb), dim3(1024), 0, st, (int)parts, n_out, k_in, co, ci, wb, pw, pb, d_w, d_b,
                       out_scale);
    GAGS_CHECK_LAUNCH();
    return GAGS_OK;
}
}  // namespace

extern "C" int64_t GAGS_DEC(gags_decoder_wgrad_scratch_bytes)(int64_t n_pix, int n_out, int k_in)
{
    return wgrad_scratch_bytes(n_pix, n_out, k_in);
}

extern "C" int GAGS_DEC(gags_decoder_wgrad)(int64_t n_pix, int n_out, int k_in, const void *dz, const void *a1, const void *a2,
                                  float *d_w, float *d_b, void *scratch, int64_t scratch_bytes, void *stream)
{
    return wgrad_impl(n_pix, n_out, k_in, dz, a1, a2, d_w, d_b, n_out, k_in, nullptr, scratch, scratch_bytes, stream);
}

extern "C" int GAGS_DEC(gags_decoder_wgrad_out)(int64_t n_pix, int n_out, int k_in, const void *dz, const void *a1, const void *a2,
                                      float *d_w, float *d_b, int co, int ci, const float *out_scale, void *scratch,
                                      int64_t scratch_bytes, void *stream)
{
    return wgrad_impl(n_pix, n_out, k_in, dz, a1, a2, d_w, d_b, co, ci, out_scale, scratch, scratch_bytes, stream);
}
