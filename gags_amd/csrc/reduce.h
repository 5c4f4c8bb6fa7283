// The small reductions several kernels of libgags_hip.so share, each defined ONCE: the 64-lane DPP sum, the order-preserving
// float <-> unsigned key and the workgroup min / max of such keys.  (The __shfl_xor / __shfl_down float and double trees of
// the decoders, the optimizer and the photometric loss are NOT here: their association order is part of the numerical
// contract -- DESIGN.md "Numerics" -- and stays next to the sum it defines.)
#pragma once
#include "common.h"

// wave64 sum on the VALU (DPP: quad swaps, half-row / row mirrors, then row broadcasts -- a pairwise tree; the total lands
// in lane 63), returned wave-uniform through readlane.  __shfl_xor goes through the LDS crossbar instead.
__device__ __forceinline__ float gags_wave_sum(float v)
{
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xB1, 0xF, 0xF, false));   // quad_perm [1,0,3,2]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x4E, 0xF, 0xF, false));   // quad_perm [2,3,0,1]
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x141, 0xF, 0xF, false));  // row_half_mirror
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x140, 0xF, 0xF, false));  // row_mirror
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x142, 0xA, 0xF, false));  // row_bcast15 into rows 1, 3
    v += __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x143, 0xC, 0xF, false));  // row_bcast31 into rows 2, 3
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// float <-> unsigned key with the same order (min / max by integer atomics: exact and order-independent)
__device__ __forceinline__ unsigned gags_f2key(float f)
{
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gags_key2f(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// min (and, with dst_max, max) of the keys of a 256-thread workgroup into *dst_min / *dst_max: a shuffle tree per wave, one
// barrier, one atomic each by thread 0.  Every thread of the workgroup calls it, once per kernel.
__device__ __forceinline__ void gags_block_minmax(unsigned kmin, unsigned kmax, unsigned *dst_min, unsigned *dst_max)
{
    __shared__ unsigned red[2][4];
    for (int off = 32; off > 0; off >>= 1) {
        kmin = min(kmin, (unsigned)__shfl_xor((int)kmin, off, 64));
        kmax = max(kmax, (unsigned)__shfl_xor((int)kmax, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = kmin; red[1][threadIdx.x >> 6] = kmax; }
    __syncthreads();
    if (threadIdx.x == 0) {
        atomicMin(dst_min, min(min(red[0][0], red[0][1]), min(red[0][2], red[0][3])));
        if (dst_max) atomicMax(dst_max, max(max(red[1][0], red[1][1]), max(red[1][2], red[1][3])));
    }
}

// wave64 min / max of an int over all lanes (a __shfl_xor butterfly: every lane holds the result)
__device__ __forceinline__ int gags_wave_min(int v)
{
    for (int off = 32; off > 0; off >>= 1) v = min(v, __shfl_xor(v, off, 64));
    return v;
}
__device__ __forceinline__ int gags_wave_max(int v)
{
    for (int off = 32; off > 0; off >>= 1) v = max(v, __shfl_xor(v, off, 64));
    return v;
}
