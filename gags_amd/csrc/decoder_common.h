// What every decoder translation unit (csrc/decoder_*.hip) includes: the MFMA vector types, the 16-bit operand functions of
// csrc/half16.h under their own names, and the two helpers more than one of those files needs.  Only types and forceinline
// device functions: the files that are compiled twice (half16.h) find nothing here that could collide at link time.
#pragma once
#include "common.h"
#include "half16.h"
#include "gags_next.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef short bf16x8 __attribute__((ext_vector_type(8)));  // eight 16-bit operands of one MFMA lane, bfloat16 or half

// the 16-bit operand type (bfloat16, or IEEE half when compiled with -DGAGS_H16): csrc/half16.h
using gags_h16::h16_mfma;
using gags_h16::h16_from;
using gags_h16::h16_to;
using gags_h16::h16_pack;
using gags_h16::h16_pack_sat;
using gags_h16::h16_lo;
using gags_h16::h16_hi;

// the sum of two packed pairs: added in fp32, rounded once
__device__ __forceinline__ unsigned add_h16x2(unsigned x, unsigned y)
{
    return h16_pack(h16_lo(x) + h16_lo(y), h16_hi(x) + h16_hi(y));
}

// 16-byte non-temporal (`nt`) stores: for tensors nothing reads before the kernel ends, so that they stream past the L2
typedef unsigned nt_u32x4 __attribute__((ext_vector_type(4)));
typedef float nt_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void nt_store(uint4 *dst, uint4 v)
{
    __builtin_nontemporal_store(nt_u32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<nt_u32x4 *>(dst));
}
__device__ __forceinline__ void nt_store(float4 *dst, float4 v)
{
    __builtin_nontemporal_store(nt_f32x4{v.x, v.y, v.z, v.w}, reinterpret_cast<nt_f32x4 *>(dst));
}
