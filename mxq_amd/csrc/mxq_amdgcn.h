// gfx950 building blocks shared by the kernel units: vector types, buffer descriptors, the 16-byte LDS-DMA, the LDS
// swizzle of 128-byte rows, the lane id, v_and_or_b32, fp16 <-> fp32 on raw bits and the 16x16x32 MFMA of either 16-bit type.  Device code only; the host-side
// format headers (mxq_format.h, mxq_pack.h, mxq_dequant.h) do not include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;

// raw buffer descriptor of `bytes` bytes at `base` (range-checked: loads beyond it read zeros)
__device__ __forceinline__ rsrc_t make_rsrc(const void* base, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, bytes, 0x00020000);
}

// LDS-DMA through a buffer descriptor: 16 B per lane, LDS destination = wave-uniform base + 16 * lane;
// global source = descriptor base + voff (per lane) + soff (scalar); out-of-range sources deliver zeros
__device__ __forceinline__ void bufdma16(rsrc_t rsrc, uint32_t voff, uint32_t soff, void* l) {
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)l, 16, voff, soff, 0, 0);
}

// byte offset of 16-B slot `slot` (0..7) of row `row` in a [rows][64 halfs] tile
__device__ __forceinline__ int swz(int row, int slot) { return row * 128 + ((slot ^ (row & 7)) << 4); }

// (a & m) | o in one op (the mask in an SGPR, the fp16 ones in a VGPR: gfx9 VOP3 takes no literals, and left to itself
// the compiler emits v_and + v_or)
__device__ __forceinline__ uint32_t and_or(uint32_t a, uint32_t m, uint32_t o) {
    uint32_t r;
    asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "s"(m), "v"(o));
    return r;
}

__device__ __forceinline__ float h2f(uint16_t h) { return (float)__builtin_bit_cast(_Float16, h); }
__device__ __forceinline__ uint16_t f2h(float f) {
    const _Float16 h = (_Float16)f;
    return __builtin_bit_cast(uint16_t, h);
}

// fp32 -> the bits of the 16-bit element type, RNE: fp16 (BF16 = false) or bf16 (NaN stays NaN)
template <bool BF16>
__device__ __forceinline__ uint16_t f2e(float f) {
    if constexpr (BF16) {
        const __bf16 b = (__bf16)f;
        return __builtin_bit_cast(uint16_t, b);
    } else {
        return f2h(f);
    }
}

// c += a . b, one 16 x 16 x 32 MFMA on 8 fp16 (BF16 = false) or 8 bf16 values per lane (both carried as half8 bit patterns):
// v_mfma_f32_16x16x32_f16 / v_mfma_f32_16x16x32_bf16, the same rate
template <bool BF16>
__device__ __forceinline__ f32x4 mfma16x32(half8 a, half8 b, f32x4 c) {
    if constexpr (BF16)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

}   // namespace

// the lane's index in its wave, as an asm result the compiler cannot see through: nothing lane-derived is hoisted (and
// spilled) across the loops that recompute it
#define MXQ_LANE_ID(ln) asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln))
