// Register-level dequantisation helpers (packed codes -> fp16 pairs), bit-exact with the
// reference's fp32 formula  w' = scale * (q - zero)  rounded once to fp16
// (reference mxq_quant/lib/quantizer.py:19-20, mxqgpt.py:448), where
// scale = qs * (scale_code - qz) (quantizer.py:121).  The same helpers with BF16 = true round that
// fp32 value once to bf16 instead (the write-back into a bf16 layer, mxqgpt.py:448): the LUT and the
// byte selections do not depend on the 16-bit element type, only the pack does.
//
// A 2-bit group has only four possible values, so it is dequantised through a 4-entry
// fp16 LUT computed in fp32 and selected with v_perm_b32 on the
// byte-spread code word (mxq_format.h): ~2.3 VALU ops per weight instead of ~4.5.
// The 4-bit arm is arithmetic: v_cvt_f32_ubyteN, sub, mul, cvt.
//
// The same inline functions compile for the host (tests/host_emu.cpp) with a software
// byte-permute so the bit manipulation is unit-tested on CPU.
#pragma once
#include "mxq_format.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define MXQ_PERM(hi, lo, sel) __builtin_amdgcn_perm((hi), (lo), (sel))
typedef _Float16 mxq_half;
MXQ_HD uint32_t mxq_pack_f16(float a, float b) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    h2 v = {(_Float16)a, (_Float16)b};   // RNE (default float mode)
    return __builtin_bit_cast(uint32_t, v);
}
MXQ_HD uint32_t mxq_pack_bf16(float a, float b) {
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    b2 v = {(__bf16)a, (__bf16)b};       // v_cvt_pk_bf16_f32: RNE, NaN stays NaN
    return __builtin_bit_cast(uint32_t, v);
}
#else
// host emulation of v_perm_b32: selector byte 0..3 -> bytes of `lo`, 4..7 -> bytes of `hi`
static inline uint32_t mxq_perm_emu(uint32_t hi, uint32_t lo, uint32_t sel) {
    uint64_t src = ((uint64_t)hi << 32) | lo;
    uint32_t out = 0;
    for (int i = 0; i < 4; ++i) {
        uint32_t s = (sel >> (8 * i)) & 0xFF;
        uint32_t b = (s < 8) ? (uint32_t)((src >> (8 * s)) & 0xFF) : (s == 0x0C ? 0u : 0xFFu);
        out |= b << (8 * i);
    }
    return out;
}
#define MXQ_PERM(hi, lo, sel) mxq_perm_emu((hi), (lo), (sel))
uint16_t mxq_host_f32_to_f16(float f);   // provided by the host harness (RNE)
MXQ_HD uint32_t mxq_pack_f16(float a, float b) {
    return (uint32_t)mxq_host_f32_to_f16(a) | ((uint32_t)mxq_host_f32_to_f16(b) << 16);
}
// fp32 -> bf16, round to nearest even; NaN stays a (quiet) NaN
static inline uint32_t mxq_host_f32_to_bf16(float f) {
    uint32_t u;
    __builtin_memcpy(&u, &f, 4);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;
    return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
MXQ_HD uint32_t mxq_pack_bf16(float a, float b) { return mxq_host_f32_to_bf16(a) | (mxq_host_f32_to_bf16(b) << 16); }
#endif
// the pair pack of the element type: fp16 (BF16 = false) or bf16
template <bool BF16>
MXQ_HD uint32_t mxq_pack16(float a, float b) {
    return BF16 ? mxq_pack_bf16(a, b) : mxq_pack_f16(a, b);
}

// scale from its 4-bit code: fp32 qs * (code - qz), one rounding per op
MXQ_HD float mxq_scale(float qs, float qz, uint32_t code) { return qs * ((float)code - qz); }

// 16 two-bit codes (byte-spread word d) -> 8 x packed fp16 (bf16) pairs, out[i] = elements (2i, 2i+1)
template <bool BF16 = false>
MXQ_HD void mxq_deq2x16(uint32_t d, float s, float z, uint32_t out[8]) {
    const uint32_t p01 = mxq_pack16<BF16>(s * (0.0f - z), s * (1.0f - z));
    const uint32_t p23 = mxq_pack16<BF16>(s * (2.0f - z), s * (3.0f - z));
    const uint32_t lut_lo = MXQ_PERM(p23, p01, 0x06040200u);   // low bytes of e0..e3
    const uint32_t lut_hi = MXQ_PERM(p23, p01, 0x07050301u);   // high bytes of e0..e3
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t m = (d >> (2 * j)) & 0x03030303u;        // codes of elements 4j..4j+3
        const uint32_t lo = MXQ_PERM(0u, lut_lo, m);
        const uint32_t hi = MXQ_PERM(0u, lut_hi, m);
        out[2 * j] = MXQ_PERM(hi, lo, 0x05010400u);
        out[2 * j + 1] = MXQ_PERM(hi, lo, 0x07030602u);
    }
}

// ... and one half of them: elements 8h .. 8h+7 -> 4 x packed fp16 pairs (the same LUT, the same selections)
template <bool BF16 = false>
MXQ_HD void mxq_deq2x8(uint32_t d, int h, float s, float z, uint32_t out[4]) {
    const uint32_t p01 = mxq_pack16<BF16>(s * (0.0f - z), s * (1.0f - z));
    const uint32_t p23 = mxq_pack16<BF16>(s * (2.0f - z), s * (3.0f - z));
    const uint32_t lut_lo = MXQ_PERM(p23, p01, 0x06040200u);
    const uint32_t lut_hi = MXQ_PERM(p23, p01, 0x07050301u);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t m = (d >> (2 * (2 * h + j))) & 0x03030303u;   // codes of elements 4(2h+j) .. +3
        const uint32_t lo = MXQ_PERM(0u, lut_lo, m);
        const uint32_t hi = MXQ_PERM(0u, lut_hi, m);
        out[2 * j] = MXQ_PERM(hi, lo, 0x05010400u);
        out[2 * j + 1] = MXQ_PERM(hi, lo, 0x07030602u);
    }
}

// byte N of a word as float (one v_cvt_f32_ubyteN; spelled as asm on the device because the optimiser folds the
// nibble masks of the caller into per-element shift+and+convert sequences otherwise: 3 ops instead of 1)
#if defined(__HIP_DEVICE_COMPILE__)
#define MXQ_UBYTE_F32(N)                                                          \
    __device__ __forceinline__ float mxq_ubyte##N(uint32_t v) {                   \
        float f;                                                                  \
        asm("v_cvt_f32_ubyte" #N " %0, %1" : "=v"(f) : "v"(v));                   \
        return f;                                                                 \
    }
MXQ_UBYTE_F32(0) MXQ_UBYTE_F32(1) MXQ_UBYTE_F32(2) MXQ_UBYTE_F32(3)
#undef MXQ_UBYTE_F32
#else
MXQ_HD float mxq_ubyte0(uint32_t v) { return (float)(v & 0xFF); }
MXQ_HD float mxq_ubyte1(uint32_t v) { return (float)((v >> 8) & 0xFF); }
MXQ_HD float mxq_ubyte2(uint32_t v) { return (float)((v >> 16) & 0xFF); }
MXQ_HD float mxq_ubyte3(uint32_t v) { return (float)(v >> 24); }
#endif

// 8 four-bit codes (byte-spread word d) -> 4 x packed fp16 pairs
template <bool BF16 = false>
MXQ_HD void mxq_deq4x8(uint32_t d, float s, float z, uint32_t out[4]) {
    const uint32_t m0 = d & 0x0F0F0F0Fu;          // elements 0..3, one per byte
    const uint32_t m1 = (d >> 4) & 0x0F0F0F0Fu;   // elements 4..7
    out[0] = mxq_pack16<BF16>(s * (mxq_ubyte0(m0) - z), s * (mxq_ubyte1(m0) - z));
    out[1] = mxq_pack16<BF16>(s * (mxq_ubyte2(m0) - z), s * (mxq_ubyte3(m0) - z));
    out[2] = mxq_pack16<BF16>(s * (mxq_ubyte0(m1) - z), s * (mxq_ubyte1(m1) - z));
    out[3] = mxq_pack16<BF16>(s * (mxq_ubyte2(m1) - z), s * (mxq_ubyte3(m1) - z));
}

#if defined(__HIPCC__) || defined(MXQ_HOST_HALF)
// The dequant FRONT of the kernels that write or multiply W' as 16-byte slots: one 16-row block `blk` of layout LAYOUT
// (mxq_format.h), row r of it, 16-byte slot `slot` (0..7) of the row's 128-byte chunk line -> the slot's 8 weights as 4 packed
// 16-bit pairs, out[i] = columns (8 slot + 2i, 8 slot + 2i + 1) of the chunk.  qt = slot >> 1 is the 16-column quarter (the
// 2-bit group, where the quarter is one), h = slot & 1 the half of it:
//   W2G16          all four quarters are 2-bit groups: the LUT of mxq_deq2x8, scale nibble qt of SC, QQ slot qt;
//   W4ROW          4-bit codes of (quarter, half) with the row's one scale and zero-point;
//   mixed, qt < 3  the 2-bit LUT, the group's fields through MxqMixed<COMPACT>;
//   mixed, qt = 3  the 4-bit arm: half h of C4 with the row's scale and zero-point.
// `rowmeta()` returns the row's {zero, scale code, qs, qz} as .x .y .z .w from wherever the caller keeps it; it is called on
// the 4-bit branches alone, so a W2G16 caller reads none.  The bit-exactness contract of W': the plain dequant (pack.hip) and the
// quantisation-error kernel (quant_error.hip, which compares W' with the original weight in registers) call this and
// tests/host_emu.cpp walks it on the CPU.  The transposing pass (dequant_t.hip), the fused dX (gemm_dx.hip) and the
// bf16 forward (linear_bf16.hip) keep the same ladder written out in their step 2 -- through this call they measured slower
// at some points (profiles/dequant_front_ab.txt) -- and tests/test_dequant_front_gpu.py holds each of them to the plain
// dequant bit for bit.
template <int LAYOUT, bool BF16, class RM>
MXQ_HD void mxq_deq_slot(const uint32_t* blk, RM&& rowmeta, int r, int slot, uint32_t out[4]) {
    typedef MxqMixed<LAYOUT == MXQ_LAYOUT_MIXEDC> F;
    const int qt = slot >> 1, h = slot & 1;
    if (LAYOUT == MXQ_LAYOUT_W2G16 || (LAYOUT != MXQ_LAYOUT_W4ROW && qt < 3)) {
        constexpr bool W2 = LAYOUT == MXQ_LAYOUT_W2G16;
        const uint32_t d = blk[W2 ? mxq_w2_c2(qt, r) : mxq_c2(qt, r)];
        float z;
        if constexpr (W2) z = __builtin_bit_cast(float, blk[mxq_w2_z2(qt, r)]);
        else z = F::z2(blk, qt, r);
        const uint32_t scw = F::scw(blk, r);      // (W2G16 keeps SC and QQ where the exact mixed layout does)
        const float qs = __builtin_bit_cast(float, blk[F::qq(qt)]), qz = __builtin_bit_cast(float, blk[F::qq(qt) + 1]);
        mxq_deq2x8<BF16>(d, h, mxq_scale(qs, qz, (scw >> (4 * qt)) & 15u), z, out);
    } else {
        const auto m = rowmeta();
        const uint32_t d = blk[LAYOUT == MXQ_LAYOUT_W4ROW ? mxq_w4_c4(qt, h, r) : mxq_c4(h, r)];
        mxq_deq4x8<BF16>(d, mxq_scale(m.z, m.w, (uint32_t)m.y), m.x, out);
    }
}
#endif

// Integer unpack (the bit-exact contract of the unpack kernel)
MXQ_HD uint32_t mxq_code2(uint32_t d, int k) { return (d >> mxq_bit2(k)) & 3u; }
MXQ_HD uint32_t mxq_code4(uint32_t d, int k) { return (d >> mxq_bit4(k)) & 15u; }
