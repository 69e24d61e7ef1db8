// Host harness for the format / dequant helpers shared with the HIP kernels
// (mxq_amd/csrc/mxq_format.h, mxq_pack.h, mxq_dequant.h compiled for the CPU with a
// software v_perm_b32).  TEST INFRASTRUCTURE: lets `pytest -m "not gpu"` check the bit
// layout, the integer unpack and the LUT dequant against the oracle without a GPU.
//   g++ -O2 -mf16c -ffp-contract=off -shared -fPIC tests/host_emu.cpp -o tests/_build/libhost_emu.so
#include <immintrin.h>
#include <stdint.h>
#include <string.h>

uint16_t mxq_host_f32_to_f16(float f) { return _cvtss_sh(f, _MM_FROUND_TO_NEAREST_INT | _MM_FROUND_NO_EXC); }

float mxq_h2f(uint16_t h) { return _cvtsh_ss(h); }

#define MXQ_HOST_HALF 1   // MxqMixed and mxq_deq_slot (the emulation has entries for the exact metadata and the uniform layouts)
#include "../mxq_amd/csrc/mxq_dequant.h"
#include "../mxq_amd/csrc/mxq_format.h"
#include "../mxq_amd/csrc/mxq_pack.h"

// The row's rowmeta as mxq_deq_slot reads it (the device passes a float4)
struct RowMeta { float x, y, z, w; };

// dequantise by walking (row, 16-byte slot) through mxq_deq_slot: the per-thread code of mxq_dequant_f16_kernel, and the
// ladder that the transposing pass, the fused dX and the bf16 forward write out
template <int LAYOUT>
static void dequant_f16(const uint32_t* qweight, const float* rowmeta, uint16_t* out, int N, int K) {
    const int NC = K / 64, BLK_DW = mxq_layout_blk_dw(LAYOUT);
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < NC; ++c)
            for (int slot = 0; slot < 8; ++slot) {
                uint32_t o[4];
                mxq_deq_slot<LAYOUT, false>(qweight + mxq_blk_index(n, c, K) * BLK_DW,
                                            [&] { return ((const RowMeta*)rowmeta)[n]; }, n & 15, slot, o);
                memcpy(out + (long)n * K + c * 64 + slot * 8, o, 16);
            }
}

extern "C" {

long emu_qweight_dwords(int N, int K) { return (long)(N / 16) * (K / 64) * MXQ_BLK_DW; }

void emu_pack(const uint8_t* codes2, const uint8_t* sc2, const float* zero2, const float* qs2, const float* qz2,
              const uint8_t* codes4, const uint8_t* sc4, const float* zero4, const float* qs4, const float* qz4,
              uint32_t* qweight, float* rowmeta, int N, int K) {
    const int NC = K / 64;
    memset(qweight, 0, emu_qweight_dwords(N, K) * 4);
    for (int n = 0; n < N; ++n) {
        for (int c = 0; c < NC; ++c) {
            uint32_t* tile = qweight + mxq_blk_index(n, c, K) * MXQ_BLK_DW;
            mxq_pack_row_chunk(tile, n & 15, codes2 + (long)n * NC * 48 + c * 48, sc2 + (long)n * NC * 3 + c * 3,
                               zero2 + (long)n * NC * 3 + c * 3, codes4 + (long)n * NC * 16 + c * 16);
            if ((n & 15) == 0)
                for (int g = 0; g < 3; ++g) {
                    memcpy(tile + mxq_qq(g), qs2 + (long)(n / 16) * NC * 3 + c * 3 + g, 4);
                    memcpy(tile + mxq_qq(g) + 1, qz2 + (long)(n / 16) * NC * 3 + c * 3 + g, 4);
                }
        }
        rowmeta[4 * n] = zero4[n];
        rowmeta[4 * n + 1] = (float)sc4[n];
        rowmeta[4 * n + 2] = qs4[n / 16];
        rowmeta[4 * n + 3] = qz4[n / 16];
    }
}

void emu_unpack(const uint32_t* qweight, uint8_t* codes2, uint8_t* sc2, float* zero2, uint8_t* codes4, int N, int K) {
    const int NC = K / 64;
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < NC; ++c)
            mxq_unpack_row_chunk(qweight + mxq_blk_index(n, c, K) * MXQ_BLK_DW, n & 15,
                                 codes2 + (long)n * NC * 48 + c * 48, sc2 + (long)n * NC * 3 + c * 3,
                                 zero2 + (long)n * NC * 3 + c * 3, codes4 + (long)n * NC * 16 + c * 16);
}

void emu_dequant_f16(const uint32_t* qweight, const float* rowmeta, uint16_t* out, int N, int K) {
    dequant_f16<MXQ_LAYOUT_MIXED>(qweight, rowmeta, out, N, K);
}

// the uniform layouts: pack the oracle's parameters (codes [N, K]; W2G16: sc / zero [N, K/16], qs / qz [N/16, K/16]; W4ROW:
// everything but the codes is the caller's rowmeta) into blocks, and dequantise them through the same front
void emu_pack_uniform(const uint8_t* codes, const uint8_t* sc, const float* zero, const float* qs, const float* qz,
                      uint32_t* qweight, int N, int K, int layout) {
    const int NC = K / 64, G = K / 16, BLK_DW = mxq_layout_blk_dw(layout);
    memset(qweight, 0, (size_t)(N / 16) * NC * BLK_DW * 4);
    for (int n = 0; n < N; ++n)
        for (int c = 0; c < NC; ++c)
            for (int qt = 0; qt < 4; ++qt) {
                uint32_t* blk = qweight + mxq_blk_index(n, c, K) * BLK_DW;
                const uint8_t* q = codes + (long)n * K + c * 64 + qt * 16;
                const int r = n & 15, g = c * 4 + qt;
                if (layout == MXQ_LAYOUT_W4ROW) {
                    for (int k = 0; k < 16; ++k) blk[mxq_w4_c4(qt, k >> 3, r)] |= (uint32_t)q[k] << mxq_bit4(k & 7);
                    continue;
                }
                for (int k = 0; k < 16; ++k) blk[mxq_w2_c2(qt, r)] |= (uint32_t)q[k] << mxq_bit2(k);
                memcpy(blk + mxq_w2_z2(qt, r), zero + (long)n * G + g, 4);
                ((uint16_t*)blk)[mxq_sc_u16(r)] |= (uint16_t)(sc[(long)n * G + g] << (4 * qt));
                memcpy(blk + mxq_qq(qt), qs + (long)(n / 16) * G + g, 4);
                memcpy(blk + mxq_qq(qt) + 1, qz + (long)(n / 16) * G + g, 4);
            }
}

void emu_dequant_uniform_f16(const uint32_t* qweight, const float* rowmeta, uint16_t* out, int N, int K, int layout) {
    if (layout == MXQ_LAYOUT_W2G16) dequant_f16<MXQ_LAYOUT_W2G16>(qweight, rowmeta, out, N, K);
    else dequant_f16<MXQ_LAYOUT_W4ROW>(qweight, rowmeta, out, N, K);
}
}
