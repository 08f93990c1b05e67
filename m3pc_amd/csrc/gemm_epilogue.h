// Shared epilogue of the bf16 MFMA GEMM kernels (gemm_glds.hip, gemm_persist.hip).
//
// Accumulator layout of v_mfma_f32_32x32x16_bf16: acc[i][j][reg] is row (reg&3) + 8*(reg>>2) + 4*(lane>>5),
// column lane&31 of 32x32 tile (i, j) of the wave tile.
//
// Fast path (full tile, identity row map): addresses are split into a wave-uniform part that lives in SGPRs
// (buffer soffset = row * ld) and ONE per-lane 32-bit offset computed once (buffer voffset); the j-tile
// distance is an immediate.  Per element that leaves: bias add, [GELU], [residual add], convert, store --
// no per-element 64-bit address arithmetic (hipcc otherwise spends ~2 VALU instructions per element on it,
// which at K = 512 costs as much as a third of the tile's MFMA time).
#pragma once
#include "device_util.h"

namespace m3pc {

// rbase / cbase: first row / column of this WAVE's tile, wave-uniform (pass values derived from readfirstlane)
// bias_pre: the TN bias values of this lane's columns when the caller fetched them earlier (a persistent kernel has
// the next tile's DMA in flight here and a load issued now would wait for all of it), else nullptr
template <int EPI, int TM, int TN>
__device__ __forceinline__ void gemm_epilogue(const GemmP& p, f32x16 (&acc)[TM][TN], int rbase, int cbase, int tile_row0,
                                              int tile_rows, int lane, const float* bias_pre = nullptr) {
    const int l31 = lane & 31, lh = lane >> 5;
    float bj[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) bj[j] = bias_pre ? bias_pre[j] : (p.bias ? p.bias[cbase + j * 32 + l31] : 0.f);
    const bool fast = p.cmap.rpg == 0 && tile_row0 + tile_rows <= p.M && !(EPI & GE_ROWTAB);
    if (fast) {
        constexpr int ES = (EPI & GE_F32OUT) ? 4 : 2;
        void* cptr = (EPI & GE_F32OUT) ? (void*)p.Cf : (void*)p.Cb;
        const __amdgpu_buffer_rsrc_t crs =
            __builtin_amdgcn_make_buffer_rsrc(cptr, 0, clamp_bytes((long long)p.M * p.ldc * ES), 0x00020000);
        const int vo_c = (4 * lh * p.ldc + l31) * ES;
        __amdgpu_buffer_rsrc_t rrs = crs;
        int vo_r = 0;
        if constexpr (EPI & GE_RES) {
            rrs = __builtin_amdgcn_make_buffer_rsrc((void*)p.res, 0, clamp_bytes((long long)p.M * p.ldr * 4), 0x00020000);
            vo_r = (4 * lh * p.ldr + l31) * 4;
        }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int rr = rbase + i * 32 + (reg & 3) + 8 * (reg >> 2);
                const int so_c = (rr * p.ldc + cbase) * ES;
                const int so_r = (rr * p.ldr + cbase) * 4;
                float vj[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) vj[j] = acc[i][j][reg] + bj[j];
                if constexpr ((EPI & GE_GELU) != 0 && (EPI & GE_GELU_EXACT) != 0) {
#pragma unroll
                    for (int j = 0; j < TN; ++j) vj[j] = gelu_exact(vj[j]);
                } else if constexpr ((EPI & GE_GELU) != 0) {
                    if constexpr (TN % 2 == 0) {
#pragma unroll
                        for (int j = 0; j < TN; j += 2) {
                            const f32x2 g2 = gelu_fast2((f32x2){vj[j], vj[j + 1]});
                            vj[j] = g2.x;
                            vj[j + 1] = g2.y;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < TN; ++j) vj[j] = gelu_fast(vj[j]);
                    }
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    float v = vj[j];
                    if constexpr (EPI & GE_RES)
                        v += __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rrs, vo_r + j * 128, so_r, 0));
                    if constexpr (EPI & GE_F32OUT)
                        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, v), crs, vo_c + j * 128, so_c, 0);
                    else
                        __builtin_amdgcn_raw_buffer_store_b16(__builtin_bit_cast(unsigned short, (bf16_t)v), crs, vo_c + j * 64,
                                                              so_c, 0);
                }
            }
        }
        return;
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int r = rbase + i * 32 + (reg & 3) + 8 * (reg >> 2) + 4 * lh;
            if (r < p.M) {
                const long long pr = map_row(p.cmap, r);
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int c = cbase + j * 32 + l31;
                    float v = acc[i][j][reg] + bj[j];
                    if constexpr (EPI & GE_ROWTAB) v += p.rowtab[(long long)(r % p.rt_mod) * p.rt_ld + c];
                    if constexpr (EPI & GE_GELU) v = (EPI & GE_GELU_EXACT) ? gelu_exact(v) : gelu_fast(v);
                    if constexpr (EPI & GE_RES) v += p.res[pr * p.ldr + c];
                    if constexpr (EPI & GE_F32OUT)
                        p.Cf[pr * p.ldc + c] = v;
                    else
                        p.Cb[pr * p.ldc + c] = (bf16_t)v;
                }
            }
        }
    }
}

}  // namespace m3pc
