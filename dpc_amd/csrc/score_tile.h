// score_tile.h -- the tile helpers the flash-style score kernels share (csrc/score_fused.hip: the in-batch score; csrc/neg_queue.hip:
// the negative queue): a workgroup of 4 waves owns 128 rows held in registers for all of K, 64-row tiles of the streamed operand
// arrive in LDS by LDS-DMA, and a wave forms its 32 x 64 tile of S on the matrix cores.  Moved here unchanged.
#pragma once
#include "dpc_rt.h"
#include "../../include/dpc_hip.h"

namespace {

constexpr float L2E = 1.4426950408889634f;
constexpr float NEG_BIG = -3.0e38f;
constexpr int BM = 128, BN = 64;

__device__ __forceinline__ int crow(int r, int lane) { return (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5); }

// rows [row0, row0 + nrows) x K of a row-major [R][ld] bf16 matrix -> LDS as 128-byte rows, chunk by chunk:
// tile[chunk c][row][8 swizzled units].  One LDS-DMA instruction of a wave fills 8 rows of one chunk; rows / columns
// outside the matrix read 16 zero bytes.
__device__ __forceinline__ void dma_rows(unsigned char* tile, const bf16_t* src, long long ld, int row0, int nrows, int row_limit, int col0,
                                         int ncols, int col_limit, int wave, int lane) {
    const char* const zero = (const char*)dpc_zero16;
    const int chunks = (ncols * 2 + 127) / 128;
    const int groups = nrows / 8;
    for (int g = wave; g < chunks * groups; g += 4) {
        const int c = g / groups, rg = g - c * groups;
        const int row = rg * 8 + (lane >> 3);
        const int u = (lane & 7) ^ lds_swz1(row);
        const int col = col0 + (c * 8 + u) * 8;
        const bool ok = (row0 + row < row_limit) && (col < col_limit) && ((c * 8 + u) * 8 < ncols);
        const char* a = (const char*)(src + (long long)(row0 + row) * ld + col);
        glds16(ok ? a : zero, tile + c * (nrows * 128) + rg * 8 * 128, lane);
    }
}

template <int KS>
__device__ __forceinline__ void load_own_ld(u32x4 (&own)[KS], const bf16_t* base, long long ld, int nrows, int r0, int lane) {
    const int row = r0 + (lane & 31), kg = lane >> 5;
    DPC_UNROLL
    for (int ks = 0; ks < KS; ++ks) {
        u32x4 v = {0u, 0u, 0u, 0u};
        if (row < nrows) v = *(const u32x4*)(base + (long long)row * ld + (ks * 2 + kg) * 8);
        own[ks] = v;
    }
}
// S[32 rows of the wave][64 columns of the tile] from the register-resident own fragments and the LDS tile.
// The B fragments of K step ks + PF are requested before the MFMAs of step ks are issued: hipcc otherwise emits
// ds_read -> s_waitcnt lgkmcnt(0) -> v_mfma per step and every MFMA eats a full LDS round trip (measured: 37 % of
// the wave's cycles parked in s_waitcnt).
// SWAP: the streamed operand goes first, so a lane holds ONE row of the wave (lane & 31) and quads of four consecutive streamed
// columns (8 (r >> 2) + 4 (lane >> 5) + (r & 3)): what a 16-byte row store wants (score_gemm_kernel).
template <int KS, bool SWAP = false>
__device__ __forceinline__ void s_tile(f32x16 (&s)[2], const u32x4 (&own)[KS], const unsigned char* tile, int lane) {
    constexpr int PF = KS >= 4 ? 3 : (KS - 1 > 0 ? KS - 1 : 1);  // K steps in flight ahead of the MFMAs
    const int j = lane & 31, kg = lane >> 5;
    DPC_UNROLL
    for (int t = 0; t < 2; ++t)
        DPC_UNROLL
        for (int r = 0; r < 16; ++r) s[t][r] = 0.f;
    u32x4 b[KS][2];
    // hand-issued reads (invisible to hipcc's wait-count pass, which would re-serialise them); in order, counted below
    auto req = [&](auto ks_) {
        constexpr int ks = decltype(ks_)::value;
        const int unit = ks * 2 + kg;
        const unsigned char* a0 = tile + (unit >> 3) * (BN * 128) + lds_unit_off(j, unit & 7);
        lds_read_b128_async(b[ks][0], a0);
        lds_read_b128_async_off<32 * 128>(b[ks][1], a0);  // row j + 32: same swizzle (swz1(r + 32) == swz1(r))
    };
    static_for<(PF < KS ? PF : KS)>([&](auto ks_) { req(ks_); });
    static_for<KS>([&](auto ks_) {
        constexpr int ks = decltype(ks_)::value;
        if constexpr (ks + PF < KS) req(std::integral_constant<int, ks + PF>{});
        constexpr int later = (KS - 1 - ks) < PF ? (KS - 1 - ks) : PF;  // K steps requested after this one
        lds_wait_tie_n(2 * later, b[ks][0], b[ks][1]);
        DPC_UNROLL
        for (int t = 0; t < 2; ++t) s[t] = SWAP ? mfma_32x32x16_bf16(b[ks][t], own[ks], s[t]) : mfma_32x32x16_bf16(own[ks], b[ks][t], s[t]);
    });
}

template <class K> int allow_lds(K kernel, size_t bytes) {
#ifndef DPC_SIMT_EMU
    if (bytes > 160 * 1024) return DPC_ERR_UNSUPPORTED;
    if (dpc_tls_plan_only) return DPC_OK;  // the plan query launches nothing (and must work without a device)
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return DPC_ERR_LAUNCH;
#else
    (void)kernel; (void)bytes;
#endif
    return DPC_OK;
}

// column splits so that (row blocks x splits) fills the chip, each split keeping at least 4 tiles
inline void plan_splits(int R, int target_wgs, int* ntiles, int* tps, int* nsplit) {
    const int nrb = (R + BM - 1) / BM;
    *ntiles = (R + BN - 1) / BN;
    int s = (target_wgs + nrb - 1) / nrb;
    if (s < 1) s = 1;
    const int max_s = *ntiles / 4 > 0 ? *ntiles / 4 : 1;
    if (s > max_s) s = max_s;
    if (s > 16) s = 16;
    *tps = (*ntiles + s - 1) / s;
    *nsplit = (*ntiles + *tps - 1) / *tps;
}

}  // namespace
