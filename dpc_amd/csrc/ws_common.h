// ws_common.h -- what the loader / compute kernels (conv_igemm_ws.hip, gemm_ws.hip) share AROUND the fragment pipeline of ws_frag.h:
// the wave prologue, the pieces of the packed bf16 epilogue (staging passes, output unit with residual addend / BatchNorm partial
// sums, the sums' reduction), the patch loader and A-fragment table of the plane kernels, and the host-side knob reader.  Every
// piece is written once; what differs between two kernels comes in as an argument or a functor, scalars by value.
// The epilogue is shared in pieces, not as one function, on purpose: igemm_ws_kernel sits at 251 of 256 VGPRs, and with the two
// passes (or just the store loop) behind one function boundary -- a helper or even a local lambda, whatever the argument
// passing -- hipcc gives igemm_ws_kernel<false, true> 213 VGPRs for 199 and 42 spilled SGPRs for 20, <true, false> 69 for 61.
#pragma once
#include "ws_frag.h"
#include <stdlib.h>

// knobs for experiments and for the small shapes of the test tiers
static inline int env_int(const char* name, int dflt) {
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}

// ---- wave prologue ------------------------------------------------------------------------------
struct WsWave { int tid, lane, wv; };   // waves 0..3 (one per SIMD) compute, waves 4..7 load
__device__ __forceinline__ WsWave ws_wave_id() {
    const int tid = threadIdx.x;
#ifdef DPC_SIMT_EMU
    const int wv = tid >> 6;
#else
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
#endif
    return {tid, tid & 63, wv};
}
__device__ __forceinline__ void ws_compute_prio() {
#ifndef DPC_SIMT_EMU
    __builtin_amdgcn_s_setprio(3);   // the compute waves win the SIMD's issue arbitration against their loader partner (-1..2 %)
#endif
}

// ---- packed bf16 epilogue -----------------------------------------------------------------------
// The MFMAs are issued with the operands swapped (weights as the first operand): acc[i][j] then holds the TRANSPOSED 32 x 32
// block -- a lane owns ONE tile row (l & 31) and four consecutive output columns per register quad -- so the epilogue stages a
// quad as one packed 8-byte LDS write (16 per 32-row pass instead of 64 two-byte writes; 37 of 347 us on layer2 were staging).
// Staging rows are 272 bytes apart: the 16 lanes of a ds_write_b64 group then hit 16 disjoint bank pairs, and the row reads
// (ds_read_b128, 4 rows per instruction) stay conflict-free.
constexpr int WS_STG_ROW = 272, WS_STG_WAVE = 32 * WS_STG_ROW;
constexpr int WS_BN = 128, WS_EPO = 8;   // columns of a tile, elements of a 16-byte output unit (16 units per row)
__device__ __forceinline__ void stage_block(unsigned char* mine, const f32x16 (&acc)[4], int l31, int lhi) {
    DPC_UNROLL
    for (int j = 0; j < 4; ++j)
        DPC_UNROLL
        for (int k = 0; k < 4; ++k) {
            u32x2 v = {bf16x2_pack(acc[j][4 * k], acc[j][4 * k + 1]), bf16x2_pack(acc[j][4 * k + 2], acc[j][4 * k + 3])};
            *(u32x2*)(mine + l31 * WS_STG_ROW + (j * 32 + 8 * k + 4 * lhi) * 2) = v;
        }
}
// One 32-row pass through a wave's 8 KB of staging: 32 rows x 128 columns in (ws_stage_pass), and back as the lane's unit
// cu = lane & 15 of rows er + 4 it, er = lane >> 4 (ws_staged_unit: the unit that starts at column col of staged row row_l).
// Wave-private region: LDS operations of one wave complete in order, no workgroup barrier.  The read-back loop, with the fence
// behind it, stays with the kernel, and the unit comes in as its column cu * WS_EPO, the term the kernel's col0 already holds:
// a helper that fills the kernel's ov[8] through a reference, or that multiplies cu out itself (helpers are simplified BEFORE
// they are inlined, cu * 16 then shares nothing with cu * 8), changes igemm_ws_kernel<true>'s set-up code and with it the
// position of its tile loop -- measured +0.9 % on that kernel with every instruction of the loop unchanged.
__device__ __forceinline__ void ws_stage_pass(unsigned char* mine, const f32x16 (&acc)[4], int l31, int lhi) {
    stage_block(mine, acc, l31, lhi);
    wave_lds_fence();
}
__device__ __forceinline__ u32x4 ws_staged_unit(const unsigned char* mine, int row_l, int col) {
    return *(const u32x4*)(mine + row_l * WS_STG_ROW + col * 2);
}
// One 16-byte output unit of a pass.  An input-gradient adds its residual addend a before the store; a forward conv (those have
// no residual addend) feeds what it stored to the BatchNorm partial sums s1 / s2 of the lane's 8 columns.  The store itself, and
// the row guard around all three, stay with the kernel: behind one function the add leaves the guard (igemm_ws_kernel<true>).
__device__ __forceinline__ u32x4 ws_unit_add(u32x4 o, u32x4 a) {
    float sv[WS_EPO];
    DPC_UNROLL
    for (int e = 0; e < WS_EPO; ++e) sv[e] = unit_get<bf16_t>(o, e) + unit_get<bf16_t>(a, e);
    return unit_pack<bf16_t>(sv);
}
__device__ __forceinline__ void ws_unit_sums(u32x4 o, float (&s1)[WS_EPO], float (&s2)[WS_EPO]) {
    DPC_UNROLL
    for (int e = 0; e < WS_EPO; ++e) {
        const float v = unit_get<bf16_t>(o, e);
        s1[e] += v;
        s2[e] += v * v;
    }
}
// BatchNorm partial sums of a workgroup, after its last tile: 16 lanes x 4 compute waves hold partial sums of the same 8 columns.
// Fold the 4 row-lanes of a wave by shuffles, then the 4 waves through LDS (the loader waves only keep the barriers company).
__device__ __forceinline__ void ws_stats_tail(unsigned char* lds, float (&s1)[WS_EPO], float (&s2)[WS_EPO], float* stats, int Ncol, int m_prog,
                                              int n_tile, int tid, int wv) {
    const int lane = tid & 63, cu = lane & 15;
    DPC_UNROLL
    for (int e = 0; e < WS_EPO; ++e) {
        s1[e] += __shfl_xor(s1[e], 16); s1[e] += __shfl_xor(s1[e], 32);
        s2[e] += __shfl_xor(s2[e], 16); s2[e] += __shfl_xor(s2[e], 32);
    }
    float* red = (float*)lds;  // [4 waves][2][128]
    __syncthreads();
    if (wv < 4 && lane < 16) {
        DPC_UNROLL
        for (int e = 0; e < WS_EPO; ++e) {
            red[(wv * 2 + 0) * WS_BN + cu * WS_EPO + e] = s1[e];
            red[(wv * 2 + 1) * WS_BN + cu * WS_EPO + e] = s2[e];
        }
    }
    __syncthreads();
    if (tid < WS_BN) {
        const int col = n_tile * WS_BN + tid;
        if (col < Ncol) {
            float a = 0.f, b = 0.f;
            DPC_UNROLL
            for (int w = 0; w < 4; ++w) {
                a += red[(w * 2 + 0) * WS_BN + tid];
                b += red[(w * 2 + 1) * WS_BN + tid];
            }
            stats[((long long)m_prog * 2 + 0) * Ncol + col] = a;
            stats[((long long)m_prog * 2 + 1) * Ncol + col] = b;
        }
    }
}

// ---- plane kernels: a tile is one 16 x 16 plane, staged once per 64-channel group as a zero-padded 18 x 18 patch ----------------
constexpr int WS_BM = 256;   // rows of a tile = positions of a plane
constexpr int WSP_PWD = 18, WSP_NPP = WSP_PWD * WSP_PWD, WSP_NPIECE = (WSP_NPP + 7) / 8, WSP_PATCH = WSP_NPIECE * 1024;  // 324 positions, 41 pieces
constexpr int WSP_BST = WS_BN * 128, WSP_NSB = 4;   // ring of four 16 KB weight stages behind the two patches
constexpr int WSP_MAXP = (WSP_NPIECE + 3) / 4;      // patch pieces per loader wave
constexpr int WSP_LDS = 2 * WSP_PATCH + WSP_NSB * WSP_BST;
static_assert(4 * WS_STG_WAVE <= WSP_PATCH, "epilogue staging fits a patch buffer");
static_assert(WSP_LDS <= 160 * 1024, "patches + ring fit the CU's LDS");

// The loader waves' whole life.  Chunks are numbered across the workgroup's tiles (total of them, cpg per channel group, G groups
// per tile; tile tl of the workgroup is plane m_prog + tl * mstride); issue_b(gc) issues the weights of chunk gc into ring stage
// gc % WSP_NSB and returns the number of LDS-DMA operations it issued.  The patch of the NEXT group (its buffer was read last by
// the previous group, i.e. free since this group's first barrier) goes out in the first pslots slots of a group; it must be
// complete at its first chunk's barrier, i.e. issued in slots <= first - 3: pslots <= cpg - 2.
// dbg: the probe mask, a kernel argument in probe builds (phases left out: 4 | 128 patch DMA, 32 barriers, 512 patches of 8
// planes only) and therefore no template parameter; product builds pass the literal 0 and its branches fold away.
// The callers fill the plan with designated initialisers, which hipcc and g++ accept under -std=c++17 as an extension (C++20).
struct WsPatchPlan { int m_prog, mstride, G, cpg, pslots, total; };
template <class IssueB>
__device__ __forceinline__ void ws_patch_loader(unsigned char* lds, const void* src, unsigned src_bytes, int src_ld, int lane, int lw,
                                                const WsPatchPlan pl, int dbg, IssueB issue_b) {
    const int m_prog = pl.m_prog, mstride = pl.mstride, G = pl.G, cpg = pl.cpg, pslots = pl.pslots, total = pl.total;
    const int rl = lane >> 3;
    const BufRsrc rs_a = make_buf_rsrc(src, src_bytes);
    // patch piece j = lw + 4i holds patch positions 8j .. 8j+7; a lane fetches unit (slot ^ swizzle(patch column)) of its
    // position.  The offsets are relative to the plane: the same for every tile.
    unsigned poff[WSP_MAXP];
    DPC_UNROLL
    for (int i = 0; i < WSP_MAXP; ++i) {
        const int pp = 8 * (lw + 4 * i) + rl;
        const int pr = pp / WSP_PWD, pc = pp - pr * WSP_PWD;
        const bool ok = pp < WSP_NPP && pr >= 1 && pr <= 16 && pc >= 1 && pc <= 16;
        const int up = (lane & 7) ^ ((pc >> 1) & 7);
        poff[i] = ok ? (unsigned)((((pr - 1) * 16 + (pc - 1)) * src_ld + up * 8) * 2) : DPC_BUF_OOB;
    }
    const int n_mine = (WSP_NPIECE - lw + 3) / 4;
    int issued = 0;               // operations issued in the current slot
    auto issue_patch = [&](int gg, int i0, int i1) {   // pieces [i0, i1) of this wave, of global group gg
        const int tl = gg / G, grp = gg - tl * G;
        const int mt = (dbg & 512) ? m_prog & 7 : m_prog + tl * mstride;
        const unsigned soff = (unsigned)((mt * WS_BM * src_ld + grp * 64) * 2);
        unsigned char* dst = lds + (gg & 1) * WSP_PATCH;
        DPC_UNROLL
        for (int i = 0; i < WSP_MAXP; ++i)
            if (i >= i0 && i < i1 && i < n_mine && !(dbg & (4 | 128))) {
                glds16_buf(rs_a, poff[i], soff, dst + (lw + 4 * i) * 1024, lane);
                ++issued;
            }
    };
    // A slot = what is issued between two chunk barriers: patch pieces first, the weights of chunk c+3 last.  The weights of
    // chunk c are the last operations of slot c-3, so "at most (slot c-2) + (slot c-1) operations outstanding" means landed --
    // they, and every patch piece issued before them (LDS-DMA of a wave completes in issue order).
    // The prologue counts as slots -3 (patch of group 0 + chunk 0), -2 (chunk 1), -1 (chunk 2).
    const int ppc = (WSP_MAXP + pslots - 1) / pslots;
    if (total > 0) {
        issue_patch(0, 0, WSP_MAXP);
        issue_b(0);
    }
    issued = 0;
    if (total > 1) issued += issue_b(1);
    int o2 = issued;
    issued = 0;
    if (total > 2) issued += issue_b(2);
    int o1 = issued;
    for (int gc = 0; gc < total; ++gc) {
        wait_vmcnt_upto(o1 + o2);
        if (!(dbg & 32)) ws_barrier();  // chunk gc (and, at a group's first chunk, its patch) is published; every reader is done with chunk gc-1
        const int gg = gc / cpg, q = gc - gg * cpg;
        issued = 0;
        if (q < pslots && (gg + 1) * cpg < total) issue_patch(gg + 1, ppc * q, ppc * q + ppc);
        if (gc + 3 < total) issued += issue_b(gc + 3);
        o2 = o1;
        o1 = issued;
        if (q == cpg - 1 && (gg + 1) % G == 0) if (!(dbg & 32)) ws_barrier();  // matches the compute waves' "tile fully read" barrier
    }
}
// A-fragment addresses of the plane kernels.  Row r of the tile is plane position (r >> 4, r & 15); shifted by (dh, dw) it reads
// patch position (r>>4 + dh) * 18 + (r&15) + dw; the second fragment (+32 rows = +2 plane rows) is 36 positions = 4608 bytes
// further in the same patch column.  The 16-byte slots of a position are XOR-swizzled by (patch column >> 1) & 7: a ds_read_b128
// lane group is 8 + 8 lanes of two plane rows (MI355X_MICROARCH.md, LDS) whose columns c+{0..3,12..15} and c+{4..11} then cover
// 16 distinct (column parity, slot) pairs = all 64 banks; swizzling by the position (row pitch 18) does not.  Everything that
// depends on the lane is tabulated per column shift dw[k]; the dh / patch-buffer part is a scalar added per chunk.
// slot bits = ((2kk + lhi) ^ p7) << 4 = ((lhi ^ p7) << 4) ^ (kk << 5), and every base is a multiple of 128: the address of
// step kk is (chunk base + va[k]) ^ (kk << 5) -- one register per column shift instead of a table per step.
template <int N>
__device__ __forceinline__ void ws_patch_va(int (&va)[N], const int (&dw)[N], int wv, int l31, int lhi) {
    const int pos0 = ((wv * 64 + l31) >> 4) * WSP_PWD + (l31 & 15);
    DPC_UNROLL
    for (int k = 0; k < N; ++k) {
        const int p7 = (((l31 & 15) + dw[k]) >> 1) & 7;
        va[k] = (pos0 + dw[k]) * 128 + ((lhi ^ p7) << 4);
    }
}
