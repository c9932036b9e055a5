// gemm_ws.hip -- split-K GEMMs with a small output and a long reduction on the loader / compute machinery of
// conv_igemm_ws.hip: the two backward products of the contrastive score (autograd of torch.matmul(pred, feature_inf),
// dpc/model_3d.py:79-84 under dpc/main.py:229's backward):
//
//   d_pred [r][d] = sum_c dS[r][c] * finf[c][d]     A = dS row-major (K = c contiguous)        gemm_ws_kernel<false>
//   d_finf [c][d] = sum_r dS[r][c] * pred[r][d]     A = dS^T, i.e. dS read "K-major"            gemm_ws_kernel<true>
//
// both with M = K = R (6 144 at cfg2, 15 680 at cfg5), N = D = 256, B = the other feature matrix transposed ([D][R], K
// contiguous).  Round 3 ran them on the generic 128 x 128 kernel (every wave issues its own LDS-DMA: 417 TFLOP/s) and on the
// weight-gradient kernel (482 TFLOP/s) -- "ordinary K >= 6 144 GEMMs, the shape on which igemm_ws reaches 1 600" (VERDICT r3).
//
// Decomposition: 256 x 128 output tiles (R/256 x 2 of them) x nks K-slices, sized so that tiles x slices fills the chip once
// (240 workgroups at R = 6 144 with 5 slices of 19-20 chunks, 248 at R = 15 680 with 2 slices); a workgroup owns ONE
// (tile, slice): 4 compute waves (64 x 128 each, fragment reads interleaved with the MFMAs, ws_frag.h) + 4 loader waves (12
// LDS-DMA pieces per 128-byte K chunk each, ring of three 48 KB stages, counted vmcnt(12)) -- the protocol of igemm_ws_kernel
// without its gather.  The f32 partial tile leaves through LDS as whole 512-byte rows into slab ks of part[nks][M][N];
// dpc_reduce_unpack sums the slabs in fixed order (deterministic; the last-arriver in-kernel reduction of the guide is for slabs
// of tens of KB -- these are 128 KB per workgroup, 5 per tile).
// Workgroup ids are dealt to the XCDs round-robin; the remap gives each XCD a contiguous range of logical ids with the two
// column tiles of a (row tile, slice) adjacent, so dS -- the only large operand, 75 / 492 MB -- crosses HBM once.
//
// TRANS_A: the A stage keeps dS's memory orientation, [k][m]: four sub-tiles of 64 k-rows x 64 m-columns (8 KB, 128-byte rows,
// 16-byte slot XORed with 2 * (k & 3) -- wgrad2_kernel's image, conflict-free for the transpose read), one per compute wave;
// fragments come from ds_read_b64_tr_b16 (two per operand register quad), eight reads per K step = one per MFMA gap.
#include "ws_common.h"
#include "../../include/dpc_hip.h"

struct GemmWsParams {
    const void* A;
    const void* B;
    float* part;
    int M, N, K, lda, ldb;
    int ntm, ntn, nks, cps;     // row tiles, column tiles, K slices, chunks per slice
    unsigned a_bytes, b_bytes;
};

#ifndef DPC_SIMT_EMU
struct FragSetT {   // transposed-A fragments: a quad = (lo, hi) halves from two transpose reads
    u32x2 alo[2], ahi[2];
    u32x4 b[4];
};
template <int N> __device__ __forceinline__ void frag_wait(FragSetT& f) {
    asm volatile("s_waitcnt lgkmcnt(%8)"
                 : "+v"(f.alo[0]), "+v"(f.ahi[0]), "+v"(f.alo[1]), "+v"(f.ahi[1]), "+v"(f.b[0]), "+v"(f.b[1]), "+v"(f.b[2]), "+v"(f.b[3])
                 : "n"(N)
                 : "memory");
}
// the eight reads of K step KK on their own; order = order of first use: a0lo a0hi b0 b1 a1lo a1hi b2 b3
template <int KK>
__device__ __forceinline__ void fragt_read(FragSetT& f, ldsa_t xa0, ldsa_t xa1, ldsa_t xb) {
    asm volatile("ds_read_b64_tr_b16 %0, %8 offset:%11\n\t"
                 "ds_read_b64_tr_b16 %1, %8 offset:%12\n\t"
                 "ds_read_b128 %4, %10\n\t"
                 "ds_read_b128 %5, %10 offset:4096\n\t"
                 "ds_read_b64_tr_b16 %2, %9 offset:%11\n\t"
                 "ds_read_b64_tr_b16 %3, %9 offset:%12\n\t"
                 "ds_read_b128 %6, %10 offset:8192\n\t"
                 "ds_read_b128 %7, %10 offset:12288"
                 : "=&v"(f.alo[0]), "=&v"(f.ahi[0]), "=&v"(f.alo[1]), "=&v"(f.ahi[1]), "=&v"(f.b[0]), "=&v"(f.b[1]), "=&v"(f.b[2]), "=&v"(f.b[3])
                 : "v"(xa0), "v"(xa1), "v"(xb), "n"(KK * 2048), "n"(KK * 2048 + 512)
                 : "memory");
}
// One K step with the NEXT step's (index KN) eight reads between its eight MFMAs.  On entry the reads that may be outstanding
// are the eight of `use`, in the order above; each MFMA waits for exactly the operand it is the first to need:
//   (0,0) a0 b0 -> 5 may stay | (0,1) b1 -> 5 (one new read was issued) | (1,0) a1 -> 4 | (1,1) | (0,2) b2 -> 5 | (1,2) | (0,3) b3 -> 6 | (1,3)
template <int KN>
__device__ __forceinline__ void step_il_t(f32x16 (&acc)[2][4], const FragSetT& use, FragSetT& ld, ldsa_t xa0, ldsa_t xa1, ldsa_t xb) {
#define DPC_ILT_RT(dst, addr, off) \
    asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off) : "memory"); \
    __builtin_amdgcn_sched_barrier(0)
#define DPC_ILT_RB(dst, addr, off) \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off) : "memory"); \
    __builtin_amdgcn_sched_barrier(0)
#define DPC_ILT_WAIT(n) \
    asm volatile("s_waitcnt lgkmcnt(" #n ")" ::: "memory"); \
    __builtin_amdgcn_sched_barrier(0)
#define DPC_ILT_MMA(i, j) \
    { const u32x4 av = {use.alo[i][0], use.alo[i][1], use.ahi[i][0], use.ahi[i][1]}; \
      acc[i][j] = mfma_32x32x16_bf16(use.b[j], av, acc[i][j]); } \
    __builtin_amdgcn_sched_barrier(0)
    __builtin_amdgcn_sched_barrier(0);
    DPC_ILT_WAIT(5); DPC_ILT_MMA(0, 0); DPC_ILT_RT(ld.alo[0], xa0, KN * 2048);
    DPC_ILT_WAIT(5); DPC_ILT_MMA(0, 1); DPC_ILT_RT(ld.ahi[0], xa0, KN * 2048 + 512);
    DPC_ILT_WAIT(4); DPC_ILT_MMA(1, 0); DPC_ILT_RB(ld.b[0], xb, 0);
    DPC_ILT_MMA(1, 1); DPC_ILT_RB(ld.b[1], xb, 4096);
    DPC_ILT_WAIT(5); DPC_ILT_MMA(0, 2); DPC_ILT_RT(ld.alo[1], xa1, KN * 2048);
    DPC_ILT_MMA(1, 2); DPC_ILT_RT(ld.ahi[1], xa1, KN * 2048 + 512);
    DPC_ILT_WAIT(6); DPC_ILT_MMA(0, 3); DPC_ILT_RB(ld.b[2], xb, 8192);
    DPC_ILT_MMA(1, 3); DPC_ILT_RB(ld.b[3], xb, 12288);
#undef DPC_ILT_RT
#undef DPC_ILT_RB
#undef DPC_ILT_WAIT
#undef DPC_ILT_MMA
}
#endif

constexpr int GW_STG_ROW = 528;   // f32 staging rows of 128 columns: 512 B + 16: the 16 lanes of a ds_write_b128 group hit 16 disjoint bank quads

template <bool TRANS_A>
__global__ __launch_bounds__(512, 2) void gemm_ws_kernel(GemmWsParams p) {
    constexpr int BM = 256, BN = 128;
    constexpr int STAGE = (BM + BN) * 128;  // 48 KB
    constexpr int NST = 3;
    static_assert(64 * GW_STG_ROW * 4 <= NST * STAGE, "f32 staging of the whole tile fits the ring");
    __shared__ __attribute__((aligned(1024))) unsigned char lds[NST * STAGE];

    const WsWave w = ws_wave_id();
    const int lane = w.lane, wv = w.wv;
    // XCD-contiguous logical id (workgroup b runs on XCD b & 7), then (column tile, row tile, slice), column tile fastest
    int id = blockIdx.x;
    {
        const int nwg = gridDim.x, q = nwg >> 3, r = nwg & 7, x = id & 7;
        id = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (id >> 3);
    }
    const int n_tile = id % p.ntn; id /= p.ntn;
    const int m_tile = id % p.ntm;
    const int ks = id / p.ntm;
    const int nch_all = (p.K + 63) >> 6;
    const int c0 = ks * p.cps;
    const int c1 = c0 + p.cps < nch_all ? c0 + p.cps : nch_all;
    const int total = c1 - c0;          // >= 1 by construction of the grid
    const int m0 = m_tile * BM, n0 = n_tile * BN;

    if (wv >= 4) {
        // ------------------------------------------------------------------ loader waves
        const int lw = wv - 4;
        const int rl = lane >> 3;
        const BufRsrc rs_a = make_buf_rsrc(p.A, p.a_bytes);
        const BufRsrc rs_b = make_buf_rsrc(p.B, p.b_bytes);
        const int ub = (lane & 7) ^ lds_swz1(8 * lw + rl);           // logical 16-byte unit of the K chunk this lane fetches (B, and A when !TRANS_A)
        unsigned brow[4], arow[8];
        DPC_UNROLL
        for (int i = 0; i < 4; ++i) {
            const int n = n0 + 8 * (lw + 4 * i) + rl;
            brow[i] = n < p.N ? (unsigned)(n * p.ldb + ub * 8) * 2u : DPC_BUF_OOB;
        }
        // A, row-major: piece j = lw + 4 i holds tile rows 8 j .. 8 j + 7 (same image as B).
        // A, K-major (TRANS_A): loader lw fills compute wave lw's sub-tile; piece i holds k-rows 8 i .. 8 i + 7, a lane fetches the 8
        // m-columns of slot (lane & 7) ^ 2 (k & 3).  Rows beyond K fall outside the buffer (zero fill); columns beyond M are masked here.
        const int ua = TRANS_A ? ((lane & 7) ^ (2 * (rl & 3))) : ub;
        DPC_UNROLL
        for (int i = 0; i < 8; ++i) {
            if (TRANS_A) {
                const int m = m0 + lw * 64 + ua * 8;
                arow[i] = m < p.M ? (unsigned)((8 * i + rl) * p.lda + m) * 2u : DPC_BUF_OOB;
            } else {
                const int m = m0 + 8 * (lw + 4 * i) + rl;
                arow[i] = m < p.M ? (unsigned)(m * p.lda + ua * 8) * 2u : DPC_BUF_OOB;
            }
        }
        // chunk offsets travel in the per-lane (bounds-checked) offset, not in the scalar one: a unit past the end of the buffer --
        // K-major rows beyond K -- is then zero-filled by the hardware; units that are in range but not part of the operand (the K
        // tail of a row-major row) are masked here
        auto issue = [&](int c, int stage) {
            unsigned char* st = lds + stage * STAGE;
            const int kc = c0 + c;
            const int klim = p.K - kc * 64;                               // elements of this chunk inside K (>= 64 except in the last chunk)
            const bool kok = ub * 8 < klim;                               // the unit starts inside K (gemm_ws_plan: what a straddling unit reads)
            const unsigned koff = (unsigned)kc * 128u;
            const unsigned aoff = TRANS_A ? (unsigned)kc * 64u * (unsigned)p.lda * 2u : koff;
            DPC_UNROLL
            for (int i = 0; i < 8; ++i) {
                const unsigned v = (TRANS_A || kok) ? arow[i] + aoff : DPC_BUF_OOB;   // OOB + offset stays >= 2 GB: out of range
                unsigned char* dst = TRANS_A ? st + lw * 8192 + i * 1024 : st + (lw + 4 * i) * 1024;
                glds16_buf(rs_a, v, 0u, dst, lane);
            }
            DPC_UNROLL
            for (int i = 0; i < 4; ++i) glds16_buf(rs_b, kok ? brow[i] + koff : DPC_BUF_OOB, 0u, st + BM * 128 + (lw + 4 * i) * 1024, lane);
        };
        issue(0, 0);
        if (total > 1) issue(1, 1);
        for (int gc = 0; gc < total; ++gc) {
            if (gc + 1 < total) wait_vmcnt<12>(); else wait_vmcnt<0>();
            ws_barrier();  // chunk gc is published; every reader is done with chunk gc-1
            if (gc + 2 < total) issue(gc + 2, (gc + 2) % NST);
        }
        ws_barrier();      // matches the compute waves' "tile fully read" barrier
        return;
    }

    // ---------------------------------------------------------------------- compute waves
    const int l31 = lane & 31, lhi = lane >> 5;
    const ldsa_t lds0 = ldsa(lds);
    const int fb0 = BM * 128 + lds_unit_off(l31, lhi);
    f32x16 acc[2][4] = {};
    ws_compute_prio();
    if (!TRANS_A) {
        const int fa0 = lds_unit_off(wv * 64 + l31, lhi);
        FragSet f0, f1;
        ws_barrier();  // first chunk published
        ldsa_t pa = lds0 + fa0, pb = lds0 + fb0;
        frag_read_p2<4096>(f0, pa, pb);
        for (int gc = 0; gc < total; ++gc) {
            step_il<true, 4096>(acc, f0, f1, pa ^ 32, pb ^ 32);
            step_il<true, 4096>(acc, f1, f0, pa ^ 64, pb ^ 64);
            step_il<true, 4096>(acc, f0, f1, pa ^ 96, pb ^ 96);
            frag_wait<0>(f1);
            ws_barrier();  // next chunk published -- or, after the last chunk, "tile fully read"
            pa = lds0 + ((gc + 1) % NST) * STAGE + fa0;
            pb = lds0 + ((gc + 1) % NST) * STAGE + fb0;
            step_il<true, 4096>(acc, f1, f0, pa, pb);   // after the last chunk these reads fetch nothing useful (MFMAs stay out of a branch) ...
        }
        WS_RETIRE_TAIL_READS(f0);                       // ... and are retired before their registers are handed on
    } else {
#ifdef DPC_SIMT_EMU
        // functional form for the host simulator: same LDS image, same fragment addresses, no pipelining
        int fo[2];
        {
            const int gq = lane >> 4, s16 = lane & 15;
            for (int i = 0; i < 2; ++i) {
                const int colb = (i * 32 + (gq & 1) * 16 + 4 * (s16 & 3)) * 2;
                fo[i] = ((gq >> 1) * 8 + (s16 >> 2)) * 128 + ((((colb >> 4) ^ (2 * (s16 >> 2))) & 7) << 4) + (colb & 15);
            }
        }
        ws_barrier();
        for (int gc = 0; gc < total; ++gc) {
            const unsigned char* st = lds + (gc % NST) * STAGE;
            for (int kk = 0; kk < 4; ++kk) {
                u32x4 fa[2], fbv[4];
                for (int i = 0; i < 2; ++i) {
                    const u32x2 lo = lds_read_tr16(st + wv * 8192 + fo[i] + kk * 2048);
                    const u32x2 hi = lds_read_tr16(st + wv * 8192 + fo[i] + kk * 2048 + 512);
                    u32x4 t = {lo[0], lo[1], hi[0], hi[1]};
                    fa[i] = t;
                }
                for (int j = 0; j < 4; ++j) fbv[j] = *(const u32x4*)(st + ((fb0 + 4096 * j) ^ (kk << 5)));
                for (int i = 0; i < 2; ++i)
                    for (int j = 0; j < 4; ++j) acc[i][j] = mfma_32x32x16_bf16(fbv[j], fa[i], acc[i][j]);
            }
            ws_barrier();
        }
#else
        // transpose-read lane offsets inside a [64 k][64 m] sub-tile (wgrad2_kernel's): lanes 0-31 fetch k 0..3 (lo) / 4..7 (hi),
        // lanes 32-63 k 8..11 / 12..15 of K step 0; step kk is 2 048 bytes further
        int fo[2];
        {
            const int gq = lane >> 4, s16 = lane & 15;
            DPC_UNROLL
            for (int i = 0; i < 2; ++i) {
                const int colb = (i * 32 + (gq & 1) * 16 + 4 * (s16 & 3)) * 2;
                fo[i] = ((gq >> 1) * 8 + (s16 >> 2)) * 128 + ((((colb >> 4) ^ (2 * (s16 >> 2))) & 7) << 4) + (colb & 15);
            }
        }
        FragSetT f0, f1;
        ws_barrier();  // first chunk published
        ldsa_t a0 = lds0 + wv * 8192 + fo[0], a1 = lds0 + wv * 8192 + fo[1], pb = lds0 + fb0;
        fragt_read<0>(f0, a0, a1, pb);
        for (int gc = 0; gc < total; ++gc) {
            step_il_t<1>(acc, f0, f1, a0, a1, pb ^ 32);
            step_il_t<2>(acc, f1, f0, a0, a1, pb ^ 64);
            step_il_t<3>(acc, f0, f1, a0, a1, pb ^ 96);
            frag_wait<0>(f1);
            ws_barrier();
            const int nb = ((gc + 1) % NST) * STAGE;
            a0 = lds0 + nb + wv * 8192 + fo[0];
            a1 = lds0 + nb + wv * 8192 + fo[1];
            pb = lds0 + nb + fb0;
            step_il_t<0>(acc, f1, f0, a0, a1, pb);
        }
        WS_RETIRE_TAIL_READS(f0);   // the reads past the last chunk land before their registers are handed on
#endif
    }

    // ---- epilogue: the wave's 64 x 128 f32 block through its own 33 KB of the (now free) ring, out as whole 512-byte rows
    unsigned char* mine = lds + wv * (64 * GW_STG_ROW);
    DPC_UNROLL
    for (int i = 0; i < 2; ++i)
        DPC_UNROLL
        for (int j = 0; j < 4; ++j)
            DPC_UNROLL
            for (int k = 0; k < 4; ++k) {
                const float e0 = acc[i][j][4 * k], e1 = acc[i][j][4 * k + 1], e2 = acc[i][j][4 * k + 2], e3 = acc[i][j][4 * k + 3];
                const u32x4 v = {__builtin_bit_cast(unsigned, e0), __builtin_bit_cast(unsigned, e1), __builtin_bit_cast(unsigned, e2),
                                 __builtin_bit_cast(unsigned, e3)};
                *(u32x4*)(mine + (i * 32 + l31) * GW_STG_ROW + (j * 32 + 8 * k + 4 * lhi) * 4) = v;
            }
    wave_lds_fence();
    float* slab = p.part + (long long)ks * p.M * p.N;
    const int cu = lane & 31, er = lane >> 5;       // 16-byte unit of the row (32 units = 128 columns), row parity
    const int col = n0 + cu * 4;
    DPC_UNROLL
    for (int it = 0; it < 32; ++it) {
        const int r = 2 * it + er;
        const int row = m0 + wv * 64 + r;
        const u32x4 v = *(const u32x4*)(mine + r * GW_STG_ROW + cu * 16);
        if (row < p.M && col < p.N) *(u32x4*)(slab + (long long)row * p.N + col) = v;
    }
}

// plans (and, with pointers, launches) the loader / compute split-K GEMM; returns 1 when the shape is not served
static int gemm_ws_plan(int trans_a, int M, int N, int K, int lda, int ldb, GemmWsParams* p) {
    static const int on = env_int("DPC_GEMM_WS", 1);
    if (!on) return 1;
    const int min_dim = env_int("DPC_GEMM_WS_MIN", 1024);                              // (read per call: the test tiers lower it for small shapes)
    if (N % 128 || lda % 8 || ldb % 8 || M < min_dim || K < min_dim) return 1;         // the contrastive head's shapes; everything else: generic kernel
    // 16-byte units must not straddle the end of an operand row.  Row-major A: K % 8 == 0.  K-major A: its rows beyond K are
    // zero-filled by the buffer bounds, so the last unit of a B row may run into the row's padding (ldb >= K rounded up, finite
    // values there), and the last unit of an A row into its padding (lda >= M rounded up; those output rows are not stored)
    if (!trans_a && K % 8) return 1;
    if (trans_a && (lda < (M + 7) / 8 * 8 || ldb < (K + 7) / 8 * 8)) return 1;
    const long long a_bytes = trans_a ? (long long)K * lda * 2 : (long long)M * lda * 2;
    const long long b_bytes = (long long)N * ldb * 2;
    if (a_bytes >= (1ll << 31) || b_bytes >= (1ll << 31)) return 1;                    // 32-bit buffer offsets (DPC_BUF_OOB = 2 GB)
    p->M = M; p->N = N; p->K = K; p->lda = lda; p->ldb = ldb;
    p->a_bytes = (unsigned)a_bytes; p->b_bytes = (unsigned)b_bytes;
    p->ntm = (M + 255) / 256; p->ntn = N / 128;
    const int tiles = p->ntm * p->ntn, nch = (K + 63) / 64;
    // The slice count is a function of the SHAPE alone: the caller sizes `part` from a planning call and launches later, possibly
    // with another CU carve-out in force (dpc_set_reserved_cus) -- a count that followed the carve-out could outgrow the buffer
    // (ADVICE r4).  These products run at the head of the backward pass, before any exchange is in flight: all 256 CUs.
    const int cus = 256;
    int want = cus / tiles;                        // slices so that tiles x slices fills the chip once ...
    if (want > nch / 8) want = nch / 8;            // ... and every slice amortises its 128 KB slab over >= 8 chunks
    if (want < 1) want = 1;
    p->cps = (nch + want - 1) / want;
    p->nks = (nch + p->cps - 1) / p->cps;
    return 0;
}

int dpc_gemm_ws_try(int trans_a, int M, int N, int K, const void* A, int lda, const void* B, int ldb, float* part, int32_t* nsplit,
                    hipStream_t stream) {
    GemmWsParams p;
    if (gemm_ws_plan(trans_a, M, N, K, lda, ldb, &p)) return 1;
    if (part && ((((uintptr_t)A | (uintptr_t)B | (uintptr_t)part) % 16) != 0)) return 1;
    if (nsplit) *nsplit = p.nks;
    if (!part) return DPC_OK;
    if (!A || !B) return DPC_ERR_ARG;
    p.A = A; p.B = B; p.part = part;
    dpc_plan_detail("splitk=%d", p.nks);
    dim3 grid((unsigned)(p.ntm * p.ntn * p.nks)), block(512);
    if (trans_a) {
        DPC_LAUNCH((gemm_ws_kernel<true>), grid, block, stream, p);
    } else {
        DPC_LAUNCH((gemm_ws_kernel<false>), grid, block, stream, p);
    }
    return dpc_launch_status();
}

// part[ks][M][N] (f32) = A^T @ B^T over K slice ks, A given K-major: A[k][m] with row stride lda -- d_finf = dS^T @ pred with
// A = dS (rows r = k), B = pred^T [D][R].  Same slab convention as dpc_gemm_nt_splitk.
extern "C" int dpc_gemm_tn_splitk(int32_t dtype, int32_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* B, int32_t ldb,
                                  float* part, int32_t* nsplit, dpc_stream_t stream_) {
    if (M <= 0 || N <= 0 || K <= 0 || lda < M || ldb < K) return DPC_ERR_ARG;
    if (dtype != DPC_BF16) return DPC_ERR_UNSUPPORTED;
    const int rc = dpc_gemm_ws_try(1, M, N, K, A, lda, B, ldb, part, nsplit, (hipStream_t)stream_);
    return rc == 1 ? DPC_ERR_UNSUPPORTED : rc;
}
