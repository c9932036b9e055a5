// neg_queue.hip -- the negative queue of the contrastive loss: the keys (feature_inf, the encoded future blocks) of the last K training
// batches stay on the device and compete, detached, against every training row.  A row of the score then has R + Q columns, Q up to
// K * R: a materialised [R][R(1 + K)] pair of logits and gradient would be 1.4 GB per step at cfg2 / K = 8 and the register-resident
// row kernels of loss.hip stop at 16 384 columns, so the queue part is contracted flash-style, tile by tile on the matrix cores, with
// the tile helpers of score_fused.hip (score_tile.h):
//
//   dpc_negq_fwd   per row (max, sum-exp, #{s > target}) over the live keys -- score_fwd_kernel with the bank as the streamed operand
//                  and no target column; the column splits are merged in split order by negq_merge_kernel.  dpc_ce_topk[_bf16]_ext
//                  (loss.hip) folds the triple into the in-batch row's log-sum-exp and rank.
//   dpc_negq_bwd   f32 slabs of sum_c exp(s_ic - lse_i) / R * q_c -- score_bwd_kernel with by_owner = 1 and no diagonal term: S is
//                  recomputed, dS rounded to bf16 through the wave-private LDS tile, second product against the transposed ring.
//   dpc_negq_push  feature_inf (and its transpose) -> the slot the device record names; dpc_negq_clear: the record back to empty.
//
// Ring: K slots of pitch = roundup(R, 64) rows of D bf16, one allocation, so the ring is a [K * pitch][D] matrix and the 64-row tile
// jt is rows [64 jt, 64 jt + 64) of it, inside ONE slot (jt / (pitch / 64)).  Slots fill in order 0 .. K-1 and stay full afterwards,
// so the live tiles are the prefix [0, filled * pitch / 64): liveness is one comparison against a value read from the record, uniform
// over the workgroup.  Dead tiles are never loaded; rows >= R of a slot come in as zeros (the DMA's row limit) and their columns of S
// are masked in the slot's last tile (the only edge tile); the columns >= R of the transposed tile are zeroed in LDS before use.  The
// grid and every argument are those of a full bank: a workgroup whose column range is dead writes the empty result and returns.
#include "score_tile.h"

namespace {

constexpr float EMPTY_MAX = -1.0e30f;

struct NegqP {
    const bf16_t* own;            // pred [R][D]
    const bf16_t* ring;           // [K * pitch][D]
    const bf16_t* ringT;          // [K][D][pitch] (backward)
    const dpc_negq_state* state;
    int R, D, K, pitch, tps_slot; // tiles per slot = pitch / 64
    int tiles_per_split, nsplit;
    // forward
    const void* tgt;
    long long tgt_stride;
    int tgt_bf16;
    float* partial;               // [nsplit][R][4]
    // backward
    const float* lse;             // [R] natural log-sum-exp over all R + Q columns
    float* out_part;              // [nsplit][R][D]
};

// column splits over the tiles of a FULL bank (the launch is the same every step), each keeping at least 4 tiles
void plan_negq(int R, int K, int target_wgs, int* tps, int* nsplit) {
    const int nrb = (R + BM - 1) / BM;
    const int ntiles = K * (DPC_NEGQ_PITCH(R) / BN);
    int s = (target_wgs + nrb - 1) / nrb;
    if (s < 1) s = 1;
    const int max_s = ntiles / 4 > 0 ? ntiles / 4 : 1;
    if (s > max_s) s = max_s;
    if (s > 16) s = 16;
    *tps = (ntiles + s - 1) / s;
    *nsplit = (ntiles + *tps - 1) / *tps;
}

// the live tile range of a split: [jt0, jt1), empty when the bank has not reached it
__device__ __forceinline__ void live_range(const NegqP& p, int split, int& jt0, int& jt1) {
    int filled = p.state->filled;
    if (filled < 0) filled = 0;
    if (filled > p.K) filled = p.K;
    const int live = filled * p.tps_slot;
    jt0 = split * p.tiles_per_split;
    jt1 = jt0 + p.tiles_per_split;
    if (jt1 > live) jt1 = live;
}

__device__ __forceinline__ void dma_ring_tile(unsigned char* tile, const NegqP& p, int jt, int wave, int lane) {
    const int slot = jt / p.tps_slot;
    dma_rows(tile, p.ring, p.D, jt * BN, BN, slot * p.pitch + p.R, 0, p.D, p.D, wave, lane);
}

// ---------------------------------------------------------------- forward
// tile_stats of score_fused.hip without a target column.  EDGE: the slot's last tile when R % 64 != 0 (columns >= ncol are padding)
template <bool EDGE>
__device__ __forceinline__ void negq_tile_stats(const f32x16 (&s)[2], float (&m)[16], float (&l)[16], float (&rk)[16], const float (&dg)[16],
                                                int ncol, int lane) {
    const int c0 = lane & 31, c1 = c0 + 32;
    DPC_UNROLL
    for (int r = 0; r < 16; ++r) {
        float v0 = s[0][r], v1 = s[1][r];
        bool a0 = v0 > dg[r], a1 = v1 > dg[r];
        if (EDGE) {
            if (c0 >= ncol) { v0 = NEG_BIG; a0 = false; }
            if (c1 >= ncol) { v1 = NEG_BIG; a1 = false; }
        }
        rk[r] += (a0 ? 1.f : 0.f) + (a1 ? 1.f : 0.f);
        const float mx = fmaxf(fmaxf(v0, v1), m[r]);
        const float nm = -mx * L2E;
        l[r] = l[r] * fast_exp2((m[r] - mx) * L2E) + fast_exp2(fmaf(v0, L2E, nm)) + fast_exp2(fmaf(v1, L2E, nm));
        m[r] = mx;
    }
}

template <int KS>
__global__ __launch_bounds__(256, 2) void negq_fwd_kernel(NegqP p) {
    DPC_DYN_SMEM(smem);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rb = blockIdx.x, split = blockIdx.y;
    const int r0 = rb * BM + wave * 32;
    const int tile_bytes = ((KS * 32 + 127) / 128) * BN * 128;
    int jt0, jt1;
    live_range(p, split, jt0, jt1);
    if (jt0 >= jt1) {   // a dead column range (uniform over the workgroup): the empty triple, nothing loaded
        const int row = rb * BM + threadIdx.x;
        if (threadIdx.x < BM && row < p.R) {
            float* o = p.partial + ((long long)split * p.R + row) * 4;
            o[0] = EMPTY_MAX; o[1] = 0.f; o[2] = 0.f; o[3] = 0.f;
        }
        return;
    }
    u32x4 own[KS];
    load_own_ld<KS>(own, p.own, p.D, p.R, r0, lane);
    float dg[16];
    {
        const int row = r0 + (lane & 31);
        float t = 0.f;
        if (row < p.R) {
            if (p.tgt_bf16) t = bf16_to_f32(((const bf16_t*)p.tgt)[(long long)row * p.tgt_stride]);
            else t = ((const float*)p.tgt)[(long long)row * p.tgt_stride];
        }
        DPC_UNROLL
        for (int r = 0; r < 16; ++r) dg[r] = __shfl(t, crow(r, lane));
    }
    float m[16], l[16], rk[16];
    DPC_UNROLL
    for (int r = 0; r < 16; ++r) { m[r] = EMPTY_MAX; l[r] = 0.f; rk[r] = 0.f; }
    const int rem = p.R - (p.tps_slot - 1) * BN;   // valid columns of a slot's last tile
    dma_ring_tile(smem, p, jt0, wave, lane);
    for (int jt = jt0; jt < jt1; ++jt) {
        const int buf = (jt - jt0) & 1;
        wait_vmcnt<0>();
        __syncthreads();  // tile jt has landed; every wave is done with the buffer the next DMA overwrites
        if (jt + 1 < jt1) dma_ring_tile(smem + (buf ^ 1) * tile_bytes, p, jt + 1, wave, lane);
        f32x16 s[2];
        s_tile<KS>(s, own, smem + buf * tile_bytes, lane);
        const bool edge = rem < BN && (jt % p.tps_slot) == p.tps_slot - 1;  // wave-uniform
        if (edge) negq_tile_stats<true>(s, m, l, rk, dg, rem, lane);
        else negq_tile_stats<false>(s, m, l, rk, dg, BN, lane);
    }
    DPC_UNROLL
    for (int r = 0; r < 16; ++r) {
        DPC_UNROLL
        for (int msk = 1; msk <= 16; msk <<= 1) {
            const float om = __shfl_xor(m[r], msk), ol = __shfl_xor(l[r], msk), ork = __shfl_xor(rk[r], msk);
            const float mx = om > m[r] ? om : m[r];
            l[r] = l[r] * fast_exp2((m[r] - mx) * L2E) + ol * fast_exp2((om - mx) * L2E);
            m[r] = mx;
            rk[r] += ork;
        }
        const int grow = r0 + crow(r, lane);
        if ((lane & 31) == 0 && grow < p.R) {
            float* o = p.partial + ((long long)split * p.R + grow) * 4;
            o[0] = m[r]; o[1] = l[r]; o[2] = rk[r]; o[3] = 0.f;
        }
    }
}

// per row: the column splits merged in split order -> (m, l, rk, 0)
__global__ void negq_merge_kernel(const float* partial, int R, int nsplit, float* stats) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= R) return;
    float M = EMPTY_MAX;
    for (int s = 0; s < nsplit; ++s) {
        const float v = partial[((long long)s * R + row) * 4];
        M = v > M ? v : M;
    }
    float Lsum = 0.f, rk = 0.f;
    for (int s = 0; s < nsplit; ++s) {
        const float* q = partial + ((long long)s * R + row) * 4;
        Lsum += q[1] * exp2f((q[0] - M) * L2E);   // a dead split holds (-1e30, 0): its term is 0 * 1 or 0 * 0
        rk += q[2];
    }
    float* o = stats + (long long)row * 4;
    o[0] = M; o[1] = Lsum; o[2] = rk; o[3] = 0.f;
}

// ---------------------------------------------------------------- backward
template <int KS>
__global__ __launch_bounds__(256) void negq_bwd_kernel(NegqP p) {
    DPC_DYN_SMEM(smem);
    constexpr int NTD = KS / 2;  // 32-column tiles of D
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rb = blockIdx.x, split = blockIdx.y;
    const int r0 = rb * BM + wave * 32;
    const int tile_bytes = ((KS * 32 + 127) / 128) * BN * 128;   // ring tile: 64 rows x D*2 bytes in 128-byte chunks
    const int tileT_bytes = KS * 16 * 128;                       // ringT tile: D rows x 128 bytes
    const int stage_bytes = tile_bytes + tileT_bytes;
    unsigned char* ptile = smem + 2 * stage_bytes + wave * (32 * 128);  // wave-private dS tile: 32 rows x 64 bf16
    float* o = p.out_part + (long long)split * p.R * p.D;
    int jt0, jt1;
    live_range(p, split, jt0, jt1);
    if (jt0 >= jt1) {   // a dead column range: a zero slab (the caller sums a fixed number of slabs), nothing loaded
        const int rows = p.R - rb * BM < BM ? p.R - rb * BM : BM;
        float* ob = o + (long long)rb * BM * p.D;
        for (int i = threadIdx.x; i < rows * p.D; i += 256) ob[i] = 0.f;
        return;
    }
    u32x4 own[KS];
    load_own_ld<KS>(own, p.own, p.D, p.R, r0, lane);
    f32x16 out[NTD];
    DPC_UNROLL
    for (int n = 0; n < NTD; ++n)
        DPC_UNROLL
        for (int r = 0; r < 16; ++r) out[n][r] = 0.f;
    float lo[16];   // (lse + ln R) log2(e) of the wave's rows
    const float lnR = logf((float)p.R);
    DPC_UNROLL
    for (int r = 0; r < 16; ++r) {
        const int grow = r0 + crow(r, lane);
        lo[r] = grow < p.R ? (p.lse[grow] + lnR) * L2E : 0.f;
    }
    const int rem = p.R - (p.tps_slot - 1) * BN;
    auto dma_stage = [&](unsigned char* st, int jt) {
        const int slot = jt / p.tps_slot, t = jt - slot * p.tps_slot;
        dma_ring_tile(st, p, jt, wave, lane);
        dma_rows(st + tile_bytes, p.ringT + (long long)slot * p.D * p.pitch, p.pitch, 0, KS * 16, KS * 16, t * BN, BN, p.R, wave, lane);
    };
    dma_stage(smem, jt0);
    for (int jt = jt0; jt < jt1; ++jt) {
        const int buf = (jt - jt0) & 1;
        wait_vmcnt<0>();
        __syncthreads();
        unsigned char* tile = smem + buf * stage_bytes;
        unsigned char* tileT = tile + tile_bytes;
        const bool edge = rem < BN && (jt % p.tps_slot) == p.tps_slot - 1;  // uniform over the workgroup
        if (edge) {   // the 16-byte unit that straddles column R brought padding along: zero the columns >= rem of the transposed tile
            for (int i = threadIdx.x; i < KS * 16 * (BN - rem); i += 256) {
                const int d = i / (BN - rem), cl = rem + (i - d * (BN - rem));
                *(bf16_t*)(tileT + lds_unit_off(d, cl >> 3) + (cl & 7) * 2) = (bf16_t)0;
            }
            __syncthreads();
        }
        if (jt + 1 < jt1) dma_stage(smem + (buf ^ 1) * stage_bytes, jt + 1);
        f32x16 s[2];
        s_tile<KS>(s, own, tile, lane);
        DPC_UNROLL
        for (int t = 0; t < 2; ++t) {
            const int cl = t * 32 + (lane & 31);
            const bool cv = !edge || cl < rem;
            unsigned char* pcol = ptile + (cl & 7) * 2;
            DPC_UNROLL
            for (int r = 0; r < 16; ++r) {
                float g = fast_exp2(fmaf(s[t][r], L2E, -lo[r]));
                if (!cv) g = 0.f;
                *(bf16_t*)(pcol + lds_unit_off(crow(r, lane), cl >> 3)) = f32_to_bf16(g);
            }
        }
        wave_lds_fence();
        {   // out[n] += dS[32 x 64] @ ringT[n][64]^T (score_bwd_kernel's second product)
            const int i = lane & 31, kg = lane >> 5;
            u32x4 a[4], b[4][NTD];
            auto req = [&](auto k2_) {
                constexpr int k2 = decltype(k2_)::value;
                const int unit = k2 * 2 + kg;
                lds_read_b128_async(a[k2], ptile + lds_unit_off(i, unit));
                const unsigned char* b0 = tileT + lds_unit_off(i, unit);
                static_for<NTD>([&](auto n_) {
                    constexpr int n = decltype(n_)::value;
                    lds_read_b128_async_off<n * 32 * 128>(b[k2][n], b0);
                });
            };
            req(std::integral_constant<int, 0>{});
            static_for<4>([&](auto k2_) {
                constexpr int k2 = decltype(k2_)::value;
                if constexpr (k2 + 1 < 4) req(std::integral_constant<int, k2 + 1>{});
                constexpr int later = k2 + 1 < 4 ? 1 + NTD : 0;
                static_for<NTD>([&](auto n_) {
                    constexpr int n = decltype(n_)::value;
                    lds_wait_tie<later>(a[k2], b[k2][n]);
                    out[n] = mfma_32x32x16_bf16(a[k2], b[k2][n], out[n]);
                });
            });
        }
        wave_lds_fence();  // the wave's next dS stores must not pass these reads
    }
    DPC_UNROLL
    for (int n = 0; n < NTD; ++n)
        DPC_UNROLL
        for (int r = 0; r < 16; ++r) {
            const int grow = r0 + crow(r, lane);
            if (grow < p.R) o[(long long)grow * p.D + n * 32 + (lane & 31)] = out[n][r];
        }
}

// ---------------------------------------------------------------- ring
// 16-byte units: [0, R * D / 8) of finf -> the slot's rows; then D rows of ldT / 8 units of finfT -> the slot's transposed rows
__global__ void negq_push_kernel(const u32x4* finf, const u32x4* finfT, int ldT8, u32x4* ring, u32x4* ringT, const dpc_negq_state* state,
                                 long long n_rows8, int D, int K, long long slot_units, int pitch8) {
    const int slot = (int)((unsigned)state->pushes % (unsigned)K);
    const long long nT = ringT ? (long long)D * ldT8 : 0;
    u32x4* dst = ring + slot * slot_units;
    u32x4* dstT = ringT ? ringT + slot * slot_units : nullptr;   // D * pitch / 8 = pitch * D / 8 units per slot, both rings
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_rows8 + nT; i += (long long)gridDim.x * blockDim.x) {
        if (i < n_rows8) {
            dst[i] = finf[i];
        } else {
            const long long j = i - n_rows8;
            const long long d = j / ldT8, u = j - d * ldT8;
            dstT[d * pitch8 + u] = finfT[j];
        }
    }
}

__global__ void negq_advance_kernel(dpc_negq_state* state, int K) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        state->pushes += 1;
        const int f = state->filled + 1;
        state->filled = f < K ? f : K;
    }
}

__global__ void negq_clear_kernel(dpc_negq_state* state, const dpc_grad_state* guard) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && (!guard || guard->skip)) {
        state->pushes = 0;
        state->filled = 0;
    }
}

bool negq_shape_ok(int R, int D, int K) { return R > 0 && K >= 1 && K <= DPC_NEGQ_MAX_SLOTS && (long long)K * DPC_NEGQ_PITCH(R) < (1ll << 30); }

}  // namespace

extern "C" int dpc_negq_ws_floats(int32_t R, int32_t D, int32_t K, int64_t* fwd_floats, int64_t* bwd_floats) {
    if (!negq_shape_ok(R, D, K) || D <= 0 || !fwd_floats || !bwd_floats) return DPC_ERR_ARG;
    if (D != 256 && D != 32) return DPC_ERR_UNSUPPORTED;
    int tps, nsf, nsb;
    plan_negq(R, K, 512, &tps, &nsf);   // forward: two workgroups per CU
    plan_negq(R, K, 256, &tps, &nsb);
    *fwd_floats = (int64_t)nsf * R * 4;
    *bwd_floats = (int64_t)nsb * R * D;
    return nsb;
}

extern "C" int dpc_negq_push(const void* finf, const void* finfT, int32_t ldT, void* ring, void* ringT, dpc_negq_state* state, int32_t R,
                             int32_t D, int32_t K, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!finf || !ring || !state || !negq_shape_ok(R, D, K) || D <= 0) return DPC_ERR_ARG;
    if (D != 256 && D != 32) return DPC_ERR_UNSUPPORTED;
    const int pitch = DPC_NEGQ_PITCH(R);
    if ((finfT != nullptr) != (ringT != nullptr)) return DPC_ERR_ARG;
    if (finfT && (ldT < R || ldT % 8 || ldT > pitch)) return DPC_ERR_ARG;
    if (((uintptr_t)finf | (uintptr_t)finfT | (uintptr_t)ring | (uintptr_t)ringT) % 16 || (uintptr_t)state % 4) return DPC_ERR_ARG;
    const long long n_rows8 = (long long)R * D / 8, total = n_rows8 + (finfT ? (long long)D * (ldT / 8) : 0);
    long long grid = (total + 255) / 256;
    if (grid > 4096) grid = 4096;
    DPC_LAUNCH(negq_push_kernel, dim3((unsigned)grid), dim3(256), stream, (const u32x4*)finf, (const u32x4*)finfT, ldT / 8, (u32x4*)ring,
               (u32x4*)ringT, (const dpc_negq_state*)state, n_rows8, D, K, (long long)pitch * D / 8, pitch / 8);
    DPC_LAUNCH(negq_advance_kernel, dim3(1), dim3(64), stream, state, K);
    return dpc_launch_status();
}

extern "C" int dpc_negq_clear(dpc_negq_state* state, const dpc_grad_state* guard, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!state || (uintptr_t)state % 4) return DPC_ERR_ARG;
    DPC_LAUNCH(negq_clear_kernel, dim3(1), dim3(64), stream, state, guard);
    return dpc_launch_status();
}

static int negq_fill(NegqP& p, const void* pred, const void* ring, const void* ringT, const dpc_negq_state* state, int R, int D, int K,
                     int target_wgs) {
    p.own = (const bf16_t*)pred; p.ring = (const bf16_t*)ring; p.ringT = (const bf16_t*)ringT; p.state = state;
    p.R = R; p.D = D; p.K = K; p.pitch = DPC_NEGQ_PITCH(R); p.tps_slot = p.pitch / BN;
    plan_negq(R, K, target_wgs, &p.tiles_per_split, &p.nsplit);
    return DPC_OK;
}

extern "C" int dpc_negq_fwd(const void* pred, const void* ring, const dpc_negq_state* state, int32_t R, int32_t D, int32_t K, const void* tgt,
                            int64_t tgt_stride, int32_t tgt_dtype, float* stats, float* ws, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!pred || !ring || !state || !tgt || !stats || !ws || !negq_shape_ok(R, D, K) || D <= 0 || tgt_stride < 0) return DPC_ERR_ARG;
    if (tgt_dtype != DPC_F32 && tgt_dtype != DPC_BF16) return DPC_ERR_ARG;
    if (D != 256 && D != 32) return DPC_ERR_UNSUPPORTED;
    if (((uintptr_t)pred | (uintptr_t)ring) % 16 || (uintptr_t)state % 4) return DPC_ERR_ARG;
    NegqP p = {};
    negq_fill(p, pred, ring, nullptr, state, R, D, K, 512);
    p.tgt = tgt; p.tgt_stride = tgt_stride; p.tgt_bf16 = tgt_dtype == DPC_BF16; p.partial = ws;
    const dim3 grid((R + BM - 1) / BM, p.nsplit);
    const size_t lds = 2 * (size_t)((D * 2 + 127) / 128) * BN * 128;
    if (D == 256) {
        if (int e = allow_lds(negq_fwd_kernel<16>, lds)) return e;
        DPC_LAUNCH_DYN((negq_fwd_kernel<16>), grid, dim3(256), lds, stream, p);
    } else {
        if (int e = allow_lds(negq_fwd_kernel<2>, lds)) return e;
        DPC_LAUNCH_DYN((negq_fwd_kernel<2>), grid, dim3(256), lds, stream, p);
    }
    DPC_LAUNCH(negq_merge_kernel, dim3((R + 255) / 256), dim3(256), stream, (const float*)ws, R, p.nsplit, stats);
    return dpc_launch_status();
}

extern "C" int dpc_negq_bwd(const void* pred, const void* ring, const void* ringT, const dpc_negq_state* state, int32_t R, int32_t D,
                            int32_t K, const float* lse, float* out_part, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!pred || !ring || !ringT || !state || !lse || !out_part || !negq_shape_ok(R, D, K) || D <= 0) return DPC_ERR_ARG;
    if (D != 256 && D != 32) return DPC_ERR_UNSUPPORTED;
    if (((uintptr_t)pred | (uintptr_t)ring | (uintptr_t)ringT) % 16 || (uintptr_t)state % 4) return DPC_ERR_ARG;
    NegqP p = {};
    negq_fill(p, pred, ring, ringT, state, R, D, K, 256);
    p.lse = lse; p.out_part = out_part;
    const dim3 grid((R + BM - 1) / BM, p.nsplit);
    const size_t chunk_tile = (size_t)((D * 2 + 127) / 128) * BN * 128;
    const size_t lds = 2 * (chunk_tile + (size_t)D * 128) + 4 * 32 * 128;
    if (D == 256) {
        if (int e = allow_lds(negq_bwd_kernel<16>, lds)) return e;
        DPC_LAUNCH_DYN((negq_bwd_kernel<16>), grid, dim3(256), lds, stream, p);
    } else {
        if (int e = allow_lds(negq_bwd_kernel<2>, lds)) return e;
        DPC_LAUNCH_DYN((negq_bwd_kernel<2>), grid, dim3(256), lds, stream, p);
    }
    const int rc = dpc_launch_status();
    return rc ? rc : p.nsplit;
}
