// retrieval.hip -- nearest-neighbour video retrieval on the device: one L2-normalised embedding per video, cosine neighbours in a
// gallery, recall@k and the 1-NN confusion matrix.
//   embed_accumulate  per chunk of windows: rows [0, n_valid) of ctx [rows][ld] added onto esum [D] IN ROW ORDER, windows counted
//   embed_finish      per video: m = esum / count, out = m / max(||m||_2, eps) (F.normalize); the per-video state is cleared
//   knn_topk          sim(i, j) = sum_d Q[i][d] G[j][d] on the exact-f32 matrix instruction, accumulated in ascending d, and per query
//                     the K best gallery rows by (sim descending, index ascending).  Two kernels:
//                       knn_partial  one workgroup per (32-query tile, gallery slab).  Per round each of its 4 waves computes one
//                                    32 x 32 similarity tile into LDS; then each wave selects for 8 of the queries from the 128
//                                    candidates of the round.  A query's sorted list is held in registers, one entry per lane;
//                                    what beats its K-th entry is found and inserted by wave votes.  The lists go to `ws`.
//                       knn_merge    one wave per query: lane s holds the head of slab s's list, K rounds of a wave-wide maximum.
//                     The nq x ng similarity matrix exists only as accumulator tiles.  (sim, index) is a strict total order over the
//                     candidates of a query and sim(i, j) is the same fma chain whichever tile computes it, so the result is the
//                     same bits for every slab count.
//   knn_recall        first_hit[i] = rank of the first neighbour with the query's label, hits[j] += #{i : first_hit[i] < ks[j]},
//                     confusion[label of the first neighbour][label of the query] += 1.  One workgroup, one writer per value.
// No atomics anywhere: same inputs, same bits.
#include "dpc_rt.h"
#include "../../include/dpc_hip.h"

namespace {

constexpr int KNN_TILE = 32;         // queries per workgroup = gallery rows per MFMA tile
constexpr int KNN_WAVES = 4;
constexpr int KNN_MAX_K = 64, KNN_MAX_SLABS = 64;
constexpr int KNN_CUS = 256;         // MI355X; the automatic slab count aims at two workgroups per CU
constexpr int KNN_EMPTY = 0x7fffffff;   // index of a slot without a candidate (sorts behind every real row; -1 on the way out)

struct Cand {
    float sim;
    int idx;
};

__device__ __forceinline__ float neg_inf() { return -__builtin_inff(); }
// the order of a neighbour list: similarity descending, then gallery index ascending
__device__ __forceinline__ bool better(float s, int i, float ts, int ti) { return s > ts || (s == ts && i < ti); }

__device__ __forceinline__ float wave_sum(float v) {
    DPC_UNROLL
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
    DPC_UNROLL
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// ---------------------------------------------------------------- embeddings
// one workgroup; thread j owns component j (j + 256, ..) and adds the rows in row order
__global__ __launch_bounds__(256) void embed_accumulate_kernel(const float* ctx, int n_valid, int D, int ld, float* esum, int32_t* count) {
    const int tid = threadIdx.x;
    for (int j = tid; j < D; j += 256) {
        float e = esum[j];
        for (int r = 0; r < n_valid; ++r) e += ctx[(long long)r * ld + j];
        esum[j] = e;
    }
    if (tid == 0) count[0] += n_valid;
}

__global__ __launch_bounds__(256) void embed_finish_kernel(float* esum, int32_t* count, int D, float eps, float* out) {
    __shared__ float sh[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = count[0];
    if (n <= 0) return;   // no window was accumulated: nothing is written
    const float fn = (float)n;
    float ss = 0.f;
    for (int j = tid; j < D; j += 256) { const float m = esum[j] / fn; ss += m * m; }
    ss = wave_sum(ss);    // a fixed tree: thread strides, the wave butterfly, then the four waves in order
    if (lane == 0) sh[wv] = ss;
    __syncthreads();      // also: every thread has read count[0]
    const float norm = sqrtf(sh[0] + sh[1] + sh[2] + sh[3]);
    const float den = norm > eps ? norm : eps;
    for (int j = tid; j < D; j += 256) {
        out[j] = esum[j] / fn / den;
        esum[j] = 0.f;    // thread j is the only reader and writer of component j
    }
    if (tid == 0) count[0] = 0;
}

// ---------------------------------------------------------------- top-K per (query tile, slab)
// LDS: sQ [D/4][64] float2 -- lane l = (query i = l & 31, half h = l >> 5) finds (Q[i][4t + h], Q[i][4t + 2 + h]) at [t][l]: the B
//      operands of MFMA steps 2t and 2t + 1 in one conflict-free 8-byte read; sS [4 waves][32 queries][36] f32 -- the similarity
//      tiles of one round (32 gallery rows each, 4 floats of padding per row).
// MFMA step s covers d = 2s (lane half 0) and 2s + 1 (half 1), the hardware adds them in that order: ascending d.
// A = gallery tile, B = query tile, so accumulator register r of lane l is sim(query l & 31, gallery row (r&3) + 8(r>>2) + 4h):
// four consecutive gallery rows per register group, one 16-byte store each.
constexpr int KNN_SROW = 36;

// one 32 x 32 similarity tile (gallery tile `tile` against the workgroup's queries) into dst [32 queries][KNN_SROW]
__device__ __forceinline__ void knn_tile(const float* G, int ng, int ldg, int DT, int tile, const float2* sQ, float* dst, int lane) {
    const int qi = lane & 31, h = lane >> 5;
    int grow = tile * KNN_TILE + qi;
    grow = grow < ng ? grow : ng - 1;   // rows past the gallery repeat its last row; the selection drops them
    const float* gp = G + (long long)grow * ldg;
    f32x16 acc;
    DPC_UNROLL
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    const float2* qf = sQ + lane;
    // 32 values of d per group (D is a multiple of 32): the next group's eight 16-byte loads fly under this group's 16 MFMAs
    float4 g[8];
    DPC_UNROLL
    for (int u = 0; u < 8; ++u) g[u] = *(const float4*)(gp + 4 * u);
    for (int t0 = 0; t0 < DT; t0 += 8) {
        float4 gn[8];
        const bool more = t0 + 8 < DT;   // wave-uniform
        if (more) {
            DPC_UNROLL
            for (int u = 0; u < 8; ++u) gn[u] = *(const float4*)(gp + 4 * (t0 + 8 + u));
        }
        DPC_UNROLL
        for (int u = 0; u < 8; ++u) {
            const float2 b = qf[(t0 + u) * 64];
            acc = mfma_32x32x2_f32(h ? g[u].y : g[u].x, b.x, acc);
            acc = mfma_32x32x2_f32(h ? g[u].w : g[u].z, b.y, acc);
        }
        if (more) {
            DPC_UNROLL
            for (int u = 0; u < 8; ++u) g[u] = gn[u];
        }
    }
    DPC_UNROLL
    for (int gq = 0; gq < 4; ++gq)
        *(float4*)(dst + qi * KNN_SROW + 8 * gq + 4 * h) = make_float4(acc[4 * gq], acc[4 * gq + 1], acc[4 * gq + 2], acc[4 * gq + 3]);
}

// A round: wave w computes gallery tile tb + w into sS, barrier, wave w selects for queries 8w .. 8w + 7 from all four tiles,
// barrier.  The list of a query lives in REGISTERS, entry e on lane e (K <= 64), sorted: of the 128 candidates of a round (two per
// lane) those that beat entry K - 1 are found by one vote; each is inserted with a vote (its position = how many entries are
// better), a shift by one lane and a lane select -- no loop over the list.
__global__ __launch_bounds__(256) void knn_partial_kernel(const float* Q, int nq, int ldq, const float* G, int ng, int ldg, int D, int K,
                                                          const int32_t* skip, int tiles_per_slab, int n_slabs, Cand* ws) {
    DPC_DYN_SMEM(smem);
    float2* sQ = (float2*)smem;
    float* sS = (float*)(smem + (size_t)D * 128);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, qi = lane & 31, h = lane >> 5;
    const int q0 = blockIdx.x * KNN_TILE, slab = blockIdx.y;
    const int n_gtiles = (ng + KNN_TILE - 1) / KNN_TILE;
    const int tile0 = slab * tiles_per_slab;
    const int tile1 = tile0 + tiles_per_slab < n_gtiles ? tile0 + tiles_per_slab : n_gtiles;
    const int DT = D >> 2;

    for (int e = tid; e < DT * 64; e += 256) {
        const int t = e >> 6, l = e & 63;
        int row = q0 + (l & 31);
        row = row < nq ? row : nq - 1;   // a tail tile repeats the last query; its lists are never written out
        const float* qp = Q + (long long)row * ldq + 4 * t + (l >> 5);
        sQ[e] = make_float2(qp[0], qp[2]);
    }
    __syncthreads();

    constexpr int QPW = KNN_TILE / KNN_WAVES;   // queries whose lists this wave keeps
    float ls[QPW], ts[QPW];                     // entry `lane` of the list of query q0 + QPW * wv + s; the similarity of its entry K - 1
    int li[QPW], ti[QPW], sk[QPW];              // .. and the gallery indices; the row the query must not return
    DPC_UNROLL
    for (int s = 0; s < QPW; ++s) {
        const int q = q0 + QPW * wv + s;
        ls[s] = ts[s] = neg_inf();
        li[s] = ti[s] = KNN_EMPTY;
        sk[s] = (skip && q < nq) ? skip[q] : -1;
    }
    for (int tb = tile0; tb < tile1; tb += KNN_WAVES) {
        if (tb + wv < tile1) knn_tile(G, ng, ldg, DT, tb + wv, sQ, sS + wv * KNN_TILE * KNN_SROW, lane);
        __syncthreads();
        // candidate c of the round: gallery row (tb + (c >> 5)) * 32 + (c & 31); this lane looks at c = lane and c = lane + 64
        DPC_UNROLL
        for (int s = 0; s < QPW; ++s) {
            const float* row = sS + (QPW * wv + s) * KNN_SROW + qi;
            DPC_UNROLL
            for (int half = 0; half < 2; ++half) {
                const int ct = 2 * half + h;
                const float c = row[ct * KNN_TILE * KNN_SROW];
                const int j = (tb + ct) * KNN_TILE + qi;
                uint64_t todo = wave_ballot(tb + ct < tile1 && j < ng && j != sk[s] && better(c, j, ts[s], ti[s]));
                while (todo) {   // wave-uniform
                    const int b = __builtin_ctzll(todo);
                    const float cs = wave_read_lane(c, b);
                    const int ci = wave_read_lane(j, b);
                    const int pos = __builtin_popcountll(wave_ballot(better(ls[s], li[s], cs, ci)));   // < K: it beats entry K - 1
                    const float us = __shfl(ls[s], (lane + 63) & 63);
                    const int ui = __shfl(li[s], (lane + 63) & 63);
                    if (lane > pos) { ls[s] = us; li[s] = ui; }
                    if (lane == pos) { ls[s] = cs; li[s] = ci; }
                    ts[s] = wave_read_lane(ls[s], K - 1);
                    ti[s] = wave_read_lane(li[s], K - 1);
                    todo &= todo - 1;
                    todo &= wave_ballot(better(c, j, ts[s], ti[s]));   // what the new entry K - 1 already beats is dropped
                }
            }
        }
        __syncthreads();
    }
    // lanes [0, K) of a list are its entries in order: straight into the slab's list
    DPC_UNROLL
    for (int s = 0; s < QPW; ++s) {
        const int q = q0 + QPW * wv + s;
        if (q < nq && lane < K) {
            Cand c;
            c.sim = ls[s];
            c.idx = li[s];
            ws[((long long)q * n_slabs + slab) * K + lane] = c;
        }
    }
}

// one wave per query: lane s < n_slabs walks slab s's sorted list; each round the wave agrees on the best head (a gallery row
// lives in exactly one slab, so the winner is one lane) and that lane steps on
__global__ __launch_bounds__(256) void knn_merge_kernel(const Cand* ws, int nq, int K, int n_slabs, float* top_sim, int32_t* top_idx) {
    const int lane = threadIdx.x & 63;
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;   // the whole wave leaves
    const Cand* mine = ws + ((long long)q * n_slabs + (lane < n_slabs ? lane : 0)) * K;
    int p = lane < n_slabs ? 0 : K;
    Cand head;
    head.sim = neg_inf();
    head.idx = KNN_EMPTY;
    if (p < K) head = mine[0];
    for (int e = 0; e < K; ++e) {
        float bs = head.sim;
        int bi = head.idx;
        DPC_UNROLL
        for (int m = 32; m >= 1; m >>= 1) {
            const float os = __shfl_xor(bs, m);
            const int oi = __shfl_xor(bi, m);
            if (better(os, oi, bs, bi)) { bs = os; bi = oi; }
        }
        if (bi != KNN_EMPTY && head.idx == bi) {
            ++p;
            if (p < K) head = mine[p];
            else { head.sim = neg_inf(); head.idx = KNN_EMPTY; }
        }
        if (lane == 0) {
            top_sim[(long long)q * K + e] = bs;
            top_idx[(long long)q * K + e] = bi == KNN_EMPTY ? -1 : bi;
        }
    }
}

// ---------------------------------------------------------------- recall@k, first hits, 1-NN confusion
__global__ __launch_bounds__(256) void knn_recall_kernel(const int32_t* top_idx, int nq, int K, const long long* q_label, const long long* g_label,
                                                         int ng, int num_class, const int32_t* ks, int nk, long long* hits, int32_t* first_hit,
                                                         long long* confusion) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int i = tid; i < nq; i += 256) {
        const long long ql = q_label[i];
        int fh = -1;
        for (int k = 0; k < K; ++k) {
            const int j = top_idx[(long long)i * K + k];
            if (j < 0 || j >= ng) continue;   // a slot without a neighbour
            if (g_label[j] == ql) { fh = k; break; }
        }
        first_hit[i] = fh;
    }
    __syncthreads();
    for (int j = wv; j < nk; j += 4) {   // wave w counts for ks[w], ks[w + 4], ..; integer sums: any order, same value
        const int kj = ks[j];
        int c = 0;
        for (int i = lane; i < nq; i += 64) { const int fh = first_hit[i]; c += (fh >= 0 && fh < kj) ? 1 : 0; }
        c = wave_sum_i(c);
        if (lane == 0) hits[j] += c;
    }
    for (int c = tid; c < num_class; c += 256) {   // thread c owns column c (the queries of class c): one writer per cell
        for (int i = 0; i < nq; ++i) {
            if (q_label[i] != c) continue;
            const int j = top_idx[(long long)i * K];
            if (j < 0 || j >= ng) continue;
            const long long gl = g_label[j];
            if (gl < 0 || gl >= num_class) continue;
            confusion[gl * num_class + c] += 1;
        }
    }
}

// slabs when the caller leaves the choice (n_slabs == 0): about two workgroups per CU, never fewer than one round of the four
// waves per slab.  n_gtiles < 0: the gallery is not known (dpc_knn_ws_bytes): the largest count the rule can give
int knn_auto_slabs(int nq, int n_gtiles) {
    const int n_qtiles = (nq + KNN_TILE - 1) / KNN_TILE;
    int s = (2 * KNN_CUS + n_qtiles - 1) / n_qtiles;
    if (s > KNN_MAX_SLABS) s = KNN_MAX_SLABS;
    if (n_gtiles >= 0) {
        const int cap = (n_gtiles + KNN_WAVES - 1) / KNN_WAVES;
        if (s > cap) s = cap;
    }
    return s < 1 ? 1 : s;
}

}  // namespace

extern "C" int dpc_embed_accumulate(const float* ctx, int32_t rows, int32_t n_valid, int32_t D, int32_t ld, float* esum, int32_t* count,
                                    dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!ctx || !esum || !count || rows <= 0 || n_valid <= 0 || n_valid > rows || D <= 0 || ld < D) return DPC_ERR_ARG;
    DPC_LAUNCH(embed_accumulate_kernel, dim3(1), dim3(256), stream, ctx, n_valid, D, ld, esum, count);
    return dpc_launch_status();
}

extern "C" int dpc_embed_finish(float* esum, int32_t* count, int32_t D, float eps, float* out, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!esum || !count || !out || D <= 0 || !(eps >= 0.f)) return DPC_ERR_ARG;
    DPC_LAUNCH(embed_finish_kernel, dim3(1), dim3(256), stream, esum, count, D, eps, out);
    return dpc_launch_status();
}

extern "C" int dpc_knn_ws_bytes(int32_t nq, int32_t K, int32_t n_slabs) {
    if (nq <= 0 || K < 1 || n_slabs < 0) return DPC_ERR_ARG;
    if (K > KNN_MAX_K || n_slabs > KNN_MAX_SLABS) return DPC_ERR_UNSUPPORTED;
    const int s = n_slabs ? n_slabs : knn_auto_slabs(nq, -1);
    const long long bytes = (long long)nq * s * K * (long long)sizeof(Cand);
    return bytes > 0x7fffffffll ? DPC_ERR_UNSUPPORTED : (int)bytes;
}

extern "C" int dpc_knn_topk(const float* Q, int32_t nq, int32_t ldq, const float* G, int32_t ng, int32_t ldg, int32_t D, int32_t K,
                            const int32_t* skip, int32_t n_slabs, float* top_sim, int32_t* top_idx, void* ws, int64_t ws_bytes,
                            dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!Q || !G || !top_sim || !top_idx || !ws || nq <= 0 || ng <= 0 || D <= 0 || K < 1 || n_slabs < 0 || ldq < D || ldg < D) return DPC_ERR_ARG;
    if (D % 32 || D > 256 || K > KNN_MAX_K || n_slabs > KNN_MAX_SLABS || (ldq & 3) || (ldg & 3) || ((uintptr_t)Q & 15) || ((uintptr_t)G & 15))
        return DPC_ERR_UNSUPPORTED;
    const int n_gtiles = (ng + KNN_TILE - 1) / KNN_TILE, n_qtiles = (nq + KNN_TILE - 1) / KNN_TILE;
    const int s = n_slabs ? n_slabs : knn_auto_slabs(nq, n_gtiles);
    if ((long long)nq * s * K * (long long)sizeof(Cand) > ws_bytes) return DPC_ERR_ARG;
    const int tiles_per_slab = (n_gtiles + s - 1) / s;   // a forced count above the tile count leaves the last slabs empty
    const size_t lds = (size_t)D * 128 + (size_t)KNN_WAVES * KNN_TILE * KNN_SROW * sizeof(float);   // at most 50 KB: three workgroups per CU
    DPC_LAUNCH_DYN(knn_partial_kernel, dim3((unsigned)n_qtiles, (unsigned)s), dim3(256), lds, stream, Q, nq, ldq, G, ng, ldg, D, K, skip,
                   tiles_per_slab, s, (Cand*)ws);
    DPC_LAUNCH(knn_merge_kernel, dim3((unsigned)((nq + 3) / 4)), dim3(256), stream, (const Cand*)ws, nq, K, s, top_sim, top_idx);
    return dpc_launch_status();
}

extern "C" int dpc_knn_recall(const int32_t* top_idx, int32_t nq, int32_t K, const int64_t* q_label, const int64_t* g_label, int32_t ng,
                              int32_t num_class, const int32_t* ks, int32_t nk, int64_t* hits, int32_t* first_hit, int64_t* confusion,
                              dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!top_idx || !q_label || !g_label || !ks || !hits || !first_hit || !confusion || nq <= 0 || K < 1 || ng <= 0 || num_class <= 0 || nk <= 0)
        return DPC_ERR_ARG;
    DPC_LAUNCH(knn_recall_kernel, dim3(1), dim3(256), stream, top_idx, nq, K, (const long long*)q_label, (const long long*)g_label, ng,
               num_class, ks, nk, (long long*)hits, first_hit, (long long*)confusion);
    return dpc_launch_status();
}
