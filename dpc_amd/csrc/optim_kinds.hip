// optim_kinds.hip -- the other update rules of the fused optimizer step (include/dpc_hip.h: dpc_adamw_*, dpc_lamb_*).  The step
// counter, the bias corrections, the gradient guard, the parameter average and the learning-rate record are those of the Adam
// step (loss.hip, grad_guard.hip); only the update differs.
//
//   dpc_adamw_dev / dpc_adamw_groups_dev   torch.optim.AdamW: adam_dev_sched_kernel / adam_groups_sched_kernel (loss.hip) with the
//                    decay taken out of the gradient and applied to the parameter first, p <- p (1 - lr wd), then Adam's own line
//                    p <- p - step m / (sqrt(v) ...): with wd = 0 the factor is 1.0f and the bits are Adam's.  One launch, as Adam.
//   dpc_lamb_moments / dpc_lamb_ratios / dpc_lamb_apply   LAMB (You et al. 2020, bias-corrected): three launches where Adam has one.
//
// LAMB's work split is the host-built chunk table (dpc_lamb_build_chunks): chunks of at most LAMB_CHUNK floats that never cross a
// segment, active segments only, each segment's chunks contiguous in the table.  Chunk c is one workgroup's work in `moments` and in
// `apply`, whatever the grid; `moments` writes one f64 pair {sum p^2, sum u^2} per chunk and `ratios` adds each segment's pairs in
// chunk order.  Determinism as in grad_guard.hip: a thread adds its elements in address order, lanes meet through xor shuffles
// 32 .. 1, waves through LDS in wave order.  No atomics, one writer per value: same arenas -> same bits, run to run, rank to rank.
#include "dpc_rt.h"
#include "../../include/dpc_hip.h"

static inline unsigned ok_grid_for(long long n, int block = 256, int cap = 8192) {
    long long g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// 1 - d of the parameter average, as loss.hip forms it (ema_weight): all in f32
__device__ __forceinline__ float ok_ema_weight(const int32_t* step_dev, float decay) {
    const int t = step_dev[0];
    const float d = fminf(decay, (float)(1 + t) / (float)(10 + t));
    return 1.f - d;
}

// ------------------------------------------------------------------------------------------------ AdamW
// p (1 - lr wd) as torch.optim.AdamW forms it: a product rounded on its own (param.mul_), never fused into the subtraction that
// follows.  keep == 1.0f (wd = 0) returns p's bits.
__device__ __forceinline__ float adamw_decayed(float p, float keep) {
#pragma clang fp contract(off)
    return p * keep;
}

// adam_dev_sched_kernel line for line except where marked.  lrs may be null: multiplier 1.
template <bool EMA>
__global__ void adamw_dev_kernel(float* p, const float* g, float* m, float* v, long long n4, long long n, float lr, float b1,
                                 float b2, float omb1, float omb2, float eps, float wd, const float* bc, float gscale,
                                 const dpc_grad_state* gs, float* ema, const int32_t* step_dev, float decay, const dpc_lr_state* lrs) {
    if (gs) {   // the gradient guard's verdict (grad_guard.hip): a skipped step loads and stores nothing
        if (gs->skip) return;
        gscale = gscale * gs->coef;
    }
    const float lr_eff = lrs ? lr * lrs->mult : lr;   // the f32 product first
    const float step = lr_eff / bc[0];
    const float keep = 1.f - lr_eff * wd;              // AdamW: the decoupled decay, a factor on p
    const float isb2 = 1.f / sqrtf(bc[1]);
    float omd = 0.f;
    if constexpr (EMA) omd = ok_ema_weight(step_dev, decay);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const long long base = i * 4;
        if (base + 4 <= n) {
            f32x4 pv = ((f32x4*)p)[i], gv = ((const f32x4*)g)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
            DPC_UNROLL
            for (int e = 0; e < 4; ++e) {
                const float gg = gv[e] * gscale;                                              // AdamW: no wd * p here
                mv[e] = b1 * mv[e] + omb1 * gg;
                vv[e] = b2 * vv[e] + omb2 * gg * gg;
                pv[e] = adamw_decayed(pv[e], keep);                                           // AdamW: the decay, then Adam's line
                pv[e] -= step * mv[e] / (sqrtf(vv[e]) * isb2 + eps);
            }
            ((f32x4*)p)[i] = pv; ((f32x4*)m)[i] = mv; ((f32x4*)v)[i] = vv;
            if constexpr (EMA) {
                f32x4 ev = ((f32x4*)ema)[i];
                DPC_UNROLL
                for (int e = 0; e < 4; ++e) ev[e] += omd * (pv[e] - ev[e]);
                ((f32x4*)ema)[i] = ev;
            }
        } else {
            for (long long k = base; k < n; ++k) {
                const float gg = g[k] * gscale;
                m[k] = b1 * m[k] + omb1 * gg;
                v[k] = b2 * v[k] + omb2 * gg * gg;
                p[k] = adamw_decayed(p[k], keep);
                p[k] -= step * m[k] / (sqrtf(v[k]) * isb2 + eps);
                if constexpr (EMA) ema[k] += omd * (p[k] - ema[k]);
            }
        }
    }
}

constexpr int ADAMW_TILE4 = 1024;  // 16-byte units per tile, as ADAM_TILE4 (loss.hip)
// adam_groups_sched_kernel line for line except where marked
template <bool EMA>
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* p, const float* g, float* m, float* v, long long n4, long long ntiles,
                                                           const dpc_adam_segment* segs, int nseg, float b1, float b2, float omb1,
                                                           float omb2, float eps, const float* bc, float gscale,
                                                           const dpc_grad_state* gs, float* ema, const int32_t* step_dev, float decay,
                                                           const dpc_lr_state* lrs) {
    if (gs) {   // as in adamw_dev_kernel
        if (gs->skip) return;
        gscale = gscale * gs->coef;
    }
    __shared__ long long s_begin[DPC_ADAM_MAX_SEGMENTS], s_end[DPC_ADAM_MAX_SEGMENTS];
    __shared__ float s_lr[DPC_ADAM_MAX_SEGMENTS], s_wd[DPC_ADAM_MAX_SEGMENTS];   // lr < 0 marks an inactive segment
    const int tid = threadIdx.x;
    const bool scheduled = lrs != nullptr;   // uniform
    const float mult = scheduled ? lrs->mult : 1.f;
    for (int s = tid; s < nseg; s += 256) {
        s_begin[s] = segs[s].begin;
        s_end[s] = segs[s].end;
        s_lr[s] = segs[s].active ? (scheduled ? segs[s].lr * mult : segs[s].lr) : -1.f;   // lr, mult >= 0: never reads as inactive
        s_wd[s] = segs[s].weight_decay;
    }
    __syncthreads();
    const float bc1 = bc[0];
    const float isb2 = 1.f / sqrtf(bc[1]);
    float omd = 0.f;
    if constexpr (EMA) omd = ok_ema_weight(step_dev, decay);
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long t0 = tile * ADAMW_TILE4 * 4;   // first float of the tile
        int lo = 0, hi = nseg;                        // first segment with end > t0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_end[mid] <= t0) lo = mid + 1; else hi = mid;
        }
        int s = lo;
        DPC_UNROLL
        for (int j = 0; j < ADAMW_TILE4 / 256; ++j) {
            const long long i = tile * ADAMW_TILE4 + tid + 256 * j;
            const long long base = i * 4;
            if (i >= n4) break;
            while (s < nseg && s_end[s] <= base) ++s;
            if (s >= nseg) break;
            if (s_begin[s] > base || s_lr[s] < 0.f) continue;   // padding between segments, or frozen
            const float step = s_lr[s] / bc1, keep = 1.f - s_lr[s] * s_wd[s];   // AdamW: the decay is a factor on p
            f32x4 pv = ((f32x4*)p)[i], gv = ((const f32x4*)g)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
            DPC_UNROLL
            for (int e = 0; e < 4; ++e) {
                const float gg = gv[e] * gscale;
                mv[e] = b1 * mv[e] + omb1 * gg;
                vv[e] = b2 * vv[e] + omb2 * gg * gg;
                pv[e] = adamw_decayed(pv[e], keep);
                pv[e] -= step * mv[e] / (sqrtf(vv[e]) * isb2 + eps);
            }
            ((f32x4*)p)[i] = pv; ((f32x4*)m)[i] = mv; ((f32x4*)v)[i] = vv;
            if constexpr (EMA) {
                f32x4 ev = ((f32x4*)ema)[i];
                DPC_UNROLL
                for (int e = 0; e < 4; ++e) ev[e] += omd * (pv[e] - ev[e]);
                ((f32x4*)ema)[i] = ev;
            }
        }
    }
}

// the average is optional (ema and step_dev both null), as in the _sched entries
static inline bool ok_ema_args(const float* p, const float* ema, const int32_t* step_dev, float decay) {
    if (!ema) return !step_dev;
    return ema != p && step_dev && decay > 0.f && decay < 1.f && ((uintptr_t)p | (uintptr_t)ema) % 16 == 0;
}

extern "C" int dpc_adamw_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2,
                             float eps, float wd, const float* bias_corr_dev, float grad_scale, const dpc_grad_state* state_dev,
                             float* ema, const int32_t* step_dev, float decay, const dpc_lr_state* lr_state_dev,
                             dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p || !g || !m || !v || n <= 0 || !bias_corr_dev || (uintptr_t)lr_state_dev % 4) return DPC_ERR_ARG;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16) return DPC_ERR_ARG;
    if (!ok_ema_args(p, ema, step_dev, decay)) return DPC_ERR_ARG;
    const long long n4 = (n + 3) / 4;
    if (ema)
        DPC_LAUNCH((adamw_dev_kernel<true>), dim3(ok_grid_for(n4)), dim3(256), stream, p, g, m, v, n4, (long long)n, lr, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, wd, bias_corr_dev, grad_scale, state_dev, ema, step_dev, decay, lr_state_dev);
    else
        DPC_LAUNCH((adamw_dev_kernel<false>), dim3(ok_grid_for(n4)), dim3(256), stream, p, g, m, v, n4, (long long)n, lr, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, wd, bias_corr_dev, grad_scale, state_dev, (float*)nullptr, (const int32_t*)nullptr, 0.f, lr_state_dev);
    return dpc_launch_status();
}

extern "C" int dpc_adamw_groups_dev(float* p, const float* g, float* m, float* v, int64_t n, const dpc_adam_segment* segments_dev,
                                    int32_t n_segments, double beta1, double beta2, float eps, const float* bias_corr_dev,
                                    float grad_scale, const dpc_grad_state* state_dev, float* ema, const int32_t* step_dev,
                                    float decay, const dpc_lr_state* lr_state_dev, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p || !g || !m || !v || n <= 0 || n % 4 || !segments_dev || n_segments <= 0 || n_segments > DPC_ADAM_MAX_SEGMENTS || !bias_corr_dev)
        return DPC_ERR_ARG;
    if ((uintptr_t)lr_state_dev % 4 || !ok_ema_args(p, ema, step_dev, decay)) return DPC_ERR_ARG;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16) return DPC_ERR_ARG;
    const long long n4 = n / 4, ntiles = (n4 + ADAMW_TILE4 - 1) / ADAMW_TILE4;
    const unsigned grid = (unsigned)(ntiles < 2048 ? ntiles : 2048);
    if (ema)
        DPC_LAUNCH((adamw_groups_kernel<true>), dim3(grid), dim3(256), stream, p, g, m, v, n4, ntiles, segments_dev, (int)n_segments, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, bias_corr_dev, grad_scale, state_dev, ema, step_dev, decay, lr_state_dev);
    else
        DPC_LAUNCH((adamw_groups_kernel<false>), dim3(grid), dim3(256), stream, p, g, m, v, n4, ntiles, segments_dev, (int)n_segments, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, bias_corr_dev, grad_scale, state_dev, (float*)nullptr, (const int32_t*)nullptr, 0.f, lr_state_dev);
    return dpc_launch_status();
}

// ------------------------------------------------------------------------------------------------ LAMB
constexpr int LAMB_CHUNK = DPC_LAMB_CHUNK;   // floats per chunk: 1024 16-byte units, 4 per thread, 16 KB of each arena
constexpr int LAMB_U = LAMB_CHUNK / 4 / 256;  // units per thread

// Host: the chunk table of a segment table.  Validates what the kernels rely on -- segments sorted, non-overlapping, begin / end
// multiples of 4 inside [0, n) -- and fills every segment's chunk0 / n_chunks (an inactive segment owns no chunk).  Returns the
// number of chunks, or DPC_ERR_ARG (too many for `capacity` included).
extern "C" int dpc_lamb_build_chunks(dpc_lamb_segment* segments, int32_t n_segments, int64_t n, dpc_lamb_chunk* chunks, int32_t capacity) {
    if (!segments || n_segments <= 0 || n_segments > DPC_ADAM_MAX_SEGMENTS || n <= 0 || n % 4 || !chunks || capacity <= 0) return DPC_ERR_ARG;
    int64_t prev = 0;
    int32_t nc = 0;
    for (int s = 0; s < n_segments; ++s) {
        dpc_lamb_segment& sg = segments[s];
        if (sg.begin % 4 || sg.end % 4 || sg.begin < prev || sg.end <= sg.begin || sg.end > n) return DPC_ERR_ARG;
        if (!(sg.lr >= 0.f) || !(sg.weight_decay >= 0.f)) return DPC_ERR_ARG;
        prev = sg.end;
        sg.chunk0 = nc;
        sg.n_chunks = 0;
        if (!sg.active) continue;
        for (int64_t b = sg.begin; b < sg.end; b += LAMB_CHUNK) {
            if (nc >= capacity) return DPC_ERR_ARG;
            const int64_t len = sg.end - b < LAMB_CHUNK ? sg.end - b : LAMB_CHUNK;
            chunks[nc].begin = b;
            chunks[nc].len = (int32_t)len;
            chunks[nc].seg = s;
            ++nc;
            ++sg.n_chunks;
        }
    }
    return nc;
}

// the update direction, formed the same way by `moments` (for its norm) and by `apply` (from the stored m, v and the old p), so that no
// sixth arena carries it: no contraction, every operation rounded on its own.
//   u = (m / bc1) / (sqrt(v) * isb2 + eps) + wd * p
__device__ __forceinline__ float lamb_u(float p, float m, float v, float bc1, float isb2, float eps, float wd) {
#pragma clang fp contract(off)
    const float mh = m / bc1;
    const float den = sqrtf(v) * isb2 + eps;
    const float q = mh / den;
    const float dp = wd * p;
    return q + dp;
}

// whether chunk c of the table may be touched at all: the table is built and validated on the host, this is the last fence
__device__ __forceinline__ bool lamb_chunk_ok(const dpc_lamb_chunk& c, long long n, int nseg) {
    return c.begin >= 0 && c.len > 0 && c.len <= LAMB_CHUNK && (c.len & 3) == 0 && (c.begin & 3) == 0 && c.begin + c.len <= n && c.seg >= 0 && c.seg < nseg;
}

__global__ __launch_bounds__(256) void lamb_moments_kernel(const float* p, const float* g, float* m, float* v, long long n,
                                                           const dpc_lamb_segment* segs, int nseg, const dpc_lamb_chunk* chunks, int nchunks,
                                                           float b1, float b2, float omb1, float omb2, float eps, const float* bc,
                                                           float gscale, const dpc_grad_state* gs, double* partials) {
    if (gs) {   // a skipped step loads and stores nothing, the partials included
        if (gs->skip) return;
        gscale = gscale * gs->coef;
    }
    __shared__ double s_wave[2][4];
    const int tid = threadIdx.x;
    const float bc1 = bc[0];
    const float isb2 = 1.f / sqrtf(bc[1]);
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const dpc_lamb_chunk ck = chunks[c];
        double ap = 0.0, au = 0.0;
        if (lamb_chunk_ok(ck, n, nseg)) {   // (uniform)
            const float wd = segs[ck.seg].weight_decay;
            const long long u0 = ck.begin / 4;
            const int nu = ck.len / 4;
            f32x4 pv[LAMB_U], gv[LAMB_U], mv[LAMB_U], vv[LAMB_U];
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            DPC_UNROLL
            for (int j = 0; j < LAMB_U; ++j) {   // the chunk's loads are issued before any is used
                const int i = tid + 256 * j;
                const bool live = i < nu;
                pv[j] = live ? ((const f32x4*)p)[u0 + i] : zero;
                gv[j] = live ? ((const f32x4*)g)[u0 + i] : zero;
                mv[j] = live ? ((const f32x4*)m)[u0 + i] : zero;
                vv[j] = live ? ((const f32x4*)v)[u0 + i] : zero;
            }
            DPC_UNROLL
            for (int j = 0; j < LAMB_U; ++j) {
                const int i = tid + 256 * j;
                if (i >= nu) continue;
                DPC_UNROLL
                for (int e = 0; e < 4; ++e) {
                    const float gg = gv[j][e] * gscale;
                    mv[j][e] = b1 * mv[j][e] + omb1 * gg;
                    vv[j][e] = b2 * vv[j][e] + omb2 * gg * gg;
                    const double pd = (double)pv[j][e];   // widened first, as grad_sumsq_kernel does
                    const double ud = (double)lamb_u(pv[j][e], mv[j][e], vv[j][e], bc1, isb2, eps, wd);
                    ap += pd * pd;
                    au += ud * ud;
                }
                ((f32x4*)m)[u0 + i] = mv[j];
                ((f32x4*)v)[u0 + i] = vv[j];
            }
        }
        DPC_UNROLL
        for (int s = 32; s >= 1; s >>= 1) {
            ap += __shfl_xor(ap, s);
            au += __shfl_xor(au, s);
        }
        if ((tid & 63) == 0) {
            s_wave[0][tid >> 6] = ap;
            s_wave[1][tid >> 6] = au;
        }
        __syncthreads();
        if (tid == 0) {
            partials[2 * (long long)c] = ((s_wave[0][0] + s_wave[0][1]) + s_wave[0][2]) + s_wave[0][3];
            partials[2 * (long long)c + 1] = ((s_wave[1][0] + s_wave[1][1]) + s_wave[1][2]) + s_wave[1][3];
        }
        __syncthreads();   // s_wave is reused by the workgroup's next chunk
    }
}

// One workgroup per segment.  The segment's pairs come in through LDS 256 at a time (coalesced); thread 0 adds the p^2 column and
// thread 64 the u^2 column, both in chunk order; thread 0 forms the record.
__global__ __launch_bounds__(256) void lamb_ratios_kernel(const dpc_lamb_segment* segs, int nseg, const double* partials, int nchunks,
                                                          const dpc_grad_state* gs, dpc_lamb_record* rec) {
    if (gs && gs->skip) return;   // the records keep the last step taken
    __shared__ double s_part[2 * 256];
    __shared__ double s_sum[2];
    const int tid = threadIdx.x, s = blockIdx.x;
    if (s >= nseg) return;
    const dpc_lamb_segment sg = segs[s];
    int c0 = sg.chunk0, nc = sg.active ? sg.n_chunks : 0;
    if (c0 < 0 || nc < 0 || c0 + (long long)nc > nchunks) nc = 0;   // (a table the host builder would not have made)
    double acc = 0.0;
    for (int r = 0; r < nc; r += 256) {
        const int cnt = nc - r < 256 ? nc - r : 256;
        for (int i = tid; i < 2 * cnt; i += 256) s_part[i] = partials[2 * (long long)(c0 + r) + i];
        __syncthreads();
        if (tid == 0 || tid == 64) {
            const int col = tid >> 6;
            for (int i = 0; i < cnt; ++i) acc += s_part[2 * i + col];
        }
        __syncthreads();
    }
    if (tid == 0 || tid == 64) s_sum[tid >> 6] = acc;
    __syncthreads();
    if (tid != 0) return;
    const double sp = s_sum[0], su = s_sum[1];
    const double pn = sqrt(sp), un = sqrt(su);
    float ratio = 1.f;
    if (sg.adapt && pn > 0.0 && un > 0.0) ratio = (float)(pn / un);   // f64, rounded once
    dpc_lamb_record out;
    out.sum_p2 = sp;
    out.sum_u2 = su;
    out.pnorm = (float)pn;
    out.unorm = (float)un;
    out.ratio = ratio;
    out.reserved = 0;
    rec[s] = out;
}

template <bool EMA>
__global__ __launch_bounds__(256) void lamb_apply_kernel(float* p, const float* m, const float* v, long long n, const dpc_lamb_segment* segs,
                                                         int nseg, const dpc_lamb_chunk* chunks, int nchunks, float eps, const float* bc,
                                                         const dpc_grad_state* gs, const dpc_lamb_record* rec, float* ema,
                                                         const int32_t* step_dev, float decay, const dpc_lr_state* lrs) {
    if (gs && gs->skip) return;
    const int tid = threadIdx.x;
    const float bc1 = bc[0];
    const float isb2 = 1.f / sqrtf(bc[1]);
    const bool scheduled = lrs != nullptr;   // uniform
    const float mult = scheduled ? lrs->mult : 1.f;
    float omd = 0.f;
    if constexpr (EMA) omd = ok_ema_weight(step_dev, decay);
    for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const dpc_lamb_chunk ck = chunks[c];
        if (!lamb_chunk_ok(ck, n, nseg)) continue;   // (uniform)
        const float wd = segs[ck.seg].weight_decay;
        const float lr_eff = scheduled ? segs[ck.seg].lr * mult : segs[ck.seg].lr;   // the f32 product first
        const float rate = lr_eff * rec[ck.seg].ratio;
        const long long u0 = ck.begin / 4;
        const int nu = ck.len / 4;
        f32x4 pv[LAMB_U], mv[LAMB_U], vv[LAMB_U], ev[LAMB_U];
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        DPC_UNROLL
        for (int j = 0; j < LAMB_U; ++j) {
            const int i = tid + 256 * j;
            const bool live = i < nu;
            pv[j] = live ? ((const f32x4*)p)[u0 + i] : zero;
            mv[j] = live ? ((const f32x4*)m)[u0 + i] : zero;
            vv[j] = live ? ((const f32x4*)v)[u0 + i] : zero;
            if constexpr (EMA) ev[j] = live ? ((const f32x4*)ema)[u0 + i] : zero;
        }
        DPC_UNROLL
        for (int j = 0; j < LAMB_U; ++j) {
            const int i = tid + 256 * j;
            if (i >= nu) continue;
            DPC_UNROLL
            for (int e = 0; e < 4; ++e) pv[j][e] -= rate * lamb_u(pv[j][e], mv[j][e], vv[j][e], bc1, isb2, eps, wd);
            ((f32x4*)p)[u0 + i] = pv[j];
            if constexpr (EMA) {
                DPC_UNROLL
                for (int e = 0; e < 4; ++e) ev[j][e] += omd * (pv[j][e] - ev[j][e]);
                ((f32x4*)ema)[u0 + i] = ev[j];
            }
        }
    }
}

static inline bool lamb_tables_ok(const dpc_lamb_segment* segs, int32_t n_segments, const void* chunks, int32_t n_chunks) {
    return segs && n_segments > 0 && n_segments <= DPC_ADAM_MAX_SEGMENTS && (uintptr_t)segs % 16 == 0 && chunks && (uintptr_t)chunks % 16 == 0 &&
           n_chunks > 0;
}

extern "C" int dpc_lamb_moments(const float* p, const float* g, float* m, float* v, int64_t n, const dpc_lamb_segment* segments_dev,
                                int32_t n_segments, const dpc_lamb_chunk* chunks_dev, int32_t n_chunks, double beta1, double beta2,
                                float eps, const float* bias_corr_dev, float grad_scale, const dpc_grad_state* state_dev,
                                double* partials, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p || !g || !m || !v || n <= 0 || n % 4 || !bias_corr_dev || !partials || (uintptr_t)partials % 16) return DPC_ERR_ARG;
    if (!lamb_tables_ok(segments_dev, n_segments, chunks_dev, n_chunks)) return DPC_ERR_ARG;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16) return DPC_ERR_ARG;
    const unsigned grid = (unsigned)(n_chunks < 4096 ? n_chunks : 4096);
    DPC_LAUNCH(lamb_moments_kernel, dim3(grid), dim3(256), stream, p, g, m, v, (long long)n, segments_dev, (int)n_segments, chunks_dev, (int)n_chunks, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, bias_corr_dev, grad_scale, state_dev, partials);
    return dpc_launch_status();
}

extern "C" int dpc_lamb_ratios(const dpc_lamb_segment* segments_dev, int32_t n_segments, const double* partials, int32_t n_chunks,
                               const dpc_grad_state* state_dev, dpc_lamb_record* records_dev, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!lamb_tables_ok(segments_dev, n_segments, partials, n_chunks) || !records_dev || (uintptr_t)records_dev % 16) return DPC_ERR_ARG;
    DPC_LAUNCH(lamb_ratios_kernel, dim3((unsigned)n_segments), dim3(256), stream, segments_dev, (int)n_segments, partials, (int)n_chunks, state_dev, records_dev);
    return dpc_launch_status();
}

extern "C" int dpc_lamb_apply(float* p, const float* m, const float* v, int64_t n, const dpc_lamb_segment* segments_dev, int32_t n_segments,
                              const dpc_lamb_chunk* chunks_dev, int32_t n_chunks, float eps, const float* bias_corr_dev,
                              const dpc_grad_state* state_dev, const dpc_lamb_record* records_dev, float* ema, const int32_t* step_dev,
                              float decay, const dpc_lr_state* lr_state_dev, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p || !m || !v || n <= 0 || n % 4 || !bias_corr_dev || !records_dev || (uintptr_t)records_dev % 16 || (uintptr_t)lr_state_dev % 4) return DPC_ERR_ARG;
    if (!lamb_tables_ok(segments_dev, n_segments, chunks_dev, n_chunks) || !ok_ema_args(p, ema, step_dev, decay)) return DPC_ERR_ARG;
    if (((uintptr_t)p | (uintptr_t)m | (uintptr_t)v) % 16) return DPC_ERR_ARG;
    const unsigned grid = (unsigned)(n_chunks < 4096 ? n_chunks : 4096);
    if (ema)
        DPC_LAUNCH((lamb_apply_kernel<true>), dim3(grid), dim3(256), stream, p, m, v, (long long)n, segments_dev, (int)n_segments, chunks_dev, (int)n_chunks, eps, bias_corr_dev, state_dev, records_dev, ema, step_dev, decay, lr_state_dev);
    else
        DPC_LAUNCH((lamb_apply_kernel<false>), dim3(grid), dim3(256), stream, p, m, v, (long long)n, segments_dev, (int)n_segments, chunks_dev, (int)n_chunks, eps, bias_corr_dev, state_dev, records_dev, (float*)nullptr, (const int32_t*)nullptr, 0.f, lr_state_dev);
    return dpc_launch_status();
}
