// grad_guard.hip -- the gradient guard of the fused optimizer step: global 2-norm of the gradient arena, the clip / skip verdict and
// the gated step counter, all on the device, so that a replayed hipGraph step can clip its gradient or drop a non-finite one with
// nothing crossing the host (torch's clip_grad_norm_ and the skip-on-overflow step of a GradScaler, without the host read-back).
//
//   dpc_grad_sumsq   DPC_GRAD_PARTIALS workgroups, one f64 partial each: sum of g^2 over the live floats
//   dpc_grad_verdict one workgroup: partials -> dpc_grad_state {sumsq, norm, coef, skip, counters}
//   dpc_step_advance_gated  dpc_step_advance unless state->skip
//   dpc_grad_scale   g *= state->coef in place (module-boundary clip_grad_norm_ only; the engine's step folds coef into Adam:
//                    loss.hip dpc_adam_dev_ex / dpc_adam_groups_dev_ex)
//
// Determinism: the work split depends on n alone (tile t belongs to workgroup t % DPC_GRAD_PARTIALS), a thread adds its elements in
// address order, lanes meet through xor shuffles 32, 16, ..., 1, waves through LDS in wave order, partials in index order.  No
// atomics.  Same arena -> same bits, run to run and rank to rank.
#include "seg_table.h"   // GRAD_TILE4, the segment table in LDS (seg_load / seg_first / seg_live), grad_args_ok

__device__ __forceinline__ bool finite_f64(double x) { return ((__builtin_bit_cast(uint64_t, x) >> 52) & 0x7ffu) != 0x7ffu; }

__global__ __launch_bounds__(256) void grad_sumsq_kernel(const float* g, long long n4, long long ntiles, const dpc_adam_segment* segs,
                                                         int nseg, double* partials) {
    __shared__ SegLds tab;
    __shared__ double s_wave[4];
    const int tid = threadIdx.x;
    if ((long long)blockIdx.x >= ntiles) {   // (uniform) a slot without a tile: written all the same
        if (tid == 0) partials[blockIdx.x] = 0.0;
        return;
    }
    if (segs) seg_load(tab, segs, nseg);
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int s = segs ? seg_first(tab, nseg, tile * GRAD_TILE4 * 4) : 0;
        f32x4 x[GRAD_TILE4 / 256];
        DPC_UNROLL
        for (int j = 0; j < GRAD_TILE4 / 256; ++j) {   // the tile's four loads are issued before any is squared
            const long long i = tile * GRAD_TILE4 + tid + 256 * j;
            const bool live = i < n4 && (!segs || seg_live(tab, nseg, s, i * 4));   // a dead unit is never loaded
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            x[j] = live ? ((const f32x4*)g)[i] : zero;
        }
        DPC_UNROLL
        for (int j = 0; j < GRAD_TILE4 / 256; ++j)
            DPC_UNROLL
            for (int e = 0; e < 4; ++e) {
                const double d = (double)x[j][e];   // widened first: (2e19)^2 is no f32
                acc[e] += d * d;
            }
    }
    double a = (acc[0] + acc[1]) + (acc[2] + acc[3]);
    DPC_UNROLL
    for (int m = 32; m >= 1; m >>= 1) a += __shfl_xor(a, m);
    if ((tid & 63) == 0) s_wave[tid >> 6] = a;
    __syncthreads();
    if (tid == 0) partials[blockIdx.x] = ((s_wave[0] + s_wave[1]) + s_wave[2]) + s_wave[3];
}

extern "C" int dpc_grad_sumsq(const float* g, int64_t n, const dpc_adam_segment* segments_dev, int32_t n_segments, double* partials,
                              dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!grad_args_ok(g, n, segments_dev, n_segments) || !partials || (uintptr_t)partials % 8) return DPC_ERR_ARG;
    const long long n4 = n / 4, ntiles = (n4 + GRAD_TILE4 - 1) / GRAD_TILE4;
    DPC_LAUNCH(grad_sumsq_kernel, dim3(DPC_GRAD_PARTIALS), dim3(256), stream, g, n4, ntiles, segments_dev, (int)n_segments, partials);
    return dpc_launch_status();
}

// One workgroup.  The partials come in through LDS (coalesced, all loads in flight at once); thread 0 adds them in index order.
__global__ __launch_bounds__(256) void grad_verdict_kernel(const double* partials, int n_partials, double max_norm, int skip_nonfinite,
                                                           dpc_grad_state* st) {
    __shared__ double s_part[DPC_GRAD_PARTIALS];
    for (int i = threadIdx.x; i < n_partials; i += 256) s_part[i] = partials[i];
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int i = 0; i < n_partials; ++i) sum += s_part[i];
    const double norm = sqrt(sum);
    float coef = 1.f;
    int skip = 0;
    if (finite_f64(sum)) {
        if (max_norm > 0.0) {
            const double c = max_norm / (norm + 1e-6);   // torch.nn.utils.clip_grad_norm_, in f64, rounded once
            coef = c < 1.0 ? (float)c : 1.f;
            if (coef < 1.f) st->n_clipped += 1;
        }
    } else if (skip_nonfinite) {
        skip = 1;
        coef = 0.f;
        st->n_skipped += 1;
    }   // (a non-finite gradient that is not to be skipped goes through unscaled, as without the guard)
    st->sumsq = sum;
    st->norm = (float)norm;
    st->coef = coef;
    st->skip = skip;
}

extern "C" int dpc_grad_verdict(const double* partials, int32_t n_partials, double max_norm, int32_t skip_nonfinite,
                                dpc_grad_state* state_dev, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!partials || !state_dev || n_partials <= 0 || n_partials > DPC_GRAD_PARTIALS || (uintptr_t)partials % 8 || (uintptr_t)state_dev % 8)
        return DPC_ERR_ARG;
    DPC_LAUNCH(grad_verdict_kernel, dim3(1), dim3(256), stream, partials, (int)n_partials, max_norm, (int)skip_nonfinite, state_dev);
    return dpc_launch_status();
}

// step_advance_kernel (loss.hip) behind the verdict: a skipped step is no optimizer step, t and the bias corrections stay
__global__ void step_advance_gated_kernel(int32_t* step, float* bc, double b1, double b2, const dpc_grad_state* st) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && !st->skip) {
        const int t = step[0] + 1;
        step[0] = t;
        bc[0] = (float)(1.0 - pow(b1, (double)t));
        bc[1] = (float)(1.0 - pow(b2, (double)t));
    }
}

extern "C" int dpc_step_advance_gated(int32_t* step_dev, float* bias_corr_dev, double beta1, double beta2,
                                      const dpc_grad_state* state_dev, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!step_dev || !bias_corr_dev || !state_dev) return DPC_ERR_ARG;
    DPC_LAUNCH(step_advance_gated_kernel, dim3(1), dim3(64), stream, step_dev, bias_corr_dev, beta1, beta2, state_dev);
    return dpc_launch_status();
}

__global__ __launch_bounds__(256) void grad_scale_kernel(float* g, long long n4, long long ntiles, const dpc_adam_segment* segs, int nseg,
                                                         const dpc_grad_state* st) {
    __shared__ SegLds tab;
    const float coef = st->coef;
    if (st->skip || coef == 1.f) return;   // (uniform) x * 1.0f is x: nothing to rewrite
    if (segs) seg_load(tab, segs, nseg);
    const int tid = threadIdx.x;
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int s = segs ? seg_first(tab, nseg, tile * GRAD_TILE4 * 4) : 0;
        DPC_UNROLL
        for (int j = 0; j < GRAD_TILE4 / 256; ++j) {
            const long long i = tile * GRAD_TILE4 + tid + 256 * j;
            if (i >= n4) break;
            if (segs && !seg_live(tab, nseg, s, i * 4)) continue;
            f32x4 x = ((const f32x4*)g)[i];
            DPC_UNROLL
            for (int e = 0; e < 4; ++e) x[e] *= coef;
            ((f32x4*)g)[i] = x;
        }
    }
}

extern "C" int dpc_grad_scale(float* g, int64_t n, const dpc_adam_segment* segments_dev, int32_t n_segments,
                              const dpc_grad_state* state_dev, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!grad_args_ok(g, n, segments_dev, n_segments) || !state_dev) return DPC_ERR_ARG;
    const long long n4 = n / 4, ntiles = (n4 + GRAD_TILE4 - 1) / GRAD_TILE4;
    const unsigned grid = (unsigned)(ntiles < DPC_GRAD_PARTIALS ? ntiles : DPC_GRAD_PARTIALS);
    DPC_LAUNCH(grad_scale_kernel, dim3(grid), dim3(256), stream, g, n4, ntiles, segments_dev, (int)n_segments, state_dev);
    return dpc_launch_status();
}
