// grad_accum.hip -- gradient accumulation in front of the fused optimizer step: several micro-batches per optimizer step, with nothing
// crossing the host, so that a replayed hipGraph step can accumulate too.  A second f32 arena `acc` of the size of the gradient arena:
//
//   DPC_ACCUM_ADD     acc = acc + g                          (every micro-batch of a cycle but the last)
//   DPC_ACCUM_FINISH  g = (acc + g) * scale, acc = +0        (the last: g then holds the cycle's mean gradient, scale = float32(1 / N))
//
// Every cycle ends with acc at +0 again, so there is no "store" mode and every non-final micro-batch is the same launch.  The sum is
// a plain f32 sum in micro-batch order: one add, rounded, per micro-batch, then one multiply, rounded.  Nothing is contracted.
//
// Shape of grad_sumsq_kernel / grad_scale_kernel (grad_guard.hip): 16-byte units, four per thread per tile, the tile's loads issued before
// any is used, grid-stride over the tiles of the arena that meet [begin, end), the segment table in LDS.  A unit outside the range or
// outside every active segment is neither loaded nor stored, in either arena.  One writer per value, no atomics.
#include "seg_table.h"

#pragma clang fp contract(off)

template <int MODE>
__global__ __launch_bounds__(256) void grad_accum_kernel(float* acc, float* g, long long u0, long long u1, long long tile0, long long tile1,
                                                         const dpc_adam_segment* segs, int nseg, float scale) {
    __shared__ SegLds tab;
    if (segs) seg_load(tab, segs, nseg);
    const int tid = threadIdx.x;
    for (long long tile = tile0 + blockIdx.x; tile < tile1; tile += gridDim.x) {
        int s = segs ? seg_first(tab, nseg, tile * GRAD_TILE4 * 4) : 0;
        f32x4 a[GRAD_TILE4 / 256], x[GRAD_TILE4 / 256];
        bool live[GRAD_TILE4 / 256];
        DPC_UNROLL
        for (int j = 0; j < GRAD_TILE4 / 256; ++j) {   // the tile's eight loads are issued before any is used
            const long long i = tile * GRAD_TILE4 + tid + 256 * j;
            live[j] = i >= u0 && i < u1 && (!segs || seg_live(tab, nseg, s, i * 4));   // a dead unit is never loaded
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            a[j] = live[j] ? ((const f32x4*)acc)[i] : zero;
            x[j] = live[j] ? ((const f32x4*)g)[i] : zero;
        }
        DPC_UNROLL
        for (int j = 0; j < GRAD_TILE4 / 256; ++j) {
            if (!live[j]) continue;   // ... and never stored
            const long long i = tile * GRAD_TILE4 + tid + 256 * j;
            f32x4 r;
            DPC_UNROLL
            for (int e = 0; e < 4; ++e) r[e] = a[j][e] + x[j][e];
            if (MODE == DPC_ACCUM_ADD) {
                ((f32x4*)acc)[i] = r;
            } else {
                DPC_UNROLL
                for (int e = 0; e < 4; ++e) r[e] = r[e] * scale;
                const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                ((f32x4*)g)[i] = r;
                ((f32x4*)acc)[i] = zero;
            }
        }
    }
}

extern "C" int dpc_grad_accumulate(float* acc, float* g, int64_t n, int64_t begin, int64_t end, const dpc_adam_segment* segments_dev,
                                   int32_t n_segments, int32_t mode, float scale, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!grad_args_ok(g, n, segments_dev, n_segments) || !acc || (uintptr_t)acc % 16 || acc == g) return DPC_ERR_ARG;
    if (begin < 0 || begin % 4 || end % 4 || begin > end || end > n) return DPC_ERR_ARG;
    if (mode != DPC_ACCUM_ADD && mode != DPC_ACCUM_FINISH) return DPC_ERR_ARG;
    if (((__builtin_bit_cast(uint32_t, scale) >> 23) & 0xffu) == 0xffu) return DPC_ERR_ARG;   // Inf or NaN
    if (begin == end) return DPC_OK;
    const long long u0 = begin / 4, u1 = end / 4;
    const long long tile0 = u0 / GRAD_TILE4, tile1 = (u1 + GRAD_TILE4 - 1) / GRAD_TILE4, ntiles = tile1 - tile0;
    const unsigned grid = (unsigned)(ntiles < DPC_GRAD_PARTIALS ? ntiles : DPC_GRAD_PARTIALS);   // as dpc_grad_scale caps it
    if (mode == DPC_ACCUM_ADD)
        DPC_LAUNCH(grad_accum_kernel<DPC_ACCUM_ADD>, dim3(grid), dim3(256), stream, acc, g, u0, u1, tile0, tile1, segments_dev, (int)n_segments, scale);
    else
        DPC_LAUNCH(grad_accum_kernel<DPC_ACCUM_FINISH>, dim3(grid), dim3(256), stream, acc, g, u0, u1, tile0, tile1, segments_dev, (int)n_segments, scale);
    return dpc_launch_status();
}
