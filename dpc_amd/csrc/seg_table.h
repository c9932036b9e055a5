// seg_table.h -- the segment table of dpc_adam_groups_dev in LDS, for the kernels that walk a gradient arena in 16-byte units and leave
// every unit outside an active segment alone (grad_guard.hip, grad_accum.hip).
#pragma once
#include "dpc_rt.h"
#include "../../include/dpc_hip.h"

constexpr int GRAD_TILE4 = 1024;   // 16-byte units per tile, as ADAM_TILE4 (loss.hip): 4 per thread, 16 KB of the arena

struct SegLds {
    long long begin[DPC_ADAM_MAX_SEGMENTS], end[DPC_ADAM_MAX_SEGMENTS];
    int active[DPC_ADAM_MAX_SEGMENTS];
};
__device__ __forceinline__ void seg_load(SegLds& t, const dpc_adam_segment* segs, int nseg) {
    for (int s = threadIdx.x; s < nseg; s += 256) {
        t.begin[s] = segs[s].begin;
        t.end[s] = segs[s].end;
        t.active[s] = segs[s].active;
    }
    __syncthreads();
}
// first segment that ends behind float t0
__device__ __forceinline__ int seg_first(const SegLds& t, int nseg, long long t0) {
    int lo = 0, hi = nseg;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t.end[mid] <= t0) lo = mid + 1; else hi = mid;
    }
    return lo;
}
// whether the 16-byte unit at float `base` lies in an active segment; s advances (a thread's units ascend)
__device__ __forceinline__ bool seg_live(const SegLds& t, int nseg, int& s, long long base) {
    while (s < nseg && t.end[s] <= base) ++s;
    return s < nseg && t.begin[s] <= base && t.active[s];
}

// what dpc_adam_groups_dev checks: n % 4, 16-byte alignment, the table's count when there is a table
static inline bool grad_args_ok(const void* g, int64_t n, const dpc_adam_segment* segs, int32_t n_segments) {
    if (!g || n <= 0 || n % 4 || (uintptr_t)g % 16) return false;
    return !segs || (n_segments > 0 && n_segments <= DPC_ADAM_MAX_SEGMENTS);
}
