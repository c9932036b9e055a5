// labels.hip -- the class labels of a synthetic classifier batch drawn on the device (dpc_amd/lc_main.py --graph), beside
// csrc/synthetic.hip's video: no torch generator and no host-to-device copy inside a captured step.
//
// Definition (include/dpc_hip.h, restated by tests/lc_graph_cases.py): label b is word b & 3 of Philox block b >> 2, keyed on
// (seed, draw counter d read on the device), scaled into [0, num_class) by the high half of a 32 x 32 -> 64 bit product:
//   (w0,w1,w2,w3) = philox4x32_10(b >> 2, d, DPC_PHILOX_STREAM_LABEL, 0; lo(seed), hi(seed))
//   label[b] = ((uint64)w_(b & 3) * num_class) >> 32
// A thread owns one Philox block = four neighbouring labels; the tail block stores only what is inside [0, B).
#include "philox.h"
#include "../../include/dpc_hip.h"

__global__ void synthetic_labels_kernel(long long* target, int B, unsigned num_class, unsigned long long seed, const int32_t* draw_dev) {
    const int blocks = (B + 3) >> 2;
    const uint32_t d = (uint32_t)draw_dev[0];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < blocks; i += (long long)gridDim.x * blockDim.x) {
        const Philox4 r = philox4x32_10((uint32_t)i, d, DPC_PHILOX_STREAM_LABEL, 0u, k0, k1);
        const long long b0 = i << 2;
        DPC_UNROLL
        for (int e = 0; e < 4; ++e)
            if (b0 + e < B) target[b0 + e] = (long long)(((unsigned long long)r.v[e] * num_class) >> 32);
    }
}

extern "C" int dpc_synthetic_labels(int64_t* target, int32_t B, int32_t num_class, uint64_t seed, const int32_t* draw_dev,
                                    dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!target || !draw_dev || B <= 0 || num_class <= 0) return DPC_ERR_ARG;
    long long g = (((long long)B + 3) / 4 + 255) / 256;
    if (g > 16384) g = 16384;
    const dim3 grid((unsigned)g), blk(256);
    DPC_LAUNCH(synthetic_labels_kernel, grid, blk, stream, (long long*)target, B, (unsigned)num_class, (unsigned long long)seed, draw_dev);
    return dpc_launch_status();
}
