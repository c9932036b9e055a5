// synthetic.hip -- the synthetic N(0,1) training input drawn on the device (dpc_amd/main.py --graph), written straight into the
// stem's space-to-depth operand: no f32 video in HBM, no torch generator inside a captured step.
//
// Definition (include/dpc_hip.h, restated by tests/test_synthetic_input_emu.py): element e of the block [BN][3][T][H][W] is
// normal j-th of Philox block q = e >> 2, keyed on (seed, draw counter d read on the device):
//   (w0,w1,w2,w3) = philox4x32_10(q, d, DPC_PHILOX_STREAM_INPUT, 0; lo(seed), hi(seed))
//   for j in {0,1}: u = ((w_2j >> 8) + 1) 2^-24, v = (w_2j+1 >> 8) 2^-24, r = sqrt(-2 log u), th = 2 pi v
//                   x[4q+2j] = r cos th, x[4q+2j+1] = r sin th
// A thread owns two neighbouring s2d cells (wb, wb+1) of one (n, t, hb): per (c, sy) that is the four elements w = 2wb .. 2wb+3
// of one image row, i.e. one whole Philox block when W % 4 == 0 (every size this build runs), so each block is computed once and
// the thread writes 2 x 16 contiguous channels.  When W % 4 == 2 a row starts half-way into a block and the pair may straddle two.
#include "philox.h"
#include "../../include/dpc_hip.h"
#include <math.h>

// one Box-Muller pair from two Philox words
__device__ __forceinline__ void box_muller(uint32_t wu, uint32_t wv, float& x0, float& x1) {
    const float u = (float)((wu >> 8) + 1u) * 5.9604644775390625e-8f;   // (0, 1]: log finite
    const float v = (float)(wv >> 8) * 5.9604644775390625e-8f;          // [0, 1)
    const float r = sqrtf(-2.f * logf(u));
    const float th = 6.2831855f * v;
    x0 = r * cosf(th);
    x1 = r * sinf(th);
}

template <class TO>
__global__ void synthetic_input_kernel(float* block, TO* out, int BN, int T, int H, int W, unsigned long long seed, const int32_t* draw_dev) {
    const int Hb = H / 2, Wb = W / 2, Wp = (Wb + 1) / 2;   // cell pairs per row of cells
    const long long pairs = (long long)BN * T * Hb * Wp;
    const uint32_t d = (uint32_t)draw_dev[0];
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < pairs; i += (long long)gridDim.x * blockDim.x) {
        const unsigned ci = (unsigned)i;  // pairs < 2^31: 32-bit index math
        const unsigned q1 = ci / (unsigned)Wp;
        const int wb = 2 * (int)(ci - q1 * (unsigned)Wp);
        const unsigned q2 = q1 / (unsigned)Hb;
        const int hb = (int)(q1 - q2 * (unsigned)Hb);
        const unsigned n_ = q2 / (unsigned)T;
        const int t = (int)(q2 - n_ * (unsigned)T);
        const int n = (int)n_;
        const bool two = wb + 1 < Wb;
        float v[2][16];
        DPC_UNROLL
        for (int k = 12; k < 16; ++k) v[0][k] = v[1][k] = 0.f;
        DPC_UNROLL
        for (int c = 0; c < 3; ++c)
            DPC_UNROLL
            for (int sy = 0; sy < 2; ++sy) {
                const long long e = ((((long long)n * 3 + c) * T + t) * H + (2 * hb + sy)) * W + 2 * wb;   // even
                const uint32_t q = (uint32_t)(e >> 2);
                const Philox4 ra = philox4x32_10(q, d, DPC_PHILOX_STREAM_INPUT, 0u, k0, k1);
                const bool odd = (e & 2) != 0;   // the first pair is the block's second half (W % 4 == 2 rows only)
                float x[4];
                box_muller(odd ? ra.v[2] : ra.v[0], odd ? ra.v[3] : ra.v[1], x[0], x[1]);
                x[2] = x[3] = 0.f;
                if (two) {
                    if (!odd) {
                        box_muller(ra.v[2], ra.v[3], x[2], x[3]);
                    } else {
                        const Philox4 rb = philox4x32_10(q + 1u, d, DPC_PHILOX_STREAM_INPUT, 0u, k0, k1);
                        box_muller(rb.v[0], rb.v[1], x[2], x[3]);
                    }
                }
                v[0][(sy * 2 + 0) * 3 + c] = x[0];
                v[0][(sy * 2 + 1) * 3 + c] = x[1];
                v[1][(sy * 2 + 0) * 3 + c] = x[2];
                v[1][(sy * 2 + 1) * 3 + c] = x[3];
                if (block) {
                    float2* p = (float2*)(block + e);
                    p[0] = make_float2(x[0], x[1]);
                    if (two) p[1] = make_float2(x[2], x[3]);
                }
            }
        if (out) {
            const long long cell = (((long long)n * T + t) * Hb + hb) * Wb + wb;
            u32x4* o = (u32x4*)(out + cell * 16);  // 16 channels = 2 (bf16) or 4 (f32) 16-byte units per cell
            constexpr int EPO = Elt<TO>::PER16;
            DPC_UNROLL
            for (int k = 0; k < 16 / EPO; ++k) o[k] = unit_pack<TO>(v[0] + k * EPO);
            if (two) {
                DPC_UNROLL
                for (int k = 0; k < 16 / EPO; ++k) o[16 / EPO + k] = unit_pack<TO>(v[1] + k * EPO);
            }
        }
    }
}

static inline unsigned grid_for(long long n, int block = 256, int cap = 16384) {
    long long g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

extern "C" int dpc_synthetic_input(float* block, void* out, int32_t dtype_out, int32_t BN, int32_t T, int32_t H, int32_t W, uint64_t seed,
                                   const int32_t* draw_dev, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if ((!block && !out) || !draw_dev || BN <= 0 || T <= 0 || H <= 0 || W <= 0) return DPC_ERR_ARG;
    if ((H & 1) || (W & 1)) return DPC_ERR_UNSUPPORTED;
    const long long pairs = (long long)BN * T * (H / 2) * ((W / 2 + 1) / 2);
    const long long elems = (long long)BN * 3 * T * H * W;
    if (pairs >= (1ll << 31) || elems > (1ll << 34)) return DPC_ERR_UNSUPPORTED;   // 32-bit cell index, 32-bit Philox block counter
    const dim3 grid(grid_for(pairs)), blk(256);
    if (dtype_out == DPC_F32) {
        DPC_LAUNCH((synthetic_input_kernel<float>), grid, blk, stream, block, (float*)out, BN, T, H, W, (unsigned long long)seed, draw_dev);
    } else if (dtype_out == DPC_BF16) {
        DPC_LAUNCH((synthetic_input_kernel<bf16_t>), grid, blk, stream, block, (bf16_t*)out, BN, T, H, W, (unsigned long long)seed, draw_dev);
    } else {
        return DPC_ERR_ARG;
    }
    return dpc_launch_status();
}
