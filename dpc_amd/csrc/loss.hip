// loss.hip -- contrastive head and optimizer of the train step:
//   mask      dpc/model_3d.py:86-96 (closed form; the reference builds it with B + B*SQ
//             Python index assignments, every step under multi-GPU DataParallel)
//   ce_topk   nn.CrossEntropyLoss + calc_topk_accuracy(1,3,5) with target = arange
//             (dpc/main.py:178-185,213-218; utils/utils.py:38-55), plus d(loss)/d(score)
//   adam      torch.optim.Adam(lr, weight_decay as L2) on the flat parameter buffer (main.py:80-81)
// All HBM-bound; row reductions use wave64 shuffles then one LDS hop across the 4 waves.
#include "dpc_rt.h"
#include "../../include/dpc_hip.h"

static inline unsigned grid_for(long long n, int block = 256, int cap = 8192) {
    long long g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

// mask[b][p][s][b2][n][s2]: 1 pos (b=b2,s=s2,p=n) | -1 temporal neg (b=b2,s=s2,p!=n) | -3 spatial neg (b=b2,s!=s2) | 0
__global__ void mask_gen_kernel(int8_t* mask, int B, int P, int SQ) {
    const long long row_len = (long long)B * P * SQ;
    const long long n = row_len * row_len;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / row_len, c = i % row_len;
        const int s = (int)(r % SQ), p = (int)((r / SQ) % P), b = (int)(r / ((long long)SQ * P));
        const int s2 = (int)(c % SQ), n2 = (int)((c / SQ) % P), b2 = (int)(c / ((long long)SQ * P));
        int8_t v = 0;
        if (b == b2) v = (s != s2) ? -3 : ((p == n2) ? 1 : -1);
        mask[i] = v;
    }
}

extern "C" int dpc_mask_gen(int8_t* mask, int32_t B, int32_t P, int32_t SQ, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!mask || B <= 0 || P <= 0 || SQ <= 0) return DPC_ERR_ARG;
    const long long rl = (long long)B * P * SQ;
    DPC_LAUNCH(mask_gen_kernel, dim3(grid_for(rl * rl)), dim3(256), stream, mask, B, P, SQ);
    return dpc_launch_status();
}

__device__ __forceinline__ float wave_max(float v) {
    DPC_UNROLL
    for (int m = 32; m >= 1; m >>= 1) { const float o = __shfl_xor(v, m); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    DPC_UNROLL
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// one workgroup per score row; three L2-resident sweeps (max, sum-exp + rank, gradient)
// EXT (dpc_ce_topk_ext, and the same arm of the two kernels below): the negative queue's per-row statistics qstats[row] = (m_q, l_q,
// rk_q, -) are folded in before the exponentials -- mx = max(mx, m_q), se += l_q exp(m_q - mx), rk += rk_q -- and lse_out[row] =
// log(se) + mx is kept for the queue's backward.  The kernels of the older entries are the EXT = false bodies: the lines they ran.
template <class TD, bool EXT>
__device__ __forceinline__ void ce_row_body(float* sh, const float* score, int rows, int cols, int ld, float* row_ws, TD* dscore, int ld_d,
                                            const float* qstats, float* lse_out) {
    const int row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* s = score + (long long)row * ld;
    const float tgt = s[row];  // target column = row (closed form of process_output on one GPU)
    float mx = -3.0e38f;
    for (int j = tid; j < cols; j += 256) { const float v = s[j]; mx = v > mx ? v : mx; }
    mx = wave_max(mx);
    if (lane == 0) sh[wv] = mx;
    __syncthreads();
    mx = sh[0];
    DPC_UNROLL
    for (int w = 1; w < 4; ++w) mx = sh[w] > mx ? sh[w] : mx;
    float mq = 0.f, lq = 0.f, rkq = 0.f;
    if constexpr (EXT) {
        mq = qstats[4 * (long long)row]; lq = qstats[4 * (long long)row + 1]; rkq = qstats[4 * (long long)row + 2];
        mx = mq > mx ? mq : mx;
    }
    float se = 0.f, rk = 0.f;
    for (int j = tid; j < cols; j += 256) {
        const float v = s[j];
        se += expf(v - mx);
        rk += (v > tgt) ? 1.f : 0.f;
    }
    se = wave_sum(se);
    rk = wave_sum(rk);
    __syncthreads();
    if (lane == 0) { sh[wv] = se; sh[4 + wv] = rk; }
    __syncthreads();
    se = sh[0] + sh[1] + sh[2] + sh[3];
    rk = sh[4] + sh[5] + sh[6] + sh[7];
    if constexpr (EXT) {
        se += lq * expf(mq - mx);
        rk += rkq;
    }
    if (tid == 0) {
        row_ws[2 * row + 0] = logf(se) + mx - tgt;
        row_ws[2 * row + 1] = rk;
        if constexpr (EXT) lse_out[row] = logf(se) + mx;
    }
    if (dscore) {
        const float inv = 1.f / se, invr = 1.f / (float)rows;
        TD* d = dscore + (long long)row * ld_d;
        for (int j = tid; j < cols; j += 256) {
            float g = expf(s[j] - mx) * inv;
            if (j == row) g -= 1.f;
            d[j] = Elt<TD>::from_f32(g * invr);
        }
        for (int j = cols + tid; j < ld_d; j += 256) d[j] = Elt<TD>::from_f32(0.f);
    }
}
template <class TD>
__global__ __launch_bounds__(256) void ce_row_kernel(const float* score, int rows, int cols, int ld, float* row_ws,
                                                     TD* dscore, int ld_d) {
    __shared__ float sh[8];
    ce_row_body<TD, false>(sh, score, rows, cols, ld, row_ws, dscore, ld_d, nullptr, nullptr);
}
template <class TD>
__global__ __launch_bounds__(256) void ce_row_ext_kernel(const float* score, int rows, int cols, int ld, float* row_ws, TD* dscore, int ld_d,
                                                         const float* qstats, float* lse_out) {
    __shared__ float sh[8];
    ce_row_body<TD, true>(sh, score, rows, cols, ld, row_ws, dscore, ld_d, qstats, lse_out);
}

// The same row kernel with the row held in REGISTERS (NV float4 per thread: one HBM read of the logits instead of three sweeps),
// 16-byte loads, one exponential per logit (kept for the gradient), 8/16-byte gradient stores.  Needs cols % 4 == 0, 16-byte
// aligned rows and cols <= 1024 NV; anything else takes ce_row_kernel.  FAST: v_exp_f32 (2^x, ~1 ulp) instead of libm expf --
// the throughput mode (bf16 gradient); the f32 parity mode keeps the exact form bit for bit.
// Measured at R = 6 144: ce_row_kernel 117 us for 151 MB of logits + 75 MB of gradient (1.9 TB/s).
template <class TD, int NV, bool FAST, bool EXT>
__device__ __forceinline__ void ce_row_vec_body(float* sh, const float* score, int rows, int cols, int ld, float* row_ws, TD* dscore, int ld_d,
                                                const float* qstats, float* lse_out) {
    const int row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* s = score + (long long)row * ld;
    const float tgt = s[row];
    const int nq = cols >> 2;
    f32x4 v[NV];
    float mx = -3.0e38f;
    DPC_UNROLL
    for (int i = 0; i < NV; ++i) {
        const int q = tid + 256 * i;
        f32x4 t = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
        if (q < nq) t = ((const f32x4*)s)[q];
        v[i] = t;
        DPC_UNROLL
        for (int e = 0; e < 4; ++e) mx = t[e] > mx ? t[e] : mx;
    }
    mx = wave_max(mx);
    if (lane == 0) sh[wv] = mx;
    __syncthreads();
    mx = sh[0];
    DPC_UNROLL
    for (int w = 1; w < 4; ++w) mx = sh[w] > mx ? sh[w] : mx;
    float mq = 0.f, lq = 0.f, rkq = 0.f;
    if constexpr (EXT) {
        mq = qstats[4 * (long long)row]; lq = qstats[4 * (long long)row + 1]; rkq = qstats[4 * (long long)row + 2];
        mx = mq > mx ? mq : mx;
    }
    float se = 0.f, rk = 0.f;
    const float nm = -mx * 1.4426950408889634f;
    DPC_UNROLL
    for (int i = 0; i < NV; ++i) {
        const bool ok = tid + 256 * i < nq;
        DPC_UNROLL
        for (int e = 0; e < 4; ++e) {
            const float x = v[i][e];
            rk += (ok && x > tgt) ? 1.f : 0.f;
            const float ex = FAST ? fast_exp2(fmaf(x, 1.4426950408889634f, nm)) : expf(x - mx);
            v[i][e] = ok ? ex : 0.f;
            se += v[i][e];
        }
    }
    se = wave_sum(se);
    rk = wave_sum(rk);
    __syncthreads();
    if (lane == 0) { sh[wv] = se; sh[4 + wv] = rk; }
    __syncthreads();
    se = sh[0] + sh[1] + sh[2] + sh[3];
    rk = sh[4] + sh[5] + sh[6] + sh[7];
    if constexpr (EXT) {
        se += lq * (FAST ? fast_exp2((mq - mx) * 1.4426950408889634f) : expf(mq - mx));
        rk += rkq;
    }
    if (tid == 0) {
        row_ws[2 * row + 0] = logf(se) + mx - tgt;
        row_ws[2 * row + 1] = rk;
        if constexpr (EXT) lse_out[row] = logf(se) + mx;
    }
    if (dscore) {
        const float inv = 1.f / se, invr = 1.f / (float)rows;
        TD* d = dscore + (long long)row * ld_d;
        DPC_UNROLL
        for (int i = 0; i < NV; ++i) {
            const int q = tid + 256 * i;
            if (q < nq) {
                float g[4];
                DPC_UNROLL
                for (int e = 0; e < 4; ++e) {
                    float t = v[i][e] * inv;
                    if (4 * q + e == row) t -= 1.f;
                    g[e] = t * invr;
                }
                if constexpr (sizeof(TD) == 2) {
                    const u32x2 o = {bf16x2_pack(g[0], g[1]), bf16x2_pack(g[2], g[3])};
                    *(u32x2*)(d + 4 * q) = o;
                } else {
                    const f32x4 o = {g[0], g[1], g[2], g[3]};
                    *(f32x4*)(d + 4 * q) = o;
                }
            }
        }
        for (int j = cols + tid; j < ld_d; j += 256) d[j] = Elt<TD>::from_f32(0.f);
    }
}
template <class TD, int NV, bool FAST>
__global__ __launch_bounds__(256) void ce_row_vec_kernel(const float* score, int rows, int cols, int ld, float* row_ws, TD* dscore, int ld_d) {
    __shared__ float sh[8];
    ce_row_vec_body<TD, NV, FAST, false>(sh, score, rows, cols, ld, row_ws, dscore, ld_d, nullptr, nullptr);
}
template <class TD, int NV, bool FAST>
__global__ __launch_bounds__(256) void ce_row_vec_ext_kernel(const float* score, int rows, int cols, int ld, float* row_ws, TD* dscore, int ld_d,
                                                             const float* qstats, float* lse_out) {
    __shared__ float sh[8];
    ce_row_vec_body<TD, NV, FAST, true>(sh, score, rows, cols, ld, row_ws, dscore, ld_d, qstats, lse_out);
}


// bf16 LOGITS (round 6): the train step never returns its score (engine.train_step), so the materialised score of that path is
// written and read in the compute dtype -- 75 MB instead of 151 MB at R = 6 144 on each side.  Same one-read row kernel: a thread
// holds NV 16-byte units of 8 logits; loss, rank and d(loss)/d(score) are those of the ROUNDED logits (the target logit included,
// so "strictly greater than the target" is decided among values of one precision).
template <int NV, bool EXT>
__device__ __forceinline__ void ce_row_vec16_body(float* sh, const bf16_t* score, int rows, int cols, int ld, float* row_ws, bf16_t* dscore, int ld_d,
                                                  const float* qstats, float* lse_out) {
    const int row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bf16_t* s = score + (long long)row * ld;
    const float tgt = bf16_to_f32(s[row]);
    const int nq = cols >> 3;
    float v[NV][8];
    float mx = -3.0e38f;
    DPC_UNROLL
    for (int i = 0; i < NV; ++i) {
        const int q = tid + 256 * i;
        if (q < nq) {
            const u32x4 t = ((const u32x4*)s)[q];
            DPC_UNROLL
            for (int e = 0; e < 8; ++e) { v[i][e] = unit_get<bf16_t>(t, e); mx = v[i][e] > mx ? v[i][e] : mx; }
        } else {
            DPC_UNROLL
            for (int e = 0; e < 8; ++e) v[i][e] = -3.0e38f;
        }
    }
    mx = wave_max(mx);
    if (lane == 0) sh[wv] = mx;
    __syncthreads();
    mx = sh[0];
    DPC_UNROLL
    for (int w = 1; w < 4; ++w) mx = sh[w] > mx ? sh[w] : mx;
    float mq = 0.f, lq = 0.f, rkq = 0.f;
    if constexpr (EXT) {
        mq = qstats[4 * (long long)row]; lq = qstats[4 * (long long)row + 1]; rkq = qstats[4 * (long long)row + 2];
        mx = mq > mx ? mq : mx;
    }
    float se = 0.f, rk = 0.f;
    const float nm = -mx * 1.4426950408889634f;
    DPC_UNROLL
    for (int i = 0; i < NV; ++i) {
        const bool ok = tid + 256 * i < nq;
        DPC_UNROLL
        for (int e = 0; e < 8; ++e) {
            const float x = v[i][e];
            rk += (ok && x > tgt) ? 1.f : 0.f;
            const float ex = fast_exp2(fmaf(x, 1.4426950408889634f, nm));
            v[i][e] = ok ? ex : 0.f;
            se += v[i][e];
        }
    }
    se = wave_sum(se);
    rk = wave_sum(rk);
    __syncthreads();
    if (lane == 0) { sh[wv] = se; sh[4 + wv] = rk; }
    __syncthreads();
    se = sh[0] + sh[1] + sh[2] + sh[3];
    rk = sh[4] + sh[5] + sh[6] + sh[7];
    if constexpr (EXT) {
        se += lq * fast_exp2((mq - mx) * 1.4426950408889634f);
        rk += rkq;
    }
    if (tid == 0) {
        row_ws[2 * row + 0] = logf(se) + mx - tgt;
        row_ws[2 * row + 1] = rk;
        if constexpr (EXT) lse_out[row] = logf(se) + mx;
    }
    if (dscore) {
        const float inv = 1.f / se, invr = 1.f / (float)rows;
        bf16_t* d = dscore + (long long)row * ld_d;
        DPC_UNROLL
        for (int i = 0; i < NV; ++i) {
            const int q = tid + 256 * i;
            if (q < nq) {
                float g[8];
                DPC_UNROLL
                for (int e = 0; e < 8; ++e) {
                    float t = v[i][e] * inv;
                    if (8 * q + e == row) t -= 1.f;
                    g[e] = t * invr;
                }
                *(u32x4*)(d + 8 * q) = unit_pack<bf16_t>(g);
            }
        }
        for (int j = cols + tid; j < ld_d; j += 256) d[j] = Elt<bf16_t>::from_f32(0.f);
    }
}
template <int NV>
__global__ __launch_bounds__(256) void ce_row_vec16_kernel(const bf16_t* score, int rows, int cols, int ld, float* row_ws, bf16_t* dscore, int ld_d) {
    __shared__ float sh[8];
    ce_row_vec16_body<NV, false>(sh, score, rows, cols, ld, row_ws, dscore, ld_d, nullptr, nullptr);
}
template <int NV>
__global__ __launch_bounds__(256) void ce_row_vec16_ext_kernel(const bf16_t* score, int rows, int cols, int ld, float* row_ws, bf16_t* dscore, int ld_d,
                                                               const float* qstats, float* lse_out) {
    __shared__ float sh[8];
    ce_row_vec16_body<NV, true>(sh, score, rows, cols, ld, row_ws, dscore, ld_d, qstats, lse_out);
}

__global__ __launch_bounds__(256) void ce_finalize_kernel(const float* row_ws, int rows, float* result) {
    __shared__ float sh[4][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float a[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = tid; r < rows; r += 256) {
        const float rk = row_ws[2 * r + 1];
        a[0] += row_ws[2 * r];
        a[1] += rk < 1.f ? 1.f : 0.f;
        a[2] += rk < 3.f ? 1.f : 0.f;
        a[3] += rk < 5.f ? 1.f : 0.f;
    }
    DPC_UNROLL
    for (int k = 0; k < 4; ++k) {
        a[k] = wave_sum(a[k]);
        if (lane == 0) sh[wv][k] = a[k];
    }
    __syncthreads();
    if (tid < 4) result[tid] = (sh[0][tid] + sh[1][tid] + sh[2][tid] + sh[3][tid]) / (float)rows;
}

extern "C" int dpc_ce_topk(const float* score, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result,
                           void* dscore, int32_t dtype_d, int32_t ld_d, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!score || !row_ws || !result || rows <= 0 || cols < rows || ld < cols) return DPC_ERR_ARG;
    if (dscore && ld_d < cols) return DPC_ERR_ARG;
    // register-resident row form: 16-byte aligned rows of the logits (and of the gradient), cols a multiple of 4, at most 16 K columns
    const bool vec = cols % 4 == 0 && ld % 4 == 0 && ((uintptr_t)score % 16) == 0 && cols <= 16384 &&
                     (!dscore || (ld_d % 4 == 0 && ((uintptr_t)dscore % 16) == 0));
    if (!dscore || dtype_d == DPC_F32) {
        if (vec && cols <= 8192) {
            DPC_LAUNCH((ce_row_vec_kernel<float, 8, false>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (float*)dscore, ld_d);
        } else if (vec) {
            DPC_LAUNCH((ce_row_vec_kernel<float, 16, false>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (float*)dscore, ld_d);
        } else {
            DPC_LAUNCH((ce_row_kernel<float>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (float*)dscore, ld_d);
        }
    } else if (dtype_d == DPC_BF16) {
        if (vec && cols <= 8192) {
            DPC_LAUNCH((ce_row_vec_kernel<bf16_t, 8, true>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (bf16_t*)dscore, ld_d);
        } else if (vec) {
            DPC_LAUNCH((ce_row_vec_kernel<bf16_t, 16, true>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (bf16_t*)dscore, ld_d);
        } else {
            DPC_LAUNCH((ce_row_kernel<bf16_t>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (bf16_t*)dscore, ld_d);
        }
    } else {
        return DPC_ERR_ARG;
    }
    DPC_LAUNCH(ce_finalize_kernel, dim3(1), dim3(256), stream, row_ws, rows, result);
    return dpc_launch_status();
}

// dpc_ce_topk on bf16 logits with a bf16 gradient (the train step's materialised score in the compute dtype): rows of 16-byte units,
// cols a multiple of 8, at most 16 384 columns -- anything else is DPC_ERR_UNSUPPORTED (the caller keeps f32 logits then).
extern "C" int dpc_ce_topk_bf16(const void* score, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result,
                                void* dscore, int32_t ld_d, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!score || !row_ws || !result || rows <= 0 || cols < rows || ld < cols) return DPC_ERR_ARG;
    if (dscore && ld_d < cols) return DPC_ERR_ARG;
    if (cols % 8 || ld % 8 || ((uintptr_t)score % 16) || cols > 16384 || (dscore && (ld_d % 8 || ((uintptr_t)dscore % 16)))) return DPC_ERR_UNSUPPORTED;
    if (cols <= 2048 * 4) {
        DPC_LAUNCH((ce_row_vec16_kernel<4>), dim3(rows), dim3(256), stream, (const bf16_t*)score, rows, cols, ld, row_ws, (bf16_t*)dscore, ld_d);
    } else {
        DPC_LAUNCH((ce_row_vec16_kernel<8>), dim3(rows), dim3(256), stream, (const bf16_t*)score, rows, cols, ld, row_ws, (bf16_t*)dscore, ld_d);
    }
    DPC_LAUNCH(ce_finalize_kernel, dim3(1), dim3(256), stream, row_ws, rows, result);
    return dpc_launch_status();
}

// ---- the same two entries with the negative queue's statistics (include/dpc_hip.h): the dispatch conditions of the entries above, the
// EXT arm of the row kernel each of them selects
extern "C" int dpc_ce_topk_ext(const float* score, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result, void* dscore,
                               int32_t dtype_d, int32_t ld_d, const float* qstats, float* lse_out, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!score || !row_ws || !result || rows <= 0 || cols < rows || ld < cols || !qstats || !lse_out) return DPC_ERR_ARG;
    if (dscore && ld_d < cols) return DPC_ERR_ARG;
    const bool vec = cols % 4 == 0 && ld % 4 == 0 && ((uintptr_t)score % 16) == 0 && cols <= 16384 &&
                     (!dscore || (ld_d % 4 == 0 && ((uintptr_t)dscore % 16) == 0));
    if (!dscore || dtype_d == DPC_F32) {
        if (vec && cols <= 8192) {
            DPC_LAUNCH((ce_row_vec_ext_kernel<float, 8, false>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (float*)dscore, ld_d, qstats, lse_out);
        } else if (vec) {
            DPC_LAUNCH((ce_row_vec_ext_kernel<float, 16, false>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (float*)dscore, ld_d, qstats, lse_out);
        } else {
            DPC_LAUNCH((ce_row_ext_kernel<float>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (float*)dscore, ld_d, qstats, lse_out);
        }
    } else if (dtype_d == DPC_BF16) {
        if (vec && cols <= 8192) {
            DPC_LAUNCH((ce_row_vec_ext_kernel<bf16_t, 8, true>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (bf16_t*)dscore, ld_d, qstats, lse_out);
        } else if (vec) {
            DPC_LAUNCH((ce_row_vec_ext_kernel<bf16_t, 16, true>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (bf16_t*)dscore, ld_d, qstats, lse_out);
        } else {
            DPC_LAUNCH((ce_row_ext_kernel<bf16_t>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (bf16_t*)dscore, ld_d, qstats, lse_out);
        }
    } else {
        return DPC_ERR_ARG;
    }
    DPC_LAUNCH(ce_finalize_kernel, dim3(1), dim3(256), stream, row_ws, rows, result);
    return dpc_launch_status();
}

extern "C" int dpc_ce_topk_bf16_ext(const void* score, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result, void* dscore,
                                    int32_t ld_d, const float* qstats, float* lse_out, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!score || !row_ws || !result || rows <= 0 || cols < rows || ld < cols || !qstats || !lse_out) return DPC_ERR_ARG;
    if (dscore && ld_d < cols) return DPC_ERR_ARG;
    if (cols % 8 || ld % 8 || ((uintptr_t)score % 16) || cols > 16384 || (dscore && (ld_d % 8 || ((uintptr_t)dscore % 16)))) return DPC_ERR_UNSUPPORTED;
    if (cols <= 2048 * 4) {
        DPC_LAUNCH((ce_row_vec16_ext_kernel<4>), dim3(rows), dim3(256), stream, (const bf16_t*)score, rows, cols, ld, row_ws, (bf16_t*)dscore, ld_d, qstats, lse_out);
    } else {
        DPC_LAUNCH((ce_row_vec16_ext_kernel<8>), dim3(rows), dim3(256), stream, (const bf16_t*)score, rows, cols, ld, row_ws, (bf16_t*)dscore, ld_d, qstats, lse_out);
    }
    DPC_LAUNCH(ce_finalize_kernel, dim3(1), dim3(256), stream, row_ws, rows, result);
    return dpc_launch_status();
}

// mean loss + top-1/3/5 from per-row (loss term, rank) pairs: the last stage of dpc_ce_topk, exposed for the fused score
// path (csrc/score_fused.hip), whose forward produces the pairs without a score matrix
extern "C" int dpc_ce_finalize(const float* row_ws, int32_t rows, float* result, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!row_ws || rows <= 0 || !result) return DPC_ERR_ARG;
    DPC_LAUNCH(ce_finalize_kernel, dim3(1), dim3(256), stream, row_ws, rows, result);
    return dpc_launch_status();
}

// Adam, weight decay folded into the gradient (torch.optim.Adam semantics), 16-byte accesses
__global__ void adam_kernel(float* p, const float* g, float* m, float* v, long long n4, long long n, float lr, float b1,
                            float b2, float eps, float wd, float bc1, float bc2, float gscale) {
    const float step = lr / bc1;
    const float isb2 = 1.f / sqrtf(bc2);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const long long base = i * 4;
        if (base + 4 <= n) {
            f32x4 pv = ((f32x4*)p)[i], gv = ((const f32x4*)g)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
            DPC_UNROLL
            for (int e = 0; e < 4; ++e) {
                const float gg = gv[e] * gscale + wd * pv[e];
                mv[e] = b1 * mv[e] + (1.f - b1) * gg;
                vv[e] = b2 * vv[e] + (1.f - b2) * gg * gg;
                pv[e] -= step * mv[e] / (sqrtf(vv[e]) * isb2 + eps);
            }
            ((f32x4*)p)[i] = pv; ((f32x4*)m)[i] = mv; ((f32x4*)v)[i] = vv;
        } else {
            for (long long k = base; k < n; ++k) {
                const float gg = g[k] * gscale + wd * p[k];
                m[k] = b1 * m[k] + (1.f - b1) * gg;
                v[k] = b2 * v[k] + (1.f - b2) * gg * gg;
                p[k] -= step * m[k] / (sqrtf(v[k]) * isb2 + eps);
            }
        }
    }
}

// ---- graph-capturable optimizer step: the step counter and Adam's bias corrections live in device memory, so a captured
// hipGraph of the whole train step advances them on every replay (host scalars would be frozen at capture time)
__global__ void step_advance_kernel(int32_t* step, float* bc, double b1, double b2) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const int t = step[0] + 1;
        step[0] = t;
        bc[0] = (float)(1.0 - pow(b1, (double)t));
        bc[1] = (float)(1.0 - pow(b2, (double)t));
    }
}

extern "C" int dpc_step_advance(int32_t* step_dev, float* bias_corr_dev, double beta1, double beta2, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!step_dev || !bias_corr_dev) return DPC_ERR_ARG;
    DPC_LAUNCH(step_advance_kernel, dim3(1), dim3(64), stream, step_dev, bias_corr_dev, beta1, beta2);
    return dpc_launch_status();
}

// ---- per-step learning-rate schedule (include/dpc_hip.h: dpc_lr_schedule): the multiplier of the step about to be taken, formed by
// the one thread that advances the counter and read by the Adam kernel of the same step -- no launch of its own.  k is the count of
// completed optimizer steps, so a step the guard skips does not move the schedule and a resumed run continues it from dev_step.
// Double throughout, no contraction: the host statement (dpc_amd/optim.py: lr_multiplier) performs the same roundings one by one.
__device__ __forceinline__ double lr_mult(const dpc_lr_schedule& s, int k) {
#pragma clang fp contract(off)
    const int W = s.warmup_steps;
    if (k < W) return (double)(k + 1) / (double)W;
    if (s.kind == DPC_LR_COSINE || s.kind == DPC_LR_LINEAR) {
        const double m0 = s.min_mult;
        const double x = (double)(k - W) / (double)(s.total_steps - W);
        if (x >= 1.0) return m0;
        const double shape = s.kind == DPC_LR_COSINE ? 0.5 * (1.0 + cos(3.141592653589793 * x)) : 1.0 - x;
        return m0 + (1.0 - m0) * shape;
    }
    double mult = 1.0;
    if (s.kind == DPC_LR_MULTISTEP)
        for (int i = 0; i < s.n_milestones; ++i)
            if (s.milestones[i] <= k) mult *= s.gamma;
    return mult;
}

__global__ void step_advance_sched_kernel(int32_t* step, float* bc, double b1, double b2, const dpc_grad_state* st, dpc_lr_schedule sched,
                                          dpc_lr_state* lrs) {
    if (threadIdx.x == 0 && blockIdx.x == 0 && !(st && st->skip)) {
        const int k = step[0], t = k + 1;
        step[0] = t;
        bc[0] = (float)(1.0 - pow(b1, (double)t));
        bc[1] = (float)(1.0 - pow(b2, (double)t));
        lrs->mult = (float)lr_mult(sched, k);
        lrs->k = k;
    }
}

static bool lr_schedule_ok(const dpc_lr_schedule* s) {
    if (!s || s->kind < DPC_LR_CONSTANT || s->kind > DPC_LR_MULTISTEP || s->warmup_steps < 0) return false;
    if (s->kind == DPC_LR_COSINE || s->kind == DPC_LR_LINEAR) {
        if (!(s->total_steps > s->warmup_steps) || !(s->min_mult >= 0.0 && s->min_mult <= 1.0)) return false;
    }
    if (s->kind == DPC_LR_MULTISTEP) {
        if (s->n_milestones < 0 || s->n_milestones > DPC_LR_MAX_MILESTONES || !(s->gamma > 0.0 && s->gamma <= 1.0)) return false;
        for (int i = 0; i < s->n_milestones; ++i)
            if (s->milestones[i] < 0 || (i && s->milestones[i] <= s->milestones[i - 1])) return false;
    }
    return true;
}

// state_dev: the gradient guard's verdict (dpc_step_advance_gated), or null (dpc_step_advance)
extern "C" int dpc_step_advance_sched(int32_t* step_dev, float* bias_corr_dev, double beta1, double beta2, const dpc_grad_state* state_dev,
                                      const dpc_lr_schedule* schedule, dpc_lr_state* lr_state_dev, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!step_dev || !bias_corr_dev || !lr_state_dev || (uintptr_t)lr_state_dev % 4 || !lr_schedule_ok(schedule)) return DPC_ERR_ARG;
    const dpc_lr_schedule by_value = *schedule;
    DPC_LAUNCH(step_advance_sched_kernel, dim3(1), dim3(64), stream, step_dev, bias_corr_dev, beta1, beta2, state_dev, by_value, lr_state_dev);
    return dpc_launch_status();
}

// draw counter of the dropout streams: advanced by every train-mode forward (not by the optimizer step), so a caller that never
// runs the engine's own Adam -- the nn.Module boundary with a torch optimizer -- still sees fresh masks each forward
__global__ void counter_advance_kernel(int32_t* ctr) {
    if (threadIdx.x == 0 && blockIdx.x == 0) ctr[0] += 1;
}

extern "C" int dpc_counter_advance(int32_t* counter_dev, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!counter_dev) return DPC_ERR_ARG;
    DPC_LAUNCH(counter_advance_kernel, dim3(1), dim3(64), stream, counter_dev);
    return dpc_launch_status();
}

// ---- EMA arm of the two device-side Adam kernels (dpc_adam_dev_ema / dpc_adam_groups_dev_ema): the exponential moving average of
// the parameters, updated by the thread that has just updated the 16-byte unit -- p_new is still in registers, so the average costs
// one more f32 arena read and written by the kernel that already streams four; no launch of its own.
//   e += (1 - d) (p_new - e),  d = min(decay, (1 + t) / (10 + t)),  t = step_dev[0] (the step count after this step's advance)
// all in f32.  The lerp form has e == p as a fixed point, bit for bit.  EMA = false is the kernel as it was: same arithmetic, same order.
__device__ __forceinline__ float ema_weight(const int32_t* step_dev, float decay) {
    const int t = step_dev[0];
    const float d = fminf(decay, (float)(1 + t) / (float)(10 + t));
    return 1.f - d;
}

template <bool EMA>
__global__ void adam_dev_kernel(float* p, const float* g, float* m, float* v, long long n4, long long n, float lr, float b1,
                                float b2, float omb1, float omb2, float eps, float wd, const float* bc, float gscale,
                                const dpc_grad_state* gs, float* ema, const int32_t* step_dev, float decay) {
    if (gs) {   // the gradient guard's verdict (grad_guard.hip): a skipped step loads and stores nothing
        if (gs->skip) return;
        gscale = gscale * gs->coef;
    }
    const float step = lr / bc[0];
    const float isb2 = 1.f / sqrtf(bc[1]);
    float omd = 0.f;
    if constexpr (EMA) omd = ema_weight(step_dev, decay);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const long long base = i * 4;
        if (base + 4 <= n) {
            f32x4 pv = ((f32x4*)p)[i], gv = ((const f32x4*)g)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
            DPC_UNROLL
            for (int e = 0; e < 4; ++e) {
                const float gg = gv[e] * gscale + wd * pv[e];
                mv[e] = b1 * mv[e] + omb1 * gg;
                vv[e] = b2 * vv[e] + omb2 * gg * gg;
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
                const float gg = g[k] * gscale + wd * p[k];
                m[k] = b1 * m[k] + omb1 * gg;
                v[k] = b2 * v[k] + omb2 * gg * gg;
                p[k] -= step * m[k] / (sqrtf(v[k]) * isb2 + eps);
                if constexpr (EMA) ema[k] += omd * (p[k] - ema[k]);
            }
        }
    }
}

// betas arrive as doubles: 1 - beta2 is formed in double like torch does (1 - 0.999f would be off by 1.3e-5 relative)
// state_dev: the gradient guard's verdict, or null (dpc_adam_dev)
extern "C" int dpc_adam_dev_ex(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2,
                               float eps, float wd, const float* bias_corr_dev, float grad_scale, const dpc_grad_state* state_dev,
                               dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p || !g || !m || !v || n <= 0 || !bias_corr_dev) return DPC_ERR_ARG;
    const long long n4 = (n + 3) / 4;
    DPC_LAUNCH((adam_dev_kernel<false>), dim3(grid_for(n4)), dim3(256), stream, p, g, m, v, n4, (long long)n, lr, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, wd, bias_corr_dev, grad_scale, state_dev, (float*)nullptr, (const int32_t*)nullptr, 0.f);
    return dpc_launch_status();
}

// dpc_adam_dev_ex plus the parameter average (see ema_weight): ema is one more f32 arena of n floats, 16-byte aligned and not p;
// step_dev is the device step counter dpc_step_advance[_gated] has already advanced for this step; 0 < decay < 1
extern "C" int dpc_adam_dev_ema(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2,
                                float eps, float wd, const float* bias_corr_dev, float grad_scale, const dpc_grad_state* state_dev,
                                float* ema, const int32_t* step_dev, float decay, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p || !g || !m || !v || n <= 0 || !bias_corr_dev) return DPC_ERR_ARG;
    if (!ema || ema == p || !step_dev || !(decay > 0.f && decay < 1.f)) return DPC_ERR_ARG;
    if (((uintptr_t)p | (uintptr_t)ema) % 16) return DPC_ERR_ARG;
    const long long n4 = (n + 3) / 4;
    DPC_LAUNCH((adam_dev_kernel<true>), dim3(grid_for(n4)), dim3(256), stream, p, g, m, v, n4, (long long)n, lr, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, wd, bias_corr_dev, grad_scale, state_dev, ema, step_dev, decay);
    return dpc_launch_status();
}

extern "C" int dpc_adam_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2,
                            float eps, float wd, const float* bias_corr_dev, float grad_scale, dpc_stream_t stream_) {
    return dpc_adam_dev_ex(p, g, m, v, n, lr, beta1, beta2, eps, wd, bias_corr_dev, grad_scale, nullptr, stream_);
}

extern "C" int dpc_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                        float eps, float wd, float bias_corr1, float bias_corr2, float grad_scale, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p || !g || !m || !v || n <= 0 || bias_corr1 <= 0.f || bias_corr2 <= 0.f) return DPC_ERR_ARG;
    const long long n4 = (n + 3) / 4;
    DPC_LAUNCH(adam_kernel, dim3(grid_for(n4)), dim3(256), stream, p, g, m, v, n4, (long long)n, lr, beta1, beta2, eps, wd, bias_corr1, bias_corr2, grad_scale);
    return dpc_launch_status();
}

// ---- Adam over the flat arenas with per-segment learning rate / weight decay and frozen segments (parameter groups of
// torch.optim.Adam: eval/test.py:76-84 builds one group per parameter; requires_grad = False or a group that leaves a parameter
// out freezes it).  One launch.  The segment table (sorted, non-overlapping, begin / end multiples of 4 floats so that a 16-byte
// unit never straddles two parameters; gaps = arena padding, never touched) is copied into LDS once per workgroup.  A workgroup
// walks contiguous tiles of ADAM_TILE4 16-byte units: one binary search per tile for the first segment that ends behind the
// tile's start, then every thread advances linearly from there (its units ascend).  A unit outside every segment or inside an
// inactive one costs no load and no store.  Per-element arithmetic: adam_dev_kernel's.
constexpr int ADAM_TILE4 = 1024;  // 16-byte units per tile: 4 per thread, 16 KB of each arena
template <bool EMA>   // the EMA arm: see adam_dev_kernel; a unit the update skips (gap, frozen segment) is skipped in ema too
__global__ __launch_bounds__(256) void adam_groups_kernel(float* p, const float* g, float* m, float* v, long long n4, long long ntiles,
                                                          const dpc_adam_segment* segs, int nseg, float b1, float b2, float omb1,
                                                          float omb2, float eps, const float* bc, float gscale,
                                                          const dpc_grad_state* gs, float* ema, const int32_t* step_dev, float decay) {
    if (gs) {   // as in adam_dev_kernel
        if (gs->skip) return;
        gscale = gscale * gs->coef;
    }
    __shared__ long long s_begin[DPC_ADAM_MAX_SEGMENTS], s_end[DPC_ADAM_MAX_SEGMENTS];
    __shared__ float s_lr[DPC_ADAM_MAX_SEGMENTS], s_wd[DPC_ADAM_MAX_SEGMENTS];   // lr < 0 marks an inactive segment
    const int tid = threadIdx.x;
    for (int s = tid; s < nseg; s += 256) {
        s_begin[s] = segs[s].begin;
        s_end[s] = segs[s].end;
        s_lr[s] = segs[s].active ? segs[s].lr : -1.f;
        s_wd[s] = segs[s].weight_decay;
    }
    __syncthreads();
    const float bc1 = bc[0];
    const float isb2 = 1.f / sqrtf(bc[1]);
    float omd = 0.f;
    if constexpr (EMA) omd = ema_weight(step_dev, decay);
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long t0 = tile * ADAM_TILE4 * 4;   // first float of the tile
        int lo = 0, hi = nseg;                       // first segment with end > t0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_end[mid] <= t0) lo = mid + 1; else hi = mid;
        }
        int s = lo;
        DPC_UNROLL
        for (int j = 0; j < ADAM_TILE4 / 256; ++j) {
            const long long i = tile * ADAM_TILE4 + tid + 256 * j;
            const long long base = i * 4;
            if (i >= n4) break;
            while (s < nseg && s_end[s] <= base) ++s;
            if (s >= nseg) break;
            if (s_begin[s] > base || s_lr[s] < 0.f) continue;   // padding between segments, or frozen
            const float step = s_lr[s] / bc1, wd = s_wd[s];
            f32x4 pv = ((f32x4*)p)[i], gv = ((const f32x4*)g)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
            DPC_UNROLL
            for (int e = 0; e < 4; ++e) {
                const float gg = gv[e] * gscale + wd * pv[e];
                mv[e] = b1 * mv[e] + omb1 * gg;
                vv[e] = b2 * vv[e] + omb2 * gg * gg;
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

// n: floats in each arena, a multiple of 4 (the arenas keep every tensor 16-byte aligned).  The table is validated where it is built
// (dpc_amd/engine.py: sorted, aligned, inside the arena); here only pointers and counts are.
extern "C" int dpc_adam_groups_dev_ex(float* p, const float* g, float* m, float* v, int64_t n, const dpc_adam_segment* segments_dev,
                                      int32_t n_segments, double beta1, double beta2, float eps, const float* bias_corr_dev,
                                      float grad_scale, const dpc_grad_state* state_dev, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p || !g || !m || !v || n <= 0 || n % 4 || !segments_dev || n_segments <= 0 || n_segments > DPC_ADAM_MAX_SEGMENTS || !bias_corr_dev)
        return DPC_ERR_ARG;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16) return DPC_ERR_ARG;
    const long long n4 = n / 4, ntiles = (n4 + ADAM_TILE4 - 1) / ADAM_TILE4;
    const unsigned grid = (unsigned)(ntiles < 2048 ? ntiles : 2048);
    DPC_LAUNCH((adam_groups_kernel<false>), dim3(grid), dim3(256), stream, p, g, m, v, n4, ntiles, segments_dev, (int)n_segments, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, bias_corr_dev, grad_scale, state_dev, (float*)nullptr, (const int32_t*)nullptr, 0.f);
    return dpc_launch_status();
}

// dpc_adam_groups_dev_ex plus the parameter average: the arguments dpc_adam_dev_ema adds, with the same requirements
extern "C" int dpc_adam_groups_dev_ema(float* p, const float* g, float* m, float* v, int64_t n, const dpc_adam_segment* segments_dev,
                                       int32_t n_segments, double beta1, double beta2, float eps, const float* bias_corr_dev,
                                       float grad_scale, const dpc_grad_state* state_dev, float* ema, const int32_t* step_dev,
                                       float decay, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p || !g || !m || !v || n <= 0 || n % 4 || !segments_dev || n_segments <= 0 || n_segments > DPC_ADAM_MAX_SEGMENTS || !bias_corr_dev)
        return DPC_ERR_ARG;
    if (!ema || ema == p || !step_dev || !(decay > 0.f && decay < 1.f)) return DPC_ERR_ARG;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema) % 16) return DPC_ERR_ARG;
    const long long n4 = n / 4, ntiles = (n4 + ADAM_TILE4 - 1) / ADAM_TILE4;
    const unsigned grid = (unsigned)(ntiles < 2048 ? ntiles : 2048);
    DPC_LAUNCH((adam_groups_kernel<true>), dim3(grid), dim3(256), stream, p, g, m, v, n4, ntiles, segments_dev, (int)n_segments, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, bias_corr_dev, grad_scale, state_dev, ema, step_dev, decay);
    return dpc_launch_status();
}

extern "C" int dpc_adam_groups_dev(float* p, const float* g, float* m, float* v, int64_t n, const dpc_adam_segment* segments_dev,
                                   int32_t n_segments, double beta1, double beta2, float eps, const float* bias_corr_dev,
                                   float grad_scale, dpc_stream_t stream_) {
    return dpc_adam_groups_dev_ex(p, g, m, v, n, segments_dev, n_segments, beta1, beta2, eps, bias_corr_dev, grad_scale, nullptr, stream_);
}

// ---- the scheduled arm of both updates (dpc_adam_dev_sched / dpc_adam_groups_dev_sched): adam_dev_kernel and adam_groups_kernel with
// the step size (lr * lrs->mult) / bc1, lrs the record step_advance_sched_kernel has just written -- the f32 product first.  Kernels of
// their own, so that every older entry launches the kernel, with the argument list, it always launched; the bodies are those kernels'
// line for line except where marked, and tests/lr_schedule_cases.py holds mult = 1 to their bits.
template <bool EMA>
__global__ void adam_dev_sched_kernel(float* p, const float* g, float* m, float* v, long long n4, long long n, float lr, float b1,
                                float b2, float omb1, float omb2, float eps, float wd, const float* bc, float gscale,
                                const dpc_grad_state* gs, float* ema, const int32_t* step_dev, float decay, const dpc_lr_state* lrs) {
    if (gs) {   // the gradient guard's verdict (grad_guard.hip): a skipped step loads and stores nothing
        if (gs->skip) return;
        gscale = gscale * gs->coef;
    }
    const float step = (lr * lrs->mult) / bc[0];   // the f32 product first, then the division adam_dev_kernel performs
    const float isb2 = 1.f / sqrtf(bc[1]);
    float omd = 0.f;
    if constexpr (EMA) omd = ema_weight(step_dev, decay);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const long long base = i * 4;
        if (base + 4 <= n) {
            f32x4 pv = ((f32x4*)p)[i], gv = ((const f32x4*)g)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
            DPC_UNROLL
            for (int e = 0; e < 4; ++e) {
                const float gg = gv[e] * gscale + wd * pv[e];
                mv[e] = b1 * mv[e] + omb1 * gg;
                vv[e] = b2 * vv[e] + omb2 * gg * gg;
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
                const float gg = g[k] * gscale + wd * p[k];
                m[k] = b1 * m[k] + omb1 * gg;
                v[k] = b2 * v[k] + omb2 * gg * gg;
                p[k] -= step * m[k] / (sqrtf(v[k]) * isb2 + eps);
                if constexpr (EMA) ema[k] += omd * (p[k] - ema[k]);
            }
        }
    }
}


template <bool EMA>
__global__ __launch_bounds__(256) void adam_groups_sched_kernel(float* p, const float* g, float* m, float* v, long long n4, long long ntiles,
                                                          const dpc_adam_segment* segs, int nseg, float b1, float b2, float omb1,
                                                          float omb2, float eps, const float* bc, float gscale,
                                                          const dpc_grad_state* gs, float* ema, const int32_t* step_dev, float decay, const dpc_lr_state* lrs) {
    if (gs) {   // as in adam_dev_kernel
        if (gs->skip) return;
        gscale = gscale * gs->coef;
    }
    __shared__ long long s_begin[DPC_ADAM_MAX_SEGMENTS], s_end[DPC_ADAM_MAX_SEGMENTS];
    __shared__ float s_lr[DPC_ADAM_MAX_SEGMENTS], s_wd[DPC_ADAM_MAX_SEGMENTS];   // lr < 0 marks an inactive segment
    const int tid = threadIdx.x;
    const float mult = lrs->mult;   // uniform
    for (int s = tid; s < nseg; s += 256) {
        s_begin[s] = segs[s].begin;
        s_end[s] = segs[s].end;
        s_lr[s] = segs[s].active ? segs[s].lr * mult : -1.f;   // lr, mult >= 0: the product never reads as inactive
        s_wd[s] = segs[s].weight_decay;
    }
    __syncthreads();
    const float bc1 = bc[0];
    const float isb2 = 1.f / sqrtf(bc[1]);
    float omd = 0.f;
    if constexpr (EMA) omd = ema_weight(step_dev, decay);
    for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const long long t0 = tile * ADAM_TILE4 * 4;   // first float of the tile
        int lo = 0, hi = nseg;                       // first segment with end > t0
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (s_end[mid] <= t0) lo = mid + 1; else hi = mid;
        }
        int s = lo;
        DPC_UNROLL
        for (int j = 0; j < ADAM_TILE4 / 256; ++j) {
            const long long i = tile * ADAM_TILE4 + tid + 256 * j;
            const long long base = i * 4;
            if (i >= n4) break;
            while (s < nseg && s_end[s] <= base) ++s;
            if (s >= nseg) break;
            if (s_begin[s] > base || s_lr[s] < 0.f) continue;   // padding between segments, or frozen
            const float step = s_lr[s] / bc1, wd = s_wd[s];
            f32x4 pv = ((f32x4*)p)[i], gv = ((const f32x4*)g)[i], mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i];
            DPC_UNROLL
            for (int e = 0; e < 4; ++e) {
                const float gg = gv[e] * gscale + wd * pv[e];
                mv[e] = b1 * mv[e] + omb1 * gg;
                vv[e] = b2 * vv[e] + omb2 * gg * gg;
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


// The entries: the _ema entries' arguments plus the record.  The average is optional here (ema and step_dev both null: the <false>
// kernels), so one entry serves guard x EMA.
static inline bool sched_ema_ok(const float* p, const float* ema, const int32_t* step_dev, float decay) {
    if (!ema) return !step_dev;
    return ema != p && step_dev && decay > 0.f && decay < 1.f && ((uintptr_t)p | (uintptr_t)ema) % 16 == 0;
}

extern "C" int dpc_adam_dev_sched(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2,
                                  float eps, float wd, const float* bias_corr_dev, float grad_scale, const dpc_grad_state* state_dev,
                                  float* ema, const int32_t* step_dev, float decay, const dpc_lr_state* lr_state_dev,
                                  dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p || !g || !m || !v || n <= 0 || !bias_corr_dev || !lr_state_dev || (uintptr_t)lr_state_dev % 4) return DPC_ERR_ARG;
    if (!sched_ema_ok(p, ema, step_dev, decay)) return DPC_ERR_ARG;
    const long long n4 = (n + 3) / 4;
    if (ema)
        DPC_LAUNCH((adam_dev_sched_kernel<true>), dim3(grid_for(n4)), dim3(256), stream, p, g, m, v, n4, (long long)n, lr, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, wd, bias_corr_dev, grad_scale, state_dev, ema, step_dev, decay, lr_state_dev);
    else
        DPC_LAUNCH((adam_dev_sched_kernel<false>), dim3(grid_for(n4)), dim3(256), stream, p, g, m, v, n4, (long long)n, lr, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, wd, bias_corr_dev, grad_scale, state_dev, (float*)nullptr, (const int32_t*)nullptr, 0.f, lr_state_dev);
    return dpc_launch_status();
}

extern "C" int dpc_adam_groups_dev_sched(float* p, const float* g, float* m, float* v, int64_t n, const dpc_adam_segment* segments_dev,
                                         int32_t n_segments, double beta1, double beta2, float eps, const float* bias_corr_dev,
                                         float grad_scale, const dpc_grad_state* state_dev, float* ema, const int32_t* step_dev,
                                         float decay, const dpc_lr_state* lr_state_dev, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!p || !g || !m || !v || n <= 0 || n % 4 || !segments_dev || n_segments <= 0 || n_segments > DPC_ADAM_MAX_SEGMENTS || !bias_corr_dev)
        return DPC_ERR_ARG;
    if (!lr_state_dev || (uintptr_t)lr_state_dev % 4 || !sched_ema_ok(p, ema, step_dev, decay)) return DPC_ERR_ARG;
    if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) % 16) return DPC_ERR_ARG;
    const long long n4 = n / 4, ntiles = (n4 + ADAM_TILE4 - 1) / ADAM_TILE4;
    const unsigned grid = (unsigned)(ntiles < 2048 ? ntiles : 2048);
    if (ema)
        DPC_LAUNCH((adam_groups_sched_kernel<true>), dim3(grid), dim3(256), stream, p, g, m, v, n4, ntiles, segments_dev, (int)n_segments, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, bias_corr_dev, grad_scale, state_dev, ema, step_dev, decay, lr_state_dev);
    else
        DPC_LAUNCH((adam_groups_sched_kernel<false>), dim3(grid), dim3(256), stream, p, g, m, v, n4, ntiles, segments_dev, (int)n_segments, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), eps, bias_corr_dev, grad_scale, state_dev, (float*)nullptr, (const int32_t*)nullptr, 0.f, lr_state_dev);
    return dpc_launch_status();
}

// ---- exchange two arenas in place, 16 bytes per lane: how evaluation sees the averaged weights while every address a packed table
// or a captured graph holds stays what it is.  A bit copy (integer lanes): NaN payloads survive.
__global__ void arena_swap_kernel(u32x4* a, u32x4* b, long long n4) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
        const u32x4 x = a[i], y = b[i];
        a[i] = y; b[i] = x;
    }
}

extern "C" int dpc_arena_swap(float* a, float* b, int64_t n, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!a || !b || a == b || n <= 0 || n % 4 || (((uintptr_t)a | (uintptr_t)b) % 16)) return DPC_ERR_ARG;
    const long long n4 = n / 4;
    DPC_LAUNCH(arena_swap_kernel, dim3(grid_for(n4)), dim3(256), stream, (u32x4*)a, (u32x4*)b, n4);
    return dpc_launch_status();
}
