// loss_sym.hip -- the symmetric InfoNCE of the train step (include/dpc_hip.h: dpc_ce_topk_sym / dpc_ce_topk_bf16_sym / dpc_ce_colpass).
// loss.hip reads the [R][R] logits by rows: prediction i picks its key among the columns.  Here key j also picks its prediction among
// the rows, over the same logits:
//   loss = a mean_i Lr_i + b mean_j Lc_j,  a = 1 - W, b = W,  Lc_j = logsumexp(S[:, j]) - S[j, j]
//   dS[i, j] = (a (pr[i, j] - [i == j]) + b (pc[i, j] - [i == j])) / R,  pc[i, j] = exp(S[i, j] - lse_c[j])
// Four launches: the column pass (two), the row kernel, the finalize.  Kernels of their own: every older entry launches what it always
// launched.  The row kernels are loss.hip's bodies line for line except where marked; at W = 0 the marked lines form 1 t + 0 c = t, so
// dscore, row_ws, result and lse_out are the older entries' bits (tests/sym_cases.py holds that on every dispatcher form).
//
// Column pass: a row-major matrix reduced down its columns without a transpose.  Lanes own columns -- one 16-byte unit of a row per lane
// (8 bf16 / 4 f32 logits), so a wave reads 1 KiB of a row at a time and covers a STRIP of 512 / 256 columns; a shape without whole
// units (R or ld no multiple of the unit, a misaligned pointer) takes one column per lane and strips of 64.  A workgroup owns one strip
// and a SLAB of rows; its four waves take the slab's rows four at a time, interleaved, each keeping a running (max, sum-exp, rank) per
// owned column in registers (five exponentials per four logits).  The waves are combined through LDS in wave order, the slabs by a
// second launch in slab order: no atomics, one writer per value, a fixed order of every sum -- same inputs, same bits.
// Rows behind R and columns in [R, ld) are never read.
#include "dpc_rt.h"
#include "../../include/dpc_hip.h"

#define SYM_L2E 1.4426950408889634f
constexpr int SYM_ROWS_STEP = 16;      // rows one trip of a workgroup covers: 4 waves x 4 rows
constexpr int SYM_TARGET_WGS = 512;    // two workgroups (eight waves) per CU of the 256

template <bool FAST> __device__ __forceinline__ float sym_exp(float d) {   // e^d for d <= 0 (and d = -3e38 - x: 0)
    return FAST ? fast_exp2(d * SYM_L2E) : expf(d);
}

__device__ __forceinline__ float sym_wave_max(float v) {
    DPC_UNROLL
    for (int m = 32; m >= 1; m >>= 1) { const float o = __shfl_xor(v, m); v = o > v ? o : v; }
    return v;
}
__device__ __forceinline__ float sym_wave_sum(float v) {
    DPC_UNROLL
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- column pass
// the slab rule: enough slabs that strips x slabs reaches SYM_TARGET_WGS workgroups, slab heights a multiple of SYM_ROWS_STEP.
// R = 6 144 bf16: 12 strips x 43 slabs of 144 rows; R = 15 680: 31 strips x 17 slabs of 928 rows.  want > 0: the caller's count.
static inline int sym_units_per_lane(int dtype_s, int R, int ld, const void* score) {
    const int U = dtype_s == DPC_BF16 ? 8 : 4;
    return (R % U == 0 && ld % U == 0 && ((uintptr_t)score % 16) == 0) ? U : 1;
}
static inline int sym_slab_rows(int R, int cols_per_strip, int want) {
    const int strips = (R + cols_per_strip - 1) / cols_per_strip;
    int slabs = want > 0 ? want : (SYM_TARGET_WGS + strips - 1) / strips;
    const int most = (R + SYM_ROWS_STEP - 1) / SYM_ROWS_STEP;
    if (slabs > most) slabs = most;
    if (slabs < 1) slabs = 1;
    const int per = (R + slabs - 1) / slabs;
    return (per + SYM_ROWS_STEP - 1) / SYM_ROWS_STEP * SYM_ROWS_STEP;
}

template <class T, int E> __device__ __forceinline__ void sym_load(const T* p, float (&x)[E]) {
    if constexpr (E == 1) {
        x[0] = Elt<T>::to_f32(p[0]);
    } else {
        const u32x4 u = *(const u32x4*)p;
        DPC_UNROLL
        for (int e = 0; e < E; ++e) x[e] = unit_get<T>(u, e);
    }
}

// part[slab][3][R]: planes of max, sum-exp and rank
template <class T, int E, bool FAST>
__global__ __launch_bounds__(256) void col_part_kernel(const T* s, int R, int ld, int rps, float* part) {
    __shared__ float sh[3][3 * E][64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int c0 = (blockIdx.x * 64 + lane) * E;      // first owned column; with E > 1 the unit is whole or absent (R % E == 0)
    const bool own = c0 < R;
    const int r0 = blockIdx.y * rps;
    const int r1 = r0 + rps < R ? r0 + rps : R;
    float m[E], l[E], rk[E], dg[E];
    DPC_UNROLL
    for (int e = 0; e < E; ++e) {
        m[e] = -3.0e38f; l[e] = 0.f; rk[e] = 0.f;
        dg[e] = own ? Elt<T>::to_f32(s[(long long)(c0 + e) * ld + c0 + e]) : 0.f;   // the column's target: row c0 + e < R
    }
    if (own) {
        const T* base = s + c0;
        for (int r = r0 + 4 * wv; r < r1; r += SYM_ROWS_STEP) {
            if (r + 4 <= r1) {
                float x[4][E];
                DPC_UNROLL
                for (int k = 0; k < 4; ++k) sym_load<T, E>(base + (long long)(r + k) * ld, x[k]);
                DPC_UNROLL
                for (int e = 0; e < E; ++e) {
                    float mn = m[e];
                    DPC_UNROLL
                    for (int k = 0; k < 4; ++k) mn = x[k][e] > mn ? x[k][e] : mn;
                    float acc = l[e] * sym_exp<FAST>(m[e] - mn);
                    DPC_UNROLL
                    for (int k = 0; k < 4; ++k) {
                        acc += sym_exp<FAST>(x[k][e] - mn);
                        rk[e] += x[k][e] > dg[e] ? 1.f : 0.f;
                    }
                    l[e] = acc; m[e] = mn;
                }
            } else {
                for (int rr = r; rr < r1; ++rr) {
                    float x[E];
                    sym_load<T, E>(base + (long long)rr * ld, x);
                    DPC_UNROLL
                    for (int e = 0; e < E; ++e) {
                        const float mn = x[e] > m[e] ? x[e] : m[e];
                        l[e] = l[e] * sym_exp<FAST>(m[e] - mn) + sym_exp<FAST>(x[e] - mn);
                        m[e] = mn;
                        rk[e] += x[e] > dg[e] ? 1.f : 0.f;
                    }
                }
            }
        }
    }
    if (wv) {
        DPC_UNROLL
        for (int e = 0; e < E; ++e) { sh[wv - 1][e][lane] = m[e]; sh[wv - 1][E + e][lane] = l[e]; sh[wv - 1][2 * E + e][lane] = rk[e]; }
    }
    __syncthreads();
    if (wv == 0 && own) {
        float* o = part + (long long)blockIdx.y * 3 * R + c0;
        DPC_UNROLL
        for (int e = 0; e < E; ++e) {
            DPC_UNROLL
            for (int w = 0; w < 3; ++w) {   // wave order; a wave without rows holds (-3e38, 0, 0) and changes nothing
                const float m2 = sh[w][e][lane], l2 = sh[w][E + e][lane];
                const float mn = m2 > m[e] ? m2 : m[e];
                l[e] = l[e] * sym_exp<FAST>(m[e] - mn) + l2 * sym_exp<FAST>(m2 - mn);
                m[e] = mn;
                rk[e] += sh[w][2 * E + e][lane];
            }
            o[e] = m[e]; o[(long long)R + e] = l[e]; o[2 * (long long)R + e] = rk[e];
        }
    }
}

// one thread per column: the slabs in slab order; col_lse[j] = lse_c[j], col_ws[j] = (lse_c[j] - S[j][j], rank_c[j])
template <class T, bool FAST>
__global__ __launch_bounds__(256) void col_merge_kernel(const float* part, const T* s, int R, int ld, int slabs, float* col_lse, float* col_ws) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= R) return;
    float m = part[j], l = part[(long long)R + j], rk = part[2 * (long long)R + j];
    for (int b = 1; b < slabs; ++b) {
        const float* p = part + (long long)b * 3 * R + j;
        const float m2 = p[0], l2 = p[R];
        const float mn = m2 > m ? m2 : m;
        l = l * sym_exp<FAST>(m - mn) + l2 * sym_exp<FAST>(m2 - mn);
        m = mn;
        rk += p[2 * (long long)R];
    }
    const float lse = logf(l) + m;
    col_lse[j] = lse;
    col_ws[2 * j] = lse - Elt<T>::to_f32(s[(long long)j * ld + j]);
    col_ws[2 * j + 1] = rk;
}

template <class T, bool FAST>
static void col_pass_launch(const T* s, int R, int ld, int want, float* col_lse, float* col_ws, float* ws, hipStream_t stream) {
    constexpr int U = Elt<T>::PER16;
    const int E = sym_units_per_lane(sizeof(T) == 2 ? DPC_BF16 : DPC_F32, R, ld, s);
    const int rps = sym_slab_rows(R, 64 * E, want);
    const int slabs = (R + rps - 1) / rps, strips = (R + 64 * E - 1) / (64 * E);
    if (E == 1) {
        DPC_LAUNCH((col_part_kernel<T, 1, FAST>), dim3(strips, slabs), dim3(256), stream, s, R, ld, rps, ws);
    } else {
        DPC_LAUNCH((col_part_kernel<T, U, FAST>), dim3(strips, slabs), dim3(256), stream, s, R, ld, rps, ws);
    }
    DPC_LAUNCH((col_merge_kernel<T, FAST>), dim3((R + 255) / 256), dim3(256), stream, (const float*)ws, s, R, ld, slabs, col_lse, col_ws);
}

static void col_pass(const void* s, int dtype_s, bool fast, int R, int ld, int want, float* col_lse, float* col_ws, float* ws, hipStream_t stream) {
    if (dtype_s == DPC_BF16) {
        if (fast) col_pass_launch<bf16_t, true>((const bf16_t*)s, R, ld, want, col_lse, col_ws, ws, stream);
        else col_pass_launch<bf16_t, false>((const bf16_t*)s, R, ld, want, col_lse, col_ws, ws, stream);
    } else {
        if (fast) col_pass_launch<float, true>((const float*)s, R, ld, want, col_lse, col_ws, ws, stream);
        else col_pass_launch<float, false>((const float*)s, R, ld, want, col_lse, col_ws, ws, stream);
    }
}

// the largest workspace any layout of an [R][.] matrix of either dtype needs: slabs x 3 x R floats, the scalar form's strips of 64
extern "C" int dpc_ce_sym_ws_floats(int32_t R, int32_t slabs, int64_t* floats) {
    if (R <= 0 || slabs < 0 || !floats) return DPC_ERR_ARG;
    int most = 0;
    for (int E : {1, 4, 8}) {
        const int rps = sym_slab_rows(R, 64 * E, slabs);
        const int n = (R + rps - 1) / rps;
        most = n > most ? n : most;
    }
    *floats = (int64_t)most * 3 * R;
    return most;
}

extern "C" int dpc_ce_colpass(const void* score, int32_t dtype_s, int32_t R, int32_t ld, int32_t fast, int32_t slabs, float* col_lse,
                              float* col_ws, float* ws, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!score || !col_lse || !col_ws || !ws || R <= 0 || ld < R || slabs < 0 || (dtype_s != DPC_F32 && dtype_s != DPC_BF16)) return DPC_ERR_ARG;
    if (fast != 0 && fast != 1) return DPC_ERR_ARG;
    col_pass(score, dtype_s, fast != 0, R, ld, slabs, col_lse, col_ws, ws, stream);
    return dpc_launch_status();
}

// ---------------------------------------------------------------------------------------------------------------- row kernels
// ce_row_body of loss.hip; SYM marks the lines that differ
template <class TD, bool EXT>
__global__ __launch_bounds__(256) void ce_row_sym_kernel(const float* score, int rows, int cols, int ld, float* row_ws, TD* dscore, int ld_d,
                                                         const float* qstats, float* lse_out, const float* col_lse, float a, float b, float lshift) {
    __shared__ float sh[8];
    const int row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* s = score + (long long)row * ld;
    const float tgt = s[row];
    float mx = -3.0e38f;
    for (int j = tid; j < cols; j += 256) { const float v = s[j]; mx = v > mx ? v : mx; }
    mx = sym_wave_max(mx);
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
    se = sym_wave_sum(se);
    rk = sym_wave_sum(rk);
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
        if constexpr (EXT) lse_out[row] = logf(se) + mx - lshift;   // SYM: lse - log a, so that dpc_negq_bwd yields a x the share
    }
    if (dscore) {
        const float inv = 1.f / se, invr = 1.f / (float)rows;
        TD* d = dscore + (long long)row * ld_d;
        for (int j = tid; j < cols; j += 256) {
            const float x = s[j];
            float g = expf(x - mx) * inv;
            float c = expf(x - col_lse[j]);                      // SYM: from the logit itself, never ex * exp(mx - lse_c)
            if (j == row) { g -= 1.f; c -= 1.f; }
            d[j] = Elt<TD>::from_f32((a * g + b * c) * invr);   // SYM
        }
        for (int j = cols + tid; j < ld_d; j += 256) d[j] = Elt<TD>::from_f32(0.f);
    }
}

// ce_row_vec_body: the row's exponentials stay in registers; the gradient loop reads the unit of logits again (it was read a moment
// ago) beside the unit of col_lse
template <class TD, int NV, bool FAST, bool EXT>
__global__ __launch_bounds__(256) void ce_row_vec_sym_kernel(const float* score, int rows, int cols, int ld, float* row_ws, TD* dscore, int ld_d,
                                                             const float* qstats, float* lse_out, const float* col_lse, float a, float b, float lshift) {
    __shared__ float sh[8];
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
    mx = sym_wave_max(mx);
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
    const float nm = -mx * SYM_L2E;
    DPC_UNROLL
    for (int i = 0; i < NV; ++i) {
        const bool ok = tid + 256 * i < nq;
        DPC_UNROLL
        for (int e = 0; e < 4; ++e) {
            const float x = v[i][e];
            rk += (ok && x > tgt) ? 1.f : 0.f;
            const float ex = FAST ? fast_exp2(fmaf(x, SYM_L2E, nm)) : expf(x - mx);
            v[i][e] = ok ? ex : 0.f;
            se += v[i][e];
        }
    }
    se = sym_wave_sum(se);
    rk = sym_wave_sum(rk);
    __syncthreads();
    if (lane == 0) { sh[wv] = se; sh[4 + wv] = rk; }
    __syncthreads();
    se = sh[0] + sh[1] + sh[2] + sh[3];
    rk = sh[4] + sh[5] + sh[6] + sh[7];
    if constexpr (EXT) {
        se += lq * (FAST ? fast_exp2((mq - mx) * SYM_L2E) : expf(mq - mx));
        rk += rkq;
    }
    if (tid == 0) {
        row_ws[2 * row + 0] = logf(se) + mx - tgt;
        row_ws[2 * row + 1] = rk;
        if constexpr (EXT) lse_out[row] = logf(se) + mx - lshift;   // SYM: lse - log a, so that dpc_negq_bwd yields a x the share
    }
    if (dscore) {
        const float inv = 1.f / se, invr = 1.f / (float)rows;
        TD* d = dscore + (long long)row * ld_d;
        DPC_UNROLL
        for (int i = 0; i < NV; ++i) {
            const int q = tid + 256 * i;
            if (q < nq) {
                const f32x4 x = ((const f32x4*)s)[q], cl = ((const f32x4*)col_lse)[q];   // SYM
                float g[4];
                DPC_UNROLL
                for (int e = 0; e < 4; ++e) {
                    float t = v[i][e] * inv;
                    float c = sym_exp<FAST>(x[e] - cl[e]);       // SYM
                    if (4 * q + e == row) { t -= 1.f; c -= 1.f; }
                    g[e] = (a * t + b * c) * invr;               // SYM
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

// ce_row_vec16_body: the packed 16-byte units are kept beside the exponentials (4 registers each) and unpacked again for the column term
template <int NV, bool EXT>
__global__ __launch_bounds__(256) void ce_row_vec16_sym_kernel(const bf16_t* score, int rows, int cols, int ld, float* row_ws, bf16_t* dscore,
                                                               int ld_d, const float* qstats, float* lse_out, const float* col_lse, float a,
                                                               float b, float lshift) {
    __shared__ float sh[8];
    const int row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bf16_t* s = score + (long long)row * ld;
    const float tgt = bf16_to_f32(s[row]);
    const int nq = cols >> 3;
    float v[NV][8];
    u32x4 raw[NV];                                               // SYM
    float mx = -3.0e38f;
    DPC_UNROLL
    for (int i = 0; i < NV; ++i) {
        const int q = tid + 256 * i;
        if (q < nq) {
            const u32x4 t = ((const u32x4*)s)[q];
            raw[i] = t;
            DPC_UNROLL
            for (int e = 0; e < 8; ++e) { v[i][e] = unit_get<bf16_t>(t, e); mx = v[i][e] > mx ? v[i][e] : mx; }
        } else {
            const u32x4 z = {0u, 0u, 0u, 0u};
            raw[i] = z;
            DPC_UNROLL
            for (int e = 0; e < 8; ++e) v[i][e] = -3.0e38f;
        }
    }
    mx = sym_wave_max(mx);
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
    const float nm = -mx * SYM_L2E;
    DPC_UNROLL
    for (int i = 0; i < NV; ++i) {
        const bool ok = tid + 256 * i < nq;
        DPC_UNROLL
        for (int e = 0; e < 8; ++e) {
            const float x = v[i][e];
            rk += (ok && x > tgt) ? 1.f : 0.f;
            const float ex = fast_exp2(fmaf(x, SYM_L2E, nm));
            v[i][e] = ok ? ex : 0.f;
            se += v[i][e];
        }
    }
    se = sym_wave_sum(se);
    rk = sym_wave_sum(rk);
    __syncthreads();
    if (lane == 0) { sh[wv] = se; sh[4 + wv] = rk; }
    __syncthreads();
    se = sh[0] + sh[1] + sh[2] + sh[3];
    rk = sh[4] + sh[5] + sh[6] + sh[7];
    if constexpr (EXT) {
        se += lq * fast_exp2((mq - mx) * SYM_L2E);
        rk += rkq;
    }
    if (tid == 0) {
        row_ws[2 * row + 0] = logf(se) + mx - tgt;
        row_ws[2 * row + 1] = rk;
        if constexpr (EXT) lse_out[row] = logf(se) + mx - lshift;   // SYM: lse - log a, so that dpc_negq_bwd yields a x the share
    }
    if (dscore) {
        const float inv = 1.f / se, invr = 1.f / (float)rows;
        bf16_t* d = dscore + (long long)row * ld_d;
        DPC_UNROLL
        for (int i = 0; i < NV; ++i) {
            const int q = tid + 256 * i;
            if (q < nq) {
                const f32x4 cl0 = ((const f32x4*)col_lse)[2 * q], cl1 = ((const f32x4*)col_lse)[2 * q + 1];   // SYM
                float g[8];
                DPC_UNROLL
                for (int e = 0; e < 8; ++e) {
                    float t = v[i][e] * inv;
                    float c = sym_exp<true>(unit_get<bf16_t>(raw[i], e) - (e < 4 ? cl0[e & 3] : cl1[e & 3]));   // SYM
                    if (8 * q + e == row) { t -= 1.f; c -= 1.f; }
                    g[e] = (a * t + b * c) * invr;                                                              // SYM
                }
                *(u32x4*)(d + 8 * q) = unit_pack<bf16_t>(g);
            }
        }
        for (int j = cols + tid; j < ld_d; j += 256) d[j] = Elt<bf16_t>::from_f32(0.f);
    }
}

// ce_finalize_kernel over the rows (the same order of sums: the same bits) and again over the columns;
// result = (a Lr + b Lc, row top-1/3/5), sym_result = (Lr, Lc, column top-1/3/5, 0, 0, 0)
__global__ __launch_bounds__(256) void ce_finalize_sym_kernel(const float* row_ws, const float* col_ws, int rows, float a, float b, float* result,
                                                              float* sym_result) {
    __shared__ float sh[2][4][4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    DPC_UNROLL
    for (int side = 0; side < 2; ++side) {
        const float* ws = side ? col_ws : row_ws;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int r = tid; r < rows; r += 256) {
            const float rk = ws[2 * r + 1];
            acc[0] += ws[2 * r];
            acc[1] += rk < 1.f ? 1.f : 0.f;
            acc[2] += rk < 3.f ? 1.f : 0.f;
            acc[3] += rk < 5.f ? 1.f : 0.f;
        }
        DPC_UNROLL
        for (int k = 0; k < 4; ++k) {
            acc[k] = sym_wave_sum(acc[k]);
            if (lane == 0) sh[side][wv][k] = acc[k];
        }
    }
    __syncthreads();
    if (tid < 4) {
        const float r = (sh[0][0][tid] + sh[0][1][tid] + sh[0][2][tid] + sh[0][3][tid]) / (float)rows;
        const float c = (sh[1][0][tid] + sh[1][1][tid] + sh[1][2][tid] + sh[1][3][tid]) / (float)rows;
        result[tid] = tid == 0 ? a * r + b * c : r;
        if (tid == 0) { sym_result[0] = r; sym_result[1] = c; }
        else { sym_result[1 + tid] = c; sym_result[4 + tid] = 0.f; }
    }
}

// ---------------------------------------------------------------------------------------------------------------- entries
static bool sym_args_ok(const void* score, int rows, int cols, int ld, const float* row_ws, const float* result, const void* dscore, int ld_d,
                        const float* qstats, const float* lse_out, float w, int slabs, const float* col_lse, const float* col_ws, const float* ws,
                        const float* sym_result) {
    if (!score || !row_ws || !result || rows <= 0 || cols != rows || ld < cols) return false;
    if (dscore && ld_d < cols) return false;
    if ((qstats == nullptr) != (lse_out == nullptr)) return false;
    if (!(w >= 0.f && w <= 1.f)) return false;   // NaN fails both comparisons
    if (!col_lse || !col_ws || !ws || !sym_result || slabs < 0 || ((uintptr_t)col_lse % 16)) return false;
    return true;
}

#define SYM_ROW_ARGS score, rows, cols, ld, row_ws, (TDP)dscore, ld_d, qstats, lse_out, (const float*)col_lse, a, b, lshift
extern "C" int dpc_ce_topk_sym(const float* score, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result, void* dscore,
                               int32_t dtype_d, int32_t ld_d, const float* qstats, float* lse_out, float w, int32_t slabs, float* col_lse,
                               float* col_ws, float* ws, float* sym_result, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!sym_args_ok(score, rows, cols, ld, row_ws, result, dscore, ld_d, qstats, lse_out, w, slabs, col_lse, col_ws, ws, sym_result)) return DPC_ERR_ARG;
    if (dscore && dtype_d != DPC_F32 && dtype_d != DPC_BF16) return DPC_ERR_ARG;
    const float a = 1.f - w, b = w;
    const float lshift = a > 0.f ? logf(a) : -1.0e38f;   // (a = 0: lse_out = 1e38, every share of the bank 0)
    const bool vec = cols % 4 == 0 && ld % 4 == 0 && ((uintptr_t)score % 16) == 0 && cols <= 16384 &&
                     (!dscore || (ld_d % 4 == 0 && ((uintptr_t)dscore % 16) == 0));
    const bool f32d = !dscore || dtype_d == DPC_F32;
    const bool ext = qstats != nullptr;
    col_pass(score, DPC_F32, vec && !f32d, rows, ld, slabs, col_lse, col_ws, ws, stream);   // fast_exp2 where the row kernel uses it
    if (f32d) {
        typedef float* TDP;
        if (vec && cols <= 8192) {
            if (ext) DPC_LAUNCH((ce_row_vec_sym_kernel<float, 8, false, true>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
            else DPC_LAUNCH((ce_row_vec_sym_kernel<float, 8, false, false>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
        } else if (vec) {
            if (ext) DPC_LAUNCH((ce_row_vec_sym_kernel<float, 16, false, true>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
            else DPC_LAUNCH((ce_row_vec_sym_kernel<float, 16, false, false>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
        } else {
            if (ext) DPC_LAUNCH((ce_row_sym_kernel<float, true>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
            else DPC_LAUNCH((ce_row_sym_kernel<float, false>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
        }
    } else {
        typedef bf16_t* TDP;
        if (vec && cols <= 8192) {
            if (ext) DPC_LAUNCH((ce_row_vec_sym_kernel<bf16_t, 8, true, true>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
            else DPC_LAUNCH((ce_row_vec_sym_kernel<bf16_t, 8, true, false>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
        } else if (vec) {
            if (ext) DPC_LAUNCH((ce_row_vec_sym_kernel<bf16_t, 16, true, true>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
            else DPC_LAUNCH((ce_row_vec_sym_kernel<bf16_t, 16, true, false>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
        } else {
            if (ext) DPC_LAUNCH((ce_row_sym_kernel<bf16_t, true>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
            else DPC_LAUNCH((ce_row_sym_kernel<bf16_t, false>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
        }
    }
    DPC_LAUNCH(ce_finalize_sym_kernel, dim3(1), dim3(256), stream, (const float*)row_ws, (const float*)col_ws, rows, a, b, result, sym_result);
    return dpc_launch_status();
}

extern "C" int dpc_ce_topk_bf16_sym(const void* score_, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result, void* dscore,
                                    int32_t ld_d, const float* qstats, float* lse_out, float w, int32_t slabs, float* col_lse, float* col_ws,
                                    float* ws, float* sym_result, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!sym_args_ok(score_, rows, cols, ld, row_ws, result, dscore, ld_d, qstats, lse_out, w, slabs, col_lse, col_ws, ws, sym_result)) return DPC_ERR_ARG;
    if (cols % 8 || ld % 8 || ((uintptr_t)score_ % 16) || cols > 16384 || (dscore && (ld_d % 8 || ((uintptr_t)dscore % 16)))) return DPC_ERR_UNSUPPORTED;
    const bf16_t* score = (const bf16_t*)score_;
    const float a = 1.f - w, b = w;
    const float lshift = a > 0.f ? logf(a) : -1.0e38f;   // (a = 0: lse_out = 1e38, every share of the bank 0)
    const bool ext = qstats != nullptr;
    typedef bf16_t* TDP;
    col_pass(score, DPC_BF16, true, rows, ld, slabs, col_lse, col_ws, ws, stream);
    if (cols <= 2048 * 4) {
        if (ext) DPC_LAUNCH((ce_row_vec16_sym_kernel<4, true>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
        else DPC_LAUNCH((ce_row_vec16_sym_kernel<4, false>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
    } else {
        if (ext) DPC_LAUNCH((ce_row_vec16_sym_kernel<8, true>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
        else DPC_LAUNCH((ce_row_vec16_sym_kernel<8, false>), dim3(rows), dim3(256), stream, SYM_ROW_ARGS);
    }
    DPC_LAUNCH(ce_finalize_sym_kernel, dim3(1), dim3(256), stream, (const float*)row_ws, (const float*)col_ws, rows, a, b, result, sym_result);
    return dpc_launch_status();
}
