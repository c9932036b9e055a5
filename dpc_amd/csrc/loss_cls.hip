// loss_cls.hip -- the row kernels of loss.hip with the negative CLASSES of dpc/model_3d.py:86-96 inside the softmax (dpc_ce_topk_cls /
// dpc_ce_topk_bf16_cls, include/dpc_hip.h).  Row r = (b, p, s), column c = (b2, n, s2), W = P SQ:
//   easy      b != b2                 every column outside the row's window [w0, w0 + W), w0 = (r / W) W, and every live bank key
//   spatial   b == b2, s != s2        inside the window, (c - w0) % SQ != (r - w0) % SQ
//   temporal  b == b2, s == s2, n != p
//   positive  c == r                  weight 1
// dpc_mask_gen's values (0 / -3 / -1 / 1) as a closed form of (r, c): no mask tensor is read.  Z = sum_c w_class e^(s_c), the loss
// term is log Z - s_rr, dS = (w e^s / Z - [c == r]) / rows; the rank stays the unweighted count over all columns.
// The bodies are ce_row_body / ce_row_vec_body / ce_row_vec16_body of loss.hip with one change per element: the STORED exponential is
// the exponential times its weight (a zero weight stores 0 without forming the product: the exponential may be inf), summed in the
// old per-thread order, so weights (1, 1, 1) give the older entries' bits.  THE TWO FILES MOVE TOGETHER: the bodies are copies (the
// class arm inside loss.hip's templates cost its siblings registers), tied to their siblings only by the (1, 1, 1) bit-identity cases
// of tests/negcls_cases.py -- a change to a body, to wave_max / wave_sum or to the dispatch conditions there is made here as well.
// A 16-byte unit wholly outside the window is easy as a unit.  The test is taken per WAVE STEP (a ballot over the 64 consecutive units,
// 256 or 512 columns, a wave holds at one register index): a step with no unit in the window multiplies by w_E and nothing else; a step
// with one classifies the elements of all its 64 units (those outside the window come out easy) -- at most ceil(W / (64 U)) + 1 of a row's
// cols / (64 U) steps, behind a wave-uniform branch.
// The report costs the rows that ask for it a second look at their own window, behind the gradient, when the row's registers are free
// again (report_pass): the W logits come back from L2, their stored exponentials are formed once more (the same expression, the same
// bits) and summed per class with the strictly-above counts.  The easy class is what is left of the row's totals, the positive's mass is
// the target's own exponential.  Without report_rows the pass does not exist.
#include "dpc_rt.h"
#include "../../include/dpc_hip.h"

namespace {

struct ClsP {
    int W, SQ;            // window width P SQ, positions per step
    FastDiv dSQ, dW;      // exact x / SQ and x / W for 0 <= x < 2^31 in a multiply and a shift: no division in the kernel
    float wS, wT, wE;
    float log_wE;         // logf(w_E), formed on the host: 0 at w_E = 1
    int allpos;           // every weight > 0: the running maximum covers every column, as in the older kernels
};

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

// the row's geometry, once per row
struct RowG {
    int row, w0, w1, srow;
};
__device__ __forceinline__ RowG row_geom(int row, const ClsP& c) {
    RowG g;
    g.row = row;
    g.w0 = (int)fdiv((uint32_t)row, c.dW) * c.W;
    g.w1 = g.w0 + c.W;
    const uint32_t o = (uint32_t)(row - g.w0);
    g.srow = (int)(o - fdiv(o, c.dSQ) * (uint32_t)c.SQ);
    return g;
}
// 0 easy, 1 spatial, 2 temporal, 3 positive
__device__ __forceinline__ int cls_kind(int col, const RowG& g, const ClsP& c) {
    const unsigned o = (unsigned)(col - g.w0);
    if (o >= (unsigned)c.W) return 0;
    if (col == g.row) return 3;
    return (int)(o - fdiv(o, c.dSQ) * (unsigned)c.SQ) == g.srow ? 2 : 1;
}
__device__ __forceinline__ float cls_weight(int kind, const ClsP& c) {
    return kind == 0 ? c.wE : kind == 1 ? c.wS : kind == 2 ? c.wT : 1.f;
}

// the form's exponential of x - mx: libm's (the f32 parity mode), or one v_exp_f32 (FAST), as in loss.hip
template <bool FAST>
struct ExpForm {
    float mx, nm;
    __device__ __forceinline__ explicit ExpForm(float m) : mx(m), nm(-m * 1.4426950408889634f) {}
    __device__ __forceinline__ float operator()(float x) const { return FAST ? fast_exp2(fmaf(x, 1.4426950408889634f, nm)) : expf(x - mx); }
};

// the sums of a row over its 256 threads, in the older kernels' order.  sh: 32 floats, [0, 8) used here
struct RowAcc {
    float se, rk;
};
__device__ __forceinline__ void reduce_row(float* sh, RowAcc& a, int lane, int wv) {
    a.se = wave_sum(a.se);
    a.rk = wave_sum(a.rk);
    __syncthreads();
    if (lane == 0) { sh[wv] = a.se; sh[4 + wv] = a.rk; }
    __syncthreads();
    a.se = sh[0] + sh[1] + sh[2] + sh[3];
    a.rk = sh[4] + sh[5] + sh[6] + sh[7];
}

// thread 0: a.se / a.rk are the in-batch totals, se / rk the row's (the bank's w_E l_q exp(m_q - mx) and rk_q added, in the older
// kernels' form).  What the report needs later is parked in sh[24, 30): no register carries it across the gradient.
__device__ __forceinline__ void write_row(float* sh, int row, const RowAcc& a, float se, float rk, float rkq, float mx, float tgt, const ClsP& c,
                                          bool bank, float* row_ws, float* lse_out, bool report) {
    row_ws[2 * row + 0] = logf(se) + mx - tgt;
    row_ws[2 * row + 1] = rk;
    if (bank) lse_out[row] = logf(se) + mx - c.log_wE;   // dpc_negq_bwd's exp(s - lse) / R is then w_E e^s / (Z R)
    if (report) { sh[24] = a.se; sh[25] = a.rk; sh[26] = se; sh[27] = rkq; sh[28] = mx; sh[29] = tgt; }
}

// the report of one row (all 256 threads, report_rows != NULL): the row's window once more, element by element
template <bool FAST, class TS>
__device__ __forceinline__ void report_pass(float* sh, const TS* s, const RowG& g, const ClsP& c, float* report_rows) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    __syncthreads();                     // thread 0's sh[24, 30) (write_row)
    const ExpForm<FAST> expf_(sh[28]);
    const float tgt = sh[29];
    float seS = 0.f, seT = 0.f, cS = 0.f, cT = 0.f;
    for (int j = g.w0 + tid; j < g.w1; j += 256) {
        const float v = Elt<TS>::to_f32(s[j]);
        const int kind = cls_kind(j, g, c);
        const float w = cls_weight(kind, c);
        const float wex = w > 0.f ? expf_(v) * w : 0.f;
        const float gt = (v > tgt) ? 1.f : 0.f;
        if (kind == 1) { seS += wex; cS += gt; }
        if (kind == 2) { seT += wex; cT += gt; }
    }
    seS = wave_sum(seS);
    seT = wave_sum(seT);
    cS = wave_sum(cS);
    cT = wave_sum(cT);
    if (lane == 0) { sh[8 + wv] = seS; sh[12 + wv] = seT; sh[16 + wv] = cS; sh[20 + wv] = cT; }
    __syncthreads();
    if (tid == 0) {
        seS = sh[8] + sh[9] + sh[10] + sh[11];
        seT = sh[12] + sh[13] + sh[14] + sh[15];
        cS = sh[16] + sh[17] + sh[18] + sh[19];
        cT = sh[20] + sh[21] + sh[22] + sh[23];
        const float se_in = sh[24], rk_in = sh[25], se = sh[26], rkq = sh[27];
        const float epos = expf_(tgt);
        const float inv = 1.f / se;
        float eE = se_in - seS - seT - epos;               // the in-batch easy columns: what is left of the in-batch sum
        eE = eE > 0.f ? eE : 0.f;
        float* o = report_rows + 8 * (long long)g.row;
        o[0] = epos * inv;
        o[1] = seS * inv;
        o[2] = seT * inv;
        o[3] = (eE + (se - se_in)) * inv;                  // ... plus the bank's share of the row's sum
        o[4] = cS;
        o[5] = cT;
        o[6] = (rk_in - cS - cT) + rkq;
        o[7] = 0.f;
    }
}

// The running maximum covers the columns of positive weight.  With every weight positive that is every column, taken while the row is
// loaded, as in the older kernels.  With a zero weight the row is swept once more for it (L2-resident, just read), element by element:
// classifying the elements beside the load loop as well would keep every element's weight in a register between the two loops.
template <class TS>
__device__ __forceinline__ float max_positive(const TS* s, int cols, int tid, const RowG& g, const ClsP& c) {
    float mx = -3.0e38f;
    for (int j = tid; j < cols; j += 256) {
        const float v = Elt<TS>::to_f32(s[j]);
        if (cls_weight(cls_kind(j, g, c), c) > 0.f) mx = v > mx ? v : mx;
    }
    return mx;
}

// ---- ce_row_body: three sweeps, any layout
template <class TD>
__global__ __launch_bounds__(256) void ce_row_cls_kernel(const float* score, int rows, int cols, int ld, float* row_ws, TD* dscore, int ld_d,
                                                         const float* qstats, float* lse_out, ClsP c, float* report_rows) {
    __shared__ float sh[32];
    const int row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* s = score + (long long)row * ld;
    const float tgt = s[row];
    const RowG g = row_geom(row, c);
    float mx = -3.0e38f;
    if (c.allpos) {
        for (int j = tid; j < cols; j += 256) { const float v = s[j]; mx = v > mx ? v : mx; }
    } else {
        mx = max_positive(s, cols, tid, g, c);
    }
    mx = wave_max(mx);
    if (lane == 0) sh[wv] = mx;
    __syncthreads();
    mx = sh[0];
    DPC_UNROLL
    for (int w = 1; w < 4; ++w) mx = sh[w] > mx ? sh[w] : mx;
    float mq = 0.f, lq = 0.f, rkq = 0.f;
    if (qstats) {
        mq = qstats[4 * (long long)row]; lq = qstats[4 * (long long)row + 1]; rkq = qstats[4 * (long long)row + 2];
        mx = mq > mx ? mq : mx;
    }
    RowAcc a = {0.f, 0.f};
    for (int j = tid; j < cols; j += 256) {
        const float v = s[j];
        const float w = cls_weight(cls_kind(j, g, c), c);
        a.se += w > 0.f ? expf(v - mx) * w : 0.f;
        a.rk += (v > tgt) ? 1.f : 0.f;
    }
    reduce_row(sh, a, lane, wv);
    float se = a.se, rk = a.rk;
    if (qstats) {
        const float lqw = lq * c.wE;
        se += lqw * expf(mq - mx);
        rk += rkq;
    }
    if (tid == 0) write_row(sh, row, a, se, rk, rkq, mx, tgt, c, qstats != nullptr, row_ws, lse_out, report_rows != nullptr);
    if (dscore) {
        const float inv = 1.f / se, invr = 1.f / (float)rows;
        TD* d = dscore + (long long)row * ld_d;
        for (int j = tid; j < cols; j += 256) {
            const float w = cls_weight(cls_kind(j, g, c), c);
            const float wex = w > 0.f ? expf(s[j] - mx) * w : 0.f;
            float gr = wex * inv;
            if (j == row) gr -= 1.f;
            d[j] = Elt<TD>::from_f32(gr * invr);
        }
        for (int j = cols + tid; j < ld_d; j += 256) d[j] = Elt<TD>::from_f32(0.f);
    }
    if (report_rows) report_pass<false>(sh, s, g, c, report_rows);
}

// one 16-byte unit of U logits held in x[U] (x[e] of a unit behind the row's end: the fill, ok = false): rank, the stored weighted
// exponentials (in place), the two sums.  EXPF(x) is the form's exponential of x - mx.
template <int U, class EXPF>
__device__ __forceinline__ void unit_exp(float* x, int c0, bool ok, float tgt, const RowG& g, const ClsP& c, RowAcc& a, EXPF expf_) {
    // easy as a unit (a unit behind the row's end is behind every window) -- decided per WAVE: the 64 units of a wave step are 64 U
    // consecutive columns, and the step classifies its elements only when one of them touches the window.  A wave-uniform branch: no
    // lane keeps a second copy of the row's registers across it.
    if (wave_ballot(!(c0 + U <= g.w0 || c0 >= g.w1)) == 0) {
        if (c.wE > 0.f) {   // kernel-uniform
            DPC_UNROLL
            for (int e = 0; e < U; ++e) {
                const float v = x[e];
                a.rk += (ok && v > tgt) ? 1.f : 0.f;
                const float wex = expf_(v) * c.wE;
                x[e] = ok ? wex : 0.f;
                a.se += x[e];
            }
        } else {            // the easy class is out of the loss: nothing is formed that could be inf
            DPC_UNROLL
            for (int e = 0; e < U; ++e) {
                a.rk += (ok && x[e] > tgt) ? 1.f : 0.f;
                x[e] = 0.f;
                a.se += x[e];
            }
        }
    } else {
        DPC_UNROLL
        for (int e = 0; e < U; ++e) {
            const float v = x[e];
            const float w = cls_weight(cls_kind(c0 + e, g, c), c);
            a.rk += (ok && v > tgt) ? 1.f : 0.f;
            const float wex = w > 0.f ? expf_(v) * w : 0.f;
            x[e] = ok ? wex : 0.f;
            a.se += x[e];
            sched_fence();   // one element at a time: the few units on this path do not set the kernel's register count
        }
    }
}
// ---- ce_row_vec_body: the row in registers, f32 logits, NV float4 per thread
template <class TD, int NV, bool FAST>
__global__ __launch_bounds__(256) void ce_row_vec_cls_kernel(const float* score, int rows, int cols, int ld, float* row_ws, TD* dscore, int ld_d,
                                                             const float* qstats, float* lse_out, ClsP c, float* report_rows) {
    __shared__ float sh[32];
    const int row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float* s = score + (long long)row * ld;
    const float tgt = s[row];
    const RowG g = row_geom(row, c);
    const int nq = cols >> 2;
    float v[NV][4];
    float mx = -3.0e38f;
    DPC_UNROLL
    for (int i = 0; i < NV; ++i) {
        const int q = tid + 256 * i;
        f32x4 t = {-3.0e38f, -3.0e38f, -3.0e38f, -3.0e38f};
        if (q < nq) t = ((const f32x4*)s)[q];
        DPC_UNROLL
        for (int e = 0; e < 4; ++e) { v[i][e] = t[e]; mx = t[e] > mx ? t[e] : mx; }
    }
    if (!c.allpos) mx = max_positive(s, cols, tid, g, c);
    mx = wave_max(mx);
    if (lane == 0) sh[wv] = mx;
    __syncthreads();
    mx = sh[0];
    DPC_UNROLL
    for (int w = 1; w < 4; ++w) mx = sh[w] > mx ? sh[w] : mx;
    float mq = 0.f, lq = 0.f, rkq = 0.f;
    if (qstats) {
        mq = qstats[4 * (long long)row]; lq = qstats[4 * (long long)row + 1]; rkq = qstats[4 * (long long)row + 2];
        mx = mq > mx ? mq : mx;
    }
    RowAcc a = {0.f, 0.f};
    const ExpForm<FAST> ex(mx);
    DPC_UNROLL
    for (int i = 0; i < NV; ++i) {
        const int q = tid + 256 * i;
        unit_exp<4>(v[i], 4 * q, q < nq, tgt, g, c, a, ex);
    }
    reduce_row(sh, a, lane, wv);
    float se = a.se, rk = a.rk;
    if (qstats) {
        const float lqw = lq * c.wE;
        se += lqw * (FAST ? fast_exp2((mq - mx) * 1.4426950408889634f) : expf(mq - mx));
        rk += rkq;
    }
    if (tid == 0) write_row(sh, row, a, se, rk, rkq, mx, tgt, c, qstats != nullptr, row_ws, lse_out, report_rows != nullptr);
    if (dscore) {
        const float inv = 1.f / se, invr = 1.f / (float)rows;
        TD* d = dscore + (long long)row * ld_d;
        DPC_UNROLL
        for (int i = 0; i < NV; ++i) {
            const int q = tid + 256 * i;
            if (q < nq) {
                float gr[4];
                DPC_UNROLL
                for (int e = 0; e < 4; ++e) {
                    float t = v[i][e] * inv;
                    if (4 * q + e == row) t -= 1.f;
                    gr[e] = t * invr;
                }
                if constexpr (sizeof(TD) == 2) {
                    const u32x2 o = {bf16x2_pack(gr[0], gr[1]), bf16x2_pack(gr[2], gr[3])};
                    *(u32x2*)(d + 4 * q) = o;
                } else {
                    const f32x4 o = {gr[0], gr[1], gr[2], gr[3]};
                    *(f32x4*)(d + 4 * q) = o;
                }
            }
        }
        for (int j = cols + tid; j < ld_d; j += 256) d[j] = Elt<TD>::from_f32(0.f);
    }
    if (report_rows) report_pass<FAST>(sh, s, g, c, report_rows);
}

// ---- ce_row_vec16_body: bf16 logits, NV units of 8 per thread, bf16 gradient
template <int NV>
__global__ __launch_bounds__(256) void ce_row_vec16_cls_kernel(const bf16_t* score, int rows, int cols, int ld, float* row_ws, bf16_t* dscore,
                                                               int ld_d, const float* qstats, float* lse_out, ClsP c, float* report_rows) {
    __shared__ float sh[32];
    const int row = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const bf16_t* s = score + (long long)row * ld;
    const float tgt = bf16_to_f32(s[row]);
    const RowG g = row_geom(row, c);
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
    if (!c.allpos) mx = max_positive(s, cols, tid, g, c);
    mx = wave_max(mx);
    if (lane == 0) sh[wv] = mx;
    __syncthreads();
    mx = sh[0];
    DPC_UNROLL
    for (int w = 1; w < 4; ++w) mx = sh[w] > mx ? sh[w] : mx;
    float mq = 0.f, lq = 0.f, rkq = 0.f;
    if (qstats) {
        mq = qstats[4 * (long long)row]; lq = qstats[4 * (long long)row + 1]; rkq = qstats[4 * (long long)row + 2];
        mx = mq > mx ? mq : mx;
    }
    RowAcc a = {0.f, 0.f};
    const ExpForm<true> ex(mx);
    DPC_UNROLL
    for (int i = 0; i < NV; ++i) {
        const int q = tid + 256 * i;
        unit_exp<8>(v[i], 8 * q, q < nq, tgt, g, c, a, ex);
    }
    reduce_row(sh, a, lane, wv);
    float se = a.se, rk = a.rk;
    if (qstats) {
        const float lqw = lq * c.wE;
        se += lqw * fast_exp2((mq - mx) * 1.4426950408889634f);
        rk += rkq;
    }
    if (tid == 0) write_row(sh, row, a, se, rk, rkq, mx, tgt, c, qstats != nullptr, row_ws, lse_out, report_rows != nullptr);
    if (dscore) {
        const float inv = 1.f / se, invr = 1.f / (float)rows;
        bf16_t* d = dscore + (long long)row * ld_d;
        DPC_UNROLL
        for (int i = 0; i < NV; ++i) {
            const int q = tid + 256 * i;
            if (q < nq) {
                float gr[8];
                DPC_UNROLL
                for (int e = 0; e < 8; ++e) {
                    float t = v[i][e] * inv;
                    if (8 * q + e == row) t -= 1.f;
                    gr[e] = t * invr;
                }
                *(u32x4*)(d + 8 * q) = unit_pack<bf16_t>(gr);
            }
        }
        for (int j = cols + tid; j < ld_d; j += 256) d[j] = Elt<bf16_t>::from_f32(0.f);
    }
    if (report_rows) report_pass<true>(sh, s, g, c, report_rows);
}

// means of the per-row report: the four masses, then the share of rows with at least one column of the class above the target
__global__ __launch_bounds__(256) void cls_report_kernel(const float* report_rows, int rows, float* report) {
    __shared__ float sh[4][8];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float a[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int r = tid; r < rows; r += 256) {
        const float* o = report_rows + 8 * (long long)r;
        DPC_UNROLL
        for (int k = 0; k < 4; ++k) a[k] += o[k];
        DPC_UNROLL
        for (int k = 4; k < 7; ++k) a[k] += o[k] > 0.f ? 1.f : 0.f;
    }
    DPC_UNROLL
    for (int k = 0; k < 7; ++k) {
        a[k] = wave_sum(a[k]);
        if (lane == 0) sh[wv][k] = a[k];
    }
    __syncthreads();
    if (tid < 7) report[tid] = (sh[0][tid] + sh[1][tid] + sh[2][tid] + sh[3][tid]) / (float)rows;
    if (tid == 7) report[7] = 0.f;
}

bool weight_ok(float w) { return w >= 0.f && w <= 65536.f; }   // false for NaN

// the descriptor against the call: DPC_OK, or DPC_ERR_ARG
int cls_check(const dpc_neg_classes& d, int cols, const float* qstats, const float* lse_out, const float* report_rows, const float* report, ClsP* out) {
    if ((qstats == nullptr) != (lse_out == nullptr)) return DPC_ERR_ARG;
    if (report && !report_rows) return DPC_ERR_ARG;
    if (d.B <= 0 || d.P <= 0 || d.SQ <= 0 || d.flags != 0 || d.reserved != 0.f) return DPC_ERR_ARG;
    if ((long long)d.B * d.P * d.SQ != (long long)cols) return DPC_ERR_ARG;
    if (!weight_ok(d.w_spatial) || !weight_ok(d.w_temporal) || !weight_ok(d.w_easy)) return DPC_ERR_ARG;
    if (qstats && !(d.w_easy > 0.f)) return DPC_ERR_ARG;
    out->W = d.P * d.SQ;
    out->SQ = d.SQ;
    out->dSQ = make_fastdiv((uint32_t)d.SQ);
    out->dW = make_fastdiv((uint32_t)out->W);
    out->wS = d.w_spatial; out->wT = d.w_temporal; out->wE = d.w_easy;
    out->log_wE = d.w_easy > 0.f ? logf(d.w_easy) : 0.f;
    out->allpos = d.w_spatial > 0.f && d.w_temporal > 0.f && d.w_easy > 0.f;
    return DPC_OK;
}

}  // namespace

extern "C" int dpc_ce_topk_cls(const float* score, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result, void* dscore,
                               int32_t dtype_d, int32_t ld_d, const float* qstats, float* lse_out, dpc_neg_classes cls,
                               float* report_rows, float* report, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!score || !row_ws || !result || rows <= 0 || cols < rows || ld < cols) return DPC_ERR_ARG;
    if (dscore && ld_d < cols) return DPC_ERR_ARG;
    if (dscore && dtype_d != DPC_F32 && dtype_d != DPC_BF16) return DPC_ERR_ARG;
    ClsP c;
    if (int e = cls_check(cls, cols, qstats, lse_out, report_rows, report, &c)) return e;
    const bool vec = cols % 4 == 0 && ld % 4 == 0 && ((uintptr_t)score % 16) == 0 && cols <= 16384 &&
                     (!dscore || (ld_d % 4 == 0 && ((uintptr_t)dscore % 16) == 0));
    if (!dscore || dtype_d == DPC_F32) {
        if (vec && cols <= 8192) {
            DPC_LAUNCH((ce_row_vec_cls_kernel<float, 8, false>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (float*)dscore, ld_d, qstats, lse_out, c, report_rows);
        } else if (vec) {
            DPC_LAUNCH((ce_row_vec_cls_kernel<float, 16, false>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (float*)dscore, ld_d, qstats, lse_out, c, report_rows);
        } else {
            DPC_LAUNCH((ce_row_cls_kernel<float>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (float*)dscore, ld_d, qstats, lse_out, c, report_rows);
        }
    } else {
        if (vec && cols <= 8192) {
            DPC_LAUNCH((ce_row_vec_cls_kernel<bf16_t, 8, true>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (bf16_t*)dscore, ld_d, qstats, lse_out, c, report_rows);
        } else if (vec) {
            DPC_LAUNCH((ce_row_vec_cls_kernel<bf16_t, 16, true>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (bf16_t*)dscore, ld_d, qstats, lse_out, c, report_rows);
        } else {
            DPC_LAUNCH((ce_row_cls_kernel<bf16_t>), dim3(rows), dim3(256), stream, score, rows, cols, ld, row_ws, (bf16_t*)dscore, ld_d, qstats, lse_out, c, report_rows);
        }
    }
    if (report) DPC_LAUNCH(cls_report_kernel, dim3(1), dim3(256), stream, report_rows, rows, report);
    return dpc_ce_finalize(row_ws, rows, result, stream_);
}

extern "C" int dpc_ce_topk_bf16_cls(const void* score, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result, void* dscore,
                                    int32_t ld_d, const float* qstats, float* lse_out, dpc_neg_classes cls, float* report_rows,
                                    float* report, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!score || !row_ws || !result || rows <= 0 || cols < rows || ld < cols) return DPC_ERR_ARG;
    if (dscore && ld_d < cols) return DPC_ERR_ARG;
    ClsP c;
    if (int e = cls_check(cls, cols, qstats, lse_out, report_rows, report, &c)) return e;
    if (cols % 8 || ld % 8 || ((uintptr_t)score % 16) || cols > 16384 || (dscore && (ld_d % 8 || ((uintptr_t)dscore % 16)))) return DPC_ERR_UNSUPPORTED;
    if (cols <= 2048 * 4) {
        DPC_LAUNCH((ce_row_vec16_cls_kernel<4>), dim3(rows), dim3(256), stream, (const bf16_t*)score, rows, cols, ld, row_ws, (bf16_t*)dscore, ld_d, qstats, lse_out, c, report_rows);
    } else {
        DPC_LAUNCH((ce_row_vec16_cls_kernel<8>), dim3(rows), dim3(256), stream, (const bf16_t*)score, rows, cols, ld, row_ws, (bf16_t*)dscore, ld_d, qstats, lse_out, c, report_rows);
    }
    if (report) DPC_LAUNCH(cls_report_kernel, dim3(1), dim3(256), stream, report_rows, rows, report);
    return dpc_ce_finalize(row_ws, rows, result, stream_);
}
