// lc_test.hip -- the video-level reduction of the downstream test (eval/test.py:317-334) on the device.
// A test video is a set of windows (eval/dataset_3d_lc.py:109-127); the model sees them in chunks of the engine's batch and
// its logits [rows][num_class] never leave the device:
//   accumulate   per chunk: softmax of every valid row summed into psum, the logits summed into lsum, rows counted
//                (`torch.mean(torch.mean(softmax(output, 2), 0), 0)` and `torch.mean(torch.mean(output, 0), 0)`, :317-326)
//   finish       per video: mean probability / mean logit; rank = #{c : p_c > p_label}, STRICTLY greater (the rule of
//                ce_row_kernel in loss.hip) -> top-1 = rank < 1, top-5 = rank < 5 (calc_topk_accuracy,
//                utils/utils.py:38-55); loss = logsumexp(mean logits) - mean logit[label] (nn.CrossEntropyLoss on one row);
//                pred = argmax(mean logits), lowest index on ties; confusion[pred][label] += 1 (ConfusionMeter.update,
//                utils/utils.py:148-153: prediction in rows, target in columns); run totals (sum loss, sum top-1, sum top-5,
//                videos); the per-video state is cleared.
// The sums run in row order and chunk order, every value has ONE writer and there is no atomic: a run is bit-reproducible
// and does not depend on how the windows were cut into chunks.  Latency-sized (<= 128 x 101 logits per chunk): one workgroup.
// Row reductions are wave64 shuffles then one LDS hop across the 4 waves, as in loss.hip.
#include "dpc_rt.h"
#include "../../include/dpc_hip.h"

namespace {

constexpr int ROW_TILE = 64;

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

// one workgroup.  Phase 1: wave w takes rows w, w + 4, .. of a tile and leaves (max, sum exp) of each in LDS; phase 2:
// thread j owns column j (j + 256, ..) and adds the tile's rows IN ROW ORDER onto the running state.
__global__ __launch_bounds__(256) void lc_test_accumulate_kernel(const float* logits, int n_valid, int C, int ld, float* psum, float* lsum,
                                                                 int32_t* count) {
    __shared__ float s_mx[ROW_TILE], s_se[ROW_TILE];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    for (int r0 = 0; r0 < n_valid; r0 += ROW_TILE) {
        const int nr = n_valid - r0 < ROW_TILE ? n_valid - r0 : ROW_TILE;
        for (int r = wv; r < nr; r += 4) {
            const float* s = logits + (long long)(r0 + r) * ld;
            float mx = -3.0e38f;
            for (int j = lane; j < C; j += 64) { const float v = s[j]; mx = v > mx ? v : mx; }
            mx = wave_max(mx);
            float se = 0.f;
            for (int j = lane; j < C; j += 64) se += expf(s[j] - mx);
            se = wave_sum(se);
            if (lane == 0) { s_mx[r] = mx; s_se[r] = se; }
        }
        __syncthreads();
        for (int j = tid; j < C; j += 256) {
            float p = psum[j], l = lsum[j];
            for (int r = 0; r < nr; ++r) {
                const float v = logits[(long long)(r0 + r) * ld + j];
                p += expf(v - s_mx[r]) / s_se[r];
                l += v;
            }
            psum[j] = p;
            lsum[j] = l;
        }
        __syncthreads();
    }
    if (tid == 0) count[0] += n_valid;
}

__global__ __launch_bounds__(256) void lc_test_finish_kernel(float* psum, float* lsum, int32_t* count, int C, int label, float* mean_prob,
                                                             float* video, double* totals, long long* confusion) {
    __shared__ float sh[12];
    __shared__ int shi[4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = count[0];
    if (n <= 0) return;   // no window was accumulated: nothing to report (the host never asks for this)
    const float fn = (float)n;
    const float p_lab = psum[label] / fn, l_lab = lsum[label] / fn;
    float rk = 0.f, mx = -3.0e38f;
    int arg = 0x7fffffff;
    for (int j = tid; j < C; j += 256) {
        const float p = psum[j] / fn, l = lsum[j] / fn;
        rk += p > p_lab ? 1.f : 0.f;
        if (l > mx) { mx = l; arg = j; }            // ascending j per thread: the first maximum is kept
        if (mean_prob) mean_prob[j] = p;
    }
    rk = wave_sum(rk);
    DPC_UNROLL
    for (int m = 32; m >= 1; m >>= 1) {
        const float om = __shfl_xor(mx, m);
        const int oa = __shfl_xor(arg, m);
        if (om > mx || (om == mx && oa < arg)) { mx = om; arg = oa; }
    }
    if (lane == 0) { sh[wv] = rk; sh[4 + wv] = mx; shi[wv] = arg; }
    __syncthreads();
    rk = sh[0] + sh[1] + sh[2] + sh[3];
    mx = sh[4];
    arg = shi[0];
    DPC_UNROLL
    for (int w = 1; w < 4; ++w)
        if (sh[4 + w] > mx || (sh[4 + w] == mx && shi[w] < arg)) { mx = sh[4 + w]; arg = shi[w]; }
    if (arg >= C) arg = 0;   // no logit compared greater than the start value (NaN rows): keep the confusion index inside the matrix
    float se = 0.f;
    for (int j = tid; j < C; j += 256) se += expf(lsum[j] / fn - mx);
    se = wave_sum(se);
    if (lane == 0) sh[8 + wv] = se;
    __syncthreads();
    se = sh[8] + sh[9] + sh[10] + sh[11];
    __syncthreads();   // every read of the state is done: clear it for the next video
    for (int j = tid; j < C; j += 256) { psum[j] = 0.f; lsum[j] = 0.f; }
    if (tid == 0) {
        const float loss = logf(se) + mx - l_lab;
        const float t1 = rk < 1.f ? 1.f : 0.f, t5 = rk < 5.f ? 1.f : 0.f;
        video[0] = loss; video[1] = t1; video[2] = t5; video[3] = (float)arg;
        totals[0] += (double)loss; totals[1] += (double)t1; totals[2] += (double)t5; totals[3] += 1.0;
        confusion[(long long)arg * C + label] += 1;
        count[0] = 0;
    }
}

}  // namespace

extern "C" int dpc_lc_test_accumulate(const float* logits, int32_t rows, int32_t n_valid, int32_t num_class, int32_t ld, float* psum,
                                      float* lsum, int32_t* count, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!logits || !psum || !lsum || !count || rows <= 0 || n_valid <= 0 || n_valid > rows || num_class <= 0 || ld < num_class) return DPC_ERR_ARG;
    DPC_LAUNCH(lc_test_accumulate_kernel, dim3(1), dim3(256), stream, logits, n_valid, num_class, ld, psum, lsum, count);
    return dpc_launch_status();
}

extern "C" int dpc_lc_test_finish(float* psum, float* lsum, int32_t* count, int32_t num_class, int32_t label, float* mean_prob, float* video,
                                  double* totals, int64_t* confusion, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!psum || !lsum || !count || !video || !totals || !confusion || num_class <= 0 || label < 0 || label >= num_class) return DPC_ERR_ARG;
    DPC_LAUNCH(lc_test_finish_kernel, dim3(1), dim3(256), stream, psum, lsum, count, num_class, label, mean_prob, video, totals,
               (long long*)confusion);
    return dpc_launch_status();
}
