// recipe_draw.hip -- the random draws of the pre-training recipes (dpc/main.py:114-132) on the device, for frames that are resident
// in HBM (dpc_amd/data.py FrameStore / ResidentFrameSource, `--resident`): per clip the start frame of idx_sampler
// (dpc/dataset_3d.py:85-92), the crop box of RandomSizedCrop / RandomCrop, the flip, RandomGray's channel per frame, ColorJitter's
// factors and shuffled chain per frame (utils/augmentation.py:99-351), and PIL's BILINEAR resampling tables for the drawn box --
// written as exactly the device tables dpc_store_to_input reads, so a captured step draws, gathers and trains without the host.
//
// The decisions and the double arithmetic are those of data._draw_sized_crop / data.resample_tables / data._jitter_get_params;
// data.recipe_from_uniforms states them on the host from the same uniforms and the two agree bit for bit (tests/resident_cases.py).
// What makes that hold:
//   * no fused multiply-add: hipcc contracts a * b + c by default, which changes the last bit of `center`, of the weights and of
//     0.5 + v * 2^22 -- contraction is switched off for this file (the pragma below);
//   * int(round(x)) of a Python float is round-half-even: rint();
//   * the f64 square root must be the correctly rounded one (math.sqrt is): __dsqrt_rn is the HIP math API's IEEE
//     round-to-nearest-even square root.  It becomes llvm.sqrt.f64 without fast-math flags, which the AMDGPU backend expands into
//     v_rsq_f64, two Goldschmidt steps and a final residual correction (visible in this file's gfx950 assembly as the fma chain after
//     v_rsq_f64) -- not the bare v_sqrt_f64, which is good to about 2^-26 only.  tests/test_resident_gpu.py holds w and h of every
//     accepted crop to math.sqrt's bits through the tables they size;
//   * weights are summed left to right, as libImaging/Resample.c does.
// The uniforms: Philox4x32-10 under stream DPC_PHILOX_STREAM_AUG, key = seed, counter block = (slot >> 2, draw counter, stream,
// clip): every clip owns DPC_RECIPE_SLOTS(N * SL) slots in the layout of include/dpc_hip.h, a rejected crop attempt keeps its
// slots, so a draw is a pure function of (seed, counter, clip, slot).  These are NOT the draws of Python's `random`: a --resident
// run sees a different, equally distributed sample than a --frames run.
// dpc_draw_recipe_ex adds what the classifier's recipes (eval/test.py:161-176; dpc_amd.lc_main --resident) need, in the same slots:
// ColorJitter(consistent=True) -- one draw, frame 0's slots, copied to every frame; the NEAREST Scale((size, size)) behind
// RandomSizedCrop(crop) -- the sized crop works at `crop` and output row i shows row scale_tab[i] of its table; a `lengths` table for
// a dense store whose videos are shorter than their slot; and the batch's labels gathered by video index into `target`.
// Latency-sized like lc_test.hip: one workgroup per clip; every lane repeats the clip's few scalar decisions (nothing shared, no barrier),
// then the lanes take the 2 * size table rows and the N * SL frames.
#include "philox.h"
#include "../../include/dpc_hip.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int RS_PREC = 32 - 8 - 2;  // PIL ImagingResample PRECISION_BITS
constexpr int SLOT_START = 0, SLOT_FLIP = 1, SLOT_SIZED_P = 2, SLOT_CROP_X = 3, SLOT_CROP_Y = 4, SLOT_JITTER_P = 5, SLOT_ATTEMPT = 8,
              ATTEMPT_SLOTS = 5, ATTEMPTS = 10, SLOT_FRAME = SLOT_ATTEMPT + ATTEMPT_SLOTS * ATTEMPTS, FRAME_SLOTS = 9;
static_assert(DPC_RECIPE_SLOTS(0) == SLOT_FRAME && DPC_RECIPE_SLOTS(1) - DPC_RECIPE_SLOTS(0) == FRAME_SLOTS, "slot layout of include/dpc_hip.h");

__device__ __forceinline__ double sqrt_rn(double x) {
#ifdef DPC_SIMT_EMU
    return sqrt(x);
#else
    return __dsqrt_rn(x);
#endif
}

struct Draw {
    const float* uniforms;
    int slots, clip;
    uint32_t d, k0, k1;
    __device__ __forceinline__ double u(int slot) const {
        if (uniforms) return (double)uniforms[(long long)clip * slots + slot];
        const Philox4 r = philox4x32_10((uint32_t)(slot >> 2), d, DPC_PHILOX_STREAM_AUG, (uint32_t)clip, k0, k1);
        const int w = slot & 3;   // selects, not r.v[w]: a dynamic index would put the four words into scratch memory
        const uint32_t word = w == 0 ? r.v[0] : (w == 1 ? r.v[1] : (w == 2 ? r.v[2] : r.v[3]));
        return (double)(word >> 8) * 5.9604644775390625e-8;   // 2^-24, exact
    }
    __device__ __forceinline__ int randint(int slot, int n) const { return (int)floor(u(slot) * (double)(n + 1)); }   // [0, n]
    __device__ __forceinline__ double uniform(int slot, double a, double b) const { return a + (b - a) * u(slot); }   // random.uniform
};

// one axis of the geometry: RESAMPLE = rows [first, first + size) of PIL's table for resizing `in` samples to `out`; IDENTITY = the
// index map i -> i; SCALE = i -> scale_tab[i] (NEAREST Scale of the crop box; identity without a table)
enum { RESAMPLE = 0, IDENTITY = 1, SCALE = 2 };
struct Axis { int mode, in, out, first; };

// data.resample_tables, one row (libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc, BILINEAR, support 1.0)
__device__ void table_row(const Axis& a, int i, int KS, const int32_t* scale_tab, int32_t* bnd, int32_t* k) {
    if (a.mode != RESAMPLE) {
        bnd[0] = (a.mode == SCALE && scale_tab) ? scale_tab[i] : i;
        bnd[1] = 1;
        k[0] = 1 << RS_PREC;
        for (int x = 1; x < KS; ++x) k[x] = 0;
        return;
    }
    const double scale = (double)a.in / (double)a.out;
    const double fscale = scale > 1.0 ? scale : 1.0;
    const double sup = 1.0 * fscale, ss = 1.0 / fscale;
    const double center = ((double)(a.first + i) + 0.5) * scale;
    int xmin = (int)(center - sup + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + sup + 0.5);
    if (xmax > a.in) xmax = a.in;
    xmax -= xmin;
    if (xmax > KS) xmax = KS;   // cannot happen for KS >= 2 ceil(sup) + 1 (the entry checks the worst case); never write past the row
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
        const double t = ((double)(x + xmin) - center + 0.5) * ss;
        const double w = 1.0 - fabs(t);
        ww += w > 0.0 ? w : 0.0;
    }
    for (int x = 0; x < xmax; ++x) {
        const double t = ((double)(x + xmin) - center + 0.5) * ss;
        double w = 1.0 - fabs(t);
        w = w > 0.0 ? w : 0.0;
        if (ww != 0.0) w = w / ww;
        k[x] = w < 0.0 ? (int)(-0.5 + w * (double)(1 << RS_PREC)) : (int)(0.5 + w * (double)(1 << RS_PREC));
    }
    for (int x = xmax > 0 ? xmax : 0; x < KS; ++x) k[x] = 0;
    bnd[0] = xmin;
    bnd[1] = xmax;
}

__global__ __launch_bounds__(256) void draw_recipe_kernel(dpc_recipe_desc rc, const int32_t* video_idx, const int32_t* step_dev, const long long* offsets,
                                                          const long long* lengths, const long long* labels, int B, int W0, int H0, int crop,
                                                          int size, int n_fr, int span_frames, int KS, const int32_t* scale_tab,
                                                          unsigned long long seed, const int32_t* draw_dev, const float* uniforms,
                                                          dpc_clip_aug* aug, long long* clip_first, int8_t* gray, dpc_frame_jitter* jitter,
                                                          int32_t* xb, int32_t* xk, int32_t* yb, int32_t* yk, long long* target) {
    const int b = blockIdx.x;
    if (b >= B) return;
    const Draw dr = {uniforms, DPC_RECIPE_SLOTS(n_fr), b, (uint32_t)draw_dev[0], (uint32_t)seed, (uint32_t)(seed >> 32)};
    const long long row = step_dev ? (long long)step_dev[0] - 1 : 0;
    const int vid = video_idx[row * B + b];
    const long long first = offsets[vid], vlen = lengths ? lengths[vid] : offsets[vid + 1] - first;
    // DPC_RECIPE_SCALE_AFTER_SIZED: the sized crop resizes to `crop` and the NEAREST Scale picks rows of that table; `out` is the side
    // RandomSizedCrop / CenterCrop work at
    const bool scale_after = (rc.flags & DPC_RECIPE_SCALE_AFTER_SIZED) != 0, consistent = (rc.flags & DPC_RECIPE_JITTER_CONSISTENT) != 0;
    const int out = scale_after ? crop : size;

    // ---- the clip's scalar decisions (every lane: a few dozen flops, cheaper than a broadcast through LDS)
    const int start = (int)floor(dr.u(SLOT_START) * (double)(vlen - span_frames));   // idx_sampler: uniform on [0, vlen - N*SL*ds)
    const int flip = (rc.flip_code != 0 && dr.u(SLOT_FLIP) < 0.5) ? rc.flip_code : 0;
    int x1 = 0, y1 = 0;
    Axis ax = {SCALE, 0, 0, 0}, ay = {SCALE, 0, 0, 0};
    if (rc.sized_p < 0.0) {   // RandomCrop(crop): draws only when there is something to crop
        if (!(W0 == crop && H0 == crop)) {
            x1 = dr.randint(SLOT_CROP_X, W0 - crop);
            y1 = dr.randint(SLOT_CROP_Y, H0 - crop);
        }
    } else if (dr.u(SLOT_SIZED_P) < rc.sized_p) {   // RandomSizedCrop: ten attempts, then Scale + CenterCrop on the whole frame
        bool found = false;
        for (int a = 0; a < ATTEMPTS && !found; ++a) {
            const int s = SLOT_ATTEMPT + ATTEMPT_SLOTS * a;
            const double target_area = dr.uniform(s, 0.5, 1.0) * (double)(W0 * H0);
            const double aspect = dr.uniform(s + 1, 3. / 4, 4. / 3);
            int w = (int)rint(sqrt_rn(target_area * aspect));
            int h = (int)rint(sqrt_rn(target_area / aspect));
            if (dr.u(s + 2) < 0.5) { const int t = w; w = h; h = t; }
            if (w <= W0 && h <= H0) {
                x1 = dr.randint(s + 3, W0 - w);
                y1 = dr.randint(s + 4, H0 - h);
                ax = {RESAMPLE, w, out, 0};
                ay = {RESAMPLE, h, out, 0};
                found = true;
            }
        }
        if (!found) {
            int ow, oh;
            if (W0 < H0) { ow = out; oh = (int)((double)(out * H0) / (double)W0); }
            else { oh = out; ow = (int)((double)(out * W0) / (double)H0); }
            ax = {RESAMPLE, W0, ow, (int)rint((double)(ow - out) / 2.)};
            ay = {RESAMPLE, H0, oh, (int)rint((double)(oh - out) / 2.)};
        }
    } else {   // the failed `p` draw: CenterCrop(out); behind it the NEAREST Scale is the index map of the SCALE mode
        x1 = (int)rint((double)(W0 - out) / 2.);
        y1 = (int)rint((double)(H0 - out) / 2.);
        if (!scale_after) ax.mode = ay.mode = IDENTITY;
    }
    const bool jit_on = rc.jitter_p >= 0.0 && dr.u(SLOT_JITTER_P) < rc.jitter_p;

    if (threadIdx.x == 0) {
        dpc_clip_aug a;
        a.start = start; a.x1 = x1; a.y1 = y1; a.flip = flip;
        aug[b] = a;
        clip_first[b] = first;
        if (target) target[b] = labels[vid];
    }
    for (int r = threadIdx.x; r < 2 * size; r += blockDim.x) {
        const bool isx = r < size;
        const int i = isx ? r : r - size;
        const long long o = (long long)b * size + i;
        const Axis& a = isx ? ax : ay;
        const int t = (scale_after && a.mode == RESAMPLE && scale_tab) ? scale_tab[i] : i;   // the row of the `crop` table output row i shows
        table_row(a, t, KS, scale_tab, (isx ? xb : yb) + o * 2, (isx ? xk : yk) + o * KS);
    }
    for (int f = threadIdx.x; f < n_fr; f += blockDim.x) {
        const int s = SLOT_FRAME + FRAME_SLOTS * f;
        int g = -1;
        if (rc.gray_p >= 0.0 && dr.u(s) < rc.gray_p) g = (int)floor(dr.u(s + 1) * 3.0);   // RandomGray: np.random.choice(3)
        gray[(long long)b * n_fr + f] = (int8_t)g;
        dpc_frame_jitter j;
        j.factor[0] = j.factor[1] = j.factor[2] = 0.f;
        j.hue_shift = 0;
        j.order[0] = j.order[1] = j.order[2] = j.order[3] = 255;
        const int sj = consistent ? SLOT_FRAME : s;   // consistent=True: ONE get_params draw, frame 0's slots, copied to every frame
        if (jit_on) {   // ColorJitter.get_params: four uniforms, then random.shuffle of the steps whose range is not 0
            const double v[4] = {rc.brightness, rc.contrast, rc.saturation, rc.hue};
            int n = 0;
            for (int op = 0; op < 4; ++op) {
                if (v[op] == 0.0) continue;
                if (op == 3) {
                    const double fh = dr.uniform(sj + 2 + op, -v[op], v[op]);
                    j.hue_shift = (int)(fh * 255.0) & 0xFF;   // np.uint8(hue_factor * 255): C truncation, uint8 wrap
                } else {
                    const double lo = 1.0 - v[op] > 0.0 ? 1.0 - v[op] : 0.0;
                    j.factor[op] = (float)dr.uniform(sj + 2 + op, lo, 1.0 + v[op]);
                }
                j.order[n++] = (uint8_t)op;
            }
            for (int i = n - 1; i >= 1; --i) {   // Fisher-Yates from the top, as random.shuffle walks
                const int q = (int)floor(dr.u(sj + 6 + (3 - i)) * (double)(i + 1));
                const uint8_t t = j.order[i]; j.order[i] = j.order[q]; j.order[q] = t;
            }
        }
        jitter[(long long)b * n_fr + f] = j;
    }
}

}  // namespace

extern "C" int dpc_draw_recipe_ex(const dpc_recipe_desc* rc, const int32_t* video_idx, const int32_t* step_dev, const int64_t* offsets,
                                  const int64_t* lengths, const int64_t* labels, int32_t B, int32_t W0, int32_t H0, int32_t crop, int32_t size,
                                  int32_t N, int32_t SL, int32_t ds, int32_t KS, const int32_t* scale_tab, uint64_t seed, const int32_t* draw_dev,
                                  const float* uniforms, dpc_clip_aug* aug, int64_t* clip_first, int8_t* gray, dpc_frame_jitter* jitter,
                                  int32_t* xb, int32_t* xk, int32_t* yb, int32_t* yk, int64_t* target, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!rc || !video_idx || !offsets || !draw_dev || !aug || !clip_first || !gray || !jitter || !xb || !xk || !yb || !yk) return DPC_ERR_ARG;
    if ((labels == nullptr) != (target == nullptr)) return DPC_ERR_ARG;   // the label gather: both tables or neither
    if (B <= 0 || W0 <= 0 || H0 <= 0 || size <= 0 || N <= 0 || SL <= 0 || ds <= 0 || KS <= 0) return DPC_ERR_ARG;
    if (B > 1024 || size > 1024 || (long long)W0 * H0 >= (1ll << 30) || (long long)N * SL * ds >= (1ll << 30)) return DPC_ERR_UNSUPPORTED;
    if (rc->flags & ~(DPC_RECIPE_JITTER_CONSISTENT | DPC_RECIPE_SCALE_AFTER_SIZED)) return DPC_ERR_ARG;
    if (rc->sized_p > 1.0 || rc->gray_p > 1.0 || rc->jitter_p > 1.0 || rc->flip_code < 0 || rc->flip_code > 2) return DPC_ERR_ARG;
    if (rc->brightness < 0.0 || rc->contrast < 0.0 || rc->saturation < 0.0 || rc->hue < 0.0 || rc->hue > 0.5) return DPC_ERR_ARG;
    const bool scale_after = (rc->flags & DPC_RECIPE_SCALE_AFTER_SIZED) != 0;
    if (rc->sized_p < 0.0) {   // RandomCrop(crop) (+ NEAREST Scale): the box must fit the frame; one tap per row
        if (scale_after) return DPC_ERR_ARG;   // the flag is about the Scale behind RandomSizedCrop
        if (crop <= 0 || crop > W0 || crop > H0 || (!scale_tab && crop != size)) return DPC_ERR_ARG;
    } else {
        const int m = W0 > H0 ? W0 : H0;
        const int out = scale_after ? crop : size;   // the side RandomSizedCrop resizes to
        if (scale_after && (crop <= 0 || (scale_tab != nullptr) != (crop != size))) return DPC_ERR_ARG;   // the table iff there is a Scale
        if (scale_after && crop > 1024) return DPC_ERR_UNSUPPORTED;                   // as `size`: out * max(W0, H0) stays inside an int
        if (KS < 2 * ((m + out - 1) / out) + 1) return DPC_ERR_ARG;                 // the widest window any accepted box can need
        if (rc->sized_p < 1.0 && (out > W0 || out > H0)) return DPC_ERR_UNSUPPORTED;   // CenterCrop(out) would leave the frame
    }
    DPC_LAUNCH(draw_recipe_kernel, dim3((unsigned)B), dim3(256), stream, *rc, video_idx, step_dev, (const long long*)offsets,
               (const long long*)lengths, (const long long*)labels, B, W0, H0, crop, size, N * SL, N * SL * ds, KS, scale_tab,
               (unsigned long long)seed, draw_dev, uniforms, aug, (long long*)clip_first, gray, jitter, xb, xk, yb, yk, (long long*)target);
    return dpc_launch_status();
}

// the entry of ABI 1: the same launch with the additions off (whatever the descriptor's last word holds, as before)
extern "C" int dpc_draw_recipe(const dpc_recipe_desc* rc, const int32_t* video_idx, const int32_t* step_dev, const int64_t* offsets,
                               int32_t B, int32_t W0, int32_t H0, int32_t crop, int32_t size, int32_t N, int32_t SL, int32_t ds, int32_t KS,
                               const int32_t* scale_tab, uint64_t seed, const int32_t* draw_dev, const float* uniforms, dpc_clip_aug* aug,
                               int64_t* clip_first, int8_t* gray, dpc_frame_jitter* jitter, int32_t* xb, int32_t* xk, int32_t* yb, int32_t* yk,
                               dpc_stream_t stream) {
    if (!rc) return DPC_ERR_ARG;
    dpc_recipe_desc plain = *rc;
    plain.flags = 0;
    return dpc_draw_recipe_ex(&plain, video_idx, step_dev, offsets, nullptr, nullptr, B, W0, H0, crop, size, N, SL, ds, KS, scale_tab, seed,
                              draw_dev, uniforms, aug, clip_first, gray, jitter, xb, xk, yb, yk, nullptr, stream);
}
