/* dpc_hip.h -- C ABI of libdpc_hip.so, the MI355X (gfx950) kernels of the DPC-RNN
 * training step.
 *
 * The reference (TengdaHan/DPC) has NO native/FFI layer: every op on its hot path is
 * a stock torch op reached through the Python nn.Module API.  This
 * header therefore *defines* the boundary a maintainer binds instead of those torch
 * ops; each entry cites the reference call site it replaces (paths relative to the
 * reference checkout).  INTEGRATION.md shows the ctypes stub on the reference side.
 *
 * Conventions
 *   - plain pointers + sizes, no torch types; all pointers are DEVICE pointers;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*), never
 *     allocates, never synchronises; workspaces are caller-owned;
 *   - return 0 on success, <0 on error (DPC_ERR_*); nothing is printed;
 *   - activations are channels-last [N][T][H][W][C]; dtype codes: 0 = f32, 1 = bf16.
 */
#ifndef DPC_HIP_H
#define DPC_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DPC_F32 0
#define DPC_BF16 1

#define DPC_ERR_ARG (-1)
#define DPC_ERR_LAUNCH (-2)
#define DPC_ERR_UNSUPPORTED (-3)

typedef void* dpc_stream_t;

int dpc_abi_version(void);

/* ---- implicit-GEMM convolution / GEMM on the matrix cores ----------------------
 * Replaces nn.Conv3d forward and its autograd input-gradient in
 *   backbone/resnet_2d3d.py:14-32 (conv3x3x3 / conv1x3x3), :211 (stem, after the
 *   space-to-depth repack of dpc_pack_input_s2d), :241-244 (1x1x1 downsample),
 * nn.Conv2d 1x1 (ConvGRU gates backbone/convrnn.py:13-15,29-33; network_pred
 *   dpc/model_3d.py:36-40) and torch.matmul for the score (dpc/model_3d.py:83).
 *
 *   out[m][co] = sum_{tap,ci} src[gather(m,tap)][ci] * wgt[co][tap*Ci+ci]  (+ addend[m][co])
 * rows m enumerate (n, rt, rh, rw); mode 0 gathers rt*st-pt+kt (forward), mode 1
 * gathers (rt+pt-kt)/st when divisible (input-gradient; wgt is then the
 * [Ci][tap][Co] transpose produced by dpc_pack_weight).  A plain NT GEMM is the
 * case N=M, all spatial dims 1, one tap.  Strides must be 1 or 2; Ci a power of two
 * when there is more than one tap; Ci, src_ld, ldw multiples of 16 bytes.
 * If `stats` != NULL it receives per-program partial sums [rows][2][Co] (sum, sum of
 * squares of the stored outputs) for the batch-norm that follows; the row count is
 * dpc_conv_stats_rows(desc).
 * Aliasing: `addend` MAY be the same buffer as `out` (an in-place residual accumulation, dx += conv): every kernel behind
 * this entry and dpc_conv_igemm_ex reads a 16-byte addend unit in the lane that afterwards stores exactly that unit.  For a
 * strided input-gradient (mode 1, a stride of 2) with addend == out the positions no tap reaches are left as they are instead
 * of being rewritten with the addend.  No other pair of arguments may overlap.  tests/kcases.py::case_conv_dgrad_alias
 * runs every dispatch variant both ways (case_conv_dgrad_inplace: the untouched positions).
 */
typedef struct dpc_conv_desc {
    int32_t dtype_in, dtype_out; /* DPC_F32 / DPC_BF16 */
    int32_t mode;                /* 0 forward gather, 1 input-gradient gather */
    int32_t N, RT, RH, RW;       /* output positions                         */
    int32_t ST, SH, SW;          /* source tensor spatial dims               */
    int32_t Ci, src_ld;          /* channels per tap, source row stride      */
    int32_t Co, ldw, ldo;        /* output cols, weight row stride, out ld   */
    int32_t KT, KH, KW;
    int32_t st, sh, sw;
    int32_t pt, ph, pw;
} dpc_conv_desc;

int dpc_conv_stats_rows(const dpc_conv_desc* d);
int dpc_conv_igemm(const dpc_conv_desc* d, const void* src, const void* wgt, void* out,
                   const void* addend, float* stats, dpc_stream_t stream);

/* dpc_conv_igemm with backward pieces of the BasicBlock fused into the epilogue of an INPUT-GRADIENT launch (autograd of
 * backbone/resnet_2d3d.py:67-80,105-116), so that they stop being separate passes over HBM:
 *  - addend_mask: out = conv + (bit ? addend : 0), addend = the gradient arriving at the block output, bit = that output's
 *    ReLU sign mask (the byte-per-16-byte-unit mask dpc_bn_apply writes): the masked gradient dz is never materialised;
 *  - bn_raw (+ bn_mask, bn_mean, bn_invstd): the reduction of dpc_bn_bwd_reduce for the unit whose output gradient `out` is --
 *    dz = out gated by bn_mask, stats rows [dpc_conv_stats_rows(d)][2][Co] = (sum dz, sum dz * xhat), xhat = (bn_raw-mean)*invstd,
 *    taken from the stored (rounded) values; finish with dpc_bn_bwd_finalize, then dpc_bn_bwd_apply as before.
 * Without bn_raw `stats` means what it means for dpc_conv_igemm.  Requires ldo == Co, dtype_in == dtype_out, 16-byte aligned
 * tensors; DPC_ERR_UNSUPPORTED otherwise (run the separate kernels).  dpc_conv_plan with DPC_PLAN_ADDEND_MASK / DPC_PLAN_BNRED
 * tells which kernel serves the combination. */
typedef struct dpc_conv_epilogue {
    const void* addend;          /* optional [rows][ldo], dtype_out */
    const uint8_t* addend_mask;  /* optional, needs addend */
    const void* bn_raw;          /* optional [rows][ldo], dtype_out: raw conv output of the unit being differentiated */
    const uint8_t* bn_mask;      /* optional, needs bn_raw: ReLU mask of that unit's activation */
    const float* bn_mean;
    const float* bn_invstd;
    float* stats;
} dpc_conv_epilogue;
int dpc_conv_igemm_ex(const dpc_conv_desc* d, const void* src, const void* wgt, void* out, const dpc_conv_epilogue* epi,
                      dpc_stream_t stream);

/* NT GEMM with the reduction split over workgroups: part[ks][M][N] (f32) = A[M][K range ks] @ B[N][K range ks]^T, A / B row-major
 * with leading dimensions lda / ldb (dtype elements).  For products with a small output and a long reduction -- d_pred = dS @
 * feature_inf of the contrastive loss (dpc/main.py:217 backward: M = R, N = 256, K = R).  *nsplit = number of slabs (query with
 * part == NULL: capacity nsplit*M*N floats); sum them with dpc_reduce_unpack(part, nsplit, out, M, 1, N, N, 0, 1, 0). */
int dpc_gemm_nt_splitk(int32_t dtype, int32_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* B, int32_t ldb,
                       float* part, int32_t* nsplit, dpc_stream_t stream);
/* The same with A given K-major: part[ks][M][N] = sum_{k in slice ks} A[k][m] * B[n][k] (A rows are lda elements apart, bf16 only).
 * d_feature_inf = dS^T @ pred of the contrastive loss (autograd of dpc/model_3d.py:83): A = dS [R][ld], B = pred^T [256][ld].
 * A rows beyond K are never read; lda >= M and ldb >= K rounded up to 8 elements, the padding of B's rows holding finite values.
 * DPC_ERR_UNSUPPORTED outside N % 128 == 0, lda % 8 == ldb % 8 == 0, M, K >= 1024 (use dpc_conv_wgrad's GEMM form there). */
int dpc_gemm_tn_splitk(int32_t dtype, int32_t M, int32_t N, int32_t K, const void* A, int32_t lda, const void* B, int32_t ldb,
                       float* part, int32_t* nsplit, dpc_stream_t stream);

/* Weight gradient: part[ks][co][tap*Ci+ci] = sum_{m in split ks} dy[m][co]*src[gather(m,tap)][ci]
 * (autograd of the same convs / 1x1 convs / matmul; f32 partials, reduced by
 * dpc_reduce_unpack).  Returns the number of K-splits through *nsplit; capacity in
 * floats of `part` must be >= nsplit*Co*KT*KH*KW*Ci (query with part == NULL). */
int dpc_conv_wgrad(const dpc_conv_desc* d, const void* src, const void* dy, int32_t dy_ld,
                   float* part, int32_t* nsplit, dpc_stream_t stream);

/* ---- kernel selection, observable --------------------------------------------------------------------------------------------
 * dpc_conv_igemm / dpc_conv_wgrad pick one of several gfx950 kernels per shape (role-specialised loader/compute kernels,
 * staged-patch kernels, the generic implicit GEMM).  dpc_conv_plan returns the name of the kernel such a call WOULD launch
 * (the same dispatch code runs with the launch skipped; pointers are assumed 16-byte aligned): op = DPC_PLAN_IGEMM with
 * flags DPC_PLAN_ADDEND / DPC_PLAN_STATS for the optional operands, or DPC_PLAN_WGRAD with dy_ld.  dpc_last_kernel returns the
 * kernel the calling thread's most recent C-ABI call launched last.  Both write a NUL-terminated string (e.g.
 * "igemm_ws_kernel<true>", "wgrad2_kernel<T,NWM,NWN,true>[T=bf16 nwm=2 nwn=3 padded=1]") and return its length, or < 0. */
#define DPC_PLAN_IGEMM 0
#define DPC_PLAN_WGRAD 1
#define DPC_PLAN_ADDEND 1
#define DPC_PLAN_STATS 2
#define DPC_PLAN_ADDEND_MASK 4 /* dpc_conv_igemm_ex: gated addend */
#define DPC_PLAN_BNRED 8       /* dpc_conv_igemm_ex: fused BatchNorm-backward reduction */
int dpc_conv_plan(const dpc_conv_desc* d, int32_t op, int32_t flags, int32_t dy_ld, char* name, int32_t cap);
int dpc_last_kernel(char* name, int32_t cap);

/* CU carve-out for a concurrent collective: the kernels that launch one persistent workgroup per CU (layer1's patch kernel, the
 * loader/compute implicit GEMMs) shrink their grids by n workgroups (multiples of 8 are kept) for launches planned while the
 * setting is in force, so that RCCL's channel kernels find CUs during the overlapped gradient all-reduce (dpc/main.py:65's
 * DataParallel reduce, here one all-reduce per step).  Process-wide host state; returns the previous value.  dpc_conv_stats_rows
 * follows the setting: query it under the same value the launch sees. */
int dpc_set_reserved_cus(int32_t n);

/* Arithmetic of the f32 kernels' contractions (dtype_in == DPC_F32 in dpc_conv_igemm / dpc_conv_wgrad / dpc_gemm_nt_splitk):
 *   0  exact f32 MFMA chains (v_mfma_f32_32x32x2_f32, 157 TFLOP/s peak) -- the default, bitwise an fmaf chain;
 *   1  "bf16x6": each f32 operand split into three bf16 pieces in registers, the six piece products of 2^-16 |a||b| and more on
 *      the bf16 matrix pipe (the three left out are 2^-24 |a||b| and less), f32 accumulation -- f32-grade results (score within
 *      2e-4 of the reference's fp32 CPU path, north_star asks 1e-3) at up to 2.7x the f32 matrix rate.  Operands, activations and
 *      outputs stay f32 in HBM.  What a result is off by is the f32 accumulator's rounding, not the split: measured on an MI355X
 *      against f64 over reductions of 576, rel-L2 3.2e-7 .. 3.5e-7 on random operands (mode 0: 3.9e-7 .. 4.1e-7) and at most
 *      6.9e-7 of sum |a||b| per element on positive operands (mode 0: 3.2e-6 -- the fmaf chain rounds the accumulator after
 *      every product, the bf16 MFMA after every eight); one missing piece product would cost 2.3e-6 .. 3.8e-6
 *      (tests/x6_cases.py).  conv_halo_kernel<float,...> (f32 1x3x3 convs over 32 channels) has no bf16x6 form and runs mode 0
 *      under either setting.
 * Process-wide host state read when a launch is planned; returns the previous mode. */
int dpc_set_f32_matmul(int32_t mode);

/* Diagnostic co-tenant ("squatter"): n_wg workgroups of `waves` (1..4) waves that hold lds_bytes of LDS (multiple of 16, up to
 * 160 KB) for usec microseconds and do nothing (mode 0), LDS traffic over their own allocation (1), 16-byte loads over
 * scratch[scratch_bytes] (2) or VALU work (3).  where[n_wg] (optional) receives 0x80000000 | XCC_ID << 16 | HW_ID[15:0] per
 * workgroup.  Emulates, on ONE GPU, what the train step meets in a multi-GPU run -- RCCL's channel kernels during the overlapped
 * all-reduce that replaces nn.DataParallel's gradient reduce (dpc/main.py:65,229) -- and any side-stream neighbour: used by
 * tests/test_cotenant_gpu.py and scripts/probes/squat_probe.py, never by the training path. */
int dpc_diag_squat(int32_t n_wg, int32_t waves, int32_t lds_bytes, int32_t mode, int32_t usec, const void* scratch,
                   int64_t scratch_bytes, uint32_t* where, uint32_t* sink, dpc_stream_t stream);

/* ---- weight / operand repacking --------------------------------------------------
 * out[i0][i1][i2] (dtype_out, dense) = in[i0*s0 + i1*s1 + i2*s2] (f32).  Turns the
 * reference's [Co][Ci][kT][kH][kW] parameters (state_dict layout, §8b) into the
 * K-contiguous operand layouts above without touching the parameters themselves. */
int dpc_pack3d(const float* in, void* out, int32_t dtype_out, int32_t d0, int32_t d1, int32_t d2,
               int64_t s0, int64_t s1, int64_t s2, dpc_stream_t stream);
/* the same for a whole table of tensors in one launch (all per-step weight repacks of the conv stack): entry e is served by
 * blocks [block0[e], block0[e+1]) of a grid of total_blocks x 256 threads; the table lives in DEVICE memory. */
typedef struct dpc_pack_entry {
    const void* in;   /* f32 source */
    void* out;        /* destination, dtype_out elements, contiguous [d0][d1][d2] */
    int32_t d0, d1, d2, block0;
    int64_t s0, s1, s2;
} dpc_pack_entry;
int dpc_pack3d_multi(const dpc_pack_entry* table_dev, int32_t n_entries, int32_t total_blocks, int32_t dtype_out, dpc_stream_t stream);
/* out[i0*s0+i1*s1+i2*s2] (f32) = sum_{k<nsplit} part[k][i0][i1][i2]  (+ out if accumulate) */
int dpc_reduce_unpack(const float* part, int32_t nsplit, float* out, int32_t d0, int32_t d1, int32_t d2,
                      int64_t s0, int64_t s1, int64_t s2, int32_t accumulate, dpc_stream_t stream);
/* two bf16 matrices of one shape in one launch: outK[j][i] = inK[i][j] (in1 / out1 may be NULL); 16-byte aligned, ld % 8 == 0.
 * pred and feature_inf -> the K-contiguous operands of the score's backward products (autograd of dpc/model_3d.py:83). */
int dpc_transpose2d_bf16x2(const void* in0, const void* in1, int32_t ld_in, void* out0, void* out1, int32_t ld_out, int32_t rows,
                           int32_t cols, dpc_stream_t stream);
/* 2-D transpose/convert between element types: out[j][i] = in[i][j] */
int dpc_transpose2d(const void* in, int32_t dtype_in, int32_t ld_in, void* out, int32_t dtype_out, int32_t ld_out,
                    int32_t rows, int32_t cols, dpc_stream_t stream);

/* Stem: Conv3d(3,64,(1,7,7),s(1,2,2),p(0,3,3)) (resnet_2d3d.py:211) is run as a 1x4x4
 * stride-1 conv over a 2x2 space-to-depth image with 16 channels (12 used).
 * dpc_pack_input_s2d: block [BN][3][T][H][W] f32 NCDHW (dpc/model_3d.py:49-50) ->
 *   [BN][T][H/2][W/2][16]; channel = (sy*2+sx)*3 + c.
 * dpc_pack_stem_weight: [Co][3][1][7][7] f32 -> [Co][16 taps][16]; dpc_unpack_stem_wgrad the inverse for grads. */
int dpc_pack_input_s2d(const float* block, void* out, int32_t dtype_out, int32_t BN, int32_t T, int32_t H, int32_t W,
                       dpc_stream_t stream);
/* dpc_synthetic_input: one N(0,1) batch drawn on the device, written to block [BN][3][T][H][W] f32 and / or straight into the
 *   stem operand out [BN][T][H/2][W/2][16] (exactly what dpc_pack_input_s2d writes from that block); either pointer may be NULL.
 *   Element e of the block, q = e >> 2: (w0..w3) = Philox4x32-10(counter (q, draw_dev[0], 2 = DPC_PHILOX_STREAM_INPUT, 0),
 *   key (lo(seed), hi(seed))); for j in {0,1}: u = ((w_2j >> 8) + 1) 2^-24, v = (w_2j+1 >> 8) 2^-24, r = sqrtf(-2 logf(u)),
 *   th = 6.2831855f v, x[4q+2j] = r cosf(th), x[4q+2j+1] = r sinf(th).  The draw counter is read on the device, never written:
 *   dpc_counter_advance in front of it gives every replay of a captured step a new batch. */
int dpc_synthetic_input(float* block, void* out, int32_t dtype_out, int32_t BN, int32_t T, int32_t H, int32_t W, uint64_t seed,
                        const int32_t* draw_dev, dpc_stream_t stream);
/* dpc_synthetic_labels: the class labels of a synthetic batch drawn on the device into target [B] int64 (csrc/labels.hip).
 *   (w0..w3) = Philox4x32-10(counter (b >> 2, draw_dev[0], 3 = DPC_PHILOX_STREAM_LABEL, 0), key (lo(seed), hi(seed)));
 *   label[b] = ((uint64)w_(b & 3) * num_class) >> 32, in [0, num_class).  The draw counter is read on the device, never written,
 *   exactly like dpc_synthetic_input: with the same seed and counter the labels belong to that call's batch.
 *   DPC_ERR_ARG for null pointers, B <= 0 or num_class <= 0. */
int dpc_synthetic_labels(int64_t* target, int32_t B, int32_t num_class, uint64_t seed, const int32_t* draw_dev, dpc_stream_t stream);
int dpc_pack_stem_weight(const float* w, void* out, int32_t dtype_out, int32_t Co, dpc_stream_t stream);
int dpc_unpack_stem_wgrad(const float* part, int32_t nsplit, float* dw, int32_t Co, dpc_stream_t stream);

/* ---- batch norm with batch statistics (track_running_stats=False, dpc/model_3d.py:28;
 *      nn.BatchNorm3d at resnet_2d3d.py:55,59,93,97,212,243) -------------------------
 * finalize: partial sums [rows][2][C] -> mean, invstd, scale=gamma*invstd, shift=beta-mean*scale
 *           (f64 accumulation; count = elements per channel). */
int dpc_bn_finalize(const float* partials, int32_t rows, int32_t C, double count, const float* gamma,
                    const float* beta, float eps, float* mean, float* invstd, float* scale, float* shift,
                    dpc_stream_t stream);
/* y = act( x*scale+shift (+ res*rscale+rshift | + res) ), act = relu if relu!=0
 * (BasicBlock tail, resnet_2d3d.py:67-80,105-116) */
int dpc_bn_apply(const void* x, void* y, int32_t dtype, int64_t rows, int32_t C, const float* scale,
                 const float* shift, const void* res, const float* rscale, const float* rshift, int32_t relu,
                 uint8_t* mask, dpc_stream_t stream);
/* backward: dz = dy * (y>0 if relu); partial sums of dz and dz*xhat -> [rows][2][C].  The ReLU pattern comes
 * from `mask` (the byte-per-16-byte-unit sign mask dpc_bn_apply wrote: 1/16 of the bytes of y) or, when mask
 * is NULL, from y itself. */
int dpc_bn_bwd_reduce(const void* dy, const void* y, const uint8_t* mask, const void* x, int32_t dtype, int64_t rows, int32_t C,
                      const float* mean, const float* invstd, int32_t relu, float* partials, int32_t* prow,
                      dpc_stream_t stream);
/* sums [prow][2][C] -> dgamma , dbeta, and coefficients c1=sum_dz/count, c2=sum_dzxhat/count */
int dpc_bn_bwd_finalize(const float* partials, int32_t prow, int32_t C, double count, float* dgamma, float* dbeta,
                        float* coef, dpc_stream_t stream);
/* dx = gamma*invstd*(dz - c1 - xhat*c2); optionally also writes dz (residual branch grad) */
int dpc_bn_bwd_apply(const void* dy, const void* y, const uint8_t* mask, const void* x, int32_t dtype, int64_t rows, int32_t C,
                     const float* mean, const float* invstd, const float* gamma, const float* coef, int32_t relu,
                     void* dx, void* dz, dpc_stream_t stream);

/* ---- stem tail: BN+ReLU+MaxPool3d((1,3,3),s(1,2,2),p(0,1,1)) (resnet_2d3d.py:212-214,260-263) */
int dpc_bn_relu_maxpool_fwd(const void* x, int32_t dtype, int32_t NT, int32_t H, int32_t W, int32_t C,
                            const float* scale, const float* shift, void* y, uint8_t* argmax, dpc_stream_t stream);
/* dz (grad at the BN output, ReLU mask applied) from the pooled gradient and the saved argmax */
int dpc_maxpool_bwd(const void* dy, const uint8_t* argmax, int32_t dtype, int32_t NT, int32_t H, int32_t W, int32_t C,
                    void* dz, dpc_stream_t stream);

/* stem backward without materialising dz: BN backward whose incoming gradient is routed through the
 * max-pool on the fly (autograd of resnet_2d3d.py:260-263 in two passes instead of five) */
int dpc_pool_bn_bwd_reduce(const void* dy, const uint8_t* argmax, const void* x, int32_t dtype, int32_t NT, int32_t H,
                           int32_t W, int32_t C, const float* mean, const float* invstd, float* partials, int32_t* prow,
                           dpc_stream_t stream);
/* the same partial sums from the POOLED tensors only (y at an argmax position is the pooled value):
 * sum dz = sum_p dp[p], sum dz*xhat = sum_p dp[p]*(ypool[p]-beta)/gamma over valid argmax bytes */
int dpc_pooled_bn_bwd_reduce(const void* dy, const uint8_t* argmax, const void* ypool, int32_t dtype, int64_t rows,
                             int32_t C, const float* gamma, const float* beta, float* partials, int32_t* prow,
                             dpc_stream_t stream);
int dpc_pool_bn_bwd_apply(const void* dy, const uint8_t* argmax, const void* x, int32_t dtype, int32_t NT, int32_t H,
                          int32_t W, int32_t C, const float* mean, const float* invstd, const float* gamma,
                          const float* coef, void* dx, dpc_stream_t stream);
/* the stem's weight gradient straight from the gradient at the pooled output (throughput mode): pool_bn_bwd_apply's arithmetic
 * runs inside the weight-gradient kernel, the 2.7 GB full-resolution dz tensor is never written or re-read.  desc = the stem's
 * weight-gradient descriptor (space-to-depth form, dtype_in bf16, dtype_out f32).  part / nsplit as dpc_conv_wgrad (finish with
 * dpc_unpack_stem_wgrad).  DPC_ERR_UNSUPPORTED -> run dpc_pool_bn_bwd_apply + dpc_conv_wgrad instead. */
int dpc_stem_wgrad_fused(const dpc_conv_desc* d, const void* src_s2d, const void* raw, const void* dpool, const uint8_t* argmax,
                         const float* mean, const float* invstd, const float* gamma, const float* coef, float* part,
                         int32_t* nsplit, dpc_stream_t stream);

/* ---- temporal mean + ReLU split (dpc/model_3d.py:53-59) -----------------------------
 * x [B*N][T][SQ][D] -> feat_relu [N][B*SQ][D] (GRU input, time-major) and
 * feat_inf [B][P][SQ][D] (pre-ReLU, last P blocks, score operand). */
int dpc_tpool_split_fwd(const void* x, int32_t dtype, int32_t B, int32_t N, int32_t T, int32_t SQ, int32_t D,
                        int32_t P, void* feat_relu, void* feat_inf, dpc_stream_t stream);
int dpc_tpool_split_bwd(const void* x, const void* d_relu, const float* d_inf, int32_t dtype, int32_t B, int32_t N,
                        int32_t T, int32_t SQ, int32_t D, int32_t P, void* dx, dpc_stream_t stream);

/* ---- pieces around the fused ConvGRU recurrence (dpc_gru_chain_* below) -------------------
 * colsum of [M][D] (leading dimension ld) into out[D] (+= when accumulate): bias gradients of the ConvGRU / network_pred */
int dpc_colsum(const void* x, int32_t dtype, int32_t ld, int32_t M, int32_t D, float* out, int32_t accumulate,
               float* ws, int64_t ws_floats /* >= min(ceil(M/256), 64)*D; 64*D always suffices */, dpc_stream_t stream);

/* ---- contrastive loss head (dpc/main.py:178-185,213-218; utils/utils.py:38-55) -------
 * mask: closed form of dpc/model_3d.py:86-96, int8 [B][P][SQ][B][P][SQ] contiguous.
 * ce_topk: rows x cols logits (ld), target[i] = i (single-GPU closed form of process_output):
 *   result[0..3] = mean CE loss, top1, top3, top5; dscore (optional, dtype/ld given) = (softmax-onehot)/rows. */
int dpc_mask_gen(int8_t* mask, int32_t B, int32_t P, int32_t SQ, dpc_stream_t stream);
int dpc_ce_topk(const float* score, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result,
                void* dscore, int32_t dtype_d, int32_t ld_d, dpc_stream_t stream);
/* the same on bf16 logits with a bf16 gradient: the materialised score of a train step that does not return it (dpc/main.py:198-218
 * reads `score_` only through the loss).  cols % 8 == 0, ld % 8 == 0, 16-byte aligned rows, cols <= 16384; else DPC_ERR_UNSUPPORTED. */
int dpc_ce_topk_bf16(const void* score_bf16, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result,
                     void* dscore_bf16, int32_t ld_d, dpc_stream_t stream);

/* ---- fused score + loss (throughput mode, bf16 operands): the [R][R] score and its gradient never touch HBM --------
 * score_fwd: S = pred @ finf^T (dpc/model_3d.py:83) tile by tile; per row the running max / sum-exp / #{s > s_target}
 *   (target = the diagonal, the closed form of process_output on one GPU) -> row_ws[R][2] = (lse - s_target, rank),
 *   diag[R] = s_target, lse2[R] = (lse + ln R) log2 e for the backward; `score` (optional, f32 [R][R]) materialises S for a
 *   caller that reads it.  Follow with dpc_ce_finalize(row_ws, R, result) for loss / top-1/3/5 (dpc/main.py:217-218).
 * score_bwd: one of the two products of the backward with dS = (softmax(S) - onehot)/R recomputed from the operands:
 *   by_owner = 1, own = pred, oth = finf, othT = finf^T  -> partial slabs of d_pred = dS @ finf
 *   by_owner = 0, own = finf, oth = pred, othT = pred^T  -> partial slabs of d_finf = dS^T @ pred
 *   othT is [D][ldT] (ldT % 8 == 0, zero beyond column R).  Returns the number of [R][D] f32 slabs written to out_part
 *   (sum them with dpc_reduce_unpack).  dpc_score_ws_floats: workspace sizes (returns the number of slabs / column splits).
 * D must be 256 (or 32, the width-reduced test networks); other widths: DPC_ERR_UNSUPPORTED (use the materialised path). */
int dpc_score_ws_floats(int32_t R, int32_t D, int64_t* fwd_floats, int64_t* bwd_floats);
int dpc_score_fwd(const void* pred, const void* finf, int32_t R, int32_t D, float* diag, float* lse2, float* row_ws,
                  float* score, float* ws, dpc_stream_t stream);
int dpc_score_bwd(const void* own, const void* oth, const void* othT, int32_t ldT, int32_t R, int32_t D, const float* lse2,
                  int32_t by_owner, float* out_part, dpc_stream_t stream);
int dpc_ce_finalize(const float* row_ws, int32_t rows, float* result, dpc_stream_t stream);

/* ---- Adam with L2 weight decay on flat f32 buffers (dpc/main.py:80-81) --------------- */
int dpc_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
             float wd, float bias_corr1, float bias_corr2, float grad_scale, dpc_stream_t stream);

/* graph-capturable optimizer step (the whole train step is replayed as ONE hipGraph, dpc_amd/engine.py): the step
 * counter t and Adam's bias corrections 1-beta^t live in device memory.  step_advance: t += 1, bc = {1-b1^t, 1-b2^t}.
 * adam_dev == dpc_adam with the two corrections read from bias_corr_dev[0..1]. */
int dpc_step_advance(int32_t* step_dev, float* bias_corr_dev, double beta1, double beta2, dpc_stream_t stream);
int dpc_adam_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2, float eps,
                 float wd, const float* bias_corr_dev, float grad_scale, dpc_stream_t stream);
/* Adam with parameter groups (torch.optim.Adam over several groups, eval/test.py:76-84): ONE launch over the flat arenas driven by a
 * segment table in device memory.  Segments are sorted and non-overlapping, begin / end in floats and multiples of 4 (the arenas keep
 * every tensor 16-byte aligned, so a 16-byte access never straddles two parameters); floats outside every segment are padding and
 * are never touched.  active = 0: a frozen segment -- g, p, m, v are neither read nor written.  An active segment with lr = 0
 * still updates m and v, as torch does.  Betas, eps, the device bias-correction pair and grad_scale are common to all segments and
 * mean what they mean for dpc_adam_dev, whose per-element arithmetic this is.  n % 4 == 0, 16-byte aligned arenas,
 * 1 <= n_segments <= DPC_ADAM_MAX_SEGMENTS; the table's contents are validated by whoever builds it (dpc_amd/engine.py). */
#define DPC_ADAM_MAX_SEGMENTS 512
typedef struct dpc_adam_segment {
    int64_t begin, end;      /* floats, multiples of 4 */
    float lr, weight_decay;
    int32_t active;          /* 0 = frozen */
    int32_t reserved;
} dpc_adam_segment;
int dpc_adam_groups_dev(float* p, const float* g, float* m, float* v, int64_t n, const dpc_adam_segment* segments_dev,
                        int32_t n_segments, double beta1, double beta2, float eps, const float* bias_corr_dev, float grad_scale,
                        dpc_stream_t stream);
/* ---- gradient guard (csrc/grad_guard.hip): global-norm clip and non-finite skip of the fused step, decided on the device so that a
 * replayed hipGraph step needs no host code between backward and update.  The verdict lives in a 32-byte device record:
 *   grad_sumsq   partials[0..DPC_GRAD_PARTIALS) = f64 sums of g^2 (every element widened before it is squared) over [0, n), or, with
 *                a dpc_adam_segment table, over its active segments only (gaps and inactive segments are never loaded).  Every slot
 *                is written by every call.  No atomics; the work split depends on n alone and every combine has a fixed order, so the
 *                same arena gives the same bits on every run and every rank.  n % 4 == 0, g 16-byte aligned; with a table,
 *                1 <= n_segments <= DPC_ADAM_MAX_SEGMENTS.
 *   grad_verdict one workgroup adds the partials in index order and writes sumsq, norm = (float)sqrt(sumsq) and, judged on the f64 sum,
 *                  finite, max_norm > 0 : coef = min(1, max_norm / (norm + 1e-6)) (torch's clip_grad_norm_; f64, rounded once),
 *                                         n_clipped += coef < 1
 *                  finite, max_norm <= 0: coef = 1
 *                  non-finite           : skip_nonfinite ? (skip = 1, coef = 0, n_skipped += 1) : (skip = 0, coef = 1)
 *   step_advance_gated  dpc_step_advance unless state->skip
 *   adam_dev_ex / adam_groups_dev_ex  dpc_adam_dev / dpc_adam_groups_dev with an optional state: the gradient scale becomes
 *                grad_scale * state->coef (one f32 product); with state->skip the launch touches none of p, m, v.  A null state, or
 *                coef == 1 and skip == 0, gives the bits of the plain entries.
 *   grad_scale   g *= state->coef in place over the live floats; nothing when state->skip (dpc_amd.optim.clip_grad_norm_). */
#define DPC_GRAD_PARTIALS 1024
typedef struct dpc_grad_state {
    double sumsq;                 /* sum of g^2 over the live floats, f64 */
    float norm;                   /* (float)sqrt(sumsq) */
    float coef;                   /* factor applied to the gradient this step */
    int32_t skip;                 /* 1: this step's update is suppressed */
    int32_t n_skipped, n_clipped; /* running counts since the state was zeroed */
    int32_t reserved;
} dpc_grad_state;
int dpc_grad_sumsq(const float* g, int64_t n, const dpc_adam_segment* segments_dev, int32_t n_segments, double* partials,
                   dpc_stream_t stream);
int dpc_grad_verdict(const double* partials, int32_t n_partials, double max_norm, int32_t skip_nonfinite, dpc_grad_state* state_dev,
                     dpc_stream_t stream);
int dpc_step_advance_gated(int32_t* step_dev, float* bias_corr_dev, double beta1, double beta2, const dpc_grad_state* state_dev,
                           dpc_stream_t stream);
int dpc_adam_dev_ex(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2, float eps,
                    float wd, const float* bias_corr_dev, float grad_scale, const dpc_grad_state* state_dev, dpc_stream_t stream);
int dpc_adam_groups_dev_ex(float* p, const float* g, float* m, float* v, int64_t n, const dpc_adam_segment* segments_dev,
                           int32_t n_segments, double beta1, double beta2, float eps, const float* bias_corr_dev, float grad_scale,
                           const dpc_grad_state* state_dev, dpc_stream_t stream);
int dpc_grad_scale(float* g, int64_t n, const dpc_adam_segment* segments_dev, int32_t n_segments, const dpc_grad_state* state_dev,
                   dpc_stream_t stream);
/* ---- gradient accumulation in front of the fused step (csrc/grad_accum.hip): several micro-batches per optimizer step.  `acc` is a
 * second f32 arena of the size and alignment of the gradient arena `g`, +0 at the start of every cycle:
 *   DPC_ACCUM_ADD     acc[i] = acc[i] + g[i]; g is only read.
 *   DPC_ACCUM_FINISH  g[i] = (acc[i] + g[i]) * scale, then acc[i] = +0.0f: one f32 add, rounded, then one f32 multiply, rounded
 *                     (never an fma).  scale = float32(1 / N), formed on the host.  Every cycle ends with acc back at +0, so there is
 *                     no "store" mode: every non-final micro-batch is the same launch with the same arguments.
 * Only the floats of [begin, end) (both multiples of 4, inside [0, n)) are touched; with a dpc_adam_segment table, of those only the
 * 16-byte units inside an active segment (the live-unit rule of dpc_grad_sumsq): every other unit is neither loaded nor stored, in
 * either arena.  One writer per value, no atomics.  begin == end is a successful no-op.  DPC_ERR_ARG, and no launch, for: a null or
 * misaligned arena, acc == g, n <= 0 or n % 4, begin / end not multiples of 4, begin > end, end > n, another mode, a non-finite scale,
 * a table with a count outside 1..DPC_ADAM_MAX_SEGMENTS. */
#define DPC_ACCUM_ADD 0
#define DPC_ACCUM_FINISH 1
int dpc_grad_accumulate(float* acc, float* g, int64_t n, int64_t begin, int64_t end, const dpc_adam_segment* segments_dev,
                        int32_t n_segments, int32_t mode, float scale, dpc_stream_t stream);
/* ---- EMA of the parameters inside the fused step (csrc/loss.hip): dpc_adam_dev_ex / dpc_adam_groups_dev_ex (state_dev nullable, as
 * there) with one more f32 arena, `ema`, updated by the thread that has just updated the 16-byte unit of p:
 *     e += (1 - d) * (p_new - e),   d = min(decay, (float)(1 + t) / (float)(10 + t)),   t = step_dev[0]
 * in f32 throughout (1 - d included).  t is the optimizer-step count AFTER this step's advance (dpc_step_advance[_gated] runs first);
 * the warm-up term is always on: without it a decay of 0.999 reports the initial weights for thousands of steps.  The lerp form has
 * e == p as a fixed point bit for bit.  p, m, v get the bits the _ex entries give them.  Nothing of ema is loaded or stored where
 * the update loads and stores nothing: a skipped step (state_dev->skip), an inactive segment, a gap of the segment table.
 * ema: non-null, 16-byte aligned, not p; step_dev non-null; 0 < decay < 1; else DPC_ERR_ARG.  No launch beside the update's own.
 *   arena_swap   exchanges a[0..n) and b[0..n) in place, 16 bytes per lane, as bits (NaN payloads survive): how evaluation sees the
 *                averaged weights while every pointer into the parameter arena -- views, pack tables, captured graphs -- stays valid.
 *                n % 4 == 0, both 16-byte aligned, a != b.  Capturable. */
int dpc_adam_dev_ema(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2, float eps,
                     float wd, const float* bias_corr_dev, float grad_scale, const dpc_grad_state* state_dev, float* ema,
                     const int32_t* step_dev, float decay, dpc_stream_t stream);
int dpc_adam_groups_dev_ema(float* p, const float* g, float* m, float* v, int64_t n, const dpc_adam_segment* segments_dev,
                            int32_t n_segments, double beta1, double beta2, float eps, const float* bias_corr_dev, float grad_scale,
                            const dpc_grad_state* state_dev, float* ema, const int32_t* step_dev, float decay, dpc_stream_t stream);
int dpc_arena_swap(float* a, float* b, int64_t n, dpc_stream_t stream);
/* ---- per-step learning-rate schedule inside the fused step (csrc/loss.hip).  k = completed optimizer steps before this one
 * (step_dev[0] before the advance; the index LambdaLR passes its lambda).  Every group steps with lr_group * mult(k); mult in double,
 * rounded to f32 once:
 *     k < W                : (k + 1) / W                                          W = warmup_steps >= 0
 *     else, x = min(1, (k - W) / (T - W)), T = total_steps, m0 = min_mult in [0, 1]:
 *       DPC_LR_CONSTANT    : 1
 *       DPC_LR_COSINE      : m0 + (1 - m0) * 0.5 * (1 + cos(pi x))    (x >= 1: m0)
 *       DPC_LR_LINEAR      : m0 + (1 - m0) * (1 - x)                  (x >= 1: m0)
 *       DPC_LR_MULTISTEP   : gamma ^ #{milestones <= k}   (steps, strictly ascending, non-negative, at most 8; 0 < gamma <= 1)
 * cosine and linear need T > W.  The descriptor is host memory, validated by the launcher (DPC_ERR_ARG, nothing launched) and passed
 * to the kernel by value: no device table, no upload.
 *   step_advance_sched  dpc_step_advance (state_dev null) or dpc_step_advance_gated (state_dev given) -- step and bias_corr get the
 *                same bits -- and lr_state_dev = {mult(k), k}, plain stores of one thread.  On state_dev->skip nothing is written.
 *   adam_dev_sched / adam_groups_dev_sched   the _ema entries with the step size (lr * lr_state_dev->mult) / bias_corr1, the product
 *                in f32 first; lr_state_dev non-null.  ema and step_dev may be null (both): no average, `decay` ignored. */
#define DPC_LR_CONSTANT 0
#define DPC_LR_COSINE 1
#define DPC_LR_LINEAR 2
#define DPC_LR_MULTISTEP 3
#define DPC_LR_MAX_MILESTONES 8
typedef struct dpc_lr_schedule {
    int32_t kind;           /* DPC_LR_* */
    int32_t warmup_steps;
    int32_t total_steps;    /* cosine, linear */
    int32_t n_milestones;   /* multistep */
    double min_mult;        /* cosine, linear */
    double gamma;           /* multistep */
    int32_t milestones[DPC_LR_MAX_MILESTONES];
} dpc_lr_schedule;          /* 64 bytes */
typedef struct dpc_lr_state {
    float mult;             /* mult(k) of the last step that was not skipped */
    int32_t k;
    int32_t reserved[2];
} dpc_lr_state;             /* 16 bytes, device memory */
int dpc_step_advance_sched(int32_t* step_dev, float* bias_corr_dev, double beta1, double beta2, const dpc_grad_state* state_dev,
                           const dpc_lr_schedule* schedule, dpc_lr_state* lr_state_dev, dpc_stream_t stream);
int dpc_adam_dev_sched(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2, float eps,
                       float wd, const float* bias_corr_dev, float grad_scale, const dpc_grad_state* state_dev, float* ema,
                       const int32_t* step_dev, float decay, const dpc_lr_state* lr_state_dev, dpc_stream_t stream);
int dpc_adam_groups_dev_sched(float* p, const float* g, float* m, float* v, int64_t n, const dpc_adam_segment* segments_dev,
                              int32_t n_segments, double beta1, double beta2, float eps, const float* bias_corr_dev, float grad_scale,
                              const dpc_grad_state* state_dev, float* ema, const int32_t* step_dev, float decay,
                              const dpc_lr_state* lr_state_dev, dpc_stream_t stream);
/* ---- the other update rules of the fused step (csrc/optim_kinds.hip).  Betas, eps, bias_corr_dev, grad_scale, state_dev (the
 * guard's record, nullable), ema / step_dev / decay (the average, nullable as a pair) and lr_state_dev (the schedule's record,
 * nullable: multiplier 1) mean what they mean for the _sched entries; lr_eff = lr * lr_state_dev->mult, the f32 product first.
 * With gg = g * grad_scale * coef,  m <- b1 m + (1 - b1) gg,  v <- b2 v + (1 - b2) gg^2  (no wd * p in the gradient):
 *   adamw_dev / adamw_groups_dev   torch.optim.AdamW:  p <- p (1 - lr_eff wd), a product rounded on its own as param.mul_ does, then
 *                p <- p - (lr_eff / bc1) m / (sqrt(v) / sqrt(bc2) + eps) as Adam; with wd = 0 p, m, v (and ema) get the bits of the
 *                Adam entries.  One launch, as Adam; all four arenas 16-byte aligned.
 *   LAMB (You et al. 2020, bias-corrected), three launches:  u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd p;  per segment
 *                r = |p| / |u| when the segment is adaptive and both norms are > 0, else 1;  p <- p - lr_eff r u.
 *     lamb_build_chunks (host)  validates a host segment table (sorted, non-overlapping, multiples of 4 inside [0, n), lr, wd >= 0),
 *                cuts every ACTIVE segment into chunks of at most DPC_LAMB_CHUNK floats that never cross a segment, in table order,
 *                and fills each segment's chunk0 / n_chunks.  Returns the number of chunks.  The work split of the launches below is
 *                this table and nothing else.
 *     lamb_moments  writes m, v in place over the chunks, forms u and writes partials[2c] = sum p^2, partials[2c + 1] = sum u^2 of
 *                chunk c in f64 (every element widened before it is squared); p is only read.
 *     lamb_ratios   one dpc_lamb_record per segment: the segment's pairs added in chunk order in f64, the norms, and the ratio
 *                formed in f64 and rounded once.  An inactive segment: sums 0, ratio 1.  adapt = 0: ratio 1, norms still reported.
 *     lamb_apply    recomputes u from the new m, v and the old p (the same device function: the same bits) and does p -= lr_eff r u,
 *                then the average's lerp by the thread that wrote p.
 *   No atomics, one writer per value, every combine in a fixed order.  On state_dev->skip none of the three loads or stores
 *   anything, the records included.  Floats outside every chunk (gaps, inactive segments) are never loaded or stored in any arena. */
#define DPC_LAMB_CHUNK 4096
typedef struct dpc_lamb_segment {
    int64_t begin, end;       /* floats, multiples of 4 */
    float lr, weight_decay;
    int32_t active;           /* 0 = frozen */
    int32_t adapt;            /* 0 = no trust ratio (r = 1) */
    int32_t chunk0, n_chunks; /* filled by dpc_lamb_build_chunks */
    int32_t reserved[2];
} dpc_lamb_segment;           /* 48 bytes */
typedef struct dpc_lamb_chunk {
    int64_t begin;            /* floats */
    int32_t len;              /* floats, a multiple of 4, <= DPC_LAMB_CHUNK */
    int32_t seg;
} dpc_lamb_chunk;             /* 16 bytes */
typedef struct dpc_lamb_record {
    double sum_p2, sum_u2;
    float pnorm, unorm, ratio;
    int32_t reserved;
} dpc_lamb_record;            /* 32 bytes */
int dpc_adamw_dev(float* p, const float* g, float* m, float* v, int64_t n, float lr, double beta1, double beta2, float eps,
                  float wd, const float* bias_corr_dev, float grad_scale, const dpc_grad_state* state_dev, float* ema,
                  const int32_t* step_dev, float decay, const dpc_lr_state* lr_state_dev, dpc_stream_t stream);
int dpc_adamw_groups_dev(float* p, const float* g, float* m, float* v, int64_t n, const dpc_adam_segment* segments_dev,
                         int32_t n_segments, double beta1, double beta2, float eps, const float* bias_corr_dev, float grad_scale,
                         const dpc_grad_state* state_dev, float* ema, const int32_t* step_dev, float decay,
                         const dpc_lr_state* lr_state_dev, dpc_stream_t stream);
int dpc_lamb_build_chunks(dpc_lamb_segment* segments, int32_t n_segments, int64_t n, dpc_lamb_chunk* chunks, int32_t capacity);
int dpc_lamb_moments(const float* p, const float* g, float* m, float* v, int64_t n, const dpc_lamb_segment* segments_dev,
                     int32_t n_segments, const dpc_lamb_chunk* chunks_dev, int32_t n_chunks, double beta1, double beta2, float eps,
                     const float* bias_corr_dev, float grad_scale, const dpc_grad_state* state_dev, double* partials,
                     dpc_stream_t stream);
int dpc_lamb_ratios(const dpc_lamb_segment* segments_dev, int32_t n_segments, const double* partials, int32_t n_chunks,
                    const dpc_grad_state* state_dev, dpc_lamb_record* records_dev, dpc_stream_t stream);
int dpc_lamb_apply(float* p, const float* m, const float* v, int64_t n, const dpc_lamb_segment* segments_dev, int32_t n_segments,
                   const dpc_lamb_chunk* chunks_dev, int32_t n_chunks, float eps, const float* bias_corr_dev,
                   const dpc_grad_state* state_dev, const dpc_lamb_record* records_dev, float* ema, const int32_t* step_dev,
                   float decay, const dpc_lr_state* lr_state_dev, dpc_stream_t stream);
/* counter_dev[0] += 1 on the stream: the dropout draw counter (one draw per train-mode forward; the `step_dev` the recurrence and
 * the classifier head key their Philox masks on), graph-capturable like dpc_step_advance */
int dpc_counter_advance(int32_t* counter_dev, dpc_stream_t stream);
/* f32 [rows][cols] window copy between two leading dimensions (ConvGRU gate-gradient scatter) */
int dpc_copy2d_f32(const float* src, int64_t src_ld, float* dst, int64_t dst_ld, int32_t rows, int32_t cols, dpc_stream_t stream);
/* the same for a device-resident table of windows in ONE launch (the nine gate slices of the ConvGRU's weight / bias gradients,
 * backbone/convrnn.py:13-15: [D][2D] parameters filled from batched [3D][D] GEMM results); block0 = first workgroup of an entry */
typedef struct dpc_copy2d_entry {
    const float* src;
    float* dst;
    int64_t src_ld, dst_ld;
    int32_t rows, cols, block0, pad;
} dpc_copy2d_entry;
int dpc_copy2d_multi(const dpc_copy2d_entry* table_dev, int32_t n_entries, int32_t total_blocks, dpc_stream_t stream);

/* ---- ConvGRU dropout (nn.Dropout(p=0.1) on the carried hidden state, backbone/convrnn.py:39,59,78) ---------------
 * mask[i] = 1/(1-p) w.p. 1-p else 0: Philox4x32-10, key = seed, counter = (i/4, step_dev[0], stream id (0 here; 1 = the LC head's dropout), 0), word i%4,
 * keep iff (word >> 8) >= round(p * 2^24).  One launch draws the masks of all recurrence steps of one train step. */
int dpc_dropout_mask(float* mask, int64_t n, float p, uint64_t seed, const int32_t* step_dev, dpc_stream_t stream);

/* ---- the whole ConvGRU aggregate / predict recurrence in one launch, and its backward in one more --------------
 * (dpc/model_3d.py:62-72: agg over the first N-P blocks, then P x {network_pred, agg step}; backbone/convrnn.py:24-34,76-79;
 *  network_pred dpc/model_3d.py:36-40).  Rows m = (b, s) of the [B*SQ][D] state are independent sequences (1x1 convolutions):
 *  a workgroup owns 32 rows for all steps.  T = compute dtype (dtype field); all buffers are caller-owned.
 *  P = 0: aggregation only (n_steps = n_agg), the classifier head of eval/model_3d_lc.py reads H_all[n_steps].
 * dpc_gru_pack repacks the five f32 parameters (gate weights [D][2D] = [x half | h half], network_pred [D][D]) into the
 *  fragment-major operand layout both kernels stream (`packed`: 16 * D * D elements of T); call it once per optimizer step.
 * Dropout on the carried state: drop_masks != NULL -> explicit pre-scaled keep masks [n_steps][M][D]; else step_dev != NULL ->
 *  Philox4x32-10 keyed on (seed, step_dev[0]) generated in the kernel (the bits dpc_dropout_mask writes); else none (eval). */
typedef struct dpc_gru_chain_desc {
    int32_t dtype, M, D, SQ, P, n_agg, n_steps, reserved;
    float p_drop;
    uint32_t reserved2;
    uint64_t seed;
    const int32_t* step_dev;
    const float* drop_masks;
    const void* packed;
    const float *bias_u, *bias_r, *bias_o, *bias_1, *bias_2;
    void* X_all;   /* [n_steps][M][D] T   in: relu'd features of the n_agg aggregation steps; out: relu(pred_i) for the others */
    void* H_all;   /* [n_steps+1][M][D] T  [0] = h_0 (read), [s+1] = state after step s (written) */
    void* HR_all;  /* [n_steps][M][D] T    h * r */
    float *U_all, *R_all, *O_all;  /* [n_steps][M][D] f32 gate activations (saved for the backward) */
    void* P1_all;  /* [P][M][D] T          relu(W1 h + b1) */
    void* pred;    /* [B][P][SQ][D] T      predictions, rows in the score's order */
    /* backward only */
    const float* d_pred;  /* [B][P][SQ][D] f32   d loss / d pred */
    void* G_all;          /* [n_steps][M][3D] T  pre-activation gradients [u | r | o] (operands of the batched weight gradients) */
    void *dP1, *dP2;      /* [P][M][D] T         gradients at the pre-activations of network_pred */
    float* d_x;           /* [n_agg][M][D] f32   gradient w.r.t. the aggregation inputs */
    float* ws;            /* [2][M][D] f32       scratch of the backward kernel */
    const float* d_hlast; /* optional [M][D] f32  d loss / d (last state): seeds the backward (P = 0: the LC classifier, eval/model_3d_lc.py:58-60) */
} dpc_gru_chain_desc;
int dpc_gru_pack(const float* w_update, const float* w_reset, const float* w_out, const float* w_pred0, const float* w_pred2,
                 int32_t D, int32_t dtype, void* packed, dpc_stream_t stream);
int dpc_gru_chain_fwd(const dpc_gru_chain_desc* c, dpc_stream_t stream);
int dpc_gru_chain_bwd(const dpc_gru_chain_desc* c, dpc_stream_t stream);

/* ---- downstream classifier LC (eval/model_3d_lc.py:12-65) ------------------------------------------
 * Shares the backbone and ConvGRU kernels; what differs:
 *  - the backbone's BatchNorm3d layers track running statistics (model_3d_lc.py:27-29): dpc_bn_finalize_running is
 *    dpc_bn_finalize + the momentum update of running_mean / running_var (unbiased) in train mode, dpc_bn_eval_coeffs builds
 *    scale / shift from the running buffers in eval mode;
 *  - relu_tpool: feat[n][(b,s)][d] = mean_t relu(x[b*N+n][t][s][d])  (ReLU BEFORE the temporal mean, model_3d_lc.py:52-54)
 *    and its backward dx = (x > 0) d_feat / T;
 *  - the head (model_3d_lc.py:58-64, eval/test.py:244-255): spatial mean of the last ConvGRU state -> BatchNorm1d ->
 *    Dropout(p) -> Linear -> CrossEntropyLoss + top-1, forward and backward.  result[0..1] = mean loss, accuracy.
 *    dpc_lc_head_bwd takes the Dropout keep values from where the forward took them (drop_mask, else the Philox draw of
 *    (seed, step_dev[0]), else 1): call it with the descriptor of the train-mode forward, before step_dev advances.
 *    It starts from whatever `dlogits` holds: the forward leaves the mean cross-entropy's gradient there; a caller that
 *    differentiates something else (torch autograd through LC.forward) overwrites it with its d loss / d logits and passes its
 *    d loss / d context in d_bn_out. */
int dpc_bn_finalize_running(const float* partials, int32_t rows, int32_t C, double count, const float* gamma, const float* beta,
                            float eps, float* mean, float* invstd, float* scale, float* shift, float* running_mean,
                            float* running_var, int64_t* num_batches_tracked, float momentum, dpc_stream_t stream);
int dpc_bn_eval_coeffs(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float eps,
                       int32_t C, float* mean, float* invstd, float* scale, float* shift, dpc_stream_t stream);
int dpc_relu_tpool_fwd(const void* x, int32_t dtype, int32_t B, int32_t N, int32_t T, int32_t SQ, int32_t D, void* feat,
                       dpc_stream_t stream);
int dpc_relu_tpool_bwd(const void* x, const float* d_feat, int32_t dtype, int32_t B, int32_t N, int32_t T, int32_t SQ, int32_t D,
                       void* dx, dpc_stream_t stream);
typedef struct dpc_lc_head_desc {
    int32_t dtype, B, SQ, D, num_class, train;
    float p_drop, momentum, eps;
    uint32_t reserved;
    uint64_t seed;
    const int32_t* step_dev;      /* Philox step counter (train, when drop_mask is NULL) */
    const float* drop_mask;       /* optional explicit pre-scaled keep mask [B][D] */
    const void* h_last;           /* [B*SQ][D] T: last ConvGRU state */
    const float *bn_weight, *bn_bias;
    float *bn_running_mean, *bn_running_var;
    int64_t* bn_num_batches;      /* optional */
    const float *fc_weight, *fc_bias;   /* [num_class][D], [num_class] */
    const int64_t* target;        /* [B] class indices */
    float *ctx, *xhat, *bn_out, *y;     /* [B][D] f32: spatial mean, normalised, BN output (= LC.forward's `context`), after dropout */
    float* stat;                  /* [2][D] mean / invstd used */
    float *logits, *dlogits;      /* [B][num_class]: LC.forward's `output`; d loss / d logits */
    float *row_ws, *result;       /* [B][2], [2] */
    /* backward */
    float *g_fc_weight, *g_fc_bias, *g_bn_weight, *g_bn_bias;
    float* dctx;                  /* [B][D] scratch */
    float* d_hlast;               /* [B*SQ][D] f32: seed of dpc_gru_chain_bwd */
    const float* d_bn_out;        /* optional [B][D] f32: an upstream gradient at bn_out (LC.forward's `context`, the BatchNorm1d output
                                     before Dropout), added to dy * keep ahead of the BatchNorm backward; NULL = none */
} dpc_lc_head_desc;
int dpc_lc_head_fwd(const dpc_lc_head_desc* c, dpc_stream_t stream);
int dpc_lc_head_bwd(const dpc_lc_head_desc* c, dpc_stream_t stream);

/* ---- GPU-side input pipeline (dpc/dataset_3d.py:85-111, utils/augmentation.py) ---------------------
 * frames u8 [B][F][H0][W0][3] (decoded RGB, HWC) -> block f32 [B][N][3][SL][H][W] (the DPC_RNN / LC input) and / or the stem's
 * space-to-depth operand (what dpc_pack_input_s2d writes), applying per clip: frame sampling frame(n, sl) = start + (n*SL + sl)*ds,
 * the crop box (x1, y1) of RandomCrop / RandomSizedCrop, RandomHorizontalFlip (flip), per-frame RandomGray channel choice
 * (gray [B][N*SL], -1 = keep colour; NULL = none), Scale with NEAREST interpolation (xtab [W] / ytab [H]: device tables output
 * column / row -> column / row inside the crop_w x crop_h crop box, produced by PIL on the host; NULL = no scaling),
 * ToTensor (/255) and Normalize(mean3, std3; HOST arrays of 3 floats).  flip: 0 none, 1 after crop + scale (k400 recipe),
 * 2 of the full frame before the crop (ucf101 recipe, dpc/main.py:114-123).  The random draws stay on the host (a handful of
 * integers per clip; dpc_amd/data.py mirrors the reference's calls of `random` / `np.random`).
 * dpc_frames_to_input_ex adds, bit-exact against PIL / torchvision's PIL path:
 *  - dpc_resample: PIL's separable resampling (Image.resize BILINEAR / NEAREST / ..., 8 bits per channel) as per-clip tables --
 *    output column x reads source columns x1 + xb[x][0] + [0, xb[x][1]) of the crop box with the 22-bit fixed-point coefficients
 *    xk[x][.]; rows likewise; horizontal pass rounded to 8 bits first (RandomSizedCrop's resize, utils/augmentation.py:144-196);
 *  - dpc_frame_jitter: ColorJitter (utils/augmentation.py:253-351), one draw per frame: order[k] = the k-th step of the shuffled
 *    chain (0 brightness, 1 contrast, 2 saturation, 3 hue, 255 none), factor[0..2] = brightness / contrast / saturation factors,
 *    hue_shift = np.uint8(hue_factor * 255).  Needs u8_ws (B*N*SL*H*W*3 bytes) and lsum_ws (B*N*SL uint64). */
typedef struct dpc_clip_aug {
    int32_t start, x1, y1, flip;
} dpc_clip_aug;
int dpc_frames_to_input(const uint8_t* frames, int32_t B, int32_t F, int32_t H0, int32_t W0, const dpc_clip_aug* aug,
                        const int8_t* gray, int32_t N, int32_t SL, int32_t ds, int32_t H, int32_t W, const int32_t* xtab,
                        const int32_t* ytab, int32_t crop_w, int32_t crop_h, const float* mean3, const float* std3, float* block,
                        void* s2d, int32_t dtype_s2d, dpc_stream_t stream);
typedef struct dpc_resample {
    const int32_t *xb, *xk;   /* device: [B][W][2] (first source column, taps), [B][W][ksx] */
    const int32_t *yb, *yk;   /* device: [B][H][2], [B][H][ksy] */
    int32_t ksx, ksy;
} dpc_resample;
typedef struct dpc_frame_jitter {
    float factor[3];
    int32_t hue_shift;
    uint8_t order[4];
} dpc_frame_jitter;
int dpc_frames_to_input_ex(const uint8_t* frames, int32_t B, int32_t F, int32_t H0, int32_t W0, const dpc_clip_aug* aug,
                           const int8_t* gray, int32_t N, int32_t SL, int32_t ds, int32_t H, int32_t W, const dpc_resample* rs,
                           const dpc_frame_jitter* jitter, uint8_t* u8_ws, uint64_t* lsum_ws, const float* mean3, const float* std3,
                           float* block, void* s2d, int32_t dtype_s2d, dpc_stream_t stream);

/* ---- frames resident in HBM (dpc_amd/data.py FrameStore, `--resident`) -------------------------------------------------------
 * dpc_store_to_input: dpc_frames_to_input_ex on the packed store u8 [total_frames][H0][W0][3] (videos of any length back to back):
 *   clip b reads frame clip_first[b] + aug[b].start + (n*SL + sl)*ds, addressed in 64-bit arithmetic (a store exceeds 2^31 bytes).
 *   clip_first int64 [B] and aug are DEVICE tables nobody can check without a host round trip: dpc_draw_recipe writes them from
 *   the store's offsets.  Same launches as dpc_frames_to_input_ex (three with jitter, one without).
 * dpc_draw_recipe: the random draws of one batch of the pre-training recipes (dpc/main.py:114-132) on the device, written as
 *   exactly the tables the gather reads: aug [B], clip_first [B], gray [B][N*SL], jitter [B][N*SL], xb / yb [B][size][2],
 *   xk / yk [B][size][KS] (zero beyond a row's taps).  Clip b reads video video_idx[(step_dev ? step_dev[0] - 1 : 0) * B + b],
 *   whose frames are [offsets[v], offsets[v + 1]) of the store (the caller has dropped videos with no legal start).
 *   Uniform number `slot` of clip b is u = (w >> 8) 2^-24 with w = word slot & 3 of
 *   philox4x32_10(slot >> 2, draw_dev[0], DPC_PHILOX_STREAM_AUG, b; lo(seed), hi(seed)), or uniforms[b * DPC_RECIPE_SLOTS(N*SL) +
 *   slot] when `uniforms` (f32, device) is given: a pure function of (seed, counter, clip, slot) whichever branch is taken.
 *   randint(0, n) = floor(u (n + 1)); uniform(a, b) = a + (b - a) u in double.  Slots (a rejected crop attempt keeps its five):
 *     0 start in [0, vlen - N*SL*ds)      1 flip (< 1/2)      2 RandomSizedCrop's p      3 RandomCrop x1      4 RandomCrop y1
 *     5 ColorJitter's p                   6, 7 unused
 *     8 + 5a + {0 area U(0.5, 1), 1 aspect U(3/4, 4/3), 2 swap (< 1/2), 3 x1, 4 y1}    attempt a = 0 .. 9
 *     58 + 9f + {0 gray (< gray_p), 1 gray channel floor(3u), 2 brightness, 3 contrast, 4 saturation, 5 hue,
 *                6, 7, 8 the Fisher-Yates steps i = 3, 2, 1 (j = floor(u (i + 1)), swap i and j) of the chain}    frame f
 *   The double arithmetic is that of data.resample_tables / data._draw_sized_crop, unfused (data.recipe_from_uniforms is the host
 *   statement of the same decisions; the two agree bit for bit).  sized_p >= 0: RandomSizedCrop(size, BILINEAR, p = sized_p) (its
 *   ten attempts, the Scale + CenterCrop fallback, CenterCrop(size) when p fails); sized_p < 0: RandomCrop(crop) and, when crop !=
 *   size, the NEAREST Scale as the device index table scale_tab int32 [size] (data.nearest_tables; NULL = identity).  gray_p < 0 /
 *   jitter_p < 0: the recipe has no RandomGray / ColorJitter; a jitter range of 0 leaves that step out of the chain.  flip_code:
 *   what aug.flip holds when the flip is drawn (1 after the crop, 2 before it; 0 = the recipe never flips).  One jitter draw per
 *   frame (consistent=False), which is what both pre-training recipes use.
 *   KS >= 2 ceil(max(W0, H0) / size) + 1, B <= 1024, size <= 1024.
 * dpc_draw_recipe_ex: dpc_draw_recipe (same slots, same Philox stream and counter block, same arithmetic) with the pieces the
 *   classifier's recipes (eval/test.py:161-176) need; dpc_draw_recipe is this entry with flags = 0 and the three tables NULL.
 *   recipe->flags (undefined bits: DPC_ERR_ARG):
 *     DPC_RECIPE_JITTER_CONSISTENT   ColorJitter(consistent=True), utils/augmentation.py:330-333: when the jitter `p` draw (slot 5)
 *       passes, ONE get_params draw from FRAME 0's slots 58 + {2 .. 8}, copied to every frame of the clip; when it fails every frame
 *       gets order = 255....  Slots 2 .. 8 of frames >= 1 are unused.
 *     DPC_RECIPE_SCALE_AFTER_SIZED   RandomSizedCrop(crop, BILINEAR, p = sized_p) followed by NEAREST Scale((size, size)); needs
 *       sized_p >= 0.  PIL's resize is separable and per output sample, so output row i of either axis is row
 *       t = scale_tab ? scale_tab[i] : i of the table that resizes to `crop`: an accepted attempt {in = w, out = crop}, row t; ten
 *       rejected attempts: ow / oh computed with `crop`, first = rint((ow - crop) / 2), row first + t; the failed `p` draw,
 *       CenterCrop(crop): x1 = rint((W0 - crop) / 2), one tap at index t.  KS >= 2 ceil(max(W0, H0) / crop) + 1; scale_tab
 *       (int32 [size], values in [0, crop)) is required iff crop != size; crop <= 1024; sized_p < 1 with crop > W0 or crop > H0 is
 *       DPC_ERR_UNSUPPORTED (CenterCrop would leave the frame).
 *   lengths int64 [videos] or NULL: vlen = lengths[v] instead of offsets[v + 1] - offsets[v] -- a dense store whose videos are
 *     shorter than their slot (the caller has dropped videos with lengths[v] <= N*SL*ds).
 *   labels int64 [videos] with target int64 [B], both or neither: the same launch writes target[b] = labels[video of clip b]. */
#define DPC_RECIPE_SLOTS(n_frames) (58 + 9 * (n_frames))
#define DPC_RECIPE_JITTER_CONSISTENT 1
#define DPC_RECIPE_SCALE_AFTER_SIZED 2
typedef struct dpc_recipe_desc {
    double sized_p, gray_p, jitter_p;
    double brightness, contrast, saturation, hue;
    int32_t flip_code, flags;   /* flags: DPC_RECIPE_*; dpc_draw_recipe ignores them */
} dpc_recipe_desc;
int dpc_store_to_input(const uint8_t* store, int32_t B, int64_t total_frames, int32_t H0, int32_t W0, const dpc_clip_aug* aug,
                       const int8_t* gray, int32_t N, int32_t SL, int32_t ds, int32_t H, int32_t W, const dpc_resample* rs,
                       const dpc_frame_jitter* jitter, uint8_t* u8_ws, uint64_t* lsum_ws, const float* mean3, const float* std3,
                       float* block, void* s2d, int32_t dtype_s2d, const int64_t* clip_first, dpc_stream_t stream);
int dpc_draw_recipe(const dpc_recipe_desc* recipe, const int32_t* video_idx, const int32_t* step_dev, const int64_t* offsets,
                    int32_t B, int32_t W0, int32_t H0, int32_t crop, int32_t size, int32_t N, int32_t SL, int32_t ds, int32_t KS,
                    const int32_t* scale_tab, uint64_t seed, const int32_t* draw_dev, const float* uniforms, dpc_clip_aug* aug,
                    int64_t* clip_first, int8_t* gray, dpc_frame_jitter* jitter, int32_t* xb, int32_t* xk, int32_t* yb, int32_t* yk,
                    dpc_stream_t stream);
int dpc_draw_recipe_ex(const dpc_recipe_desc* recipe, const int32_t* video_idx, const int32_t* step_dev, const int64_t* offsets,
                       const int64_t* lengths, const int64_t* labels, int32_t B, int32_t W0, int32_t H0, int32_t crop, int32_t size,
                       int32_t N, int32_t SL, int32_t ds, int32_t KS, const int32_t* scale_tab, uint64_t seed, const int32_t* draw_dev,
                       const float* uniforms, dpc_clip_aug* aug, int64_t* clip_first, int8_t* gray, dpc_frame_jitter* jitter,
                       int32_t* xb, int32_t* xk, int32_t* yb, int32_t* yk, int64_t* target, dpc_stream_t stream);

/* The test-time windows of eval/dataset_3d_lc.py:109-127 from ONE resident video: `video` u8 [F][H0][W0][3] is read by every clip
 * of the batch, clip b = the window whose first frame is aug[b].start (aug[b].flip as above; the test transform never flips).
 * dpc_frames_to_input_ex without gray / jitter; rs [B] tables as there (NULL = plain crop of H x W at (x1, y1)).  The caller has
 * checked aug[b].start + (N*SL - 1)*ds < F and the crop box / resampling windows against the frame. */
int dpc_video_windows_to_input(const uint8_t* video, int32_t B, int32_t F, int32_t H0, int32_t W0, const dpc_clip_aug* aug,
                               int32_t N, int32_t SL, int32_t ds, int32_t H, int32_t W, const dpc_resample* rs, const float* mean3,
                               const float* std3, float* block, void* s2d, int32_t dtype_s2d, dpc_stream_t stream);

/* ---- video-level test reduction (eval/test.py:317-334; csrc/lc_test.hip) ------------------------------------------------------
 * Per-video state on the device: psum [num_class] (softmax of every window, summed), lsum [num_class] (logits summed), count [1]
 * (windows so far) -- zero before the first video, cleared by dpc_lc_test_finish.
 * dpc_lc_test_accumulate: logits f32 [rows][ld >= num_class]; rows [0, n_valid) are added in row order, rows beyond n_valid (the
 *   padding of a last chunk) are never read.
 * dpc_lc_test_finish: mean probability p and mean logit l of the video; rank = #{c : p_c > p_label} (strictly greater);
 *   video[4] = (loss = logsumexp(l) - l[label], top-1 = rank < 1, top-5 = rank < 5, pred = argmax l with the lowest index on
 *   ties); mean_prob [num_class] (NULL = not wanted) = p; totals f64[4] += (loss, top-1, top-5, 1); confusion i64
 *   [num_class][num_class] gets confusion[pred][label] += 1.  No atomics: same inputs, same bits. */
int dpc_lc_test_accumulate(const float* logits, int32_t rows, int32_t n_valid, int32_t num_class, int32_t ld, float* psum, float* lsum,
                           int32_t* count, dpc_stream_t stream);
int dpc_lc_test_finish(float* psum, float* lsum, int32_t* count, int32_t num_class, int32_t label, float* mean_prob, float* video,
                       double* totals, int64_t* confusion, dpc_stream_t stream);

/* ---- nearest-neighbour video retrieval (csrc/retrieval.hip) ------------------------------------------------------------------------
 * Per-video state on the device: esum [D] (the context vectors of the windows so far, summed), count [1] -- zero before the first
 * video, cleared by dpc_embed_finish.
 * dpc_embed_accumulate: ctx f32 [rows][ld >= D]; rows [0, n_valid) are added in row order, rows beyond n_valid are never read.
 * dpc_embed_finish: m = esum / count, out[d] = m[d] / max(||m||_2, eps) (F.normalize); count == 0: nothing is written.
 * dpc_knn_topk: Q f32 [nq][ldq], G f32 [ng][ldg], sim(i, j) = sum_d Q[i][d] G[j][d] on the exact-f32 matrix instruction in ascending
 *   d; per query the K best gallery rows by (sim descending, index ascending) -> top_idx int32 [nq][K], top_sim f32 [nq][K]; slots
 *   without a candidate hold -1 / -inf.  skip int32 [nq] (NULL = none): query i never returns row skip[i].  The gallery is cut into
 *   n_slabs slabs (0 = chosen from nq, ng and the CU count; 1..64 forced), one workgroup per (32 queries, slab) writes a partial list
 *   into ws (dpc_knn_ws_bytes(nq, K, n_slabs) bytes: with n_slabs == 0 enough for whatever ng turns out to be), a second kernel merges
 *   them: the same bits for every n_slabs.  D a multiple of 32 in [32, 256], 1 <= K <= 64, rows 16-byte aligned, else
 *   DPC_ERR_UNSUPPORTED.  Inputs must be finite.
 * dpc_knn_recall: labels int64; ks int32 [nk] ascending, each <= K; first_hit int32 [nq] = 0-based rank of the first neighbour with
 *   the query's label (-1: none; slots holding -1 are ignored); hits int64 [nk] += #{i : 0 <= first_hit[i] < ks[j]}; confusion int64
 *   [num_class][num_class]: confusion[g_label[top_idx[i][0]]][q_label[i]] += 1 where a first neighbour exists.
 * No atomics, no allocation, no host synchronisation: same inputs, same bits. */
int dpc_embed_accumulate(const float* ctx, int32_t rows, int32_t n_valid, int32_t D, int32_t ld, float* esum, int32_t* count,
                         dpc_stream_t stream);
int dpc_embed_finish(float* esum, int32_t* count, int32_t D, float eps, float* out, dpc_stream_t stream);
int dpc_knn_ws_bytes(int32_t nq, int32_t K, int32_t n_slabs);
int dpc_knn_topk(const float* Q, int32_t nq, int32_t ldq, const float* G, int32_t ng, int32_t ldg, int32_t D, int32_t K,
                 const int32_t* skip, int32_t n_slabs, float* top_sim, int32_t* top_idx, void* ws, int64_t ws_bytes, dpc_stream_t stream);
int dpc_knn_recall(const int32_t* top_idx, int32_t nq, int32_t K, const int64_t* q_label, const int64_t* g_label, int32_t ng,
                   int32_t num_class, const int32_t* ks, int32_t nk, int64_t* hits, int32_t* first_hit, int64_t* confusion,
                   dpc_stream_t stream);

/* ---- negative queue (csrc/neg_queue.hip): the keys (feature_inf) of the last K training batches, kept on the device and used,
 * detached, as extra negatives of every training row.  bf16 operands, D = 256 or 32, 1 <= K <= DPC_NEGQ_MAX_SLOTS.
 *   ring   [K][pitch][D] bf16, pitch = DPC_NEGQ_PITCH(R): slot k holds one batch's R keys in its first R rows.
 *   ringT  [K][D][pitch] bf16: the same keys transposed, the B operand of the backward's second product.
 *   state  the device record.  Slots fill in order, so slots [0, filled) are live and nothing else is ever read into a result:
 *          rows / columns >= R of a slot, slots >= filled and everything at filled = 0 may hold anything (NaN included).
 * Every launch argument is the same every step; what changes (the slot to write, the number of live slots) is read from the record.
 * No atomics, one writer per value, fixed combine orders: same inputs, same bits. */
#define DPC_NEGQ_MAX_SLOTS 64
#define DPC_NEGQ_PITCH(R) (((R) + 63) / 64 * 64)
typedef struct dpc_negq_state {
    int32_t pushes;   /* batches pushed since the bank was last empty */
    int32_t filled;   /* live slots: min(pushes, K) */
    int32_t reserved[2];
} dpc_negq_state;           /* 16 bytes, device memory */
/* floats of `ws` for dpc_negq_fwd / dpc_negq_bwd; returns the backward's slab count (what dpc_negq_bwd returns) */
int dpc_negq_ws_floats(int32_t R, int32_t D, int32_t K, int64_t* fwd_floats, int64_t* bwd_floats);
/* finf [R][D] -> slot (pushes % K) of ring, finfT [D][ldT] (columns >= R zero, ldT % 8 == 0, R <= ldT <= pitch) -> the same slot of
 * ringT; then pushes += 1, filled = min(filled + 1, K).  The slot index is read on the device. */
int dpc_negq_push(const void* finf, const void* finfT, int32_t ldT, void* ring, void* ringT, dpc_negq_state* state, int32_t R, int32_t D,
                  int32_t K, dpc_stream_t stream);
/* one thread: the record back to empty.  guard != NULL: only if the gradient guard's verdict says skip */
int dpc_negq_clear(dpc_negq_state* state, const dpc_grad_state* guard, dpc_stream_t stream);
/* stats[R][4] = (m, l, rk, 0) per row of pred over the live keys: m = max s, l = sum exp(s - m), rk = #{s > tgt_i}, s = pred_i . q_c
 * (f32 accumulators, unrounded); tgt_i = tgt[i * tgt_stride] of dtype tgt_dtype (DPC_F32 / DPC_BF16).  Empty bank: (-1e30, 0, 0). */
int dpc_negq_fwd(const void* pred, const void* ring, const dpc_negq_state* state, int32_t R, int32_t D, int32_t K, const void* tgt,
                 int64_t tgt_stride, int32_t tgt_dtype, float* stats, float* ws, dpc_stream_t stream);
/* out_part[slab][R][D] (f32): partial sums of  sum_c exp(s_ic - lse_i) / R * q_c  over the live keys (dS rounded to bf16); slabs of
 * dead column ranges are zero.  Returns the slab count; the caller sums the slabs (dpc_reduce_unpack). */
int dpc_negq_bwd(const void* pred, const void* ring, const void* ringT, const dpc_negq_state* state, int32_t R, int32_t D, int32_t K,
                 const float* lse, float* out_part, dpc_stream_t stream);
/* dpc_ce_topk / dpc_ce_topk_bf16 with the queue's per-row statistics qstats[rows][4] (dpc_negq_fwd) folded in before the
 * exponentials: mx = max(mx_in, m_q), se += l_q exp(m_q - mx), rk += rk_q; lse_out[rows] = log(se) + mx for dpc_negq_bwd.  The same
 * row kernels and dispatch; with empty statistics row_ws, result and dscore are those of the older entries bit for bit. */
int dpc_ce_topk_ext(const float* score, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result, void* dscore, int32_t dtype_d,
                    int32_t ld_d, const float* qstats, float* lse_out, dpc_stream_t stream);
int dpc_ce_topk_bf16_ext(const void* score, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result, void* dscore,
                         int32_t ld_d, const float* qstats, float* lse_out, dpc_stream_t stream);

/* ---- negative classes in the loss (csrc/loss_cls.hip): a weight per class of dpc_mask_gen inside the softmax, and a per-class report.
 * Row r = (b, p, s), column c = (b2, n, s2), cols = B P SQ, W = P SQ; the class of (r, c) is dpc_mask_gen's value in closed form:
 *   b != b2 easy (0) | b == b2, s != s2 spatial (-3) | b == b2, s == s2, n != p temporal (-1) | c == r positive (1); bank keys are easy.
 *   Z_r = e^(s_rr) + sum_{c != r} w_class e^(s_rc) + w_easy sum_{q live} e^(pred_r . q);  row_ws[r] = (log Z_r - s_rr, rank);
 *   dscore_rc = (w_class e^(s_rc) / Z_r - [c == r]) / rows: a class of weight 0 gets exactly 0.  The rank (and top-1/3/5) is the
 *   unweighted count of strictly greater logits over all columns and the bank, as in the older entries.
 * The argument lists of the _ext entries, with: qstats / lse_out NULL together (no bank); with a bank lse_out[r] = log Z_r - log w_easy,
 * so that dpc_negq_bwd yields the weighted share unchanged; the descriptor by value; two optional outputs:
 *   report_rows [rows][8] f32: the shares of Z_r (positive, spatial, temporal, easy -- the bank under easy; they sum to 1), the number
 *                of columns of each negative class strictly above the target (they add up to the rank; rk_q under easy), 0;
 *   report [8] f32 (needs report_rows): the means of the four shares, the fraction of rows whose count is not 0 per class, 0.
 * DPC_ERR_ARG: cols != B P SQ, a weight that is not finite or outside [0, DPC_NEGCLS_MAX_WEIGHT], flags / reserved not 0, w_easy = 0
 * with a bank, one of qstats / lse_out alone, report without report_rows.  Dispatch, DPC_ERR_UNSUPPORTED and every other argument
 * error: those of dpc_ce_topk / dpc_ce_topk_bf16.  At weights (1, 1, 1) row_ws, result, dscore and lse_out are the older entries'
 * bits.  The geometry comes from cols; rows may be fewer. */
#define DPC_NEGCLS_MAX_WEIGHT 65536.0f
typedef struct dpc_neg_classes {
    int32_t B, P, SQ;
    int32_t flags;      /* 0 */
    float w_spatial, w_temporal, w_easy;
    float reserved;     /* 0 */
} dpc_neg_classes;          /* 32 bytes, by value */
int dpc_ce_topk_cls(const float* score, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result, void* dscore, int32_t dtype_d,
                    int32_t ld_d, const float* qstats, float* lse_out, dpc_neg_classes cls, float* report_rows, float* report,
                    dpc_stream_t stream);
int dpc_ce_topk_bf16_cls(const void* score, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result, void* dscore,
                         int32_t ld_d, const float* qstats, float* lse_out, dpc_neg_classes cls, float* report_rows, float* report,
                         dpc_stream_t stream);

/* ---- symmetric InfoNCE (csrc/loss_sym.hip): over the square logits S [R][R] each key (column) also picks its prediction among the
 * rows.  With a = 1 - w, b = w (f32):
 *   Lr_i = logsumexp(S[i, :], bank) - S[i, i]   (the row direction: dpc_ce_topk[_bf16][_ext]'s)
 *   Lc_j = logsumexp(S[:, j]) - S[j, j]         (the bank has keys but no predictions: it takes no part)
 *   result      = (a mean Lr + b mean Lc, row top-1, top-3, top-5)          row_ws[i] = (Lr_i, rank_i) as ever
 *   sym_result  = (mean Lr, mean Lc, column top-1, top-3, top-5, 0, 0, 0)   col_ws[j] = (Lc_j, #{i : S[i, j] > S[j, j]})
 *   dscore[i,j] = (a (pr[i, j] - [i == j]) + b (exp(S[i, j] - col_lse[j]) - [i == j])) / R, rounded once into dscore's dtype
 * dpc_ce_colpass is the column direction alone: col_lse [R] (16-byte aligned for the _sym entries) and col_ws [R][2] of a row-major
 * matrix of dtype_s (DPC_F32 / DPC_BF16), `fast` = 1 with v_exp_f32 exponentials, 0 with expf; rows behind R and columns in [R, ld)
 * are never read; shapes without whole 16-byte units (R or ld no multiple of 4 / 8, a misaligned pointer) take a scalar form.  Two
 * launches, no atomics, a fixed order of every sum: same inputs, same bits.  `slabs` = 0 lets the library cut the rows (the rule that
 * fills the device), > 0 asks for that many slabs (fewer where R is short); ws holds dpc_ce_sym_ws_floats(R, slabs) floats, which
 * returns the largest slab count any layout takes.
 * The _sym entries run the column pass, the row kernel their sibling's dispatch selects, and the finalize: four launches.  The
 * sibling's argument list (qstats / lse_out NULL together: no bank) plus w, slabs and the four buffers.  With a bank lse_out[i] =
 * lse_i - log a (1e38 at a = 0), so that dpc_negq_bwd yields a x the bank's share unchanged.  DPC_ERR_ARG: rows != cols,
 * w outside [0, 1] or not finite, a NULL or (col_lse) misaligned buffer, one of qstats / lse_out alone, and the sibling's argument
 * errors; DPC_ERR_UNSUPPORTED: the sibling's.  Nothing is launched then.  At w = 0 row_ws, result, dscore and lse_out are the
 * sibling's bits. */
int dpc_ce_sym_ws_floats(int32_t R, int32_t slabs, int64_t* floats);
int dpc_ce_colpass(const void* score, int32_t dtype_s, int32_t R, int32_t ld, int32_t fast, int32_t slabs, float* col_lse, float* col_ws,
                   float* ws, dpc_stream_t stream);
int dpc_ce_topk_sym(const float* score, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result, void* dscore, int32_t dtype_d,
                    int32_t ld_d, const float* qstats, float* lse_out, float w, int32_t slabs, float* col_lse, float* col_ws, float* ws,
                    float* sym_result, dpc_stream_t stream);
int dpc_ce_topk_bf16_sym(const void* score, int32_t rows, int32_t cols, int32_t ld, float* row_ws, float* result, void* dscore,
                         int32_t ld_d, const float* qstats, float* lse_out, float w, int32_t slabs, float* col_lse, float* col_ws, float* ws,
                         float* sym_result, dpc_stream_t stream);

/* ---- cosine score (csrc/score_norm.hip): L2 normalisation of the score's two operands in front of the contraction, and its backward.
 * Rows [R][D] of `dtype` (DPC_F32 / DPC_BF16), D = 256 or 32 (else DPC_ERR_UNSUPPORTED); one launch serves operand a and, when
 * xb != NULL, operand b (xb and yb / gb are NULL together).  rnorm is f32 [2R]: operand a's rows first, then b's.
 *   fwd   n = sqrtf(sum x_d^2) (f32), rn = 1 / max(n, eps), y_d = round_to_dtype(x_d * (scale * rn)), rnorm[row] = rn
 *   bwd   in place on the f32 gradients g [R][D] at y:  u_d = x_d * rn, t = sum g_d u_d,  g_d <- (scale * rn) * (g_d - u_d * t);
 *         a row the forward clamped (rn >= 1 / eps):  g_d <- (scale * rn) * g_d
 * F.normalize's semantics times a scale (1 / temperature for pred, 1 for the keys).  Fixed summation order, no atomics, nothing
 * contracted: same inputs, same bits.  DPC_ERR_ARG: a NULL or misaligned (16 bytes; rnorm 4) pointer, R < 1, a scale or an eps that
 * is not finite and positive. */
int dpc_rownorm_fwd(const void* xa, const void* xb, void* ya, void* yb, float* rnorm, int32_t R, int32_t D, int32_t dtype, float scale_a,
                    float scale_b, float eps, dpc_stream_t stream);
int dpc_rownorm_bwd(const void* xa, const void* xb, const float* rnorm, float* ga, float* gb, int32_t R, int32_t D, int32_t dtype,
                    float scale_a, float scale_b, float eps, dpc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DPC_HIP_H */
