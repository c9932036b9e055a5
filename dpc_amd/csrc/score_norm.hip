// score_norm.hip -- the cosine score's two row passes: L2 normalisation (times a scale) in front of the score contraction, and its
// backward behind the score's.  With x a row of pred or feature_inf ([R][D], compute dtype) and g the f32 gradient at the normalised row:
//
//   dpc_rownorm_fwd   n2 = sum x_d^2 (f32), n = sqrtf(n2), rn = 1 / max(n, eps), k = scale * rn, y_d = round(x_d * k); rnorm[row] = rn
//   dpc_rownorm_bwd   u_d = x_d * rn, t = sum g_d u_d (f32):  g_d <- (scale * rn) * (g_d - u_d * t)      (in place)
//                     a row the forward clamped (rn >= 1 / eps):  g_d <- (scale * rn) * g_d               (torch's clamp_min)
//
// F.normalize's semantics; scale = float32(1 / T) for pred, 1 for the keys.  One launch serves both operands (as
// dpc_transpose2d_bf16x2 does): rows [0, R) are operand a, rows [R, 2R) operand b, rnorm is [2R] with a first.
//
// Shape: HBM-bound row passes (cfg2: 12.6 MB forward, 31 MB backward).  A row belongs to a group of G = D / 8 lanes (4 at D = 32, 32 at
// D = 256), eight elements per lane: one 16-byte unit of bf16 or two of f32 (units l and l + G, so that a load instruction of the
// group covers consecutive units).  The lane's eight terms are summed in element order, the group's partial sums with a __shfl_xor
// butterfly from G / 2 down to 1 -- a + b == b + a, so every lane of the group holds the same bits.  No LDS, no atomics, one writer
// per value; nothing is contracted, every product and sum is rounded once, so the host simulator and the device agree bit for bit
// (sqrtf and the division are the correctly rounded forms on both).  A lane of a row past the end loads and stores nothing but takes
// part in the butterfly.  The backward reads a row completely (every lane its own eight elements of x and g) before the butterfly
// and writes only what it read: in place is safe.
#include "dpc_rt.h"
#include "../../include/dpc_hip.h"

#pragma clang fp contract(off)

// column of element e (0 .. 7) of lane l of a group of G lanes
template <class T, int G> __device__ __forceinline__ int rn_col(int l, int e) {
    return Elt<T>::PER16 == 8 ? 8 * l + e : 4 * (l + G * (e >> 2)) + (e & 3);
}

// the lane's eight elements of row x (D elements of T) as f32
template <class T, int G> __device__ __forceinline__ void rn_load(const T* x, int l, float (&v)[8]) {
    constexpr int U = 8 / Elt<T>::PER16;   // 16-byte units per lane
    u32x4 u[U];
    DPC_UNROLL
    for (int j = 0; j < U; ++j) u[j] = *(const u32x4*)(x + rn_col<T, G>(l, j * Elt<T>::PER16));
    DPC_UNROLL
    for (int e = 0; e < 8; ++e) v[e] = unit_get<T>(u[e / Elt<T>::PER16], e % Elt<T>::PER16);
}

template <int G> __device__ __forceinline__ float rn_group_sum(float s) {
    DPC_UNROLL
    for (int m = G / 2; m >= 1; m >>= 1) s = s + __shfl_xor(s, m);
    return s;
}

__device__ __forceinline__ float rn_rnorm(float n2, float eps) {
    const float n = sqrtf(n2);
    return 1.f / (n < eps ? eps : n);   // a NaN norm stays NaN, as torch's clamp_min keeps it
}

template <class T, int D>
__global__ __launch_bounds__(256) void rownorm_fwd_kernel(const T* xa, const T* xb, T* ya, T* yb, float* rnorm, int R, int rows, float scale_a,
                                                          float scale_b, float eps) {
    constexpr int G = D / 8, U = 8 / Elt<T>::PER16;
    const int l = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (256 / G) + threadIdx.x / G;
    const bool live = row < rows, second = row >= R;
    const long long r = second ? row - R : row;
    const T* x = (second ? xb : xa) + r * D;
    float v[8];
    if (live) {
        rn_load<T, G>(x, l, v);
    } else {
        DPC_UNROLL
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
    }
    float s = 0.f;
    DPC_UNROLL
    for (int e = 0; e < 8; ++e) s = s + v[e] * v[e];
    const float rn = rn_rnorm(rn_group_sum<G>(s), eps);
    if (!live) return;
    const float k = (second ? scale_b : scale_a) * rn;
    float o[8];
    DPC_UNROLL
    for (int e = 0; e < 8; ++e) o[e] = v[e] * k;
    T* y = (second ? yb : ya) + r * D;
    DPC_UNROLL
    for (int j = 0; j < U; ++j) *(u32x4*)(y + rn_col<T, G>(l, j * Elt<T>::PER16)) = unit_pack<T>(o + j * Elt<T>::PER16);
    if (l == 0) rnorm[row] = rn;
}

template <class T, int D>
__global__ __launch_bounds__(256) void rownorm_bwd_kernel(const T* xa, const T* xb, const float* rnorm, float* ga, float* gb, int R, int rows,
                                                          float scale_a, float scale_b, float eps) {
    constexpr int G = D / 8;
    const int l = threadIdx.x % G;
    const long long row = (long long)blockIdx.x * (256 / G) + threadIdx.x / G;
    const bool live = row < rows, second = row >= R;
    const long long r = second ? row - R : row;
    float* g = (second ? gb : ga) + r * D;
    float v[8], d[8];
    float rn = 0.f;
    if (live) {
        rn_load<T, G>((second ? xb : xa) + r * D, l, v);
        DPC_UNROLL
        for (int j = 0; j < 2; ++j) {   // g in the element order of x: the lane's two f32 units
            const f32x4 q = *(const f32x4*)(g + rn_col<T, G>(l, 4 * j));
            DPC_UNROLL
            for (int e = 0; e < 4; ++e) d[4 * j + e] = q[e];
        }
        rn = rnorm[row];
    } else {
        DPC_UNROLL
        for (int e = 0; e < 8; ++e) v[e] = d[e] = 0.f;
    }
    float s = 0.f;
    DPC_UNROLL
    for (int e = 0; e < 8; ++e) {
        v[e] = v[e] * rn;   // u_d
        s = s + d[e] * v[e];
    }
    const float t = rn_group_sum<G>(s);
    if (!live) return;
    const float k = (second ? scale_b : scale_a) * rn;
    const bool clamped = rn >= 1.f / eps;
    DPC_UNROLL
    for (int j = 0; j < 2; ++j) {
        f32x4 q;
        DPC_UNROLL
        for (int e = 0; e < 4; ++e) q[e] = clamped ? k * d[4 * j + e] : k * (d[4 * j + e] - v[4 * j + e] * t);
        *(f32x4*)(g + rn_col<T, G>(l, 4 * j)) = q;
    }
}

static bool rn_positive_finite(float v) { return v > 0.f && ((__builtin_bit_cast(uint32_t, v) >> 23) & 0xffu) != 0xffu; }

// what both entries refuse; DPC_OK when the launch may go ahead
static int rn_args(const void* a, const void* b, const void* pa, const void* pb, const void* rnorm, int32_t R, int32_t D, int32_t dtype,
                   float scale_a, float scale_b, float eps) {
    if (!a || !pa || !rnorm || (b == nullptr) != (pb == nullptr) || R < 1) return DPC_ERR_ARG;
    if ((((uintptr_t)a | (uintptr_t)b | (uintptr_t)pa | (uintptr_t)pb) % 16) || (uintptr_t)rnorm % 4) return DPC_ERR_ARG;
    if (dtype != DPC_F32 && dtype != DPC_BF16) return DPC_ERR_ARG;
    if (!rn_positive_finite(scale_a) || !rn_positive_finite(scale_b) || !rn_positive_finite(eps)) return DPC_ERR_ARG;
    if (R > (1 << 30)) return DPC_ERR_ARG;
    if (D != 32 && D != 256) return DPC_ERR_UNSUPPORTED;
    return DPC_OK;
}

extern "C" int dpc_rownorm_fwd(const void* xa, const void* xb, void* ya, void* yb, float* rnorm, int32_t R, int32_t D, int32_t dtype,
                               float scale_a, float scale_b, float eps, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = rn_args(xa, xb, ya, yb, rnorm, R, D, dtype, scale_a, scale_b, eps);
    if (rc != DPC_OK) return rc;
    const int rows = xb ? 2 * R : R, per = 256 / (D / 8);
    const dim3 grid((unsigned)((rows + per - 1) / per)), block(256);
    if (dtype == DPC_BF16) {
        if (D == 256)
            DPC_LAUNCH((rownorm_fwd_kernel<bf16_t, 256>), grid, block, stream, (const bf16_t*)xa, (const bf16_t*)xb, (bf16_t*)ya, (bf16_t*)yb, rnorm, (int)R, rows, scale_a, scale_b, eps);
        else
            DPC_LAUNCH((rownorm_fwd_kernel<bf16_t, 32>), grid, block, stream, (const bf16_t*)xa, (const bf16_t*)xb, (bf16_t*)ya, (bf16_t*)yb, rnorm, (int)R, rows, scale_a, scale_b, eps);
    } else {
        if (D == 256)
            DPC_LAUNCH((rownorm_fwd_kernel<float, 256>), grid, block, stream, (const float*)xa, (const float*)xb, (float*)ya, (float*)yb, rnorm, (int)R, rows, scale_a, scale_b, eps);
        else
            DPC_LAUNCH((rownorm_fwd_kernel<float, 32>), grid, block, stream, (const float*)xa, (const float*)xb, (float*)ya, (float*)yb, rnorm, (int)R, rows, scale_a, scale_b, eps);
    }
    return dpc_launch_status();
}

extern "C" int dpc_rownorm_bwd(const void* xa, const void* xb, const float* rnorm, float* ga, float* gb, int32_t R, int32_t D, int32_t dtype,
                               float scale_a, float scale_b, float eps, dpc_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int rc = rn_args(xa, xb, ga, gb, rnorm, R, D, dtype, scale_a, scale_b, eps);
    if (rc != DPC_OK) return rc;
    const int rows = xb ? 2 * R : R, per = 256 / (D / 8);
    const dim3 grid((unsigned)((rows + per - 1) / per)), block(256);
    if (dtype == DPC_BF16) {
        if (D == 256)
            DPC_LAUNCH((rownorm_bwd_kernel<bf16_t, 256>), grid, block, stream, (const bf16_t*)xa, (const bf16_t*)xb, rnorm, ga, gb, (int)R, rows, scale_a, scale_b, eps);
        else
            DPC_LAUNCH((rownorm_bwd_kernel<bf16_t, 32>), grid, block, stream, (const bf16_t*)xa, (const bf16_t*)xb, rnorm, ga, gb, (int)R, rows, scale_a, scale_b, eps);
    } else {
        if (D == 256)
            DPC_LAUNCH((rownorm_bwd_kernel<float, 256>), grid, block, stream, (const float*)xa, (const float*)xb, rnorm, ga, gb, (int)R, rows, scale_a, scale_b, eps);
        else
            DPC_LAUNCH((rownorm_bwd_kernel<float, 32>), grid, block, stream, (const float*)xa, (const float*)xb, rnorm, ga, gb, (int)R, rows, scale_a, scale_b, eps);
    }
    return dpc_launch_status();
}
