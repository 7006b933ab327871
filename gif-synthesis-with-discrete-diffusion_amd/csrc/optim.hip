// Optimiser stage of the training step (include/gsdd.h, "optimiser stage"): global gradient norm, clip coefficient and non-finite
// flag, AdamW with decoupled weight decay, the running average of the weights, and the exchange of weights and average.  Streaming
// kernels over the wide block table {p, g, m, v, n, e, flags}: one workgroup of 256 lanes per block of up to 4096 elements, lane l takes
// the four consecutive elements 4 l + 1024 k + (0..3) for k = 0..3.  m, v and e are 16-byte aligned at every block and p and g almost
// always are: such a group of four is read and written as one 16-byte access; a block whose p or g is not 16-byte aligned, and the
// ragged last group of a tensor, go element by element.  Every load of a group is issued before its first store (the pointers may not
// be declared restrict: nothing in the ABI forbids a caller's views from touching).
#include "common.hpp"

namespace gsdd {

constexpr int OPT_COLS = 7;          // table row: p, g, m, v, n, e, flags
constexpr int OPT_LANES = 256;
constexpr int OPT_GROUPS = 4;        // groups of four elements per lane: 256 * 4 * 4 = 4096 = the largest block

// up to four consecutive floats; `wide`: all four are there and q is 16-byte aligned
__device__ __forceinline__ void load4(const float* q, bool wide, int cnt, float (&o)[4]) {
    if (wide) {
        const float4 t = *reinterpret_cast<const float4*>(q);
        o[0] = t.x; o[1] = t.y; o[2] = t.z; o[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = j < cnt ? q[j] : 0.f;
    }
}

__device__ __forceinline__ void store4(float* q, bool wide, int cnt, const float (&o)[4]) {
    if (wide) {
        *reinterpret_cast<float4*>(q) = make_float4(o[0], o[1], o[2], o[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < cnt) q[j] = o[j];
    }
}

__device__ __forceinline__ bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// sum over the workgroup in a fixed order (lanes of a wave by halving shuffles, then the four waves in ascending order); the result is
// valid in lane 0
__device__ __forceinline__ double block_sum(double s, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

__global__ __launch_bounds__(OPT_LANES) void grad_sqnorm_kernel(const int64_t* __restrict__ table, double* __restrict__ partials) {
    __shared__ double sh[OPT_LANES / 64];
    const int64_t* row = table + (int64_t)blockIdx.x * OPT_COLS;
    const float* g = reinterpret_cast<const float*>(row[1]);
    const int n = (int)row[4];
    const bool al = aligned16(g);
    float x[OPT_GROUPS][4];
#pragma unroll
    for (int k = 0; k < OPT_GROUPS; ++k) {                      // (no store in this kernel: all of a lane's loads are in flight at once)
        const int b = 4 * threadIdx.x + 4 * OPT_LANES * k;
        const int cnt = n - b;                                  // (<= 0: nothing of this group exists, load4 gives zeros)
        load4(g + b, al && cnt >= 4, cnt, x[k]);
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < OPT_GROUPS; ++k)
#pragma unroll
        for (int j = 0; j < 4; ++j) s += (double)x[k][j] * (double)x[k][j];
    s = block_sum(s, sh);
    if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(OPT_LANES) void grad_norm_finalize_kernel(const double* __restrict__ partials, int n_blocks, float max_norm,
                                                                       int skip_nonfinite, gsdd_optim_state* __restrict__ state) {
    __shared__ double sh[OPT_LANES / 64];
    double s = 0.0;
    for (int i = threadIdx.x; i < n_blocks; i += OPT_LANES) s += partials[i];
    s = block_sum(s, sh);
    if (threadIdx.x != 0) return;
    const double norm = sqrt(s);
    const bool finite = norm <= 1.7976931348623157e308;        // false for +inf and for NaN
    float coef = 1.f;
    if (max_norm <= 3.4028234663852886e38f) {                  // (+inf: no clipping)
        const double c = (double)max_norm / (norm + 1e-6);
        coef = c < 1.0 ? (float)c : (c >= 1.0 ? 1.f : (float)c);     // min(1, c); NaN stays NaN
    }
    state->grad_norm = (float)norm;
    state->clip_coef = coef;
    const bool skip = skip_nonfinite != 0 && !finite;
    state->finite = skip ? 0 : 1;
    if (skip) state->skipped_steps += 1;
}

__global__ __launch_bounds__(OPT_LANES) void adamw_ema_multi_kernel(const int64_t* __restrict__ table, float b1, float b2, float eps,
                                                                    float wd, float ema_decay,
                                                                    const gsdd_optim_state* __restrict__ state) {
    if (state->finite == 0) return;
    const double st = (double)state->step;
    const float lr = state->lr, coef = state->clip_coef;
    const float bc1 = (float)(1.0 - pow((double)b1, st)), bc2 = (float)(1.0 - pow((double)b2, st));
    const int64_t* row = table + (int64_t)blockIdx.x * OPT_COLS;
    float* p = reinterpret_cast<float*>(row[0]);
    const float* g = reinterpret_cast<const float*>(row[1]);
    float* m = reinterpret_cast<float*>(row[2]);
    float* v = reinterpret_cast<float*>(row[3]);
    const int n = (int)row[4];
    float* e = reinterpret_cast<float*>(row[5]);
    const float keep = (row[6] & GSDD_OPTIM_DECAYS) ? 1.f - lr * wd : 1.f;       // (p * 1.f is p: tensors that do not decay are untouched by it)
    const double dw = (1.0 + st) / (10.0 + st);
    const float d = (float)((double)ema_decay < dw ? (double)ema_decay : dw);
    const bool al_pg = aligned16(p) && aligned16(g);
#pragma unroll 1
    for (int k = 0; k < OPT_GROUPS; ++k) {
        const int b = 4 * threadIdx.x + 4 * OPT_LANES * k;
        const int cnt = n - b;
        if (cnt <= 0) break;
        const bool full = cnt >= 4, wide = full && al_pg;
        float pi[4], gi[4], mi[4], vi[4], ei[4];
        load4(g + b, wide, cnt, gi);
        load4(m + b, full, cnt, mi);
        load4(v + b, full, cnt, vi);
        load4(p + b, wide, cnt, pi);
        if (e) load4(e + b, full, cnt, ei);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float gc = coef * gi[j];
            const float pd = pi[j] * keep;
            const float mn = b1 * mi[j] + (1.f - b1) * gc;
            const float vn = b2 * vi[j] + (1.f - b2) * gc * gc;
            const float denom = sqrtf(vn) / sqrtf(bc2) + eps;
            const float pn = pd - (lr / bc1) * (mn / denom);
            mi[j] = mn; vi[j] = vn; pi[j] = pn;
            if (e) ei[j] = d * ei[j] + (1.f - d) * pn;
        }
        store4(m + b, full, cnt, mi);
        store4(v + b, full, cnt, vi);
        store4(p + b, wide, cnt, pi);
        if (e) store4(e + b, full, cnt, ei);
    }
}

__global__ __launch_bounds__(OPT_LANES) void swap_multi_kernel(const int64_t* __restrict__ table) {
    const int64_t* row = table + (int64_t)blockIdx.x * OPT_COLS;
    float* p = reinterpret_cast<float*>(row[0]);
    const int n = (int)row[4];
    float* e = reinterpret_cast<float*>(row[5]);
    if (e == nullptr) return;
    const bool al_p = aligned16(p);
#pragma unroll 1
    for (int k = 0; k < OPT_GROUPS; ++k) {
        const int b = 4 * threadIdx.x + 4 * OPT_LANES * k;
        const int cnt = n - b;
        if (cnt <= 0) break;
        const bool full = cnt >= 4;
        float pi[4], ei[4];
        load4(p + b, full && al_p, cnt, pi);
        load4(e + b, full, cnt, ei);
        store4(p + b, full && al_p, cnt, ei);
        store4(e + b, full, cnt, pi);
    }
}

}  // namespace gsdd

using namespace gsdd;

extern "C" int gsdd_grad_sqnorm(const int64_t* table, int n_blocks, double* partials, void* stream) {
    GSDD_CHECK_ARG(table != nullptr && partials != nullptr, "null pointer");
    GSDD_CHECK_ARG(n_blocks > 0, "no blocks");
    hipLaunchKernelGGL(grad_sqnorm_kernel, dim3((unsigned)n_blocks), dim3(OPT_LANES), 0, (hipStream_t)stream, table, partials);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_grad_norm_finalize(const double* partials, int n_blocks, float max_norm, int skip_nonfinite, gsdd_optim_state* state,
                                       void* stream) {
    GSDD_CHECK_ARG(partials != nullptr && state != nullptr, "null pointer");
    GSDD_CHECK_ARG(n_blocks > 0, "no blocks");
    GSDD_CHECK_ARG(max_norm > 0.f, "max_norm must be positive (+infinity: no clipping)");
    hipLaunchKernelGGL(grad_norm_finalize_kernel, dim3(1), dim3(OPT_LANES), 0, (hipStream_t)stream, partials, n_blocks, max_norm,
                       skip_nonfinite, state);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_adamw_ema_multi(const int64_t* table, int n_blocks, float beta1, float beta2, float eps, float weight_decay,
                                    float ema_decay, const gsdd_optim_state* state, void* stream) {
    GSDD_CHECK_ARG(table != nullptr && state != nullptr, "null pointer");
    GSDD_CHECK_ARG(n_blocks > 0, "no blocks");
    GSDD_CHECK_ARG(weight_decay >= 0.f, "weight_decay must not be negative");
    GSDD_CHECK_ARG(ema_decay >= 0.f && ema_decay < 1.f, "ema_decay must be in [0, 1)");
    hipLaunchKernelGGL(adamw_ema_multi_kernel, dim3((unsigned)n_blocks), dim3(OPT_LANES), 0, (hipStream_t)stream, table, beta1, beta2, eps,
                       weight_decay, ema_decay, state);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_swap_multi(const int64_t* table, int n_blocks, void* stream) {
    GSDD_CHECK_ARG(table != nullptr, "null pointer");
    GSDD_CHECK_ARG(n_blocks > 0, "no blocks");
    hipLaunchKernelGGL(swap_multi_kernel, dim3((unsigned)n_blocks), dim3(OPT_LANES), 0, (hipStream_t)stream, table);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}
