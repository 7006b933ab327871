// Classifier-free training of the denoiser: condition dropout and the gradient of the learned null embedding (Improved VQ-Diffusion;
// the reference substitutes empty_text_embed at diffusion_transformer.py:541-543).
//
// gsdd_cond_dropout: one workgroup per sample.  The workgroup derives its sample's decision itself -- word 0 of Philox4x32-10 on the
// counter (global sample row, stream id of the step's q_sample draw, 1), so that the draw shares no counter with any other draw of the
// step (all of those have 0 in counter word 3) and does not depend on the rank count or the local batch size -- or takes it from the
// caller's mask, and copies the sample's (Te, C) condition rows or the null rows.  The stream id is read from device memory: a
// captured training step bakes nothing step-dependent in.
//
// gsdd_cond_null_grad: one workgroup per condition token j.  The dropped samples' dk[b, j, :] and dv[b, j, :] are summed in ascending
// b into LDS (one thread per feature), then thread c forms sum_d (sk[d] Wk[d, c]) + sum_d (sv[d] Wv[d, c]) in ascending d and adds it
// onto dnull[j, c].  A fixed summation order and no atomics: the same inputs give the same bits.  A token of a step without a dropped
// sample writes nothing.
//
// Both are tiny and latency-bound (B workgroups copying 45 KB each; 22 workgroups reading two 64 x 512 matrices): plain f32 vector
// code.
#include "common.hpp"

namespace gsdd {

constexpr int COND_MAX_TE = 77;           // the rows of empty_text_embed (CLIP's context length)
constexpr int NULL_GRAD_MAX_D = 4096;     // 2 D floats of dynamic LDS: 32 KB at most

__global__ __launch_bounds__(256) void cond_dropout_kernel(const float4* __restrict__ cond, const float4* __restrict__ null_rows,
                                                           int n4, float p, uint64_t seed, const int64_t* __restrict__ sid,
                                                           int64_t row0, const uint8_t* __restrict__ drop_in,
                                                           float4* __restrict__ out, uint8_t* __restrict__ drop_out) {
    const int b = blockIdx.x;
    bool drop;
    if (drop_in != nullptr) {
        drop = drop_in[b] != 0;
    } else {
        const uint64_t row = (uint64_t)(row0 + b);
        const uint4 r = philox4x32_10((uint32_t)row, (uint32_t)(row >> 32), (uint32_t)sid[0], 1u, (uint32_t)seed, (uint32_t)(seed >> 32));
        drop = (float)(r.x >> 8) * (1.0f / 16777216.0f) < p;
    }
    const float4* src = drop ? null_rows : cond + (int64_t)b * n4;
    float4* dst = out + (int64_t)b * n4;
    for (int i = threadIdx.x; i < n4; i += 256) dst[i] = src[i];
    if (threadIdx.x == 0) drop_out[b] = drop ? 1 : 0;
}

__global__ __launch_bounds__(256) void cond_null_grad_kernel(const float* __restrict__ dk, const float* __restrict__ dv,
                                                             const uint8_t* __restrict__ drop, const float* __restrict__ wk,
                                                             const float* __restrict__ wv, int B, int Te, int D, int C,
                                                             float* __restrict__ dnull) {
    extern __shared__ float lds[];          // sk[D] | sv[D]
    float* sk = lds;
    float* sv = lds + D;
    const int j = blockIdx.x;
    bool any = false;
    for (int b = 0; b < B; ++b) any = any || drop[b] != 0;
    if (!any) return;                       // (uniform over the workgroup, ahead of the barrier) dnull keeps its bits
    for (int d = threadIdx.x; d < D; d += 256) {
        float ak = 0.f, av = 0.f;
        for (int b = 0; b < B; ++b) {
            if (drop[b] == 0) continue;
            const int64_t at = ((int64_t)b * Te + j) * D + d;
            av += dv[at];
            if (dk != nullptr) ak += dk[at];
        }
        sk[d] = ak;
        sv[d] = av;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        float ak = 0.f, av = 0.f;
        for (int d = 0; d < D; ++d) {
            av += sv[d] * wv[(int64_t)d * C + c];
            if (wk != nullptr) ak += sk[d] * wk[(int64_t)d * C + c];
        }
        dnull[(int64_t)j * C + c] += ak + av;
    }
}

static inline bool overlap(const void* a, const void* b, int64_t a_bytes, int64_t b_bytes) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + (uintptr_t)b_bytes && y < x + (uintptr_t)a_bytes;
}

}  // namespace gsdd

using namespace gsdd;

extern "C" int gsdd_cond_dropout(const float* cond, const float* null_rows, int B, int Te, int C, float p, uint64_t seed,
                                 const int64_t* sid, int64_t row0, const uint8_t* drop_in, float* out, uint8_t* drop_out,
                                 void* stream) {
    GSDD_CHECK_ARG(cond && null_rows && out && drop_out, "null pointer");
    GSDD_CHECK_ARG(drop_in != nullptr || sid != nullptr, "the draw needs the device word holding the stream id");
    GSDD_CHECK_ARG(B > 0 && Te >= 1 && Te <= COND_MAX_TE, "bad sizes (B > 0, 1 <= Te <= 77)");
    GSDD_CHECK_ARG(C > 0 && C % 4 == 0, "C must be a multiple of 4");
    GSDD_CHECK_ARG(p >= 0.f && p <= 1.f, "p must lie in [0, 1]");
    GSDD_CHECK_ARG(row0 >= 0, "row0 must be >= 0");
    GSDD_CHECK_ARG(aligned16(cond) && aligned16(null_rows) && aligned16(out), "rows must be 16-byte aligned");
    const int64_t row_bytes = (int64_t)Te * C * 4, all_bytes = row_bytes * B;
    GSDD_CHECK_ARG(!overlap(out, cond, all_bytes, all_bytes), "out must not alias cond");
    GSDD_CHECK_ARG(!overlap(out, null_rows, all_bytes, row_bytes), "out must not alias null_rows");
    hipLaunchKernelGGL(cond_dropout_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const float4*>(cond), reinterpret_cast<const float4*>(null_rows), Te * C / 4, p, seed, sid, row0,
                       drop_in, reinterpret_cast<float4*>(out), drop_out);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_cond_null_grad(const float* dk, const float* dv, const uint8_t* drop, const float* wk, const float* wv, int B,
                                   int Te, int D, int C, float* dnull, void* stream) {
    GSDD_CHECK_ARG(dv && drop && wv && dnull, "null pointer");
    GSDD_CHECK_ARG((dk == nullptr) == (wk == nullptr), "dk and wk come together");
    GSDD_CHECK_ARG(B > 0 && Te >= 1 && Te <= COND_MAX_TE, "bad sizes (B > 0, 1 <= Te <= 77)");
    GSDD_CHECK_ARG(D >= 1 && D <= NULL_GRAD_MAX_D && C >= 1, "bad sizes (1 <= D <= 4096, C >= 1)");
    hipLaunchKernelGGL(cond_null_grad_kernel, dim3((unsigned)Te), dim3(256), (size_t)(2 * D) * sizeof(float), (hipStream_t)stream, dk, dv,
                       drop, wk, wv, B, Te, D, C, dnull);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}
