// Composed guidance: N conditional logit rows and the unconditional row of a position folded into one row,
//   x_i = clamp(log_softmax(logits_i), -70, 0)   (predict_start; x_u likewise)
//   e   = x_u + sum_i w_i (x_i - x_u)            f32, i = 0, 1, ... in order, the first term as the step's mix: x_u + w_0 * (x_0 - x_u)
// which the reverse step then takes as its logits_c with logits_u = NULL (gsdd_compose_desc, include/gsdd.h).
//
// One wave64 owns one position, four positions per workgroup, lane owns quads k = 4*lane + 256*j, as the step (d3pm_rows.hpp).
//   J <= 16: one pass.  Three rows live in registers (x_u, the sum, the current x_i: 192 VGPRs at J = 16, two waves per SIMD) and every
//            x_i is log_softmax_clamp's own value.  Every block is read once.
//   J = 32:  three rows are 384 registers.  Two passes: the N + 1 log-sum-exps first (one 128-register row at a time; row_lse is the first
//            half of log_softmax_clamp, the same operations in the same order), then the combination quad by quad on a second read of
//            the rows, which comes from L1 / L2.  The values are the same bits as one pass would give (tests/test_gpu_compose.py holds
//            a zero-weight row against the step's own x0 at every width).
// `out` may be block 0: a lane reads element k of every block before it writes element k, and no other lane touches element k.
#include "common.hpp"
#include "d3pm_rows.hpp"

namespace gsdd {

template <int J, bool FULL>
__device__ __forceinline__ void load_row(float (&x)[J][4], const float* row, int lane, int K) {
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k = 4 * lane + 256 * j;
        if (FULL || k < K) {
            const float4 v = *reinterpret_cast<const float4*>(row + k);
            x[j][0] = v.x; x[j][1] = v.y; x[j][2] = v.z; x[j][3] = v.w;
        } else {
            x[j][0] = x[j][1] = x[j][2] = x[j][3] = -INFINITY;
        }
    }
}

// the log-sum-exp log_softmax_clamp subtracts: maximum, fp64 sum of exp_term in slot order, fp64 wave sum, fp64 log
template <int J>
__device__ __forceinline__ double row_lse(const float (&x)[J][4]) {
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) mx = fmaxf(mx, x[j][e]);
    mx = wave_max(mx);
    double se = 0.0;
#pragma unroll
    for (int j = 0; j < J; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) se += (double)exp_term(x[j][e] - mx);
    se = wave_sum(se);
    return (double)mx + log(se);
}
// ... and its last line
__device__ __forceinline__ float lsm_clamp(float v, double lse) { return clamp70((float)((double)v - lse)); }

template <int J, bool FULL>
__global__ __launch_bounds__(256, 2) void d3pm_compose_kernel(gsdd_compose_desc d) {
    const int lane = threadIdx.x & 63;
    const int64_t pos = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t npos = (int64_t)d.B * d.L;
    if (pos >= npos) return;
    const int K = d.K, N = d.n_cond;
    const float* w = d.weights + (pos / d.L) * N;                 // wave-uniform: scalar loads
    const int64_t block = npos * K;                               // floats per block of `logits`
    const float* row0 = d.logits + pos * (int64_t)K;              // this position's row of block 0
    float* orow = d.out + pos * (int64_t)K;

    if constexpr (J <= 16) {
        float xu[J][4], acc[J][4], x[J][4];
        load_row<J, FULL>(xu, row0 + N * block, lane, K);
        log_softmax_clamp<J>(xu);
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) acc[j][e] = xu[j][e];
        for (int i = 0; i < N; ++i) {
            load_row<J, FULL>(x, row0 + i * block, lane, K);
            log_softmax_clamp<J>(x);
            const float wi = w[i];
#pragma unroll
            for (int j = 0; j < J; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float diff = x[j][e] - xu[j][e];
                    const float sc = wi * diff;
                    acc[j][e] = acc[j][e] + sc;
                }
        }
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int k = 4 * lane + 256 * j;
            if (FULL || k < K) *reinterpret_cast<float4*>(orow + k) = make_float4(acc[j][0], acc[j][1], acc[j][2], acc[j][3]);
        }
    } else {
        // pass 1: lane i keeps the log-sum-exp of block i (N + 1 <= 5 of them)
        double mine = 0.0;
        {
            float x[J][4];
            for (int i = 0; i <= N; ++i) {
                load_row<J, FULL>(x, row0 + i * block, lane, K);
                const double lse = row_lse<J>(x);
                if (lane == i) mine = lse;
            }
        }
        double lse[GSDD_COMPOSE_MAX_COND];
        float wi[GSDD_COMPOSE_MAX_COND];
#pragma unroll
        for (int i = 0; i < GSDD_COMPOSE_MAX_COND; ++i) {
            lse[i] = __shfl(mine, i);
            wi[i] = i < N ? w[i] : 0.f;
        }
        const double lse_u = __shfl(mine, N);
        // pass 2: quad by quad
#pragma unroll 4
        for (int j = 0; j < J; ++j) {
            const int k = 4 * lane + 256 * j;
            if (FULL || k < K) {
                const float4 vu = *reinterpret_cast<const float4*>(row0 + N * block + k);
                const float xu[4] = {lsm_clamp(vu.x, lse_u), lsm_clamp(vu.y, lse_u), lsm_clamp(vu.z, lse_u), lsm_clamp(vu.w, lse_u)};
                float acc[4] = {xu[0], xu[1], xu[2], xu[3]};
#pragma unroll
                for (int i = 0; i < GSDD_COMPOSE_MAX_COND; ++i) {
                    if (i < N) {                                  // scalar branch
                        const float4 v = *reinterpret_cast<const float4*>(row0 + i * block + k);
                        const float xi[4] = {lsm_clamp(v.x, lse[i]), lsm_clamp(v.y, lse[i]), lsm_clamp(v.z, lse[i]), lsm_clamp(v.w, lse[i])};
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float diff = xi[e] - xu[e];
                            const float sc = wi[i] * diff;
                            acc[e] = acc[e] + sc;
                        }
                    }
                }
                *reinterpret_cast<float4*>(orow + k) = make_float4(acc[0], acc[1], acc[2], acc[3]);
            }
        }
    }
}

}  // namespace gsdd

using namespace gsdd;

extern "C" int gsdd_d3pm_compose(const gsdd_compose_desc* d, void* stream) {
    GSDD_CHECK_ARG(d != nullptr, "null descriptor");
    GSDD_CHECK_ARG(d->logits && d->weights && d->out, "null pointer");
    GSDD_CHECK_ARG(d->n_cond >= 1 && d->n_cond <= GSDD_COMPOSE_MAX_COND, "n_cond must be in [1, 4]");
    GSDD_CHECK_ARG(d->B > 0 && d->L > 0, "bad sizes");
    GSDD_CHECK_ARG(d->K >= 4 && d->K % 4 == 0 && d->K <= 8192, "K must be a multiple of 4 in [4, 8192]");
    GSDD_CHECK_ARG(aligned16(d->logits) && aligned16(d->out), "logits and out must be 16-byte aligned");
    const int64_t npos = (int64_t)d->B * d->L;
    const int64_t block = npos * d->K;
    // out is block 0 itself, or lies clear of all N + 1 blocks (a partial overlap with block 0 is no more in-place than one with block 1)
    const uintptr_t lo = (uintptr_t)d->logits, o = (uintptr_t)d->out, bytes = (uintptr_t)block * sizeof(float);
    GSDD_CHECK_ARG(o == lo || o + bytes <= lo || o >= lo + (uintptr_t)(d->n_cond + 1) * bytes,
                   "out may be block 0 of logits or must not overlap logits at all");
    const dim3 grid((unsigned)((npos + 3) / 4)), blk(256);
    hipStream_t st = (hipStream_t)stream;
    // FULL at K = 4096 only, as the step's families
    if (d->K == 4096) hipLaunchKernelGGL((d3pm_compose_kernel<16, true>), grid, blk, 0, st, *d);
    else for_class_width(d->K, [&](auto jc) {
        constexpr int J = decltype(jc)::value;
        hipLaunchKernelGGL((d3pm_compose_kernel<J, false>), grid, blk, 0, st, *d);
    });
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}
