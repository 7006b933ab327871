// Purity-prior reverse step (Improved VQ-Diffusion's high-quality inference; p_sample with prior_rule 1 / 2,
// diffusion_transformer.py:304-346): instead of resampling every position, a call reveals the n most trusted [MASK] positions.
//
//   d3pm_purity_kernel   one wave64 per position, the class row in registers as in d3pm_step_kernel: log_softmax (fp64 sum) x2 ->
//                        classifier-free mix -> renormalise -> clamp = log_x_recon (no posterior: the t > 0 branch drops it), then
//                        score = exp(max_k log_x_recon) (rule 2; 1 for rule 1) and the candidate token = Gumbel arg-max of `prob`.
//   purity_smax_kernel   smax[b] = max_l score[b][l]: the one cross-position dependency.  For rule 2 with prior_weight r > 0 `prob`
//                        depends on it, so the logits are read twice: scores, this kernel, then the draw.
//   purity_select_kernel one workgroup per sample: Gumbel-top-n of the [MASK] positions with weights score / (smax + 1e-10), by a
//                        bitonic sort of (key, ~index) pairs in LDS.
//   advance_plan_kernel  steps the device-resident call counter and loads the next call's (t, n) from the plan arrays, so that one
//                        captured graph replays every purity call.
#include "common.hpp"
#include "d3pm_rows.hpp"

namespace gsdd {

// MODE 0: score and draw from log_x_recon in one pass (rule 1, or rule 2 with prior_weight == 0).
// MODE 1: score only (first pass of rule 2 with prior_weight > 0).
// MODE 2: draw only; `prob` is the re-weighted row when prior_rule == 2 and prior_weight > 0 (reads smax[b]), log_x_recon otherwise.
//         The debug hooks exist in this mode only (the host runs MODE 1 -> smax -> MODE 2 whenever a hook is set).
// FULL / OCC as in d3pm_step_kernel: at K = 4096 two 64-register rows are live through the guidance mix, which needs the 256-VGPR
// budget of two waves per SIMD to stay out of scratch memory.
// TRUNC: top-r truncation of log_x_recon (truncate_row) before the score and `prob`, in a kernel family of its own
// (d3pm_purity_trunc_kernel); the plain kernels compile the body with TRUNC = false.  The row maximum is always kept, so the score
// of a truncated call is the plain call's.
template <int J, bool FULL, int MODE, bool DBG, bool TRUNC>
__device__ __forceinline__ void d3pm_purity_body(const gsdd_purity_desc& d) {
    const int lane = threadIdx.x & 63;
    const int64_t pos = (int64_t)blockIdx.x * 4 + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (pos >= (int64_t)d.B * d.L) return;
    const int b = (int)(pos / d.L), l = (int)(pos % d.L);
    const int K = d.K;
    const float NEG = -INFINITY;

    float x0[J][4];
    {   // ---- predict_start on the conditional logits
        const float* row = d.logits_c + pos * (int64_t)K;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int k = 4 * lane + 256 * j;
            if (FULL || k < K) {
                const float4 v = *reinterpret_cast<const float4*>(row + k);
                x0[j][0] = v.x; x0[j][1] = v.y; x0[j][2] = v.z; x0[j][3] = v.w;
            } else {
                x0[j][0] = x0[j][1] = x0[j][2] = x0[j][3] = NEG;
            }
        }
        log_softmax_clamp<J>(x0);
    }
    if (d.logits_u != nullptr) {  // ---- cf_predict_start (:240-249)
        float xu[J][4];
        const float* row = d.logits_u + pos * (int64_t)K;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int k = 4 * lane + 256 * j;
            if (FULL || k < K) {
                const float4 v = *reinterpret_cast<const float4*>(row + k);
                xu[j][0] = v.x; xu[j][1] = v.y; xu[j][2] = v.z; xu[j][3] = v.w;
            } else {
                xu[j][0] = xu[j][1] = xu[j][2] = xu[j][3] = NEG;
            }
        }
        log_softmax_clamp<J>(xu);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const bool valid = FULL || (4 * lane + 256 * j) < K;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float diff = x0[j][e] - xu[j][e];
                const float sc = d.guidance * diff;
                x0[j][e] = valid ? (xu[j][e] + sc) : NEG;
            }
        }
        const float lse = wave_logsumexp<J, !FULL>(x0, 0.f, false);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const bool valid = FULL || (4 * lane + 256 * j) < K;
#pragma unroll
            for (int e = 0; e < 4; ++e) x0[j][e] = valid ? clamp70(x0[j][e] - lse) : NEG;
        }
    }
    if (TRUNC && MODE != 1) truncate_row<J, FULL>(x0, d.trunc_rate, lane, K);     // (the score pass reads the maximum only)
    if (DBG && d.recon_dbg != nullptr) {
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = 4 * lane + 256 * j + e;
                if (k < K) d.recon_dbg[((int64_t)b * (K + 1) + k) * d.L + l] = x0[j][e];
            }
        if (lane == 0) d.recon_dbg[((int64_t)b * (K + 1) + K) * d.L + l] = -70.f;
    }

    // ---- score (:313-316): exp of the row maximum (the [MASK] row, -70, is the floor of the clamp and never above it)
    float score = 1.f;
    if (d.prior_rule == 2) {
        float mx = -70.f;
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) mx = fmaxf(mx, x0[j][e]);
        score = exp_le0(wave_max(mx));
    }
    if (MODE != 2 && lane == 0) d.score[pos] = score;
    if (MODE == 1) return;

    // ---- prob (:319-324)
    float probK = -70.f;                                  // the [MASK] row of `prob`
    if (MODE == 2 && d.prior_rule == 2 && d.prior_weight > 0.f) {
        const float w = score / (d.smax[b] + 1e-10f);     // the normalised score of :317
        if (DBG && d.score_dbg != nullptr && lane == 0) d.score_dbg[pos] = w;
        const float a = 1.f + w * d.prior_weight;
#pragma unroll
        for (int j = 0; j < J; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e) x0[j][e] = a * x0[j][e];          // (a > 0: an empty slot stays -inf)
        const float yK = a * -70.f;
        const float lse = wave_logsumexp<J, !FULL>(x0, yK, true);
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const bool valid = FULL || (4 * lane + 256 * j) < K;
#pragma unroll
            for (int e = 0; e < 4; ++e) x0[j][e] = valid ? clamp70(x0[j][e] - lse) : NEG;
        }
        probK = clamp70(yK - lse);
    } else if (DBG && d.score_dbg != nullptr && lane == 0) {
        d.score_dbg[pos] = d.prior_rule == 2 ? score / (d.smax[b] + 1e-10f) : 1.f;
    }

    // ---- candidate token: log_sample_categorical(prob) (:326, :354-357) on the (B, K+1, L) uniforms of the step kernel
    float best = NEG;
    int best_k = 0;
    const uint32_t kp4 = (uint32_t)((K + 1 + 3) / 4);
    const uint32_t stream_id = (uint32_t)d.stream_dev[0];
    const uint64_t grow = (uint64_t)(d.row0 + pos);
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int k0 = 4 * lane + 256 * j;
        if (FULL || k0 < K) {
            const float4 u4 = philox_uniform4(d.seed, stream_id, grow, kp4, (uint32_t)(k0 >> 2));
            const float u[4] = {u4.x, u4.y, u4.z, u4.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float o = x0[j][e];
                if (DBG && d.prob_dbg != nullptr) d.prob_dbg[((int64_t)b * (K + 1) + k0 + e) * d.L + l] = o;
                const float v = gumbel(u[e]) + o;
                if (v > best) { best = v; best_k = k0 + e; }
            }
        }
    }
    if (lane == ((K >> 2) & 63)) {  // the [MASK] class k = K (K % 4 == 0 -> word 0 of quad K/4)
        const float4 u4 = philox_uniform4(d.seed, stream_id, grow, kp4, (uint32_t)(K >> 2));
        if (DBG && d.prob_dbg != nullptr) d.prob_dbg[((int64_t)b * (K + 1) + K) * d.L + l] = probK;
        const float v = gumbel(u4.x) + probK;
        if (v > best) { best = v; best_k = K; }
    }
    const int win = wave_argmax(best, best_k);
    if (lane == 0) d.cand[pos] = win;
}

template <int J, bool FULL, int MODE, bool DBG, int OCC = 3>
__global__ __launch_bounds__(256, OCC) void d3pm_purity_kernel(gsdd_purity_desc d) {
    d3pm_purity_body<J, FULL, MODE, DBG, false>(d);
}

template <int J, bool FULL, int MODE, bool DBG>
__global__ __launch_bounds__(256, 2) void d3pm_purity_trunc_kernel(gsdd_purity_desc d) {
    d3pm_purity_body<J, FULL, MODE, DBG, true>(d);
}

// smax[b] = max_l score[b][l]   (scores are in (0, 1])
__global__ __launch_bounds__(256) void purity_smax_kernel(const float* score, int L, float* smax) {
    __shared__ float red[4];
    const int b = blockIdx.x, tid = threadIdx.x;
    float m = 0.f;
    for (int l = tid; l < L; l += 256) m = fmaxf(m, score[(int64_t)b * L + l]);
    m = wave_max(m);
    if ((tid & 63) == 0) red[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) smax[b] = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}

constexpr int SELECT_MAX_L = 4096;
constexpr int SELECT_THREADS = 1024;

// Weighted selection without replacement (torch.multinomial(_score[i], n), :341) as Gumbel-top-n: key_l = log w_l + Gumbel(u_l) on the
// [MASK] positions, the n largest keys win, ties go to the lower index.  The pairs (ordered key bits, ~l) are sorted in LDS, largest
// first; a position that is not [MASK] (weight 0 in the reference) and the padding up to the power of two sort as 0, below every key.
__global__ __launch_bounds__(SELECT_THREADS) void purity_select_kernel(gsdd_purity_select_desc d) {
    __shared__ uint64_t s[SELECT_MAX_L];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int L = d.L, K = d.K;
    int P = 1;
    while (P < L) P <<= 1;
    const int64_t base = (int64_t)b * L;
    const float den = d.prior_rule == 2 ? d.smax[b] + 1e-10f : 1.f;
    const uint32_t kp4 = (uint32_t)((L + 3) / 4);
    const uint32_t stream_id = (uint32_t)(d.stream_dev[0] + d.stream_add);
    const uint64_t grow = (uint64_t)(d.row0 / L + b);                 // the global sample index
    for (int l = tid; l < P; l += SELECT_THREADS) {
        uint64_t c = 0;
        if (l < L) {
            const int64_t tok = d.tok_in[base + l];
            const float4 u4 = philox_uniform4(d.seed, stream_id, grow, kp4, (uint32_t)(l >> 2));
            const float u = (l & 3) == 0 ? u4.x : (l & 3) == 1 ? u4.y : (l & 3) == 2 ? u4.z : u4.w;
            const float w = d.prior_rule == 2 ? d.score[base + l] / den : 1.f;
            const float key = logf(w) - logf(-logf(u + 1e-30f) + 1e-30f);
            if (d.key_dbg != nullptr) d.key_dbg[base + l] = key;
            if (tok == K) c = ((uint64_t)ordered_bits(key) << 32) | (uint32_t)~(uint32_t)l;
            if (d.tok_out != d.tok_in) d.tok_out[base + l] = tok;
        }
        s[l] = c;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)                 // bitonic sort, descending
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += SELECT_THREADS) {
                const int p = i ^ j;
                if (p > i) {
                    const uint64_t a = s[i], c = s[p];
                    const bool desc = (i & k) == 0;
                    if (desc ? a < c : a > c) { s[i] = c; s[p] = a; }
                }
            }
            __syncthreads();
        }
    int64_t n = d.n_dev[0];
    n = n < 0 ? 0 : (n > L ? L : n);
    for (int i = tid; i < (int)n; i += SELECT_THREADS) {
        const uint64_t c = s[i];
        if (c != 0) {                                 // (fewer [MASK] positions than n: nothing else is touched)
            const uint32_t l = ~(uint32_t)c;
            d.tok_out[base + l] = d.cand[base + l];
        }
    }
}

// one workgroup: step <- step + 1; t[b] <- plan_t[i], n <- plan_n[i] with i = min(step, n_calls - 1); stream += ds
__global__ __launch_bounds__(256) void advance_plan_kernel(int64_t* step_dev, const int64_t* plan_t, const int64_t* plan_n,
                                                           int64_t n_calls, int64_t* t_dev, int B, int64_t* n_dev,
                                                           int64_t* stream_dev, int64_t ds) {
    const int64_t step = step_dev[0] + 1;
    const int64_t i = step < n_calls ? step : n_calls - 1;
    const int64_t t = plan_t[i];
    __syncthreads();                                  // every thread has read the counter before thread 0 moves it
    for (int q = threadIdx.x; q < B; q += 256) t_dev[q] = t;
    if (threadIdx.x == 0) {
        step_dev[0] = step;
        n_dev[0] = plan_n[i];
        if (stream_dev != nullptr) stream_dev[0] += ds;
    }
}

}  // namespace gsdd

using namespace gsdd;

extern "C" int gsdd_d3pm_purity_step(const gsdd_purity_desc* d, void* stream) {
    GSDD_CHECK_ARG(d != nullptr, "null descriptor");
    GSDD_CHECK_ARG(d->logits_c && d->stream_dev && d->score && d->smax && d->cand, "null pointer");
    GSDD_CHECK_ARG(d->B > 0 && d->L > 0, "bad sizes");
    GSDD_CHECK_ARG(d->K >= 4 && d->K % 4 == 0 && d->K <= 8192, "K must be a multiple of 4 in [4, 8192]");
    GSDD_CHECK_ARG(d->prior_rule == 1 || d->prior_rule == 2, "prior_rule must be 1 or 2 (0 is the plain step: gsdd_d3pm_step)");
    GSDD_CHECK_ARG(d->prior_weight >= 0.f, "prior_weight must be >= 0");
    GSDD_CHECK_ARG(d->trunc_rate == 0.f || (d->trunc_rate > 0.f && d->trunc_rate < 1.f), "trunc_rate must be 0 (off) or in (0, 1)");
    const int64_t npos = (int64_t)d->B * d->L;
    const dim3 grid((unsigned)((npos + 3) / 4)), block(256);
    hipStream_t st = (hipStream_t)stream;
    const bool dbg = d->recon_dbg != nullptr || d->prob_dbg != nullptr || d->score_dbg != nullptr;
    const bool two_pass = dbg || (d->prior_rule == 2 && d->prior_weight > 0.f);
    const bool trunc = d->trunc_rate != 0.f;
    // pass: 0 = the fused score + draw, 1 = scores, 2 = draw
    auto launch = [&](int mode) {
        // top-r truncation: the d3pm_purity_trunc_kernel family (the score pass has no use for it), FULL at K = 4096 only
        if (trunc && mode != 1 && d->K == 4096) {
            if (mode == 0) hipLaunchKernelGGL((d3pm_purity_trunc_kernel<16, true, 0, false>), grid, block, 0, st, *d);
            else if (!dbg) hipLaunchKernelGGL((d3pm_purity_trunc_kernel<16, true, 2, false>), grid, block, 0, st, *d);
            else hipLaunchKernelGGL((d3pm_purity_trunc_kernel<16, true, 2, true>), grid, block, 0, st, *d);
        } else if (trunc && mode != 1) {
            for_class_width(d->K, [&](auto jc) {
                constexpr int J = decltype(jc)::value;
                if (mode == 0) hipLaunchKernelGGL((d3pm_purity_trunc_kernel<J, false, 0, false>), grid, block, 0, st, *d);
                else if (!dbg) hipLaunchKernelGGL((d3pm_purity_trunc_kernel<J, false, 2, false>), grid, block, 0, st, *d);
                else hipLaunchKernelGGL((d3pm_purity_trunc_kernel<J, false, 2, true>), grid, block, 0, st, *d);
            });
        } else if (d->K == 4096 && !dbg) {           // the production shape: every slot holds a class, no hooks, OCC = 2 (no scratch)
            if (mode == 0) hipLaunchKernelGGL((d3pm_purity_kernel<16, true, 0, false, 2>), grid, block, 0, st, *d);
            else if (mode == 1) hipLaunchKernelGGL((d3pm_purity_kernel<16, true, 1, false, 2>), grid, block, 0, st, *d);
            else hipLaunchKernelGGL((d3pm_purity_kernel<16, true, 2, false, 2>), grid, block, 0, st, *d);
        } else {                                     // never FULL, OCC = 3; test hooks in the draw pass only
            for_class_width(d->K, [&](auto jc) {
                constexpr int J = decltype(jc)::value;
                if (mode == 0) hipLaunchKernelGGL((d3pm_purity_kernel<J, false, 0, false>), grid, block, 0, st, *d);
                else if (mode == 1) hipLaunchKernelGGL((d3pm_purity_kernel<J, false, 1, false>), grid, block, 0, st, *d);
                else if (!dbg) hipLaunchKernelGGL((d3pm_purity_kernel<J, false, 2, false>), grid, block, 0, st, *d);
                else hipLaunchKernelGGL((d3pm_purity_kernel<J, false, 2, true>), grid, block, 0, st, *d);
            });
        }
    };
    launch(two_pass ? 1 : 0);
    GSDD_CHECK_LAUNCH();
    hipLaunchKernelGGL(purity_smax_kernel, dim3((unsigned)d->B), dim3(256), 0, st, (const float*)d->score, d->L, d->smax);
    GSDD_CHECK_LAUNCH();
    if (two_pass) {
        launch(2);
        GSDD_CHECK_LAUNCH();
    }
    return GSDD_OK;
}

extern "C" int gsdd_d3pm_purity_select(const gsdd_purity_select_desc* d, void* stream) {
    GSDD_CHECK_ARG(d != nullptr, "null descriptor");
    GSDD_CHECK_ARG(d->tok_in && d->tok_out && d->cand && d->n_dev && d->stream_dev, "null pointer");
    GSDD_CHECK_ARG(d->B > 0 && d->L > 0 && d->K > 0, "bad sizes");
    GSDD_CHECK_ARG(d->L <= SELECT_MAX_L, "the selection sorts one sample in LDS: L must be <= 4096");
    GSDD_CHECK_ARG(d->prior_rule == 1 || d->prior_rule == 2, "prior_rule must be 1 or 2");
    GSDD_CHECK_ARG(d->prior_rule == 1 || (d->score && d->smax), "prior_rule 2 needs score and smax");
    GSDD_CHECK_ARG(d->row0 >= 0 && d->row0 % d->L == 0, "row0 must be a multiple of L (the draw is keyed by the sample index)");
    hipLaunchKernelGGL(purity_select_kernel, dim3((unsigned)d->B), dim3(SELECT_THREADS), 0, (hipStream_t)stream, *d);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}

extern "C" int gsdd_advance_plan(int64_t* step_dev, const int64_t* plan_t, const int64_t* plan_n, int64_t n_calls, int64_t* t_dev,
                                 int B, int64_t* n_dev, int64_t* stream_dev, int64_t ds, void* stream) {
    GSDD_CHECK_ARG(step_dev && plan_t && plan_n && t_dev && n_dev, "null pointer");
    GSDD_CHECK_ARG(n_calls > 0, "empty plan");
    GSDD_CHECK_ARG(B > 0 && B <= 65536, "bad B");
    hipLaunchKernelGGL(advance_plan_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, step_dev, plan_t, plan_n, n_calls, t_dev, B,
                       n_dev, stream_dev, ds);
    GSDD_CHECK_LAUNCH();
    return GSDD_OK;
}
